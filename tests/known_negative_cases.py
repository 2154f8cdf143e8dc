"""Case table, batch builder and float64 statement of the training step with known triples left out of the negatives
(dglke_train --exclude_positive, include/kge_hip.h kge_step_fused_known).  Test infrastructure; a plain module, not a conftest.
Shared by
  tests/test_known_negative_inputs.py   (CPU): the statement collapses to the oracle's step for an empty set, the -1e6 entries
                                        give exact zeros in float64, every case carries the edge cases listed below;
  tests/test_gpu_known_negatives.py     (GPU): the mask kernel, the whole step, the exactness properties, the entry points.

The statement is composed from the oracle's public pieces (score_pos, pos_side, score_neg, loss_fwd_bwd, score_neg_bwd,
pos_side_bwd, score_pos_bwd, reg_grad, adagrad_update); the entries of the float64 negative block whose corrupted triple is known
are replaced by -1e6 before loss_fwd_bwd.  TransR has no such pieces in the oracle: its statement is written out below.

Every case's two batches (tail corruption, then head corruption) are PLANTED against one known set K:
  row 0            every column known, and its list carries HUB more entities that are not in the batch (a list > 64);
  row 1            no column known (its uncorrupted entity occurs in no other row and in no triple of K but its own positive);
  row 2            known in the last column and in column min(32, N - 1) (there is no column 32 below N = 33);
  row 3            its own corrupted entity sits in slot 1 of its chunk (known through the positive triple itself);
  one entity       occurs once in the batch, as a negative of the last chunk, and is known for every row of that chunk: nothing of
                   this step may move its row;
  everything else  known with probability P_KNOWN; K also holds every positive and 300 unrelated triples.
"""
import numpy as np

import loss_option_cases as L
from oracle import kge_oracle as O

KNOWN_SCORE = -1.0e6        # include/kge_hip.h KGE_KNOWN_SCORE
HUB = 80
P_KNOWN = 0.2

# id -> model, hidden, de, dr, B, chunk, N, gamma, scale, lr, genre, pairwise, adv, adv_temp, reg_coef
# widths: 32 / 34 / 400 are where the score kernels change instance (vector / scalar rows, one / several k-steps); N = 4 / 40 / 200:
# the packed row layout of the loss kernel at one and at 50 lanes (N % 4 == 0) and, with N = 4 .. 200 on unaligned rows, the
# strided one (chunk * N * 4 bytes is 16-byte aligned for every case here, so the strided layout is reached through 'l1-n5').
# TransR: 12 x 24 (the engine's widths are hidden or 2 * hidden: 16 x 24 cannot be asked for; 24 keeps the ragged relation width)
_T = [
    ("l2-d400-n200-adv", "TransE_l2", 400, False, False, 64, 32, 200, 48.0, 19.2, 0.25, "Logsigmoid", False, True, 1.0, 1e-9),
    ("l2-d32-n40", "TransE_l2", 32, False, False, 32, 16, 40, 12.0, 4.8, 0.1, "Logsigmoid", False, False, 1.0, 0.0),
    ("l2-d34-n4-adv", "TransE_l2", 34, False, False, 16, 8, 4, 12.0, 4.8, 0.1, "Logsigmoid", False, True, 1.0, 0.0),
    ("dist-d400-n200", "DistMult", 400, False, False, 64, 32, 200, 143.0, 2.1, 0.08, "Logsigmoid", False, False, 1.0, 2e-6),
    ("dist-d34-n40-hinge-adv", "DistMult", 34, False, False, 32, 8, 40, 12.0, 1.6, 0.1, "Hinge", False, True, 0.5, 0.0),
    ("complex-d32-n200-logistic", "ComplEx", 32, True, True, 32, 16, 200, 12.0, 1.0, 0.1, "Logistic", False, False, 1.0, 0.0),
    ("simple-d32-n40-bce-adv", "SimplE", 32, True, True, 32, 16, 40, 12.0, 1.3, 0.1, "BCE", False, True, 1.0, 0.0),
    ("rotate-d32-n40-adv", "RotatE", 32, True, False, 32, 16, 40, 24.0, 0.89, 0.05, "Logsigmoid", False, True, 1.0, 1e-7),
    ("l1-d32-n200-hinge-pw", "TransE_l1", 32, False, False, 16, 8, 200, 12.0, 1.18, 0.01, "Hinge", True, False, 1.0, 0.0),
    ("l1-d400-n5-adv", "TransE_l1", 400, False, False, 16, 8, 5, 48.0, 1.18, 0.01, "Logsigmoid", False, True, 1.0, 0.0),
    # the generic loss kernel (more than 512 negatives per row: no register-resident row)
    ("dist-d32-n600-adv", "DistMult", 32, False, False, 16, 8, 600, 12.0, 1.6, 0.1, "Logsigmoid", False, True, 1.0, 0.0),
    ("rescal-d16-n40-adv", "RESCAL", 16, False, False, 32, 16, 40, 6.0, 4.0, 0.05, "Logsigmoid", False, True, 1.0, 0.0),
    ("transr-12x24-n40-adv", "TransR", 12, False, True, 32, 16, 40, 20.0, 0.5, 0.05, "Logsigmoid", False, True, 1.0, 0.0),
]
N_ENT, N_REL = 600, 7


def _case(row):
    cid, model, hidden, de, dr, B, chunk, N, gamma, scale, lr, genre, pw, adv, temp, rc = row
    return dict(id=cid, shape="known", model=model, n_ent=N_ENT, n_rel=N_REL, hidden=hidden, de=de, dr=dr, B=B, chunk=chunk, N=N,
                gamma=gamma, lr=lr, scale=scale, genre=genre, pairwise=pw, margin=1.0, adv=adv, adv_temp=temp, reg_coef=rc, reg_norm=3,
                impts=False, neg_deg=False, flags=(0,), rows=5e-3, seed=len(cid))


CASES = [_case(r) for r in _T]


def corrupted(bt):
    """(uncorrupted entity, corrupted entity) per positive"""
    return (bt["t"], bt["h"]) if bt["neg_head"] else (bt["h"], bt["t"])


def triple_of(bt, i, n):
    """the corrupted triple of row i with entity n"""
    return (int(n), int(bt["r"][i]), int(bt["t"][i])) if bt["neg_head"] else (int(bt["h"][i]), int(bt["r"][i]), int(n))


def build(c):
    """-> (batches [tail step, head step], K as three int64 arrays, notes per batch: dict(lone=entity, lone_slot=slot))"""
    rng = np.random.RandomState(9100 + c["seed"])
    B, chunk, N, n_ent, n_rel = c["B"], c["chunk"], c["N"], c["n_ent"], c["n_rel"]
    C = B // chunk
    K, bts, notes = set(), [], []
    # entities 0 .. 399 feed the batches; 400 .. 599 are reserved: hub members, the lone negative, row 1's private entity
    for step in (1, 2):
        neg_head = step % 2 == 0
        h = rng.randint(0, 400, size=B).astype(np.int64)
        t = rng.randint(0, 400, size=B).astype(np.int64)
        same = h == t                                   # (TransR: no edge with h == t, tests/loss_option_cases.py batches)
        t[same] = (t[same] + 1) % 400
        r = rng.randint(0, n_rel, size=B).astype(np.int64)
        neg = rng.randint(0, 400, size=C * N).astype(np.int64)
        x, y = (t, h) if neg_head else (h, t)           # views: uncorrupted / corrupted side
        x[0], x[1] = 0, 590 + step                      # row 0: entity id 0; row 1: private
        if y[3] == y[1]:
            y[3] = (y[3] + 1) % 400
        c1 = neg[(1 // chunk) * N:(1 // chunk + 1) * N]  # row 1 stays clean: its own corrupted entity is not among its negatives
        c1[c1 == y[1]] = (y[1] + 1) % 400
        lone, lone_slot = 580 + step, (C - 1) * N + 2   # (the LAST chunk: rows 0 .. 3 sit in the first; every case has C >= 2, chunk >= 4)
        neg[lone_slot] = lone
        neg[C * N - 1] = n_ent - 1                      # the last entity id, in the last column of the last chunk
        neg[(3 // chunk) * N + 1] = y[3]                # row 3's own corrupted entity in slot 1 of its chunk (y[3] != y[1]: row 1 stays clean)
        bt = dict(h=h, t=t, r=r, neg=neg, neg_head=neg_head, C=C, w=None)
        nid, inv = np.unique(np.concatenate([h, t]), return_inverse=True)
        bt.update(nid=nid.astype(np.int64), h_local=inv[:B].astype(np.int64), t_local=inv[B:].astype(np.int64))
        for i in range(B):
            K.add((int(h[i]), int(r[i]), int(t[i])))
            cn = neg[(i // chunk) * N:(i // chunk + 1) * N]
            if i == 1:
                continue
            for j in range(N):
                forced = i == 0 or (i == 2 and j in (N - 1, min(32, N - 1))) or (i // chunk == C - 1 and cn[j] == lone)
                if forced or rng.rand() < P_KNOWN:
                    K.add(triple_of(bt, i, cn[j]))
        for e in range(400, 400 + HUB):                 # row 0's list: a hub
            K.add(triple_of(bt, 0, e))
        bts.append(bt)
        notes.append(dict(lone=lone, lone_slot=lone_slot))
    for _ in range(300):
        K.add((int(rng.randint(0, 400)), int(rng.randint(0, n_rel)), int(rng.randint(0, 400))))
    k = np.array(sorted(K), dtype=np.int64)
    return bts, (k[:, 0].copy(), k[:, 1].copy(), k[:, 2].copy()), notes


def known_matrix(K, bt, chunk, N):
    """[B, N] bool by set membership: pair (i, j) is known when row i's corrupted triple with column j's entity is in K"""
    S = set(zip(K[0].tolist(), K[1].tolist(), K[2].tolist()))
    B = len(bt["h"])
    out = np.zeros((B, N), bool)
    for i in range(B):
        cn = bt["neg"][(i // chunk) * N:(i // chunk + 1) * N]
        for j in range(N):
            out[i, j] = triple_of(bt, i, cn[j]) in S
    return out


EMPTY = (np.zeros(0, np.int64),) * 3


# --------------------------------------------------------------------------------------------------------------------------
# the masked step in the dtype of the tables
# --------------------------------------------------------------------------------------------------------------------------
def masked_forward_backward(c, ent, rel, proj, bt, known):
    """known: [B, N] bool.  Same outputs as O.forward_backward / O.transr_forward_backward."""
    cfg = L.config(c)
    if c["model"] == "TransR":
        return _transr_masked(cfg, ent, rel, proj, bt, c["chunk"], c["N"], known)
    dt = ent.dtype
    chunk, N = c["chunk"], c["N"]
    B = len(bt["h"])
    C = B // chunk
    pos_emb, r, neg = O.gather_rows(ent, bt["nid"]), O.gather_rows(rel, bt["r"]), O.gather_rows(ent, bt["neg"])
    h, t = pos_emb[bt["h_local"]], pos_emb[bt["t_local"]]
    gamma = dt.type(cfg.gamma)
    neg_head = bt["neg_head"]
    p = O.score_pos(cfg.model, h, r, t, gamma, cfg.emb_init)
    x = t if neg_head else h
    a = O.pos_side(cfg.model, neg_head, x, r, cfg.emb_init)
    n = O.score_neg(cfg.model, a, neg, C, chunk, N, gamma)
    n = np.where(known.reshape(n.shape), dt.type(KNOWN_SCORE), n)
    (pl, nl, loss), dpos, dneg = O.loss_fwd_bwd(p, n.reshape(B, N), None, cfg.loss_genre, cfg.adv, cfg.adv_temp, cfg.pairwise, cfg.margin)
    use_reg = cfg.reg_coef > 0.0 and cfg.reg_norm > 0
    reg = 0.0
    if use_reg:
        reg = O.reg_value([pos_emb, neg], cfg.reg_coef, cfg.reg_norm) + O.reg_value([r], cfg.reg_coef, cfg.reg_norm)
    gh, gr, gt = O.score_pos_bwd(cfg.model, h, r, t, dpos, gamma, cfg.emb_init)
    ga, g_neg = O.score_neg_bwd(cfg.model, a, neg, dneg.reshape(C, chunk, N), C, chunk, N, gamma)
    gx, gr2 = O.pos_side_bwd(cfg.model, neg_head, x, r, ga, cfg.emb_init)
    gr = gr + gr2
    if neg_head:
        gt = gt + gx
    else:
        gh = gh + gx
    g_pos = np.zeros_like(pos_emb)
    np.add.at(g_pos, bt["h_local"], gh.astype(dt))
    np.add.at(g_pos, bt["t_local"], gt.astype(dt))
    if use_reg:
        g_pos += O.reg_grad(pos_emb, cfg.reg_coef, cfg.reg_norm).astype(dt)
        g_neg = g_neg + O.reg_grad(neg, cfg.reg_coef, cfg.reg_norm)
        gr = gr + O.reg_grad(r, cfg.reg_coef, cfg.reg_norm)
    return dict(pos_score=p, neg_score=n, log=(pl, nl, loss, reg), dneg=dneg, g_pos_ent=g_pos.astype(dt), g_rel=gr.astype(dt),
                g_neg=g_neg.astype(dt))


def _transr_masked(cfg, ent, rel, proj, bt, chunk, N, known):
    """TransR (score_fun.py:110-220): p = gamma - |h P + r - t P|_1; negatives n_ij = gamma - |neg_j P_i - (x_i P_i - r_i)|_1 with
    x the uncorrupted entity (both closures subtract the relation, :203-204, :212-213); two projection traces"""
    dt = ent.dtype
    B = len(bt["h"])
    C = B // chunk
    De, Dr = ent.shape[1], rel.shape[1]
    pos_emb, r, neg = ent[bt["nid"]], rel[bt["r"]], ent[bt["neg"]]
    P = proj[bt["r"]].reshape(B, De, Dr)
    Pc = P.reshape(C, chunk, De, Dr)
    h, t = pos_emb[bt["h_local"]], pos_emb[bt["t_local"]]
    gamma = dt.type(cfg.gamma)
    u = np.einsum("ab,abc->ac", h, P) + r - np.einsum("ab,abc->ac", t, P)
    p = gamma - np.abs(u).sum(-1)
    x = t if bt["neg_head"] else h
    q = np.einsum("ab,abc->ac", x, P) - r
    D = np.einsum("cjd,cide->cije", neg.reshape(C, N, De), Pc) - q.reshape(C, chunk, 1, Dr)
    n = gamma - np.abs(D).sum(-1)
    n = np.where(known.reshape(n.shape), dt.type(KNOWN_SCORE), n)
    (pl, nl, loss), dpos, dneg = O.loss_fwd_bwd(p, n.reshape(B, N), None, cfg.loss_genre, cfg.adv, cfg.adv_temp, cfg.pairwise, cfg.margin)
    use_reg = cfg.reg_coef > 0.0 and cfg.reg_norm > 0
    reg = O.reg_value([pos_emb, neg], cfg.reg_coef, cfg.reg_norm) + O.reg_value([r], cfg.reg_coef, cfg.reg_norm) if use_reg else 0.0
    s = np.sign(u)
    ghp, gtp = -dpos[:, None] * s, dpos[:, None] * s
    gr = -dpos[:, None] * s
    g_proj0 = h[:, :, None] * ghp[:, None, :] + t[:, :, None] * gtp[:, None, :]
    gh, gt = np.einsum("abc,ac->ab", P, ghp), np.einsum("abc,ac->ab", P, gtp)
    dY = -dneg.reshape(C, chunk, N, 1) * np.sign(D)
    dq = -dY.sum(2).reshape(B, Dr)
    g_neg = np.einsum("cije,cide->cjd", dY, Pc).reshape(C * N, De)
    g_proj1 = np.einsum("cjd,cije->cide", neg.reshape(C, N, De), dY).reshape(B, De, Dr) + x[:, :, None] * dq[:, None, :]
    gx = np.einsum("abc,ac->ab", P, dq)
    gr = gr - dq
    if bt["neg_head"]:
        gt = gt + gx
    else:
        gh = gh + gx
    g_pos = np.zeros_like(pos_emb)
    np.add.at(g_pos, bt["h_local"], gh)
    np.add.at(g_pos, bt["t_local"], gt)
    if use_reg:
        g_pos += O.reg_grad(pos_emb, cfg.reg_coef, cfg.reg_norm)
        g_neg = g_neg + O.reg_grad(neg, cfg.reg_coef, cfg.reg_norm)
        gr = gr + O.reg_grad(r, cfg.reg_coef, cfg.reg_norm)
    return dict(pos_score=p, neg_score=n, log=(pl, nl, loss, reg), dneg=dneg, g_pos_ent=g_pos.astype(dt), g_rel=gr.astype(dt),
                g_neg=g_neg.astype(dt), g_proj0=g_proj0.reshape(B, De * Dr).astype(dt), g_proj1=g_proj1.reshape(B, De * Dr).astype(dt))


def masked_step(c, ent, es, rel, rs, proj, ps, bt, known):
    """forward + backward + the reference's update order (entity traces, relation trace, TransR: the two projection traces), in place"""
    out = masked_forward_backward(c, ent, rel, proj, bt, known)
    lr = c["lr"]
    O.adagrad_update(ent, es, bt["nid"], out["g_pos_ent"], lr)
    O.adagrad_update(ent, es, bt["neg"], out["g_neg"], lr)
    O.adagrad_update(rel, rs, bt["r"], out["g_rel"], lr)
    if c["model"] == "TransR":
        O.adagrad_update(proj, ps, bt["r"], out["g_proj0"], lr)
        O.adagrad_update(proj, ps, bt["r"], out["g_proj1"], lr)
    return out
