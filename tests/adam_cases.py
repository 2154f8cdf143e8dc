"""--optimizer Adam (include/kge_hip.h, kge_step_optim with KGE_OPT_ADAM): the statement in float64, the case tables and the input
builders of tests/test_adam_inputs.py (CPU guard) and tests/test_gpu_adam.py (the device).

THE STATEMENT.  Lazy (row-sparse) Adam with a PER-ROW step count, the rule of DGL's sparse Adam.  G_x = the sum of a table row's
gradient traces in a step - the positive trace, then the negative trace, regulariser terms where the Adagrad step adds them
(oracle.kge_oracle.forward_backward: g_pos_ent per positive node, g_neg per negative slot, g_rel per edge; QuatE, PairRE and the
Softmax genre: the float64 statements of quate_cases.py, pairre_cases.py and softmax_loss_cases.py).  For a row x touched by a step:

    c   = min(c + 1, 2^24)
    m   = b1 m + (1 - b1) G
    v   = b2 v + (1 - b2) G * G
    x  -= lr (m / (1 - b1^c)) / (sqrt(v / (1 - b2^c)) + eps)            1 - b^c = -expm1(c log b)

one update per row per step; rows the step does not touch keep value, moments and count bit for bit.

AMBIGUITY.  Adam's first step is lr * sign(G): an element whose gradient lies inside the suite's gradient tolerance may move the
other way.  Element (i, k) of a table is ambiguous from step s on if 0 < |G64_ik| < 3e-4 * max|G64| over that table's touched rows
in step s; from then on that element of the row and of both moments is left out of the case's comparisons.  No compared array of
any case may lose more than AMBIGUITY_CAP of its elements (test_adam_inputs.py checks every case; seeds are chosen to stay inside).

THE COMPARISON of test_gpu_adam.py is step by step: the statement's step s starts from the tables, moments and counts the device
holds after step s - 1 (read back, exact in float64), so what is compared is one step of the statement against one step of the
kernels, four times in a row, and a sign an ambiguous element took in an earlier step does not leak into the other rows' gradients.
"""
import contextlib

import numpy as np

import known_negative_cases as KN
import loss_option_cases as L
import pairre_cases as PR
import quate_cases as QT
import softmax_loss_cases as SM
from modular_op_cases import GRAD_RTOL
from oracle import kge_oracle as O

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
CMAX = float(2 ** 24)
AMBIGUITY_CAP = 0.05
STEPS = 4
OPT_ADAGRAD, OPT_ADAM = 0, 1            # include/kge_hip.h


# --------------------------------------------------------------------------------------------------------------------------
# the statement
# --------------------------------------------------------------------------------------------------------------------------
def bias_correction(c, beta):
    with np.errstate(divide="ignore"):
        return -np.expm1(c * np.log(beta))


def adam_rows(x, mom, cnt, idx, G, lr, b1=BETA1, b2=BETA2, eps=EPS):
    """in place: rows idx (unique) of table x [n, d], moments mom [n, 2, d], counts cnt [n] take one Adam update with G [len, d]"""
    idx = np.asarray(idx, np.int64)
    assert len(np.unique(idx)) == len(idx)
    c = np.minimum(cnt[idx] + 1.0, CMAX)
    m = b1 * mom[idx, 0] + (1.0 - b1) * G
    v = b2 * mom[idx, 1] + (1.0 - b2) * G * G
    x[idx] -= lr * (m / bias_correction(c, b1)[:, None]) / (np.sqrt(v / bias_correction(c, b2)[:, None]) + eps)
    mom[idx, 0], mom[idx, 1], cnt[idx] = m, v, c


@contextlib.contextmanager
def _softmax_hook():
    saved = O.loss_fwd_bwd
    O.loss_fwd_bwd = SM.hooked_loss_fwd_bwd
    try:
        yield
    finally:
        O.loss_fwd_bwd = saved


def gradients(c, ent, rel, bt, known=None):
    """the three trace gradients of one step in the dtype of the tables (known: [B, N] bool or None)"""
    if c["model"] == "QuatE":
        return QT.forward_backward(c, ent, rel, bt, known)
    if c["model"] == "PairRE":
        return PR.forward_backward(c, ent, rel, bt, known)
    with _softmax_hook():
        if known is not None:
            assert bt.get("w") is None
            return KN.masked_forward_backward(c, ent, rel, None, bt, known)
        return O.forward_backward(L.config(c), ent, rel, bt["nid"], bt["h_local"], bt["t_local"], bt["r"], bt["neg"], bt["neg_head"],
                                  c["chunk"], c["N"], bt.get("w"))


def row_sums(out, bt, n_ent, n_rel):
    """-> (entity ids touched, G [len, d_e]), (relation ids touched, G [len, d_r]): traces summed per row, positive trace first"""
    Ge = np.zeros((n_ent, out["g_pos_ent"].shape[1]), out["g_pos_ent"].dtype)
    Gr = np.zeros((n_rel, out["g_rel"].shape[1]), out["g_rel"].dtype)
    np.add.at(Ge, bt["nid"], out["g_pos_ent"])
    np.add.at(Ge, bt["neg"], out["g_neg"])
    np.add.at(Gr, bt["r"], out["g_rel"])
    ie, ir = np.union1d(bt["nid"], bt["neg"]), np.unique(bt["r"])
    return (ie, Ge[ie]), (ir, Gr[ir])


def step(c, st, bt, known=None):
    """one step of the statement on the state st = dict(ent, rel, ent_mom, rel_mom, ent_cnt, rel_cnt), in place (any float dtype);
    -> dict(ent=(ids, G), rel=(ids, G), out=the oracle's outputs)"""
    out = gradients(c, st["ent"], st["rel"], bt, known)
    (ie, Ge), (ir, Gr) = row_sums(out, bt, st["ent"].shape[0], st["rel"].shape[0])
    b1, b2, eps = c.get("beta1", BETA1), c.get("beta2", BETA2), c.get("eps", EPS)
    adam_rows(st["ent"], st["ent_mom"], st["ent_cnt"], ie, Ge, c["lr"], b1, b2, eps)
    adam_rows(st["rel"], st["rel_mom"], st["rel_cnt"], ir, Gr, c["lr"], b1, b2, eps)
    return dict(ent=(ie, Ge), rel=(ir, Gr), out=out)


def ambiguous(ids, G, n):
    """[n, d] bool: the elements the ambiguity rule takes out in a step with row sums G of the touched rows ids"""
    mask = np.zeros((n, G.shape[1]), bool)
    a = np.abs(G)
    mask[ids] = (a > 0) & (a < GRAD_RTOL * a.max())
    return mask


def tol(ref):
    """3e-4 of the compared array's largest component + 3e-4 relative (modular_op_cases.grad_tol)"""
    ref = np.asarray(ref, np.float64)
    return GRAD_RTOL * max(float(np.abs(ref).max()) if ref.size else 0.0, 1e-12) + GRAD_RTOL * np.abs(ref)


# --------------------------------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------------------------------
def widths(c):
    """(d_e, d_r) of a case"""
    d_e = c["hidden"] * (2 if c["de"] else 1)
    return d_e, c["hidden"] * (2 if c["dr"] else 1)


def case(cid, model, hidden, de=False, dr=False, n_ent=48, n_rel=5, B=32, chunk=8, N=16, lr=0.01, genre="Logsigmoid", adv=False,
         adv_temp=1.0, pairwise=False, margin=1.0, reg_coef=0.0, reg_norm=3, neg_deg=False, known=False, edge_w=False, hub=False,
         seed=0, gamma=4.0, dev_plans=False):
    """gamma 4: at the suite's usual 12 the TransE_l2 scores of these small shapes saturate the criterion for most negatives and
    17 % of the entity elements fall under the ambiguity threshold (measured on the float64 statement; 1 % at gamma 4)"""
    if model == "PairRE":
        gamma = PR.GAMMA
    return dict(id=cid, model=model, hidden=hidden, de=de, dr=dr, n_ent=n_ent, n_rel=n_rel, B=B, chunk=chunk, N=N, lr=lr, genre=genre,
                adv=adv, adv_temp=adv_temp, pairwise=pairwise, margin=margin, reg_coef=reg_coef, reg_norm=reg_norm, neg_deg=neg_deg,
                known=known, edge_w=edge_w, hub=hub, seed=seed, gamma=gamma, scale=1.0, impts=edge_w)


WIDTHS = (16, 256, 260, 512, 516, 1024)          # the kernel changes instance at 256 / 512; 260 and 516 run a partial wavefront
# every width on the Q-mode TransE fast path and on per-edge gradient rows
WIDTH_CASES = [case("%s-w%d" % (m, w), m, w, adv=True) for m in ("TransE_l2", "DistMult") for w in WIDTHS]
# (the wide L1-type cases without -adv: a wide row of sign sums under self-adversarial weights has 5 - 13 % of its elements
#  below the ambiguity threshold - measured on the float64 statement)
MODEL_CASES = [
    case("TransE_l1-w16", "TransE_l1", 16, adv=True), case("TransE_l1-w260", "TransE_l1", 260, gamma=8.0),
    case("ComplEx-w16", "ComplEx", 8, True, True, adv=True), case("ComplEx-w512", "ComplEx", 256, True, True, adv=True),
    case("RotatE-w16", "RotatE", 8, True, False, adv=True), case("RotatE-w264", "RotatE", 132, True, False),
    case("SimplE-w16", "SimplE", 16, adv=True), case("SimplE-w260", "SimplE", 260, adv=True),
    case("QuatE-w16", "QuatE", 8, True, True, adv=True), case("QuatE-w260", "QuatE", 130, True, True, adv=True),
    case("PairRE-w16", "PairRE", 16, False, True, adv=True), case("PairRE-w512", "PairRE", 512, False, True, adv=True),
]
OPTION_CASES = [
    case("l2-reg3", "TransE_l2", 16, adv=True, reg_coef=1e-3, reg_norm=3),
    case("l2-reg2", "TransE_l2", 16, adv=True, reg_coef=1e-3, reg_norm=2),
    case("distmult-reg2", "DistMult", 16, adv=True, reg_coef=1e-3, reg_norm=2),
    case("l2-hinge", "TransE_l2", 16, genre="Hinge"),
    case("distmult-softmax", "DistMult", 16, genre=SM.GENRE),
    case("distmult-negdeg", "DistMult", 16, adv=True, neg_deg=True, reg_coef=1e-3),
    case("l2-known", "TransE_l2", 16, adv=True, known=True),
    case("distmult-edge_w", "DistMult", 16, adv=True, edge_w=True),
]
# lists beyond 64 entries and the shared relation list; the shared-list threshold at width 516 (5 entries above 512)
LIST_CASES = [
    case("l2-hub", "TransE_l2", 16, n_ent=4, n_rel=1, B=96, chunk=8, N=8, adv=True, hub=True),
    case("distmult-hub", "DistMult", 16, n_ent=4, n_rel=1, B=96, chunk=8, N=8, adv=True, hub=True),
    case("distmult-w516-rel2", "DistMult", 516, n_rel=2, B=64, adv=True),
]
CASES = WIDTH_CASES + MODEL_CASES + OPTION_CASES + LIST_CASES
# the ambiguity figures of the issue were taken on these
GUARD_SHAPE = [case("guard-%s-%s" % (m, g), m, 16 if m not in ("ComplEx",) else 8, m == "ComplEx" or m == "RotatE", m == "ComplEx",
                    adv=(g == "Logsigmoid"), genre=g, reg_coef=1e-3, gamma=12.0)
               for m in ("TransE_l1", "TransE_l2", "DistMult", "ComplEx", "RotatE") for g in ("Logsigmoid", "Hinge")]


def by_id(cid):
    return [c for c in CASES if c["id"] == cid][0]


def _seed(c):
    return 7700 + 131 * c["seed"] + sum(ord(ch) for ch in c["id"])


def tables(c):
    """float32 tables U(-emb_init, emb_init) (general_models.py:217-218)"""
    d_e, d_r = widths(c)
    s = (c["gamma"] + 2.0) / c["hidden"]
    rng = np.random.RandomState(_seed(c))
    return rng.uniform(-s, s, (c["n_ent"], d_e)).astype(np.float32), rng.uniform(-s, s, (c["n_rel"], d_r)).astype(np.float32)


def _finish(bt, B):
    nid, inv = np.unique(np.concatenate([bt["h"], bt["t"]]), return_inverse=True)
    bt.update(nid=nid.astype(np.int64), h_local=inv[:B].astype(np.int64), t_local=inv[B:].astype(np.int64))
    return bt


def batches(c, steps=STEPS):
    """the batches of steps 1 .. steps: odd steps corrupt tails, even steps heads (oracle.synth_batch).  Every batch has a
    positive-only entity, a negative-only entity and one in both traces (planted: entities n_ent - 3 .. n_ent - 1 of the plain
    cases).  hub: entity 0 heads most edges and fills most negative slots - lists beyond 65 entries."""
    rng = np.random.RandomState(_seed(c) + 1)
    out = []
    n_ent, B, N, chunk = c["n_ent"], c["B"], c["N"], c["chunk"]
    for s in range(1, steps + 1):
        if c["hub"]:
            C = B // chunk
            h = np.where(rng.rand(B) < 0.85, 0, rng.randint(0, n_ent, B)).astype(np.int64)
            t = rng.randint(1, n_ent, B).astype(np.int64)
            neg = np.where(rng.rand(C * N) < 0.8, 0, rng.randint(0, n_ent, C * N)).astype(np.int64)
            bt = dict(h=h, t=t, r=np.zeros(B, np.int64), neg=neg, neg_head=(s % 2 == 0), C=C)
        else:
            bt = O.synth_batch(rng, n_ent - 3, c["n_rel"], B, N, chunk, s)
            bt = {k: bt[k] for k in ("h", "t", "r", "neg", "neg_head", "C")}
            bt["h"][0] = n_ent - 3                                    # positive trace only
            bt["neg"][1] = n_ent - 2                                  # negative trace only
            bt["t"][2] = n_ent - 1
            bt["neg"][3] = n_ent - 1                                  # both traces
            if c["n_rel"] > 1:                                        # relation 0: a long list; the last relation: one entry
                bt["r"][:] = np.where(bt["r"] == c["n_rel"] - 1, 0, bt["r"])
                bt["r"][4] = c["n_rel"] - 1
                bt["r"][5:5 + 14] = 0
        bt["w"] = rng.uniform(0.5, 1.5, B) if c["edge_w"] else None
        out.append(_finish(bt, B))
    return out


def known_pairs(c, bt, share=0.15):
    """[B, N] bool: the pairs a planted known-triple index takes out of a batch's negatives, and the triples that plant them"""
    rng = np.random.RandomState(_seed(c) + 17 + int(bt["neg_head"]))
    B, N, chunk = c["B"], c["N"], c["chunk"]
    want = rng.rand(B, N) < share
    triples = set()
    for i, j in zip(*np.nonzero(want)):
        e = int(bt["neg"][(i // chunk) * N + j])
        triples.add((e, int(bt["r"][i]), int(bt["t"][i])) if bt["neg_head"] else (int(bt["h"][i]), int(bt["r"][i]), e))
    K = np.array(sorted(triples), np.int64).reshape(-1, 3)
    # membership decides: a planted triple also masks every other pair that forms it
    kset = set(map(tuple, K.tolist()))
    mask = np.zeros((B, N), bool)
    for i in range(B):
        for j in range(N):
            e = int(bt["neg"][(i // chunk) * N + j])
            tr = (e, int(bt["r"][i]), int(bt["t"][i])) if bt["neg_head"] else (int(bt["h"][i]), int(bt["r"][i]), e)
            mask[i, j] = tr in kset
    return mask, (K[:, 0].copy(), K[:, 1].copy(), K[:, 2].copy())


def zero_state(c, ent, rel, dtype=np.float64):
    d_e, d_r = widths(c)
    return dict(ent=ent.astype(dtype), rel=rel.astype(dtype), ent_mom=np.zeros((c["n_ent"], 2, d_e), dtype),
                rel_mom=np.zeros((c["n_rel"], 2, d_r), dtype), ent_cnt=np.zeros(c["n_ent"], dtype), rel_cnt=np.zeros(c["n_rel"], dtype))


PRELOAD_CASES = {"TransE_l2-w16": 5, "DistMult-w260": 6}          # case id -> seed of the preloaded state


def preloaded(c, seed):
    """float32 state to start from: counts 0, 1, 1000, 2^24 - 1 and 2^24 over the rows, non-zero moments"""
    d_e, d_r = widths(c)
    rng = np.random.RandomState(seed)
    counts = np.array([0, 1, 1000, 2 ** 24 - 1, 2 ** 24], np.float32)
    pre = {}
    for tab, n, d in (("ent", c["n_ent"], d_e), ("rel", c["n_rel"], d_r)):
        mom = np.empty((n, 2, d), np.float32)
        mom[:, 0] = rng.uniform(-1e-2, 1e-2, (n, d))
        mom[:, 1] = rng.uniform(0, 1e-4, (n, d))
        pre[tab + "_mom"] = mom
        pre[tab + "_state"] = counts[np.arange(n) % len(counts)]
    return pre


def rel_shared_threshold(d_r, d_e):
    """entries from which a relation list is shared by the workgroup (kge_update_body.hpp: 2 * LBR + 1 extra entries -> 13 + 1;
    widths above 512: 5 + 1).  A list of n entries has n - 1 extra ones; the issue counts the list: 13 / 5 extra entries"""
    return 13 if max(d_r, d_e) <= 512 else 5


def row_classes(c, bt):
    """what the update kernel sees of a batch: trace membership of the entities, list lengths"""
    pos, neg = set(bt["nid"].tolist()), set(bt["neg"].tolist())
    ent_pos = np.bincount(np.concatenate([bt["h"], bt["t"]]), minlength=c["n_ent"])
    ent_neg = np.bincount(bt["neg"], minlength=c["n_ent"])
    rel_len = np.bincount(bt["r"], minlength=c["n_rel"])
    return dict(pos_only=len(pos - neg), neg_only=len(neg - pos), both=len(pos & neg), ent_pos_max=int(ent_pos.max()),
                ent_neg_max=int(ent_neg.max()), rel_len=rel_len[rel_len > 0])
