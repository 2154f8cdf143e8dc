"""Float64 statement, case tables and input builders of the TransH score function (include/kge_hip.h, enum kge_model, KGE_TRANSH = 12).
Test infrastructure; a plain module, not a conftest.  Shared by
  tests/test_transh_inputs.py  (CPU): the statement against torch.autograd, its identities, the conditions on the inputs of every
                               case, the integer-grid ranking inputs, the host refusals;
  tests/test_gpu_transh.py     (GPU): the per-op entries, the fused step, exact ranks of every ranking entry, the interface.

The statement (dtype of the inputs; entity rows d_e wide, relation rows 2 d_e wide, r = [d | w]):
    w^ = w / |w|_2,  w^ = 0 where |w|_2 == 0;   x_perp = x - (w^ . x) w^
    s(h, r, t) = gamma - |h_perp + d - t_perp|_2
    per-edge pair: tails corrupted a = h_perp + d;  heads corrupted a = t_perp - d;  both with w^
    chunked score s_ij = gamma - |a_i - n_j + (w^_i . n_j) w^_i|_2                                         (score_neg, the direct form)
    matrix form: p = a_i . n_j, q = w^_i . n_j, alpha_i = |a_i|^2, beta_j = |n_j|^2, c_i = w^_i . a_i, omega_i = |w^_i|^2:
        |.|^2 = alpha_i + beta_j - 2 p + 2 c_i q - (2 - omega_i) q^2                                        (score_neg_matrix)
    backward: E = -(dL/ds) / (2 dist), P' = -2 E, Q' = 2 E (c_i - q_ij), kappa_i = sum_j 2 E_ij q_ij,
        Ga_i = sum_j P'_ij n_j + 2 a_i sum_j E_ij + kappa_i w^_i,  Gw^_i = sum_j Q'_ij n_j + kappa_i a_i,
        Gn_j = sum_i (P'_ij a_i + Q'_ij w^_i) + 2 n_j sum_i E_ij                                            (score_neg_bwd)
    then the adjoints of the projections and of the normalisation, Gw = (Gw^ - (Gw^ . w^) w^) / |w|        (pair_bwd)
The oracle (oracle/kge_oracle.py) has no TransH: `forward_backward` / `step` below restate its train step with these formulas and
its own loss, regulariser and Adagrad functions (the Softmax genre: tests/softmax_loss_cases.py).

Tolerances are the suite's (tests/modular_op_cases.py): scores 1e-4 abs + 1e-4 rel; gradients and updated rows 3e-4 of the
compared array's largest component + 3e-4 relative.

Conditions on the inputs (test_transh_inputs.py checks them on this statement alone, for every case, with nothing excluded):
every float64 distance of every compared pair - the chunked ones and the positive ones - is at least DIST_SHARE of
sqrt(alpha_i + beta_j): the derivative of the norm and the cancellation of the matrix form are then both far from the bounds.
And no gradient row of a step is a cancellation residual (residual_rows): under -pw a sampled negative that IS the edge's own
corrupted entity, alone active in its row, cancels the positive's gradient of the uncorrupted entity exactly; what two different
evaluation routes leave of it (1e-17 in float64, 1e-9 in float32) Adagrad's first step, g / sqrt(mean g^2), scales to lr in any
precision.  Such a row says nothing about the kernels: the batches' seeds are chosen to hold none."""
import contextlib
import functools
import zlib

import numpy as np

import adam_cases as A
import softmax_loss_cases as SM
from pairre_cases import chunked_ranks_of, filter_lists, ranks_of, tie_candidates      # noqa: F401 - model-independent, re-exported
from modular_op_cases import GRAD_RTOL, SCORE_ATOL, SCORE_RTOL, grad_bound, score_bound, worst      # noqa: F401 - re-exported
from oracle import kge_oracle as O

MODEL = "TransH"
MODEL_ID = 12               # include/kge_hip.h KGE_TRANSH
NEG_DEG = 32                # KGE_FLAG_NEG_DEG_SAMPLE
KNOWN_SCORE = -1.0e6        # KGE_KNOWN_SCORE
DIST_SHARE = 0.05
GAMMA = 4.0


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


# --------------------------------------------------------------------------------------------------------------------------
# the statement
# --------------------------------------------------------------------------------------------------------------------------
def halves(r):
    d = r.shape[-1] // 2
    return r[..., :d], r[..., d:]


def norm(x):
    return np.sqrt((x * x).sum(-1, keepdims=True))


def unit(x):
    n = norm(x)
    return np.where(n > 0, x / np.where(n > 0, n, 1), 0)


def unit_bwd(x, g):
    """dL/dx from g = dL/dx^: (g - x^ <x^, g>) / |x|, 0 where |x| == 0"""
    n = norm(x)
    xu = unit(x)
    return np.where(n > 0, (g - xu * (xu * g).sum(-1, keepdims=True)) / np.where(n > 0, n, 1), 0)


def dot(x, y):
    return (x * y).sum(-1, keepdims=True)


def proj(x, wu):
    return x - dot(wu, x) * wu


def proj_bwd(x, wu, g):
    """(dL/dx, dL/dw^) from g = dL/dx_perp"""
    return proj(g, wu), -dot(wu, x) * g - dot(wu, g) * x


def score(h, r, t, gamma=GAMMA):
    d, w = halves(r)
    wu = unit(w)
    return gamma - norm(proj(h, wu) + d - proj(t, wu))[..., 0]


def score_bwd(h, r, t, dp):
    """(gh, gr, gt) of sum_i dp_i s(h_i, r_i, t_i); no gradient where the distance is 0"""
    d, w = halves(r)
    wu = unit(w)
    u = proj(h, wu) + d - proj(t, wu)
    n = norm(u)
    gu = np.where(n > 0, -dp[:, None] * u / np.where(n > 0, n, 1), 0)
    gx, gwu = proj_bwd(h - t, wu, gu)
    return gx, np.concatenate([gu, unit_bwd(w, gwu)], -1), -gx


def pair(neg_head, x, r):
    """(a, w^) of the edges whose uncorrupted entity rows are x"""
    d, w = halves(r)
    wu = unit(w)
    return (proj(x, wu) - d if neg_head else proj(x, wu) + d), wu


def pair_bwd(neg_head, x, r, ga, gwu):
    """(dL/dx, dL/dr) from (Ga, Gw^)"""
    d, w = halves(r)
    wu = unit(w)
    gx, g2 = proj_bwd(x, wu, ga)
    return gx, np.concatenate([-ga if neg_head else ga, unit_bwd(w, gwu + g2)], -1)


def _blocks(a, wu, neg, C, chunk, N):
    return a.reshape(C, chunk, 1, -1), wu.reshape(C, chunk, 1, -1), neg.reshape(C, 1, N, -1)


def dist_neg(a, wu, neg, C, chunk, N):
    """[C, chunk, N] distances |a_i - n_j + (w^_i . n_j) w^_i|, the direct form"""
    A_, W_, N_ = _blocks(a, wu, neg, C, chunk, N)
    q = (W_ * N_).sum(-1, keepdims=True)
    return norm(A_ - N_ + q * W_)[..., 0]


def score_neg(a, wu, neg, C, chunk, N, gamma=GAMMA):
    return gamma - dist_neg(a, wu, neg, C, chunk, N)


def matrix_terms(a, wu, neg, C, chunk, N):
    """p, q [C, chunk, N]; alpha, c, omega [C, chunk, 1]; beta [C, 1, N]"""
    A_, W_, N_ = _blocks(a, wu, neg, C, chunk, N)
    return ((A_ * N_).sum(-1), (W_ * N_).sum(-1), (A_ * A_).sum(-1), (N_ * N_).sum(-1), (W_ * A_).sum(-1), (W_ * W_).sum(-1))


def dist2_matrix(a, wu, neg, C, chunk, N):
    p, q, al, be, c, om = matrix_terms(a, wu, neg, C, chunk, N)
    return al + be - 2 * p + 2 * c * q - (2 - om) * q * q


def score_neg_matrix(a, wu, neg, C, chunk, N, gamma=GAMMA):
    return gamma - np.sqrt(np.maximum(dist2_matrix(a, wu, neg, C, chunk, N), 0))


def score_neg_bwd(a, wu, neg, G, C, chunk, N):
    """(Ga, Gw^, Gn) by the formulas of the header, omega treated as a constant"""
    A_, W_, N_ = _blocks(a, wu, neg, C, chunk, N)
    p, q, al, be, c, om = matrix_terms(a, wu, neg, C, chunk, N)
    dist = dist_neg(a, wu, neg, C, chunk, N)
    E = np.where(dist > 0, -G.reshape(C, chunk, N) / (2 * np.where(dist > 0, dist, 1)), 0)
    P = -2 * E
    Qc = 2 * E * (c - q)
    kap = (2 * E * q).sum(2, keepdims=True)
    ga = (P[..., None] * N_).sum(2) + 2 * A_[:, :, 0] * E.sum(2, keepdims=True) + kap * W_[:, :, 0]
    gw = (Qc[..., None] * N_).sum(2) + kap * A_[:, :, 0]
    gn = (P[..., None] * A_ + Qc[..., None] * W_).sum(1) + 2 * N_[:, 0] * E.sum(1)[..., None]
    return ga.reshape(a.shape), gw.reshape(a.shape), gn.reshape(neg.shape)


def dist_shares(a, wu, neg, C, chunk, N):
    """[C, chunk, N]: dist_ij / sqrt(alpha_i + beta_j) (1 where both norms are 0)"""
    _, _, al, be, _, _ = matrix_terms(a, wu, neg, C, chunk, N)
    s = np.sqrt(al + be)
    return np.where(s > 0, dist_neg(a, wu, neg, C, chunk, N) / np.where(s > 0, s, 1), 1.0)


def pos_shares(h, r, t):
    """[B]: the same share for the positive triples (the chunked form with n = t)"""
    a, wu = pair(False, h, r)
    return np.stack([dist_shares(a[i:i + 1], wu[i:i + 1], t[i:i + 1], 1, 1, 1)[0, 0, 0] for i in range(len(h))])


def residual_rows(out, floor=1e-6):
    """rows of the three gradient traces that are neither exactly zero nor at least `floor` of their array's largest component"""
    bad = 0
    for k in ("g_pos_ent", "g_neg", "g_rel"):
        m = np.abs(out[k]).max(1)
        bad += int(((m > 0) & (m < floor * m.max())).sum())
    return bad


def loss_fwd_bwd(c, p, n, w):
    if c["genre"] == SM.GENRE:
        return SM.softmax_fwd_bwd(p, n, w)
    return O.loss_fwd_bwd(p, n, w, c["genre"], c["adv"], c["adv_temp"], c["pairwise"], c["margin"])


def forward_backward(c, ent, rel, bt, known=None):
    """oracle.kge_oracle.forward_backward with the TransH formulas, in the dtype of the tables.  known: [B, N] bool, the pairs that
    take KGE_KNOWN_SCORE (tests/known_negative_cases.py masked_forward_backward).  `share`: the smallest distance share of the step."""
    dt = ent.dtype
    chunk, N, neg_head = c["chunk"], c["N"], bt["neg_head"]
    gamma = c.get("gamma", GAMMA)
    B = len(bt["h"])
    C = B // chunk
    pos_emb, r, neg = ent[bt["nid"]], rel[bt["r"]], ent[bt["neg"]]
    h, t = pos_emb[bt["h_local"]], pos_emb[bt["t_local"]]
    w = None if bt.get("w") is None else bt["w"].astype(dt)
    p = score(h, r, t, gamma)
    x = t if neg_head else h
    a, wu = pair(neg_head, x, r)
    nd = c["neg_deg"]
    if nd:          # the chunk's own corrupted-side entities in front, the positive edge's own column at score 0 (general_models.py:396-432)
        Np = chunk + N
        y = (h if neg_head else t).reshape(C, chunk, -1)
        neg_all = np.concatenate([y, neg.reshape(C, N, -1)], 1).reshape(C * Np, -1)
        mask = np.ones((C, chunk, Np), dt)
        mask[:, np.arange(chunk), np.arange(chunk)] = 0
        n = score_neg(a, wu, neg_all, C, chunk, Np, gamma) * mask
    else:
        Np, neg_all, mask = N, neg, 1
        n = score_neg(a, wu, neg, C, chunk, N, gamma)
    if known is not None:
        n = np.where(known.reshape(n.shape), dt.type(KNOWN_SCORE), n)
    (pl, nl, loss), dpos, dneg = loss_fwd_bwd(c, p, n.reshape(B, Np), w)
    dneg = dneg.reshape(C, chunk, Np) * mask
    if known is not None:
        dneg = np.where(known.reshape(dneg.shape), 0, dneg)
    use_reg = c["reg_coef"] > 0.0 and c["reg_norm"] > 0
    reg = O.reg_value([pos_emb, neg], c["reg_coef"], c["reg_norm"]) + O.reg_value([r], c["reg_coef"], c["reg_norm"]) if use_reg else 0.0
    gh, gr, gt = score_bwd(h, r, t, dpos)
    ga, gw, g_all = score_neg_bwd(a, wu, neg_all, dneg, C, chunk, Np)
    g_all = g_all.reshape(C, Np, -1)
    g_neg = g_all[:, Np - N:].reshape(C * N, -1)
    gx, gr2 = pair_bwd(neg_head, x, r, ga, gw)
    gr = gr + gr2
    if neg_head:
        gt = gt + gx
    else:
        gh = gh + gx
    if nd:
        g_inb = g_all[:, :chunk].reshape(B, -1)
        if neg_head:
            gh = gh + g_inb
        else:
            gt = gt + g_inb
    g_pos = np.zeros_like(pos_emb)
    np.add.at(g_pos, bt["h_local"], gh)
    np.add.at(g_pos, bt["t_local"], gt)
    if use_reg:
        g_pos = g_pos + O.reg_grad(pos_emb, c["reg_coef"], c["reg_norm"])
        g_neg = g_neg + O.reg_grad(neg, c["reg_coef"], c["reg_norm"])
        gr = gr + O.reg_grad(r, c["reg_coef"], c["reg_norm"])
    sh = dist_shares(a, wu, neg_all, C, chunk, Np)
    if nd:          # (the masked own columns are not compared pairs)
        sh = np.where(mask > 0, sh, 1.0)
    share = float(min(sh.min(), pos_shares(h, r, t).min()))
    return dict(pos_score=p, neg_score=n, log=(pl, nl, loss, reg), g_pos_ent=g_pos.astype(dt), g_rel=gr.astype(dt),
                g_neg=g_neg.astype(dt), share=share)


def step(c, ent, es, rel, rs, bt, known=None):
    """forward + backward + the reference's update order (entity trace 0, entity trace 1, relation trace), tables in place"""
    out = forward_backward(c, ent, rel, bt, known)
    O.adagrad_update(ent, es, bt["nid"], out["g_pos_ent"], c["lr"])
    O.adagrad_update(ent, es, bt["neg"], out["g_neg"], c["lr"])
    O.adagrad_update(rel, rs, bt["r"], out["g_rel"], c["lr"])
    return out


# --------------------------------------------------------------------------------------------------------------------------
# 1. the per-op entries.  Widths: 4 and 8 (below one k-stage of any tile), 36 (a partial k-stage), 64, 260.  Shapes: partial 16-row /
#    16-column tiles of the forward product on each edge and none, and (1, 12, 20): 12 rows stay inside one 16-row tile of the forward
#    product, one 16-row tile of the backward's Ga | Gw^ product and one 16-value macro step of its Gn product; the STACKED 24 rows
#    cross all three, and the w^ rows start inside a tile
# --------------------------------------------------------------------------------------------------------------------------
OP_WIDTHS = (4, 8, 36, 64, 260)
OP_SHAPES = ((2, 5, 33), (2, 33, 5), (1, 32, 32), (1, 12, 20))           # (C, chunk, N)
OP_SEEDS = {}               # seed per (d_e, shape index, neg_head), chosen so that the distance condition holds; 0 unless listed


def op_inputs(d_e, C, chunk, N, neg_head):
    """float32 x [B, d_e] (the uncorrupted side), y [B, d_e] (the other entity of the positive), r [B, 2 d_e], nb [C * N, d_e],
    W [C, chunk, N] and dp [B] (random signed upstream gradients).  The normal of r[1] and the rows x[2] and nb[3] are all zero."""
    si = OP_SHAPES.index((C, chunk, N))
    rng = np.random.RandomState(_seed("transh-op", d_e, C, chunk, N, bool(neg_head), OP_SEEDS.get((d_e, si, bool(neg_head)), 0)))
    B = C * chunk
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    inp = dict(x=u(B, d_e), y=u(B, d_e), r=u(B, 2 * d_e), nb=u(C * N, d_e), W=u(C, chunk, N), dp=u(B))
    inp["r"][1, d_e:] = 0.0
    inp["x"][2] = 0.0
    inp["nb"][3] = 0.0
    return inp


def op_reference(inp, C, chunk, N, neg_head, dtype=np.float64):
    """the outputs of the four per-op entries and the smallest distance share of the compared pairs"""
    x, y, r, nb, W, dp = (inp[k].astype(dtype) for k in ("x", "y", "r", "nb", "W", "dp"))
    h, t = (y, x) if neg_head else (x, y)
    a, wu = pair(neg_head, x, r)
    ga, gw, gn = score_neg_bwd(a, wu, nb, W, C, chunk, N)
    gx, gr = pair_bwd(neg_head, x, r, ga, gw)
    gh, grp, gt = score_bwd(h, r, t, dp)
    share = float(min(dist_shares(a, wu, nb, C, chunk, N).min(), pos_shares(h, r, t).min()))
    return dict(pos=score(h, r, t), gh=gh, grp=grp, gt=gt, score=score_neg(a, wu, nb, C, chunk, N), gx=gx, gr=gr, gn=gn, share=share)


OP_GRADS = ("gh", "grp", "gt", "gx", "gr", "gn")


# --------------------------------------------------------------------------------------------------------------------------
# 2. the fused step: the shapes and the option table of tests/pairre_cases.py
# --------------------------------------------------------------------------------------------------------------------------
STEP_B, STEP_CHUNK, STEP_N, STEP_ENT, STEP_REL = 16, 8, 24, 40, 5
STEP_WIDTHS = (32, 36)
# seeds of the batches, per case: chosen so that the conditions hold (0 unless listed).  hinge-pw: seeds 0, 3 and 5 hold 4, 2 and 3
# residual rows (a negative equal to the edge's own tail / head, alone active)
STEP_SEEDS = {"hinge-pw": 1}
ZERO_W_RELS = (1, 3)        # step_tables(zero_w=True): the relations whose normal is exactly zero


def _step_cases():
    import pairre_cases as PR
    return [dict(c) for c in PR.STEP_CASES]


STEP_CASES = _step_cases()


def step_tables(d_e, zero_w=False):
    rng = np.random.RandomState(_seed("transh-step-tables", d_e))
    ent, rel = rng.uniform(-1, 1, (STEP_ENT, d_e)).astype(np.float32), rng.uniform(-1, 1, (STEP_REL, 2 * d_e)).astype(np.float32)
    if zero_w:
        rel[list(ZERO_W_RELS), d_e:] = 0.0
    return ent, rel


def step_batches(c, steps=2):
    """tail then head corruption (oracle.kge_oracle.synth_batch); w: edge importance or None"""
    rng = np.random.RandomState(_seed("transh-step-batch", c["id"], STEP_SEEDS.get(c["id"], 0)))
    out = []
    for s in range(1, steps + 1):
        bt = O.synth_batch(rng, c["n_ent"], c["n_rel"], c["B"], c["N"], c["chunk"], s)
        bt["w"] = rng.uniform(0.5, 1.5, c["B"]).astype(np.float32) if c["impts"] else None
        out.append(bt)
    return out


def planted_known(bt, chunk, N):
    import pairre_cases as PR
    return PR.planted_known(bt, chunk, N)


# the Adam case: adam_cases.step with this statement's gradients
ADAM_CASE = A.case("TransH-w16", "TransH", 16, False, True, adv=True)


@contextlib.contextmanager
def adam_gradients():
    """adam_cases.step / .gradients know the oracle's models, QuatE and PairRE: inside this block they take TransH from here"""
    saved = A.gradients

    def gradients(c, ent, rel, bt, known=None):
        return forward_backward(c, ent, rel, bt, known) if c["model"] == MODEL else saved(c, ent, rel, bt, known)
    A.gradients = gradients
    try:
        yield
    finally:
        A.gradients = saved


# --------------------------------------------------------------------------------------------------------------------------
# 3. exact ranks: integer-grid tables.  Every normal has exactly four entries +-1, so |w| = 2 and w^ is in {0, +-1/2}: exact.
#    Translations and entity entries are integers in -2 .. 2 and gamma is an integer: w^ . x is a multiple of 1/2, projections are
#    multiples of 1/4 and every squared distance - in the direct and in the matrix form, in any summation order - a small multiple
#    of 1/16, exact in float32; sqrtf is correctly rounded, so equal squares give equal scores and distinct ones (they differ by
#    >= 1/16 at a magnitude of a few hundred: far more than one float32 step of the root) distinct scores: ties are real ties.
# --------------------------------------------------------------------------------------------------------------------------
TIE_CASES = [(7, 8), (130, 8), (130, 32)]            # (entities = relations = candidates, d_e), as pairre_cases.TIE_CASES
TIE_E = 40                      # test triples
TIE_CHUNK = 16                  # chunked_ranks: two chunks of 16 and one of 8
# several tiles, as pairre_cases.TIE_WIDE_CASES: 150 test triples are also three of rank_gemm_transh_kernel's 64-query tiles
# (RANK_TH_BM), the last of 22.  Four entries +-1 keep |w| = 2 at any width: both widths stay exact
TIE_WIDE_CASES = [(300, 32), (300, 36)]
TIE_WIDE_E = 150
TIE_WIDE_CHUNK = 100
TIE_GAMMA = 6.0


class Case(object):
    pass


def tie_scores(c, h, r, t, neg_head, dtype=np.float64):
    """(p [E], S [E, n_ent]) in `dtype`: the positive scores and the scores of every entity in the corrupted slot"""
    ent, rel = c.ent.astype(dtype), c.rel.astype(dtype)
    g = dtype(TIE_GAMMA)
    a, wu = pair(neg_head, ent[t if neg_head else h], rel[r])
    return score(ent[h], rel[r], ent[t], g), score_neg(a, wu, ent, 1, len(h), len(ent), g)[0]


@functools.lru_cache(maxsize=None)
def tie_inputs(n, d_e, E=None):
    """tables, E (default: TIE_E, read at the call) test triples and known triples: the test triples and, for the first 12 of them
    and both sides, one planted triple whose corrupted entity TIES the positive where there is one.  Entity entries are sparse
    (most are 0) so that few distinct distances are shared by many candidates."""
    E = TIE_E if E is None else E
    rng = np.random.RandomState(_seed("transh-tie", n, d_e))
    c = Case()
    c.n, c.d_e = n, d_e
    c.ent = np.zeros((n, d_e), np.float32)
    for i in range(n):
        c.ent[i, rng.choice(d_e, 3, replace=False)] = rng.choice([-2.0, -1.0, 1.0, 2.0], 3)
    c.rel = np.zeros((n, 2 * d_e), np.float32)
    for i in range(n):
        c.rel[i, rng.choice(d_e, 2, replace=False)] = rng.choice([-1.0, 1.0], 2)
        c.rel[i, d_e + rng.choice(d_e, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    c.rel[0, d_e:] = 0.0                                  # one relation without a hyperplane
    c.h, c.r, c.t = rng.randint(0, n, E), rng.randint(0, n, E), rng.randint(0, n, E)
    c.r[0] = 0
    extra = []
    for side in ("tail", "head"):
        p, S = tie_scores(c, c.h, c.r, c.t, side == "head")
        own = c.h if side == "head" else c.t
        for i in range(12):
            cols = np.nonzero((S[i] == p[i]) & (np.arange(S.shape[1]) != own[i]))[0]
            if len(cols):
                e = int(cols[len(cols) // 2])
                extra.append((c.h[i], c.r[i], e) if side == "tail" else (e, c.r[i], c.t[i]))
    extra = np.array(extra, np.int64).reshape(-1, 3)
    c.kh, c.kr, c.kt = (np.concatenate([x, extra[:, k]]) for k, x in enumerate((c.h, c.r, c.t)))
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def f32_scores_two_forms(c, h, r, t, neg_head):
    """the [E, n] scores evaluated in float32 in the direct form and in the matrix form with the sums over k running backward"""
    ent, rel = c.ent, c.rel
    a, wu = pair(neg_head, ent[t if neg_head else h], rel[r])
    assert a.dtype == np.float32 and wu.dtype == np.float32
    E, n = len(h), len(ent)
    s1 = score_neg(a, wu, ent, 1, E, n, np.float32(TIE_GAMMA))[0]
    p, q = np.zeros((E, n), np.float32), np.zeros((E, n), np.float32)
    al, be, cc = np.zeros((E, 1), np.float32), np.zeros((1, n), np.float32), np.zeros((E, 1), np.float32)
    for k in range(c.d_e - 1, -1, -1):
        p += a[:, k:k + 1] * ent[None, :, k]
        q += wu[:, k:k + 1] * ent[None, :, k]
        al += a[:, k:k + 1] ** 2
        be += ent[None, :, k] ** 2
        cc += wu[:, k:k + 1] * a[:, k:k + 1]
    d2 = (al + be - np.float32(2) * p) + q * (np.float32(2) * cc - q)
    assert d2.dtype == np.float32 and s1.dtype == np.float32
    return s1, np.float32(TIE_GAMMA) - np.sqrt(np.maximum(d2, np.float32(0)))


# --------------------------------------------------------------------------------------------------------------------------
# 4. the interface: 40 entities, 6 relations, 16 wide
# --------------------------------------------------------------------------------------------------------------------------
IF_ENT, IF_REL, IF_D, IF_K = 40, 6, 16, 5
IF_GAMMA = 3.0


def interface_tables():
    rng = np.random.RandomState(_seed("transh-interface"))
    return rng.uniform(-1, 1, (IF_ENT, IF_D)).astype(np.float32), rng.uniform(-1, 1, (IF_REL, 2 * IF_D)).astype(np.float32)


def all_scores(ent, rel, gamma=IF_GAMMA):
    """[n_ent, n_rel, n_ent] float64 scores of every triple"""
    e, r = ent.astype(np.float64), rel.astype(np.float64)
    out = np.zeros((len(e), len(r), len(e)))
    for k in range(len(r)):
        rr = np.repeat(r[k:k + 1], len(e), 0)
        a, wu = pair(False, e, rr)
        out[:, k, :] = score_neg(a, wu, e, 1, len(e), len(e), gamma)[0]
    return out
