"""Float64 statement, case tables and input builders of the TransD score function (include/kge_hip.h, enum kge_model, KGE_TRANSD = 14).
Test infrastructure; a plain module, not a conftest.  Shared by
  tests/test_transd_inputs.py         (CPU): the statement against torch.autograd, its identities, the conditions on the inputs of
                                      every case, the integer-grid ranking inputs, the host refusals;
  tests/test_gpu_transd.py            (GPU): the per-op entries, the fused step, exact ranks of every ranking entry, the interface;
  tests/test_gpu_transd_contracts.py  (GPU): the workspace and stream contracts of the entries the model runs through.

The statement (dtype of the inputs; entity rows [e | e_p] and relation rows [r | r_p], both 2 k wide):
    x_perp = x + (x_p . x) r_p                                                  (M_rx = r_p x_p^T + I, equal widths)
    s(h, r, t) = gamma - |h_perp + r - t_perp|_2
    per-edge pair (a, rho), rho = r_p: tails corrupted a = h_perp + r;  heads corrupted a = t_perp - r
    per candidate row [n | m]: c = m . n
    chunked score s_ij = gamma - |a_i - n_j - c_j rho_i|_2                                                  (score_neg, the direct form)
    matrix form: p = a_i . n_j, q = rho_i . n_j, alpha_i = |a_i|^2, beta_j = |n_j|^2, sigma_i = |rho_i|^2, u_i = a_i . rho_i:
        |.|^2 = alpha_i + beta_j + c_j^2 sigma_i - 2 p + 2 c_j (q - u_i)                                    (score_neg_matrix)
    backward: E = -(dL/ds) / (2 dist), P' = -2 E, Q'_ij = 2 E_ij c_j,
        Ga_i = sum_j P'_ij n_j + 2 a_i sum_j E_ij - 2 rho_i sum_j E_ij c_j
        Grho_i = sum_j Q'_ij n_j + 2 rho_i sum_j E_ij c_j^2 - 2 a_i sum_j E_ij c_j
        Gc_j = sum_i E_ij (2 c_j sigma_i - 2 u_i + 2 q_ij)
        Gn_j = sum_i (P'_ij a_i + Q'_ij rho_i) + 2 n_j sum_i E_ij + Gc_j m_j,   Gm_j = Gc_j n_j              (score_neg_bwd)
    then the adjoint of a projection: Gx = Gx_perp + (Gx_perp . r_p) x_p, Gx_p = (Gx_perp . r_p) x, Gr_p += (x_p . x) Gx_perp,
    and Gr = +-Ga                                                                                           (proj_bwd, pair_bwd)
The oracle (oracle/kge_oracle.py) has no TransD: `forward_backward` / `step` below restate its train step with these formulas and
its own loss, regulariser and Adagrad functions (the Softmax genre: tests/softmax_loss_cases.py; Adam: tests/adam_cases.py).

Tolerances are the suite's (tests/modular_op_cases.py): scores 1e-4 abs + 1e-4 rel; gradients and updated rows 3e-4 of the
compared array's largest component + 3e-4 relative.

Conditions on the inputs (test_transd_inputs.py checks them on this statement alone, for every case, with nothing excluded):
every float64 distance of every compared pair - the chunked ones and the positive ones - is at least DIST_SHARE of
sqrt(alpha_i + beta_j + c_j^2 sigma_i), the size of the terms the matrix form cancels; no gradient row of a step is a cancellation
residual (transh_cases.residual_rows); and |c_j| stays of order 1 (C_MAX): the rows of a half-width k are drawn
from uniform(-1, 1) * row_scale(k), which keeps the standard deviation of c = m . n at 2/3 for every k."""
import contextlib
import functools
import zlib

import numpy as np

import adam_cases as A
import softmax_loss_cases as SM
from pairre_cases import chunked_ranks_of, filter_lists, ranks_of, tie_candidates      # noqa: F401 - model-independent, re-exported
from modular_op_cases import GB_MAXK, GRAD_RTOL, SCORE_ATOL, SCORE_RTOL, grad_bound, score_bound, worst      # noqa: F401 - re-exported
from transh_cases import residual_rows                                                  # noqa: F401 - model-independent, re-exported
from oracle import kge_oracle as O

MODEL = "TransD"
MODEL_ID = 14               # include/kge_hip.h KGE_TRANSD
NEG_DEG = 32                # KGE_FLAG_NEG_DEG_SAMPLE
KNOWN_SCORE = -1.0e6        # KGE_KNOWN_SCORE
DIST_SHARE = 0.05           # TransH's value
C_MAX = 4.0                 # |c_j| = |m_j . n_j| of every case table stays below this
GAMMA = 4.0
# the tile constants the shapes of tests/new_model_shape_cases.py are chosen against, read from kge_transd.hip (transd_coef_kernel:
# a column-sum workgroup takes TD_CT columns of one chunk, its rows split over TD_CR row groups); GB_MAXK (modular_op_cases, read
# from kge_neg_gemm.hip): beyond it own_bwd_products (kge_own_fwd.hpp) leaves the backward GEMM tiles - max(2 chunk, N) counts here,
# the operand being stacked
TD_CT = 32
TD_CR = 8


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def row_scale(k):
    """the factor on uniform(-1, 1) entries of a half-width k: c = m . n is a sum of k products of variance scale^4 / 9, so
    scale = (4 / k)^(1/4) keeps its standard deviation at 2/3 for every k (1 at k = 4)"""
    return float((4.0 / k) ** 0.25)


# --------------------------------------------------------------------------------------------------------------------------
# the statement
# --------------------------------------------------------------------------------------------------------------------------
def halves(x):
    k = x.shape[-1] // 2
    return x[..., :k], x[..., k:]


def norm(x):
    return np.sqrt((x * x).sum(-1, keepdims=True))


def dot(x, y):
    return (x * y).sum(-1, keepdims=True)


def proj(xrow, rp):
    """x_perp [.., k] of rows [x | x_p] under the relation's mapping vector r_p"""
    x, xp = halves(xrow)
    return x + dot(xp, x) * rp


def proj_bwd(xrow, rp, g):
    """(dL/d[x | x_p], dL/dr_p) from g = dL/dx_perp"""
    x, xp = halves(xrow)
    s = dot(g, rp)
    return np.concatenate([g + s * xp, s * x], -1), dot(xp, x) * g


def score(h, r, t, gamma=GAMMA):
    rv, rp = halves(r)
    return gamma - norm(proj(h, rp) + rv - proj(t, rp))[..., 0]


def score_bwd(h, r, t, dp):
    """(gh, gr, gt) of sum_i dp_i s(h_i, r_i, t_i); no gradient where the distance is 0"""
    rv, rp = halves(r)
    e = proj(h, rp) + rv - proj(t, rp)
    n = norm(e)
    ge = np.where(n > 0, -dp[:, None] * e / np.where(n > 0, n, 1), 0)
    gh, gp1 = proj_bwd(h, rp, ge)
    gt, gp2 = proj_bwd(t, rp, -ge)
    return gh, np.concatenate([ge, gp1 + gp2], -1), gt


def pair(neg_head, x, r):
    """(a, rho) of the edges whose uncorrupted entity rows are x"""
    rv, rp = halves(r)
    return (proj(x, rp) - rv if neg_head else proj(x, rp) + rv), rp


def pair_bwd(neg_head, x, r, ga, grho):
    """(dL/dx, dL/dr) from (Ga, Grho)"""
    rv, rp = halves(r)
    gx, g2 = proj_bwd(x, rp, ga)
    return gx, np.concatenate([-ga if neg_head else ga, grho + g2], -1)


def _blocks(a, rho, neg, C, chunk, N):
    """a, rho [C, chunk, 1, k]; n, m [C, 1, N, k]; c [C, 1, N]"""
    n, m = halves(neg)
    k = a.shape[-1]
    return (a.reshape(C, chunk, 1, k), rho.reshape(C, chunk, 1, k), n.reshape(C, 1, N, k), m.reshape(C, 1, N, k),
            (n * m).sum(-1).reshape(C, 1, N))


def dist_neg(a, rho, neg, C, chunk, N):
    """[C, chunk, N] distances |a_i - n_j - c_j rho_i|, the direct form"""
    A_, R_, N_, _, c = _blocks(a, rho, neg, C, chunk, N)
    return norm(A_ - N_ - c[..., None] * R_)[..., 0]


def score_neg(a, rho, neg, C, chunk, N, gamma=GAMMA):
    return gamma - dist_neg(a, rho, neg, C, chunk, N)


def matrix_terms(a, rho, neg, C, chunk, N):
    """p, q [C, chunk, N]; alpha, sigma, u [C, chunk, 1]; beta, c [C, 1, N]"""
    A_, R_, N_, _, c = _blocks(a, rho, neg, C, chunk, N)
    return ((A_ * N_).sum(-1), (R_ * N_).sum(-1), (A_ * A_).sum(-1), (R_ * R_).sum(-1), (A_ * R_).sum(-1), (N_ * N_).sum(-1), c)


def dist2_matrix(a, rho, neg, C, chunk, N):
    p, q, al, sg, u, be, c = matrix_terms(a, rho, neg, C, chunk, N)
    return al + be + c * c * sg - 2 * p + 2 * c * (q - u)


def score_neg_matrix(a, rho, neg, C, chunk, N, gamma=GAMMA):
    return gamma - np.sqrt(np.maximum(dist2_matrix(a, rho, neg, C, chunk, N), 0))


def score_neg_bwd(a, rho, neg, G, C, chunk, N):
    """(Ga, Grho, G[n | m]) by the formulas of the header"""
    A_, R_, N_, M_, c = _blocks(a, rho, neg, C, chunk, N)
    p, q, al, sg, u, be, _ = matrix_terms(a, rho, neg, C, chunk, N)
    dist = dist_neg(a, rho, neg, C, chunk, N)
    E = np.where(dist > 0, -G.reshape(C, chunk, N) / (2 * np.where(dist > 0, dist, 1)), 0)
    P = -2 * E
    Qc = 2 * E * c
    sE, sEc, sEc2 = E.sum(2, keepdims=True), (E * c).sum(2, keepdims=True), (E * c * c).sum(2, keepdims=True)
    ga = (P[..., None] * N_).sum(2) + 2 * A_[:, :, 0] * sE - 2 * R_[:, :, 0] * sEc
    grho = (Qc[..., None] * N_).sum(2) + 2 * R_[:, :, 0] * sEc2 - 2 * A_[:, :, 0] * sEc
    gc = (E * (2 * c * sg - 2 * u + 2 * q)).sum(1)[..., None]                       # [C, N, 1]
    gn = (P[..., None] * A_ + Qc[..., None] * R_).sum(1) + 2 * N_[:, 0] * E.sum(1)[..., None] + gc * M_[:, 0]
    gm = gc * N_[:, 0]
    return ga.reshape(a.shape), grho.reshape(a.shape), np.concatenate([gn, gm], -1).reshape(neg.shape)


def dist_shares(a, rho, neg, C, chunk, N):
    """[C, chunk, N]: dist_ij / sqrt(alpha_i + beta_j + c_j^2 sigma_i) (1 where all three are 0)"""
    _, _, al, sg, _, be, c = matrix_terms(a, rho, neg, C, chunk, N)
    s = np.sqrt(al + be + c * c * sg)
    return np.where(s > 0, dist_neg(a, rho, neg, C, chunk, N) / np.where(s > 0, s, 1), 1.0)


def pos_shares(h, r, t):
    """[B]: the same share for the positive triples (the chunked form with the candidate = t)"""
    a, rho = pair(False, h, r)
    return np.stack([dist_shares(a[i:i + 1], rho[i:i + 1], t[i:i + 1], 1, 1, 1)[0, 0, 0] for i in range(len(h))])


def c_of(rows):
    """[n] c_j = m_j . n_j of rows [n | m]"""
    n, m = halves(rows)
    return (n * m).sum(-1)


def loss_fwd_bwd(c, p, n, w):
    if c["genre"] == SM.GENRE:
        return SM.softmax_fwd_bwd(p, n, w)
    return O.loss_fwd_bwd(p, n, w, c["genre"], c["adv"], c["adv_temp"], c["pairwise"], c["margin"])


def forward_backward(c, ent, rel, bt, known=None):
    """oracle.kge_oracle.forward_backward with the TransD formulas, in the dtype of the tables.  known: [B, N] bool, the pairs that
    take KGE_KNOWN_SCORE (tests/known_negative_cases.py masked_forward_backward).  `share`: the smallest distance share of the step,
    `cmax`: the largest |c_j| of its candidate rows."""
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
    a, rho = pair(neg_head, x, r)
    nd = c["neg_deg"]
    if nd:          # the chunk's own corrupted-side entities in front, the positive edge's own column at score 0 (general_models.py:396-432)
        Np = chunk + N
        y = (h if neg_head else t).reshape(C, chunk, -1)
        neg_all = np.concatenate([y, neg.reshape(C, N, -1)], 1).reshape(C * Np, -1)
        mask = np.ones((C, chunk, Np), dt)
        mask[:, np.arange(chunk), np.arange(chunk)] = 0
        n = score_neg(a, rho, neg_all, C, chunk, Np, gamma) * mask
    else:
        Np, neg_all, mask = N, neg, 1
        n = score_neg(a, rho, neg, C, chunk, N, gamma)
    if known is not None:
        n = np.where(known.reshape(n.shape), dt.type(KNOWN_SCORE), n)
    (pl, nl, loss), dpos, dneg = loss_fwd_bwd(c, p, n.reshape(B, Np), w)
    dneg = dneg.reshape(C, chunk, Np) * mask
    if known is not None:
        dneg = np.where(known.reshape(dneg.shape), 0, dneg)
    use_reg = c["reg_coef"] > 0.0 and c["reg_norm"] > 0
    reg = O.reg_value([pos_emb, neg], c["reg_coef"], c["reg_norm"]) + O.reg_value([r], c["reg_coef"], c["reg_norm"]) if use_reg else 0.0
    gh, gr, gt = score_bwd(h, r, t, dpos)
    ga, grho, g_all = score_neg_bwd(a, rho, neg_all, dneg, C, chunk, Np)
    g_all = g_all.reshape(C, Np, -1)
    g_neg = g_all[:, Np - N:].reshape(C * N, -1)
    gx, gr2 = pair_bwd(neg_head, x, r, ga, grho)
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
    sh = dist_shares(a, rho, neg_all, C, chunk, Np)
    if nd:          # (the masked own columns are not compared pairs)
        sh = np.where(mask > 0, sh, 1.0)
    share = float(min(sh.min(), pos_shares(h, r, t).min()))
    return dict(pos_score=p, neg_score=n, log=(pl, nl, loss, reg), g_pos_ent=g_pos.astype(dt), g_rel=gr.astype(dt),
                g_neg=g_neg.astype(dt), share=share, cmax=float(np.abs(c_of(neg_all)).max()))


def step(c, ent, es, rel, rs, bt, known=None):
    """forward + backward + the reference's update order (entity trace 0, entity trace 1, relation trace), tables in place"""
    out = forward_backward(c, ent, rel, bt, known)
    O.adagrad_update(ent, es, bt["nid"], out["g_pos_ent"], c["lr"])
    O.adagrad_update(ent, es, bt["neg"], out["g_neg"], c["lr"])
    O.adagrad_update(rel, rs, bt["r"], out["g_rel"], c["lr"])
    return out


# --------------------------------------------------------------------------------------------------------------------------
# 1. the per-op entries.  Half-widths k: 4 and 8 (below one k-stage of any tile), 36 (a partial k-stage), 64, 260.  Shapes: TransH's
#    (transh_cases.OP_SHAPES) - partial 16-row / 16-column tiles of the forward product on each edge and none, and (1, 12, 20), whose
#    STACKED 24 rows cross tile boundaries that its 12 rows alone do not
# --------------------------------------------------------------------------------------------------------------------------
OP_WIDTHS = (4, 8, 36, 64, 260)                                          # k; the rows are 2 k wide
OP_SHAPES = ((2, 5, 33), (2, 33, 5), (1, 32, 32), (1, 12, 20))           # (C, chunk, N)
OP_SEEDS = {}               # seed per (k, shape index, neg_head), chosen so that the conditions hold; 0 unless listed


def op_inputs(k, C, chunk, N, neg_head):
    """float32 x [B, 2 k] (the uncorrupted side), y [B, 2 k] (the other entity of the positive), r [B, 2 k], nb [C * N, 2 k],
    W [C, chunk, N] and dp [B] (random signed upstream gradients).  The mapping vector of r[1], the mapping vectors of x[2] and
    nb[3], and the whole row nb[4] are zero."""
    si = OP_SHAPES.index((C, chunk, N))
    rng = np.random.RandomState(_seed("transd-op", k, C, chunk, N, bool(neg_head), OP_SEEDS.get((k, si, bool(neg_head)), 0)))
    B = C * chunk
    sc = np.float32(row_scale(k))
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    inp = dict(x=u(B, 2 * k) * sc, y=u(B, 2 * k) * sc, r=u(B, 2 * k) * sc, nb=u(C * N, 2 * k) * sc, W=u(C, chunk, N), dp=u(B))
    inp["r"][1, k:] = 0.0
    inp["x"][2, k:] = 0.0
    inp["nb"][3, k:] = 0.0
    inp["nb"][4] = 0.0
    return inp


def op_reference(inp, C, chunk, N, neg_head, dtype=np.float64):
    """the outputs of the four per-op entries, the smallest distance share of the compared pairs and the largest |c_j|"""
    x, y, r, nb, W, dp = (inp[k].astype(dtype) for k in ("x", "y", "r", "nb", "W", "dp"))
    h, t = (y, x) if neg_head else (x, y)
    a, rho = pair(neg_head, x, r)
    ga, grho, gn = score_neg_bwd(a, rho, nb, W, C, chunk, N)
    gx, gr = pair_bwd(neg_head, x, r, ga, grho)
    gh, grp, gt = score_bwd(h, r, t, dp)
    share = float(min(dist_shares(a, rho, nb, C, chunk, N).min(), pos_shares(h, r, t).min()))
    return dict(pos=score(h, r, t), gh=gh, grp=grp, gt=gt, score=score_neg(a, rho, nb, C, chunk, N), gx=gx, gr=gr, gn=gn, share=share,
                cmax=float(max(np.abs(c_of(nb)).max(), np.abs(c_of(t)).max())))


OP_GRADS = ("gh", "grp", "gt", "gx", "gr", "gn")


# --------------------------------------------------------------------------------------------------------------------------
# 2. the fused step: the shapes and the option table of tests/pairre_cases.py
# --------------------------------------------------------------------------------------------------------------------------
STEP_B, STEP_CHUNK, STEP_N, STEP_ENT, STEP_REL = 16, 8, 24, 40, 5
STEP_WIDTHS = (32, 36)      # k (36: a partial k-stage); the rows are 64 and 72 wide
# seeds of the batches, per case: chosen so that the conditions hold (0 unless listed)
STEP_SEEDS = {}


def _step_cases():
    import pairre_cases as PR
    return [dict(c) for c in PR.STEP_CASES]


STEP_CASES = _step_cases()


def step_tables(k, zero_p=False):
    """zero_p: every mapping vector - the second half of every entity and relation row - is exactly zero (TransE_l2 on the first)"""
    rng = np.random.RandomState(_seed("transd-step-tables", k))
    sc = np.float32(row_scale(k))
    ent, rel = rng.uniform(-1, 1, (STEP_ENT, 2 * k)).astype(np.float32) * sc, rng.uniform(-1, 1, (STEP_REL, 2 * k)).astype(np.float32) * sc
    if zero_p:
        ent[:, k:] = 0.0
        rel[:, k:] = 0.0
    return ent, rel


def step_batches(c, steps=2):
    """tail then head corruption (oracle.kge_oracle.synth_batch); w: edge importance or None"""
    rng = np.random.RandomState(_seed("transd-step-batch", c["id"], STEP_SEEDS.get(c["id"], 0)))
    out = []
    for s in range(1, steps + 1):
        bt = O.synth_batch(rng, c["n_ent"], c["n_rel"], c["B"], c["N"], c["chunk"], s)
        bt["w"] = rng.uniform(0.5, 1.5, c["B"]).astype(np.float32) if c["impts"] else None
        out.append(bt)
    return out


def planted_known(bt, chunk, N):
    import pairre_cases as PR
    return PR.planted_known(bt, chunk, N)


# the Adam case: adam_cases.step with this statement's gradients (k = 8: rows 16 wide on both tables)
ADAM_CASE = A.case("TransD-w16", "TransD", 8, True, True, adv=True)


@contextlib.contextmanager
def adam_gradients():
    """adam_cases.step / .gradients know the oracle's models, QuatE and PairRE: inside this block they take TransD from here"""
    saved = A.gradients

    def gradients(c, ent, rel, bt, known=None):
        return forward_backward(c, ent, rel, bt, known) if c["model"] == MODEL else saved(c, ent, rel, bt, known)
    A.gradients = gradients
    try:
        yield
    finally:
        A.gradients = saved


# --------------------------------------------------------------------------------------------------------------------------
# 3. exact ranks: integer-grid tables.  Every entry of every row is an integer: first halves have three entries in -2 .. 2, mapping
#    vectors two entries +-1 (relations: three), gamma is an integer.  x_p . x is then an integer of magnitude <= 4, projections
#    are integer vectors with entries <= 2 + 4 = 6, a has entries <= 8, c_j = m_j . n_j is an integer <= 4, and every intermediate
#    of the direct and of the matrix form - alpha <= 64 k, sigma = 3, c^2 sigma <= 48, p, q, u, 2 c (q - u) - is an integer far
#    below 2^24 (test_transd_inputs.py computes the bound from the tables): exact in float32 in any summation order.  sqrtf is
#    correctly rounded, so equal squares give equal scores and distinct ones - integers a few hundred at most, at least 1 apart -
#    distinct scores: ties are real ties.
# --------------------------------------------------------------------------------------------------------------------------
TIE_CASES = [(5, 4), (5, 36), (129, 4), (129, 36), (300, 4), (300, 36)]       # (entities = relations = candidates, k): partial tiles, several
#                                                                       column tiles; the VALU top-K instance (k < 32) and the MFMA one
TIE_E = 40                      # test triples
TIE_E_WIDE = 150                # at 300 entities: three of the ranking kernel's 64-query tiles, the last of 22
TIE_CHUNK = 16                  # chunked_ranks: two chunks of 16 and one of 8 (wide: 9 and one of 6)
TIE_GAMMA = 6.0
# several tiles, as pairre_cases.TIE_WIDE_CASES (tests/new_model_shape_cases.py): (entities, k) - tie_inputs takes the half-width
TIE_WIDE_CASES = [(300, 32), (300, 36)]
TIE_WIDE_E = 150
TIE_WIDE_CHUNK = 100


def tie_E(n):
    return TIE_E_WIDE if n >= 300 else TIE_E


class Case(object):
    pass


def tie_scores(c, h, r, t, neg_head, dtype=np.float64):
    """(p [E], S [E, n_ent]) in `dtype`: the positive scores and the scores of every entity in the corrupted slot"""
    ent, rel = c.ent.astype(dtype), c.rel.astype(dtype)
    g = dtype(TIE_GAMMA)
    a, rho = pair(neg_head, ent[t if neg_head else h], rel[r])
    return score(ent[h], rel[r], ent[t], g), score_neg(a, rho, ent, 1, len(h), len(ent), g)[0]


@functools.lru_cache(maxsize=None)
def tie_inputs(n, k, E=None):
    """tables, E test triples and known triples: the test triples and, for the first 12 of them and both sides, one planted triple
    whose corrupted entity TIES the positive where there is one.  Entries are sparse so that few distinct distances are shared by
    many candidates.  Entity 0 and relation 0 have no mapping vector."""
    E = tie_E(n) if E is None else E
    rng = np.random.RandomState(_seed("transd-tie", n, k))
    c = Case()
    c.n, c.k, c.d_e = n, k, 2 * k
    c.ent = np.zeros((n, 2 * k), np.float32)
    c.rel = np.zeros((n, 2 * k), np.float32)
    for i in range(n):
        c.ent[i, rng.choice(k, 3, replace=False)] = rng.choice([-2.0, -1.0, 1.0, 2.0], 3)
        c.ent[i, k + rng.choice(k, 2, replace=False)] = rng.choice([-1.0, 1.0], 2)
        c.rel[i, rng.choice(k, 2, replace=False)] = rng.choice([-1.0, 1.0], 2)
        c.rel[i, k + rng.choice(k, 3, replace=False)] = rng.choice([-1.0, 1.0], 3)
    c.ent[0, k:] = 0.0
    c.rel[0, k:] = 0.0
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
    c.kh, c.kr, c.kt = (np.concatenate([x, extra[:, j]]) for j, x in enumerate((c.h, c.r, c.t)))
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _direct_d2(a, rho, ent, E, n):
    """[1, E, n] squared distances of the direct form, without the root"""
    A_, R_, N_, _, cc = _blocks(a, rho, ent, 1, E, n)
    d = A_ - N_ - cc[..., None] * R_
    return (d * d).sum(-1)


def tie_intermediates(c, h, r, t, neg_head):
    """every intermediate of the two forms in float64, as one flat array: the entries of a, the projections' dots, and per pair
    alpha, beta, sigma, c, c^2 sigma, p, q, u, 2 c (q - u), the partial sums alpha + beta, - 2 p + ..., the squared distance"""
    ent, rel = c.ent.astype(np.float64), c.rel.astype(np.float64)
    E, n = len(h), len(ent)
    x = ent[t if neg_head else h]
    a, rho = pair(neg_head, x, rel[r])
    p, q, al, sg, u, be, cc = matrix_terms(a, rho, ent, 1, E, n)
    parts = [a, dot(halves(x)[1], halves(x)[0]), p, q, al, sg, u, be, cc, cc * cc * sg, cc * sg, 2 * (q - u), cc * (cc * sg + 2 * (q - u)),
             al + be, al + be - 2 * p, dist2_matrix(a, rho, ent, 1, E, n), _direct_d2(a, rho, ent, E, n),
             np.abs(a).sum(-1, keepdims=True) * np.abs(halves(ent)[0]).sum(-1).max()]      # the largest partial sum of any order
    return np.concatenate([np.asarray(v, np.float64).reshape(-1) for v in parts])


def f32_scores_two_forms(c, h, r, t, neg_head):
    """the [E, n] scores evaluated in float32 in the direct form and in the matrix form with the sums over k running backward"""
    ent, rel = c.ent, c.rel
    a, rho = pair(neg_head, ent[t if neg_head else h], rel[r])
    assert a.dtype == np.float32 and rho.dtype == np.float32
    E, n, k = len(h), len(ent), c.k
    s1 = score_neg(a, rho, ent, 1, E, n, np.float32(TIE_GAMMA))[0]
    p, q = np.zeros((E, n), np.float32), np.zeros((E, n), np.float32)
    al, sg, uu = np.zeros((E, 1), np.float32), np.zeros((E, 1), np.float32), np.zeros((E, 1), np.float32)
    be, cc = np.zeros((1, n), np.float32), np.zeros((1, n), np.float32)
    for j in range(k - 1, -1, -1):
        p += a[:, j:j + 1] * ent[None, :, j]
        q += rho[:, j:j + 1] * ent[None, :, j]
        al += a[:, j:j + 1] ** 2
        sg += rho[:, j:j + 1] ** 2
        uu += a[:, j:j + 1] * rho[:, j:j + 1]
        be += ent[None, :, j] ** 2
        cc += ent[None, :, j] * ent[None, :, k + j]
    d2 = cc * (cc * sg + np.float32(2) * (q - uu)) + ((al + be) - np.float32(2) * p)
    assert d2.dtype == np.float32 and s1.dtype == np.float32
    return s1, np.float32(TIE_GAMMA) - np.sqrt(np.maximum(d2, np.float32(0)))


# --------------------------------------------------------------------------------------------------------------------------
# 4. the interface: 40 entities, 6 relations, k = 8 (rows 16 wide)
# --------------------------------------------------------------------------------------------------------------------------
IF_ENT, IF_REL, IF_K_HALF, IF_K = 40, 6, 8, 5
IF_D = 2 * IF_K_HALF
IF_GAMMA = 3.0


def interface_tables():
    rng = np.random.RandomState(_seed("transd-interface"))
    sc = np.float32(row_scale(IF_K_HALF))
    return rng.uniform(-1, 1, (IF_ENT, IF_D)).astype(np.float32) * sc, rng.uniform(-1, 1, (IF_REL, IF_D)).astype(np.float32) * sc


def all_scores(ent, rel, gamma=IF_GAMMA):
    """[n_ent, n_rel, n_ent] float64 scores of every triple"""
    e, r = ent.astype(np.float64), rel.astype(np.float64)
    out = np.zeros((len(e), len(r), len(e)))
    for j in range(len(r)):
        rr = np.repeat(r[j:j + 1], len(e), 0)
        a, rho = pair(False, e, rr)
        out[:, j, :] = score_neg(a, rho, e, 1, len(e), len(e), gamma)[0]
    return out
