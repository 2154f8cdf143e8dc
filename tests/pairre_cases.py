"""Float64 statement, case tables and input builders of the PairRE score function (include/kge_hip.h, enum kge_model, KGE_PAIRRE = 10).
Test infrastructure; a plain module, not a conftest.  Shared by
  tests/test_pairre_inputs.py  (CPU): the statement against torch.autograd, its identities, the ambiguity cap of every case, the
                               integer-grid ranking inputs, the host refusals;
  tests/test_gpu_pairre.py     (GPU): the per-op entries, the fused step, exact ranks of every ranking entry, the interface.

The statement (dtype of the inputs; entity rows d_e wide, relation rows 2 d_e wide, r = [rH | rT]):
    x^ = x / |x|_2,  x^ = 0 where |x|_2 == 0
    s(h, r, t) = gamma - sum_k |h^_k rH_k - t^_k rT_k|
    per-edge pair: tails corrupted a = h^ o rH, w = rT;  heads corrupted a = t^ o rT, w = rH
    chunked score s_ij = gamma - sum_k |a_ik - w_ik n^_jk|
    sigma = sign(a - w n^), sign(0) = 0, G = dL/ds:  Ga = -sum_j G sigma,  Gw = sum_j G sigma n^,  Gn^ = sum_i G sigma w
    through a normalisation  gx = (gx^ - x^ <x^, gx^>) / |x|  (0 where |x| == 0)
The oracle (oracle/kge_oracle.py) has no PairRE: `forward_backward` / `step` below restate its train step with these formulas and
its own loss, regulariser and Adagrad functions (the Softmax genre: tests/softmax_loss_cases.py).

Tolerances are the suite's (tests/modular_op_cases.py): scores 1e-4 abs + 1e-4 rel; gradients and updated rows 3e-4 of the
compared array's largest component + 3e-4 relative.

Sign ambiguity (the l1_ambiguous rule of tests/modular_op_cases.py): an element with |u| < tau in float64, u = a - w n^ and
tau = (|a| + |w n^|) (d_e + 8) 2^-24 - the worst-case rounding of a norm over d_e squares plus the handful of products and the
subtraction - may round to the other sign in float32.  Gradient rows fed by such an element are left out of the comparison
(through the normalisation adjoint one element taints its whole row).  No compared array may lose more than ROW_CAP of its rows;
the seeds of the per-op inputs are chosen for that, and the step inputs are chosen to hold no such element at all."""
import functools
import zlib

import numpy as np

import softmax_loss_cases as SM
from modular_op_cases import GRAD_RTOL, SCORE_ATOL, SCORE_RTOL, grad_bound, score_bound, worst      # noqa: F401 - re-exported
from oracle import kge_oracle as O

MODEL = "PairRE"
MODEL_ID = 10               # include/kge_hip.h KGE_PAIRRE
NEG_DEG = 32                # KGE_FLAG_NEG_DEG_SAMPLE
KNOWN_SCORE = -1.0e6        # KGE_KNOWN_SCORE
ROW_CAP = 0.10              # share of the rows of a compared array that sign ambiguity may take out
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


def score(h, r, t, gamma=GAMMA):
    rH, rT = halves(r)
    return gamma - np.abs(unit(h) * rH - unit(t) * rT).sum(-1)


def score_bwd(h, r, t, dp):
    """(gh, gr, gt) of sum_i dp_i s(h_i, r_i, t_i)"""
    rH, rT = halves(r)
    hu, tu = unit(h), unit(t)
    sg = dp[:, None] * np.sign(hu * rH - tu * rT)
    return unit_bwd(h, -sg * rH), np.concatenate([-sg * hu, sg * tu], -1), unit_bwd(t, sg * rT)


def pair(neg_head, x, r):
    """(a, w) of the edges whose uncorrupted entity rows are x"""
    rH, rT = halves(r)
    return (unit(x) * rT, rH) if neg_head else (unit(x) * rH, rT)


def pair_bwd(neg_head, x, r, ga, gw):
    """(dL/dx, dL/dr) from (Ga, Gw)"""
    rH, rT = halves(r)
    xu = unit(x)
    if neg_head:
        return unit_bwd(x, ga * rT), np.concatenate([gw, ga * xu], -1)
    return unit_bwd(x, ga * rH), np.concatenate([ga * xu, gw], -1)


def _diff(a, w, neg, C, chunk, N):
    """u [C, chunk, N, d] = a_ik - w_ik n^_jk and n^ [C, N, d]"""
    nu = unit(neg).reshape(C, N, -1)
    A, W = a.reshape(C, chunk, 1, -1), w.reshape(C, chunk, 1, -1)
    return A - W * nu[:, None, :, :], nu


def score_neg(a, w, neg, C, chunk, N, gamma=GAMMA):
    return gamma - np.abs(_diff(a, w, neg, C, chunk, N)[0]).sum(-1)


def score_neg_bwd(a, w, neg, G, C, chunk, N):
    """(Ga, Gw, dL/dneg) - the last one through the candidates' normalisation"""
    u, nu = _diff(a, w, neg, C, chunk, N)
    gs = G.reshape(C, chunk, N, 1) * np.sign(u)
    ga = -gs.sum(2).reshape(a.shape)
    gw = (gs * nu[:, None, :, :]).sum(2).reshape(a.shape)
    gnu = (gs * w.reshape(C, chunk, 1, -1)).sum(1).reshape(neg.shape)
    return ga, gw, unit_bwd(neg, gnu)


def ambiguous(a, w, neg, C, chunk, N):
    """[C, chunk, N] bool: the pairs that hold an element with |u| < tau"""
    d = a.shape[-1]
    u, nu = _diff(a, w, neg, C, chunk, N)
    tau = (np.abs(a.reshape(C, chunk, 1, -1)) + np.abs(w.reshape(C, chunk, 1, -1) * nu[:, None, :, :])) * (d + 8) * 2.0 ** -24
    return (np.abs(u) < tau).any(-1)


def ambiguous_pos(h, r, t):
    """[B] bool: the edges whose positive score holds such an element"""
    rH, rT = halves(r)
    a, b = unit(h) * rH, unit(t) * rT
    return (np.abs(a - b) < (np.abs(a) + np.abs(b)) * (h.shape[-1] + 8) * 2.0 ** -24).any(-1)


def tau_share(a, w, neg, C, chunk, N, got_u):
    """largest |got_u - u| / tau over the elements (a float32 evaluation `got_u` of u against the float64 one)"""
    d = a.shape[-1]
    u, nu = _diff(a, w, neg, C, chunk, N)
    tau = (np.abs(a.reshape(C, chunk, 1, -1)) + np.abs(w.reshape(C, chunk, 1, -1) * nu[:, None, :, :])) * (d + 8) * 2.0 ** -24
    m = tau > 0
    return float((np.abs(got_u - u)[m] / tau[m]).max())


def loss_fwd_bwd(c, p, n, w):
    if c["genre"] == SM.GENRE:
        return SM.softmax_fwd_bwd(p, n, w)
    return O.loss_fwd_bwd(p, n, w, c["genre"], c["adv"], c["adv_temp"], c["pairwise"], c["margin"])


def forward_backward(c, ent, rel, bt, known=None):
    """oracle.kge_oracle.forward_backward with the PairRE formulas, in the dtype of the tables.  known: [B, N] bool, the pairs that
    take KGE_KNOWN_SCORE (tests/known_negative_cases.py masked_forward_backward).  `amb`: whether any element of the step is
    sign-ambiguous."""
    dt = ent.dtype
    chunk, N, neg_head = c["chunk"], c["N"], bt["neg_head"]
    B = len(bt["h"])
    C = B // chunk
    pos_emb, r, neg = ent[bt["nid"]], rel[bt["r"]], ent[bt["neg"]]
    h, t = pos_emb[bt["h_local"]], pos_emb[bt["t_local"]]
    w = None if bt.get("w") is None else bt["w"].astype(dt)
    p = score(h, r, t)
    x = t if neg_head else h
    a, wv = pair(neg_head, x, r)
    nd = c["neg_deg"]
    if nd:          # the chunk's own corrupted-side entities in front, the positive edge's own column at score 0 (general_models.py:396-432)
        Np = chunk + N
        y = (h if neg_head else t).reshape(C, chunk, -1)
        neg_all = np.concatenate([y, neg.reshape(C, N, -1)], 1).reshape(C * Np, -1)
        mask = np.ones((C, chunk, Np), dt)
        mask[:, np.arange(chunk), np.arange(chunk)] = 0
        n = score_neg(a, wv, neg_all, C, chunk, Np) * mask
    else:
        Np, neg_all, mask = N, neg, 1
        n = score_neg(a, wv, neg, C, chunk, N)
    if known is not None:
        n = np.where(known.reshape(n.shape), dt.type(KNOWN_SCORE), n)
    (pl, nl, loss), dpos, dneg = loss_fwd_bwd(c, p, n.reshape(B, Np), w)
    dneg = dneg.reshape(C, chunk, Np) * mask
    if known is not None:
        dneg = np.where(known.reshape(dneg.shape), 0, dneg)
    use_reg = c["reg_coef"] > 0.0 and c["reg_norm"] > 0
    reg = O.reg_value([pos_emb, neg], c["reg_coef"], c["reg_norm"]) + O.reg_value([r], c["reg_coef"], c["reg_norm"]) if use_reg else 0.0
    gh, gr, gt = score_bwd(h, r, t, dpos)
    ga, gw, g_all = score_neg_bwd(a, wv, neg_all, dneg, C, chunk, Np)
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
    amb = bool(ambiguous(a, wv, neg_all, C, chunk, Np).any() or ambiguous_pos(h, r, t).any())
    return dict(pos_score=p, neg_score=n, log=(pl, nl, loss, reg), g_pos_ent=g_pos.astype(dt), g_rel=gr.astype(dt),
                g_neg=g_neg.astype(dt), amb=amb)


def step(c, ent, es, rel, rs, bt, known=None):
    """forward + backward + the reference's update order (entity trace 0, entity trace 1, relation trace), tables in place"""
    out = forward_backward(c, ent, rel, bt, known)
    O.adagrad_update(ent, es, bt["nid"], out["g_pos_ent"], c["lr"])
    O.adagrad_update(ent, es, bt["neg"], out["g_neg"], c["lr"])
    O.adagrad_update(rel, rs, bt["r"], out["g_rel"], c["lr"])
    return out


# --------------------------------------------------------------------------------------------------------------------------
# 1. the per-op entries.  The kernels have ONE instance for every width (scalar lane-strided rows, 32-wide k slabs; no width limit,
#    so no case near 1024).  Widths: 2 (below one vector), 6 (no multiple of 4), 30 (a partial slab), 32 (the exact slab), 36 (slab
#    + 4), 200 (the recipe's).  Shapes: partial tiles on each edge of the 32 x 32 tile and none.
# --------------------------------------------------------------------------------------------------------------------------
OP_WIDTHS = (2, 6, 30, 32, 36, 200)
OP_SHAPES = ((2, 5, 33), (2, 33, 5), (1, 32, 32))           # (C, chunk, N)
# seed per (d_e, shape index, neg_head), chosen so that sign ambiguity takes out at most ROW_CAP of the rows of every compared
# array (test_pairre_inputs.py asserts it); 0 unless listed
OP_SEEDS = {}


def op_inputs(d_e, C, chunk, N, neg_head):
    """float32 x [B, d_e] (the uncorrupted side), y [B, d_e] (the other entity of the positive), r [B, 2 d_e], nb [C * N, d_e],
    W [C, chunk, N] and dp [B] (random signed upstream gradients).  Rows x[1], y[2] and nb[3] are all zero."""
    si = OP_SHAPES.index((C, chunk, N))
    rng = np.random.RandomState(_seed("pairre-op", d_e, C, chunk, N, bool(neg_head), OP_SEEDS.get((d_e, si, bool(neg_head)), 0)))
    B = C * chunk
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    inp = dict(x=u(B, d_e), y=u(B, d_e), r=u(B, 2 * d_e), nb=u(C * N, d_e), W=u(C, chunk, N), dp=u(B))
    inp["x"][1] = 0.0
    inp["y"][2] = 0.0
    inp["nb"][3] = 0.0
    return inp


def op_reference(inp, C, chunk, N, neg_head, dtype=np.float64):
    """the outputs of the four per-op entries, and the rows sign ambiguity takes out: amb_e (edges of the chunked score), amb_n
    (candidate rows), amb_p (edges of the positive score)"""
    x, y, r, nb, W, dp = (inp[k].astype(dtype) for k in ("x", "y", "r", "nb", "W", "dp"))
    h, t = (y, x) if neg_head else (x, y)
    a, w = pair(neg_head, x, r)
    ga, gw, gn = score_neg_bwd(a, w, nb, W, C, chunk, N)
    gx, gr = pair_bwd(neg_head, x, r, ga, gw)
    gh, grp, gt = score_bwd(h, r, t, dp)
    amb = ambiguous(a, w, nb, C, chunk, N)
    return dict(pos=score(h, r, t), gh=gh, grp=grp, gt=gt, score=score_neg(a, w, nb, C, chunk, N), gx=gx, gr=gr, gn=gn,
                amb_e=amb.any(2).reshape(-1), amb_n=amb.any(1).reshape(-1), amb_p=ambiguous_pos(h, r, t))


OP_ROWS = dict(gh="amb_p", grp="amb_p", gt="amb_p", gx="amb_e", gr="amb_e", gn="amb_n")     # gradient -> the mask of its excluded rows


# --------------------------------------------------------------------------------------------------------------------------
# 2. the fused step: B = 16, chunk = 8, N = 24 on 40 entities and 5 relations - entities and relations repeat inside a batch and
#    among the negatives, so the owner-computes update walks lists longer than one (asserted by the CPU file).  Every step starts
#    from the fixed tables, so that the CPU file can assert that no element of any step is sign-ambiguous.
# --------------------------------------------------------------------------------------------------------------------------
STEP_B, STEP_CHUNK, STEP_N, STEP_ENT, STEP_REL = 16, 8, 24, 40, 5
STEP_WIDTHS = (32, 36)
# seeds of the batches, per case: chosen so that no element of any step is sign-ambiguous at either width (0 unless listed;
# test_pairre_inputs.py asserts it)
STEP_SEEDS = {"logistic": 1, "reg2": 1}


def step_case(cid, genre="Logsigmoid", adv=False, adv_temp=1.0, pairwise=False, margin=1.0, reg_coef=0.0, reg_norm=3, neg_deg=False,
              impts=False, lr=0.1):
    return dict(id=cid, genre=genre, adv=adv, adv_temp=adv_temp, pairwise=pairwise, margin=margin, reg_coef=reg_coef,
                reg_norm=reg_norm, neg_deg=neg_deg, impts=impts, lr=lr, B=STEP_B, chunk=STEP_CHUNK, N=STEP_N, n_ent=STEP_ENT,
                n_rel=STEP_REL)


# regulariser coefficients: at these values the regulariser is a few per cent of the largest gradient component (asserted by the
# CPU file)
STEP_CASES = [
    step_case("logsigmoid", "Logsigmoid"),
    step_case("logsigmoid-adv", adv=True),
    step_case("logistic", "Logistic"),
    step_case("hinge", "Hinge"),
    step_case("hinge-pw", "Hinge", pairwise=True, margin=0.2),
    step_case("bce", "BCE"),
    step_case("softmax", SM.GENRE),
    step_case("neg-deg", adv=True, neg_deg=True),
    step_case("impts", adv=True, impts=True),
    step_case("reg1", adv=True, reg_coef=2e-3, reg_norm=1),
    step_case("reg2", adv=True, reg_coef=2e-3, reg_norm=2),
    step_case("reg3", adv=True, reg_coef=2e-3, reg_norm=3),
]


def step_tables(d_e):
    rng = np.random.RandomState(_seed("pairre-step-tables", d_e))
    return (rng.uniform(-1, 1, (STEP_ENT, d_e)).astype(np.float32), rng.uniform(-1, 1, (STEP_REL, 2 * d_e)).astype(np.float32))


def step_batches(c, steps=2):
    """tail then head corruption (oracle.kge_oracle.synth_batch); w: edge importance or None"""
    rng = np.random.RandomState(_seed("pairre-step-batch", c["id"], STEP_SEEDS.get(c["id"], 0)))
    out = []
    for s in range(1, steps + 1):
        bt = O.synth_batch(rng, c["n_ent"], c["n_rel"], c["B"], c["N"], c["chunk"], s)
        bt["w"] = rng.uniform(0.5, 1.5, c["B"]).astype(np.float32) if c["impts"] else None
        out.append(bt)
    return out


def planted_known(bt, chunk, N):
    """known triples (h, r, t) whose corruption is column 3 of row 0 and column N - 1 of row chunk (the second chunk), and the
    [B, N] matrix of the pairs they take out (every row of the chunk that shares the uncorrupted side and the relation)"""
    B = len(bt["h"])
    K = []
    for i, j in ((0, 3), (chunk, N - 1)):
        e = int(bt["neg"][(i // chunk) * N + j])
        K.append((e, int(bt["r"][i]), int(bt["t"][i])) if bt["neg_head"] else (int(bt["h"][i]), int(bt["r"][i]), e))
    S = set(K)
    known = np.zeros((B, N), bool)
    for i in range(B):
        for j in range(N):
            e = int(bt["neg"][(i // chunk) * N + j])
            tr = (e, int(bt["r"][i]), int(bt["t"][i])) if bt["neg_head"] else (int(bt["h"][i]), int(bt["r"][i]), e)
            known[i, j] = tr in S
    K = np.array(K, np.int64)
    return (K[:, 0].copy(), K[:, 1].copy(), K[:, 2].copy()), known


# --------------------------------------------------------------------------------------------------------------------------
# 3. exact ranks: integer-grid tables.  Every entity row has exactly four non-zero entries +-1, so |x| = 2 and x^ is in {0, +-1/2};
#    relation entries are integers in -2 .. 2 and gamma is an integer: every score is a small multiple of 1/2 - exact in float32 in
#    any summation order - and few distinct values are shared by many candidates: ties occur.
# --------------------------------------------------------------------------------------------------------------------------
TIE_CASES = [(7, 8), (130, 8), (130, 32)]            # (entities = relations = candidates, d_e)
TIE_E = 40                      # test triples
TIE_CHUNK = 16                  # chunked_ranks: two chunks of 16 and one of 8
# several tiles (tests/test_gpu_new_model_shapes.py): 300 candidates are three 128-column tiles, the last of 44; 150 test triples are
# two 128-row tiles, the last of 22; chunks of 100 triples: the second one spans both row tiles.  Width 36 = one 32-wide slab + 4:
# four entries +-1 keep |x| = 2 at any width, so both widths stay exact
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
    a, w = pair(neg_head, ent[t if neg_head else h], rel[r])
    return score(ent[h], rel[r], ent[t], g), score_neg(a, w, ent, 1, len(h), len(ent), g)[0]


@functools.lru_cache(maxsize=None)
def tie_inputs(n, d_e, E=None):
    """tables, E (default: TIE_E, read at the call) test triples and known triples: the test triples and, for the first 12 of them
    and both sides, one planted triple whose corrupted entity TIES the positive where there is one"""
    E = TIE_E if E is None else E
    rng = np.random.RandomState(_seed("pairre-tie", n, d_e))
    c = Case()
    c.n, c.d_e = n, d_e
    c.ent = np.zeros((n, d_e), np.float32)
    for i in range(n):
        c.ent[i, rng.choice(d_e, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    c.rel = rng.randint(-2, 3, (n, 2 * d_e)).astype(np.float32)
    c.h, c.r, c.t = rng.randint(0, n, E), rng.randint(0, n, E), rng.randint(0, n, E)
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


def filter_lists(c, neg_head):
    """per test triple the ascending unique entity ids whose corruption is a known triple: (ranges [E, 2], ids), the layout of
    eval.build_filter, built independently of it"""
    lists = []
    for i in range(len(c.h)):
        if neg_head:
            lists.append(np.unique(c.kh[(c.kt == c.t[i]) & (c.kr == c.r[i])]))
        else:
            lists.append(np.unique(c.kt[(c.kh == c.h[i]) & (c.kr == c.r[i])]))
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return np.stack([ptr[:-1], ptr[1:]], 1), np.concatenate(lists).astype(np.int64)


def ranks_of(p, S, lists=None, strict=False):
    """[E] int64: 1 + #{columns j outside list_i : S[i, j] >= p[i]} (strict: >, the wrong comparison the inputs are measured against)"""
    out = np.zeros(len(p), np.int64)
    for i in range(len(p)):
        keep = np.ones(S.shape[1], bool)
        if lists is not None:
            keep[lists[1][lists[0][i, 0]:lists[0][i, 1]]] = False
        out[i] = 1 + int((keep & ((S[i] > p[i]) if strict else (S[i] >= p[i]))).sum())
    return out


def tie_candidates(n, E=None, chunk=None):
    """[n_chunks, 12] candidate ids per chunk of `chunk` (default: TIE_CHUNK) of E (default: TIE_E) triples, drawn with replacement,
    two slots per list -1"""
    E, chunk = TIE_E if E is None else E, TIE_CHUNK if chunk is None else chunk
    n_chunks = (E + chunk - 1) // chunk
    rng = np.random.RandomState(_seed("pairre-tie-cand", n))
    cand = rng.randint(0, n, (n_chunks, 12)).astype(np.int64)
    for k in range(n_chunks):
        cand[k, rng.choice(12, 2, replace=False)] = -1
    return cand


def chunked_ranks_of(c, p, S, neg_head, cand=None, self_cand=False, chunk=None):
    """ranks against per-chunk candidate lists (-1: an empty slot); self_cand: the chunk's own corrupted-side entities are prepended
    and the triple's own column scores 0.0 (the --neg_deg_sample_eval protocol, tests/chunked_eval_cases.py)"""
    side = c.h if neg_head else c.t
    E = len(p)
    chunk = TIE_CHUNK if chunk is None else chunk
    out = np.zeros(E, np.int64)
    for i in range(E):
        k = i // chunk
        ids = cand[k][cand[k] >= 0] if cand is not None else np.arange(c.n)
        s = S[i, ids]
        if self_cand:
            own_ids = side[k * chunk:min(E, (k + 1) * chunk)]
            so = S[i, own_ids].copy()
            so[i - k * chunk] = 0.0
            s = np.concatenate([so, s])
        out[i] = 1 + int((s >= p[i]).sum())
    return out


def f32_scores_two_orders(c, h, r, t, neg_head):
    """the [E, n] scores evaluated in float32 with the sum over k running forward and backward"""
    ent, rel = c.ent, c.rel
    a, w = pair(neg_head, ent[t if neg_head else h], rel[r])
    nu = unit(ent)
    assert a.dtype == np.float32 and nu.dtype == np.float32
    s1 = np.zeros((len(h), len(ent)), np.float32)
    s2 = np.zeros_like(s1)
    for k in range(c.d_e):
        s1 += np.abs(a[:, k:k + 1] - w[:, k:k + 1] * nu[None, :, k])
        kk = c.d_e - 1 - k
        s2 += np.abs(a[:, kk:kk + 1] - w[:, kk:kk + 1] * nu[None, :, kk])
    g = np.float32(TIE_GAMMA)
    return g - s1, g - s2


# --------------------------------------------------------------------------------------------------------------------------
# 4. the interface: 40 entities, 6 relations, 16 wide
# --------------------------------------------------------------------------------------------------------------------------
IF_ENT, IF_REL, IF_D, IF_K = 40, 6, 16, 5
IF_GAMMA = 3.0


def interface_tables():
    rng = np.random.RandomState(_seed("pairre-interface"))
    return rng.uniform(-1, 1, (IF_ENT, IF_D)).astype(np.float32), rng.uniform(-1, 1, (IF_REL, 2 * IF_D)).astype(np.float32)


def all_scores(ent, rel, gamma=IF_GAMMA):
    """[n_ent, n_rel, n_ent] float64 scores of every triple"""
    e, r = ent.astype(np.float64), rel.astype(np.float64)
    rH, rT = halves(r)
    eu = unit(e)
    return gamma - np.abs((eu[:, None, :] * rH[None, :, :])[:, :, None, :] - (eu[None, :, :] * rT[:, None, :])[None, :, :, :]).sum(-1)
