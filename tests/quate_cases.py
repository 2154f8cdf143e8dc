"""Float64 statement, case tables and input builders of the QuatE score function (include/kge_hip.h, enum kge_model, KGE_QUATE = 8).
Test infrastructure; a plain module, not a conftest.  Shared by
  tests/test_quate_inputs.py   (CPU): the statement against torch.autograd, its identities, the integer-grid ranking inputs, the
                               host refusals;
  tests/test_gpu_quate.py      (GPU): the per-op entries, the fused step, exact ties of every ranking entry, the interface.

The statement (dtype of the inputs; rows are four quarters [a | b | c | d] of q = d_e / 4 columns, column k of a row is the
quaternion a_k + b_k i + c_k j + d_k k):
    r^_k = r_k / n_k,  n_k = sqrt(ra^2 + rb^2 + rc^2 + rd^2),  r^_k = 0 where n_k == 0
    x (x) y = (ap - bq - cu - dv, aq + bp + cv - du, au - bv + cp + dq, av + bu - cq + dp)     x = (a, b, c, d), y = (p, q, u, v)
    s(h, r, t) = sum_k <(h (x) r^)_k, t_k>
    A = h (x) r^ (tails corrupted),  A = t (x) conj(r^) (heads corrupted);  chunked score = A . candidate
    ds/dt = h (x) r^,  ds/dh = t (x) conj(r^),  g = ds/dr^ = conj(h) (x) t,  ds/dr = (g - r^ <r^, g>) / n  (0 where n == 0)
The oracle (oracle/kge_oracle.py) has no QuatE: `forward_backward` / `step` below restate its train step with these formulas and
its own loss, regulariser and Adagrad functions (the Softmax genre: tests/softmax_loss_cases.py).

Tolerances are the suite's (tests/modular_op_cases.py): scores 1e-4 abs + 1e-4 rel; gradients and updated rows 3e-4 of the
compared array's largest component + 3e-4 relative."""
import functools
import zlib

import numpy as np

import softmax_loss_cases as SM
from modular_op_cases import GRAD_RTOL, SCORE_ATOL, SCORE_RTOL, grad_bound, score_bound, worst      # noqa: F401 - re-exported
from oracle import kge_oracle as O

MODEL = "QuatE"
MODEL_ID = 8                # include/kge_hip.h KGE_QUATE
FORCE_PAIRWISE = 1          # include/kge_hip.h KGE_FLAG_FORCE_PAIRWISE
NEG_DEG = 32                # KGE_FLAG_NEG_DEG_SAMPLE
KNOWN_SCORE = -1.0e6        # KGE_KNOWN_SCORE


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


# --------------------------------------------------------------------------------------------------------------------------
# the statement
# --------------------------------------------------------------------------------------------------------------------------
def quarters(x):
    q = x.shape[-1] // 4
    return x[..., :q], x[..., q:2 * q], x[..., 2 * q:3 * q], x[..., 3 * q:]


def cat(parts):
    return np.concatenate(parts, -1)


def hamilton(x, y):
    a, b, c, d = quarters(x)
    p, q, u, v = quarters(y)
    return cat([a * p - b * q - c * u - d * v, a * q + b * p + c * v - d * u, a * u - b * v + c * p + d * q,
                a * v + b * u - c * q + d * p])


def conj(x):
    a, b, c, d = quarters(x)
    return cat([a, -b, -c, -d])


def norms(r):
    """[..., q] norm of every relation quaternion"""
    a, b, c, d = quarters(r)
    return np.sqrt(a * a + b * b + c * c + d * d)


def unit(r):
    n = norms(r)
    safe = np.where(n > 0, n, 1)
    return cat([np.where(n > 0, p / safe, 0) for p in quarters(r)])


def unit_bwd(r, g):
    """dL/dr from g = dL/dr^: (g - r^ <r^, g>) / n per quaternion, 0 where n == 0"""
    n = norms(r)
    ru = unit(r)
    dot = sum(p * q for p, q in zip(quarters(ru), quarters(g)))
    safe = np.where(n > 0, n, 1)
    return cat([np.where(n > 0, (q - p * dot) / safe, 0) for p, q in zip(quarters(ru), quarters(g))])


def score(h, r, t):
    return (hamilton(h, unit(r)) * t).sum(-1)


def score_bwd(h, r, t, dp):
    """(gh, gr, gt) of sum_i dp_i s(h_i, r_i, t_i)"""
    ru = unit(r)
    d = dp[:, None]
    return d * hamilton(t, conj(ru)), unit_bwd(r, d * hamilton(conj(h), t)), d * hamilton(h, ru)


def pos_side(neg_head, x, r):
    return hamilton(x, conj(unit(r))) if neg_head else hamilton(x, unit(r))


def pos_side_bwd(neg_head, x, r, ga):
    """(dL/dx, dL/dr) from ga = dL/dA: <ga, x (x) r^> = <ga (x) conj(r^), x>;  <ga, x (x) conj(r^)> = <ga (x) r^, x>"""
    ru = unit(r)
    if neg_head:
        return hamilton(ga, ru), unit_bwd(r, hamilton(conj(ga), x))
    return hamilton(ga, conj(ru)), unit_bwd(r, hamilton(conj(x), ga))


def score_neg(a, neg, C, chunk, N):
    return np.einsum("cik,cjk->cij", a.reshape(C, chunk, -1), neg.reshape(C, N, -1))


def score_neg_bwd(a, neg, G, C, chunk, N):
    A, Bn, G = a.reshape(C, chunk, -1), neg.reshape(C, N, -1), G.reshape(C, chunk, N)
    return np.einsum("cij,cjk->cik", G, Bn).reshape(a.shape), np.einsum("cij,cik->cjk", G, A).reshape(neg.shape)


def rel_query(h, t):
    """the query row of relation ranking: s_j = <conj(h) (x) t, r^_j>"""
    return hamilton(conj(h), t)


def loss_fwd_bwd(c, p, n, w):
    if c["genre"] == SM.GENRE:
        return SM.softmax_fwd_bwd(p, n, w)
    return O.loss_fwd_bwd(p, n, w, c["genre"], c["adv"], c["adv_temp"], c["pairwise"], c["margin"])


def forward_backward(c, ent, rel, bt, known=None):
    """oracle.kge_oracle.forward_backward with the QuatE formulas, in the dtype of the tables.  known: [B, N] bool, the pairs that
    take KGE_KNOWN_SCORE (tests/known_negative_cases.py masked_forward_backward)."""
    dt = ent.dtype
    chunk, N, neg_head = c["chunk"], c["N"], bt["neg_head"]
    B = len(bt["h"])
    C = B // chunk
    pos_emb, r, neg = ent[bt["nid"]], rel[bt["r"]], ent[bt["neg"]]
    h, t = pos_emb[bt["h_local"]], pos_emb[bt["t_local"]]
    w = None if bt.get("w") is None else bt["w"].astype(dt)
    p = score(h, r, t)
    x = t if neg_head else h
    a = pos_side(neg_head, x, r)
    nd = c["neg_deg"]
    if nd:          # the chunk's own corrupted-side entities in front, the positive edge's own column at score 0 (general_models.py:396-432)
        Np = chunk + N
        y = (h if neg_head else t).reshape(C, chunk, -1)
        neg_all = np.concatenate([y, neg.reshape(C, N, -1)], 1).reshape(C * Np, -1)
        mask = np.ones((C, chunk, Np), dt)
        mask[:, np.arange(chunk), np.arange(chunk)] = 0
        n = score_neg(a, neg_all, C, chunk, Np) * mask
    else:
        Np, neg_all, mask = N, neg, 1
        n = score_neg(a, neg, C, chunk, N)
    if known is not None:
        n = np.where(known.reshape(n.shape), dt.type(KNOWN_SCORE), n)
    (pl, nl, loss), dpos, dneg = loss_fwd_bwd(c, p, n.reshape(B, Np), w)
    dneg = dneg.reshape(C, chunk, Np) * mask
    if known is not None:
        dneg = np.where(known.reshape(dneg.shape), 0, dneg)
    use_reg = c["reg_coef"] > 0.0 and c["reg_norm"] > 0
    reg = O.reg_value([pos_emb, neg], c["reg_coef"], c["reg_norm"]) + O.reg_value([r], c["reg_coef"], c["reg_norm"]) if use_reg else 0.0
    gh, gr, gt = score_bwd(h, r, t, dpos)
    ga, g_all = score_neg_bwd(a, neg_all, dneg, C, chunk, Np)
    g_all = g_all.reshape(C, Np, -1)
    g_neg = g_all[:, Np - N:].reshape(C * N, -1)
    gx, gr2 = pos_side_bwd(neg_head, x, r, ga)
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
    return dict(pos_score=p, neg_score=n, log=(pl, nl, loss, reg), g_pos_ent=g_pos.astype(dt), g_rel=gr.astype(dt),
                g_neg=g_neg.astype(dt), pos_side=a)


def step(c, ent, es, rel, rs, bt, known=None):
    """forward + backward + the reference's update order (entity trace 0, entity trace 1, relation trace), tables in place"""
    out = forward_backward(c, ent, rel, bt, known)
    O.adagrad_update(ent, es, bt["nid"], out["g_pos_ent"], c["lr"])
    O.adagrad_update(ent, es, bt["neg"], out["g_neg"], c["lr"])
    O.adagrad_update(rel, rs, bt["r"], out["g_rel"], c["lr"])
    return out


# --------------------------------------------------------------------------------------------------------------------------
# 1. the per-op entries.  Widths: 4 (one quaternion, scalar packs), 36 (q = 9: scalar packs; a multiple of 4, so the matrix-core
#    route serves it), 32 and 48 (vector packs), 1040 (q = 260: 65 packs of 4 - the pack loop of the edge kernels runs a second round)
# --------------------------------------------------------------------------------------------------------------------------
OP_WIDTHS = (4, 36, 32, 48, 1040)
OP_SHAPES = ((2, 8, 24), (1, 16, 130))           # (C, chunk, N)
OP_FLAGS = (0, FORCE_PAIRWISE)


def vector_packs(d_e):
    """the edge kernels' instance: 16-byte packs when every quarter is a whole number of them"""
    return (d_e // 4) % 4 == 0


def neg_route(d_e, flags):
    """the kernels kge_score_neg_fwd / _bwd reach (kge_api.hip use_mfma; kge_neg_pair.hip: the bcast kernels where d_e % 16 == 0)"""
    if d_e % 4 == 0 and not (flags & FORCE_PAIRWISE):
        return "gemm"
    return "bcast" if d_e % 16 == 0 else "pair32"


def op_inputs(d_e, C, chunk, N, neg_head):
    """float32 x [B, d_e] (the uncorrupted side), y [B, d_e] (the other entity of the positive), r [B, d_e], nb [C * N, d_e],
    W [C, chunk, N] and dp [B] (random signed upstream gradients).  Edge 0's first relation quaternion is all zero."""
    rng = np.random.RandomState(_seed("quate-op", d_e, C, chunk, N, bool(neg_head)))
    B = C * chunk
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    inp = dict(x=u(B, d_e), y=u(B, d_e), r=u(B, d_e), nb=u(C * N, d_e), W=u(C, chunk, N), dp=u(B))
    inp["r"][0, ::d_e // 4] = 0.0
    return inp


def op_reference(inp, C, chunk, N, neg_head, dtype=np.float64):
    x, y, r, nb, W, dp = (inp[k].astype(dtype) for k in ("x", "y", "r", "nb", "W", "dp"))
    h, t = (y, x) if neg_head else (x, y)
    a = pos_side(neg_head, x, r)
    ga, gn = score_neg_bwd(a, nb, W, C, chunk, N)
    gx, gr = pos_side_bwd(neg_head, x, r, ga)
    gh, grp, gt = score_bwd(h, r, t, dp)
    return dict(pos=score(h, r, t), gh=gh, grp=grp, gt=gt, score=score_neg(a, nb, C, chunk, N), gx=gx, gr=gr, gn=gn)


# --------------------------------------------------------------------------------------------------------------------------
# 2. the fused step: B = 16, chunk = 8, N = 24 on 40 entities and 5 relations - entities and relations repeat inside a batch, so
#    the owner-computes update walks lists longer than one (asserted by the CPU file)
# --------------------------------------------------------------------------------------------------------------------------
STEP_B, STEP_CHUNK, STEP_N, STEP_ENT, STEP_REL = 16, 8, 24, 40, 5
STEP_WIDTHS = (32, 36)


def step_case(cid, genre="Logsigmoid", adv=False, adv_temp=1.0, pairwise=False, margin=1.0, reg_coef=0.0, reg_norm=3, neg_deg=False,
              impts=False, lr=0.1):
    return dict(id=cid, genre=genre, adv=adv, adv_temp=adv_temp, pairwise=pairwise, margin=margin, reg_coef=reg_coef,
                reg_norm=reg_norm, neg_deg=neg_deg, impts=impts, lr=lr, B=STEP_B, chunk=STEP_CHUNK, N=STEP_N, n_ent=STEP_ENT,
                n_rel=STEP_REL)


# regulariser coefficients: the loss gradient is O(1 / B) per element and d/dx coef |x|^q = coef q |x|^(q - 1) with |x| <= 1 - at
# these values the regulariser is a few per cent of the largest gradient component (asserted by the CPU file)
STEP_CASES = [
    step_case("logsigmoid-adv", adv=True),
    step_case("hinge-pw", "Hinge", pairwise=True),
    step_case("bce", "BCE"),
    step_case("softmax", SM.GENRE),
    step_case("neg-deg", adv=True, neg_deg=True),
    step_case("impts", adv=True, impts=True),
    step_case("reg2", adv=True, reg_coef=2e-3, reg_norm=2),
    step_case("reg3", adv=True, reg_coef=2e-3, reg_norm=3),
]


def step_tables(d_e):
    rng = np.random.RandomState(_seed("quate-step-tables", d_e))
    return (rng.uniform(-1, 1, (STEP_ENT, d_e)).astype(np.float32), rng.uniform(-1, 1, (STEP_REL, d_e)).astype(np.float32))


def step_batches(c, steps=2):
    """tail then head corruption (oracle.kge_oracle.synth_batch); w: edge importance or None"""
    rng = np.random.RandomState(_seed("quate-step-batch", c["id"]))
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
# 3. exact ties: integer-grid tables.  Entity components in {-3 .. 3}; every relation quaternion one of (+-s, 0, 0, 0), (0, +-s, 0, 0),
#    (0, 0, +-s, 0), (0, 0, 0, +-s), (+-s, +-s, +-s, +-s) with s in {1, 2, 4}: every norm is s or 2 s, a power of two, so r^ has
#    components in {0, +-1, +-1/2} exactly and every score is a small multiple of 1/2 - exact in float32 in any summation order.
# --------------------------------------------------------------------------------------------------------------------------
TIE_SIZES = (7, 130)            # entities = relations = candidates of a case
TIE_WIDTHS = (8, 32)
TIE_CASES = [(n, d) for n in TIE_SIZES for d in TIE_WIDTHS]
TIE_E = 40                      # test triples
TIE_SEEDS = {(7, 8): 0, (7, 32): 0, (130, 8): 0, (130, 32): 0}      # (asserted to give the ties the tests need: test_quate_inputs.py)
TIE_CHUNK = 16                  # chunked_ranks: two chunks of 16 and one of 8
# several tiles, as pairre_cases.TIE_WIDE_CASES (width 36: quarter 9, scalar packs; integer entries stay exact at any width)
TIE_WIDE_CASES = [(300, 32), (300, 36)]
TIE_WIDE_E = 150
TIE_WIDE_CHUNK = 100
TIE_SEEDS.update({(300, 32, TIE_WIDE_E): 0, (300, 36, TIE_WIDE_E): 0})


class Case(object):
    pass


def grid_relations(rng, n, d_e):
    q = d_e // 4
    out = np.zeros((n, 4, q), np.float32)
    kind = rng.randint(0, 5, (n, q))
    s = np.array([1.0, 2.0, 4.0], np.float32)[rng.randint(0, 3, (n, q))]
    sign = np.where(rng.randint(0, 2, (n, 4, q)) == 1, np.float32(1), np.float32(-1))
    for c in range(4):
        out[:, c, :] = np.where((kind == c) | (kind == 4), sign[:, c, :] * s, 0)
    return out.reshape(n, d_e)


def tie_scores(c, h, r, t, neg_head, dtype=np.float64):
    """(p [E], S [E, n_ent]) in `dtype`: the positive scores and the scores of every entity in the corrupted slot"""
    ent, rel = c.ent.astype(dtype), c.rel.astype(dtype)
    a = pos_side(neg_head, ent[t if neg_head else h], rel[r])
    return score(ent[h], rel[r], ent[t]), a @ ent.T


def rel_tie_scores(c, h, r, t, dtype=np.float64):
    """(p [E], S [E, n_rel]): S[i, j] = s(h_i, j, t_i)"""
    ent, rel = c.ent.astype(dtype), c.rel.astype(dtype)
    S = rel_query(ent[h], ent[t]) @ unit(rel).T
    return S[np.arange(len(h)), r].copy(), S


@functools.lru_cache(maxsize=None)
def tie_inputs(n, d_e, E=None):
    """tables, E (default: TIE_E, read at the call) test triples - the first half picked from a pool for a candidate other than the
    own entity that ties the positive score on the tail side, the head side or the relation side, in turn - and known triples: the test triples and, for
    the first 12 of them and every side, one planted triple whose corrupted entity (relation) TIES the positive where there is one"""
    key = (n, d_e) if E is None else (n, d_e, E)
    E = TIE_E if E is None else E
    rng = np.random.RandomState(_seed("quate-tie", n, d_e, TIE_SEEDS[key]))
    c = Case()
    c.n, c.d_e = n, d_e
    c.ent = rng.randint(-3, 4, (n, d_e)).astype(np.float32)
    c.rel = grid_relations(rng, n, d_e)
    P = 600
    ph, pr, pt = rng.randint(0, n, P), rng.randint(0, n, P), rng.randint(0, n, P)
    tied = []
    for side in ("tail", "head", "rel"):
        if side == "rel":
            p, S = rel_tie_scores(c, ph, pr, pt)
            own = pr
        else:
            p, S = tie_scores(c, ph, pr, pt, side == "head")
            own = ph if side == "head" else pt
        m = S == p[:, None]
        m[np.arange(P), own] = False
        tied.append(m.any(1))
    pick, k = [], 0
    while len(pick) < E // 2 and k < 3 * P:
        i = k // 3
        if tied[k % 3][i] and i not in pick:
            pick.append(i)
        k += 1
    rest = [i for i in range(P) if i not in pick][:E - len(pick)]
    idx = rng.permutation(np.array(pick + rest))
    c.h, c.r, c.t = ph[idx].copy(), pr[idx].copy(), pt[idx].copy()
    extra = []
    for side in ("tail", "head", "rel"):
        if side == "rel":
            p, S = rel_tie_scores(c, c.h, c.r, c.t)
            own = c.r
        else:
            p, S = tie_scores(c, c.h, c.r, c.t, side == "head")
            own = c.h if side == "head" else c.t
        for i in range(12):
            cols = np.nonzero((S[i] == p[i]) & (np.arange(S.shape[1]) != own[i]))[0]
            if len(cols):
                e = int(cols[len(cols) // 2])
                extra.append({"tail": (c.h[i], c.r[i], e), "head": (e, c.r[i], c.t[i]), "rel": (c.h[i], e, c.t[i])}[side])
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


def relation_lists(c, filtered):
    """per test triple the relation ids that do not count: its own, and filtered every j for which (h, j, t) is known"""
    lists = []
    for i in range(len(c.h)):
        own = np.array([c.r[i]], np.int64)
        lists.append(np.union1d(c.kr[(c.kh == c.h[i]) & (c.kt == c.t[i])], own).astype(np.int64) if filtered else own)
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


def f32_scores_three_orders(c, h, r, t, neg_head):
    """the [E, n] scores evaluated in float32 in three summation orders: numpy's matrix product, a forward loop over the columns
    of the row and a backward loop"""
    ent, rel = c.ent, c.rel
    a = pos_side(neg_head, ent[t if neg_head else h], rel[r]).astype(np.float32)
    assert a.dtype == np.float32
    s0 = a @ ent.T
    s1 = np.zeros_like(s0)
    s2 = np.zeros_like(s0)
    for k in range(c.d_e):
        s1 += a[:, k:k + 1] * ent[None, :, k]
        s2 += a[:, c.d_e - 1 - k:c.d_e - k] * ent[None, :, c.d_e - 1 - k]
    return s0, s1, s2


# --------------------------------------------------------------------------------------------------------------------------
# 4. the interface: 40 entities, 6 relations, 16 wide; float64 top-K with ties by position
# --------------------------------------------------------------------------------------------------------------------------
IF_ENT, IF_REL, IF_D, IF_K = 40, 6, 16, 5


def interface_tables():
    rng = np.random.RandomState(_seed("quate-interface"))
    return rng.uniform(-1, 1, (IF_ENT, IF_D)).astype(np.float32), rng.uniform(-1, 1, (IF_REL, IF_D)).astype(np.float32)


def all_scores(ent, rel):
    """[n_ent, n_rel, n_ent] float64 scores of every triple"""
    e, r = ent.astype(np.float64), rel.astype(np.float64)
    hr = hamilton(e[:, None, :], unit(r)[None, :, :])
    return np.einsum("hrk,tk->hrt", hr, e)
