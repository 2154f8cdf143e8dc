"""Shared inputs and expected ranks of the exact-tie ranking tests (test_rank_tie_inputs.py on the CPU, test_gpu_rank_ties.py on
the device): tables on which fp32 arithmetic is EXACT, so that the device's ranks must EQUAL the fp64 ones - no band.

Every table entry is a small integer (the grid), gamma is an integer.  Every intermediate of every score is then an integer (a
half-integer for SimplE) far below 2^24: exact in fp32 under any summation order, FMA contraction or MFMA k-split.  The score range
is a few hundred values against 257 candidates, so candidates that score EXACTLY the positive score are everywhere, and

    rank_i = 1 + #{candidates j that count : S[i, j] >= p[i]}                                   (tolerance 0)

tells `>=` from `>`, a comparison before SimplE's clamp from one after it, and a dropped tied column from a counted one.

Kinds of case (CASES = (kind, model, d_e)):
  grid       random integer tables in {-2 .. 2} (TransR's projection {-1 .. 1}), the seven models other than RotatE.
  collapsed  all entity rows identical and non-zero, all eight models; relations zero for the translational and rotational models
             (RotatE: phase 0, cos = 1, sin = 0 exactly).  Every candidate ties: raw rank 1 + n_cand.
  saturated  SimplE on {-4 .. 4}: most scores exceed the clamp, so they are exactly +20 or -20.
  zero_rel   DistMult / ComplEx / RESCAL; relation rows 0 (all +0.0) and 1 (all -0.0) serve half of the triples, whose scores are all
             +0.0 or -0.0 and tie.  Entity 0 is all positive and entity 1 all negative, so that sums of -0.0 terms exist.

TransE_l2: d^2 = |h + r - t|^2 is an exact integer in the direct form and in |a|^2 + |b|^2 - 2 a.b, so equal d^2 give equal scores
and distinct d^2 distinct ones (test_rank_tie_inputs.py checks both on the fp32 formula).  oracle.kge_oracle.score_neg follows the
reference's batched_l2_dist, whose sqrt(.)^2 of the norms is not exact even in fp64, so the expectation here takes d^2 in the direct
form.  Its score gamma - sqrt(d^2) is irrational in general: `pos32` gives the fp32 value an IEEE evaluation of the two operations
must produce (correctly rounded sqrt, then one subtraction), which is what the device's positive scores are compared with.

gamma: 12, except the translational models' grid cases - there the most frequent positive distance (TransE_l2: its most frequent
integer value), so that several positive scores are exactly 0 and tie with the zeroed own column of --neg_deg_sample_eval.  The test
triples are 130 of 3000 pooled ones, up to 12 of them picked for a positive score of exactly 0.

Shapes: 257 entities (two 128-candidate tiles + one column), 130 triples (a 128-row block + 2), d_e 36 (off the 32-wide k stage),
64, 6 (no multiple of 4: the score-block fallback of flags = 0), RESCAL 8, TransR 8 x 6, 11 relations.

Relation ranking (REL_CASES): 70 and 129 relations (under and over one 128-candidate tile), tables in {-1, 0, 1} - a narrower
score range, since 70 candidates must still tie with most positive scores; `collapsed` there means all relation rows (and TransR's
projections) identical, so every relation ties and rank = 1 + n_rel - |list_i|: the own relation never counts."""
import functools
import zlib

import numpy as np

from oracle import kge_oracle as O

N_ENT, E, N_REL, N_POOL = 257, 130, 11, 3000
N_RELS = (70, 129)
GAMMA = 12.0
TRANSR_DR = 6
TRANSLATIONAL = ("TransE_l1", "TransE_l2", "RotatE", "TransR")

_WIDE = ("TransE_l1", "TransE_l2", "DistMult", "ComplEx", "SimplE")
GRID = [(m, d) for m in _WIDE for d in (36, 64, 6)] + [("RESCAL", 8), ("TransR", 8)]
COLLAPSED = [(m, 36) for m in _WIDE + ("RotatE",)] + [("RESCAL", 8), ("TransR", 8)]
SATURATED = [("SimplE", 36), ("SimplE", 64)]
ZERO_REL = [("DistMult", 36), ("DistMult", 6), ("ComplEx", 36), ("RESCAL", 8)]
CASES = [(k, m, d) for k, lst in (("grid", GRID), ("collapsed", COLLAPSED), ("saturated", SATURATED), ("zero_rel", ZERO_REL))
         for m, d in lst]
CASE_IDS = ["%s-%s-%d" % c for c in CASES]

# relation ranking: (kind, model, d_e, n_rel).  collapsed = all relation rows (and TransR's projections) identical
REL_SHAPES = [(m, 36) for m in _WIDE] + [("DistMult", 6), ("RESCAL", 8), ("TransR", 8)]
REL_CASES = [("grid", m, d, n) for m, d in REL_SHAPES for n in N_RELS] + \
            [("collapsed", m, d, n) for m, d in COLLAPSED for n in N_RELS]
REL_CASE_IDS = ["%s-%s-%d-r%d" % c for c in REL_CASES]

CHUNK = 16               # 130 triples: eight chunks and a last one of 2
LIST_LENS = (70, 257)    # explicit candidate lists of Ranker.ranks (with repeats)
CHUNK_LIST = 40          # per-chunk lists of chunked_ranks (pads and repeats)
SHARD_CUTS = (0, 128, 129, 257, 257)   # kge_rank_eval_split: a full tile, one row, the rest, an empty shard


def dims(model, d_e):
    if model == "RotatE":
        return d_e, d_e // 2
    if model == "RESCAL":
        return d_e, d_e * d_e
    if model == "TransR":
        return d_e, TRANSR_DR
    return d_e, d_e


class Case(object):
    pass


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _grid(rng, shape, amp, nonzero=False):
    vals = np.array([v for v in range(-amp, amp + 1) if v or not nonzero], np.float32)
    return vals[rng.randint(0, len(vals), shape)]


def _freeze(c):
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def pos_scores(c, h, r, t, dtype=np.float64, rel=None, proj=None):
    """the positive scores of the triples (h, r, t) on c's tables in `dtype` (oracle.kge_oracle.score_pos; TransR, which it does
    not take: gamma - |h P_r + c_r - t P_r|_1, score_fun.py:131-166)"""
    ent = c.ent.astype(dtype)
    rel = (c.rel if rel is None else rel).astype(dtype)
    if c.model == "TransR":
        P = (c.proj if proj is None else proj).astype(dtype)[r].reshape(len(r), c.d_e, c.d_r)
        hp, tp = np.einsum("ab,abc->ac", ent[h], P), np.einsum("ab,abc->ac", ent[t], P)
        return dtype(c.gamma) - np.abs(hp + rel[r] - tp).sum(-1)
    return O.score_pos(c.model, ent[h], rel[r], ent[t], dtype(c.gamma), c.emb_init)


def _pick_gamma(c, ph, pr, pt):
    """the translational models' grid cases: the integer gamma at which most pooled positive scores are exactly 0"""
    c.gamma = 0.0
    dist = -pos_scores(c, ph, pr, pt)
    if c.model == "TransE_l2":
        root = np.rint(dist)
        dist = root[(root * root == np.rint(dist * dist)) & (root >= 1)]      # the distances that are integers
    vals, cnt = np.unique(dist[dist >= 1], return_counts=True)
    return float(vals[np.argmax(cnt)])


def _pick_triples(c, rng, ph, pr, pt):
    """130 of the pooled triples: in a grid case up to 12 whose positive score is exactly 0, then the pool's first ones, shuffled"""
    p = pos_scores(c, ph, pr, pt)
    zero = np.nonzero(p == 0.0)[0][:12 if c.kind == "grid" else 0]
    rest = np.setdiff1d(np.arange(N_POOL), zero, assume_unique=True)[:E - len(zero)]
    idx = rng.permutation(np.concatenate([zero, rest]))
    return ph[idx].copy(), pr[idx].copy(), pt[idx].copy()


@functools.lru_cache(maxsize=None)
def _base(kind, model, d_e):
    rng = np.random.RandomState(_seed(kind, model, d_e))
    c = Case()
    c.kind, c.model, c.n_rel = kind, model, N_REL
    c.d_e, c.d_r = dims(model, d_e)
    c.gamma, c.emb_init = GAMMA, 1.0
    amp = 4 if kind == "saturated" else 2
    c.ent = _grid(rng, (N_ENT, c.d_e), amp, nonzero=kind == "zero_rel")
    c.rel = _grid(rng, (N_REL, c.d_r), amp)
    c.proj = _grid(rng, (N_REL, c.d_e * c.d_r), 1) if model == "TransR" else None
    ph, pr, pt = rng.randint(0, N_ENT, N_POOL), rng.randint(0, N_REL, N_POOL), rng.randint(0, N_ENT, N_POOL)
    if kind == "collapsed":
        c.ent = np.tile(_grid(rng, (1, c.d_e), amp, nonzero=True), (N_ENT, 1))
        if model in TRANSLATIONAL:
            c.rel = np.zeros_like(c.rel)
    if kind == "zero_rel":
        c.ent[0], c.ent[1] = np.abs(c.ent[0]), -np.abs(c.ent[1])
        c.rel[0], c.rel[1] = 0.0, -0.0
        half = rng.rand(N_POOL) < 0.5
        pr = np.where(half, rng.randint(0, 2, N_POOL), rng.randint(2, N_REL, N_POOL))
        u = rng.rand(N_POOL)                                      # entity 0 on either side of an eighth of the pool
        ph, pt = np.where(u < 0.125, 0, ph), np.where(u > 0.875, 0, pt)
    if kind == "grid" and model in TRANSLATIONAL:
        c.gamma = _pick_gamma(c, ph, pr, pt)
    c.ph, c.pr, c.pt = ph, pr, pt
    c.h, c.r, c.t = _pick_triples(c, rng, ph, pr, pt)
    return c


def _scores(c, neg_head):
    """(p [E], S [E, N_ENT]) in fp64 from oracle.kge_oracle.rank_eval; TransE_l2's S from d^2 in the direct form (see above)"""
    e64, r64 = c.ent.astype(np.float64), c.rel.astype(np.float64)
    p64 = c.proj.astype(np.float64) if c.proj is not None else None
    _, p, S = O.rank_eval(c.model, e64, r64, c.h, c.r, c.t, neg_head, c.gamma, c.emb_init, proj=p64)
    if c.model == "TransE_l2":
        S = c.gamma - np.sqrt(l2_d2(c, neg_head))
    return np.asarray(p, np.float64), np.asarray(S, np.float64)


def l2_d2(c, neg_head, dtype=np.float64):
    """TransE_l2: [E, N_ENT] squared distances in the direct form"""
    ent, rel = c.ent.astype(dtype), c.rel.astype(dtype)
    a = O.pos_side(c.model, neg_head, ent[c.t if neg_head else c.h], rel[c.r])
    return ((a[:, None, :] - ent[None, :, :]) ** 2).sum(-1)


@functools.lru_cache(maxsize=None)
def inputs(kind, model, d_e):
    """the case: tables, gamma, test triples (h, r, t) and known triples (kh, kr, kt) = the pool, the test triples and, for the
    first 40 test triples and both sides, one planted known triple whose corrupted entity is a candidate that TIES with the
    positive score (so that filter lists hold tied columns)"""
    b = _base(kind, model, d_e)
    c = Case()
    vars(c).update(vars(b))
    extra = []
    for neg_head in (False, True):
        p, S = _scores(b, neg_head)
        for i in range(40):
            own = b.h[i] if neg_head else b.t[i]
            tied = np.nonzero((S[i] == p[i]) & (np.arange(N_ENT) != own))[0]
            if len(tied):
                e = int(tied[len(tied) // 2])
                extra.append((e, b.r[i], b.t[i]) if neg_head else (b.h[i], b.r[i], e))
    extra = np.array(extra, np.int64).reshape(-1, 3)
    c.kh = np.concatenate([b.ph, b.h, extra[:, 0]])
    c.kr = np.concatenate([b.pr, b.r, extra[:, 1]])
    c.kt = np.concatenate([b.pt, b.t, extra[:, 2]])
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def oracle_scores(kind, model, d_e, neg_head):
    """(p [E], S [E, N_ENT]) in fp64; computed once per case and side, never modified"""
    p, S = _scores(_base(kind, model, d_e), neg_head)
    p.setflags(write=False)
    S.setflags(write=False)
    return p, S


def pos32(c, p):
    """the fp32 positive scores an exact device must return for the fp64 scores p: p itself (an integer or half-integer), except
    TransE_l2: gamma - sqrt(d^2) evaluated in IEEE fp32 on the exact integer d^2"""
    if c.model != "TransE_l2":
        return p.astype(np.float32)
    d2 = np.rint((c.gamma - p) ** 2).astype(np.float32)
    return np.float32(c.gamma) - np.sqrt(d2)


@functools.lru_cache(maxsize=None)
def filter_lists(kind, model, d_e, neg_head):
    """per test triple the ascending unique entity ids whose corruption is a known triple, as (ranges [E, 2], ids) - the layout of
    eval.build_filter, built here independently of it"""
    c = inputs(kind, model, d_e)
    lists = []
    for i in range(E):
        if neg_head:
            lists.append(np.unique(c.kh[(c.kt == c.t[i]) & (c.kr == c.r[i])]))
        else:
            lists.append(np.unique(c.kt[(c.kh == c.h[i]) & (c.kr == c.r[i])]))
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    rng, ids = np.stack([ptr[:-1], ptr[1:]], 1), np.concatenate(lists).astype(np.int64)
    rng.setflags(write=False)
    ids.setflags(write=False)
    return rng, ids


@functools.lru_cache(maxsize=None)
def cand_list(n):
    """an explicit candidate list of n entity ids drawn with replacement; the first two slots repeat one id"""
    rng = np.random.RandomState(7000 + n)
    cand = rng.randint(0, N_ENT, n).astype(np.int64)
    cand[1] = cand[0]
    cand.setflags(write=False)
    return cand


@functools.lru_cache(maxsize=None)
def chunk_lists():
    """[n_chunks, CHUNK_LIST] per-chunk candidate ids with replacement; three slots per list are -1 pads, two repeat one id"""
    n_chunks = (E + CHUNK - 1) // CHUNK
    rng = np.random.RandomState(7100)
    cand = rng.randint(0, N_ENT, (n_chunks, CHUNK_LIST)).astype(np.int64)
    for k in range(n_chunks):
        slots = rng.choice(CHUNK_LIST, 5, replace=False)
        cand[k, slots[:3]] = -1
        cand[k, slots[3]] = cand[k, slots[4]]
    cand.setflags(write=False)
    return cand


def ranks_of(c, p, S, neg_head, cand=None, filt=None, chunk=None, self_cand=False, strict=False):
    """[E] int64 ranks by the protocol, tolerance 0: 1 + #{candidates that count : s >= p} (strict: s > p, the wrong comparison
    the CPU guard measures the inputs against).  cand: None (all entities), [n] ids or, with chunk, [n_chunks, n] ids (-1: an
    empty slot); filt: (ranges, entity ids) - every position of a listed id does not count; self_cand: the chunk's own
    corrupted-side entities are prepended and the triple's own column scores exactly 0 (include/kge_hip.h, kge_rank_eval_chunked)."""
    side = c.h if neg_head else c.t
    out = np.zeros(E, np.int64)
    for i in range(E):
        ids = np.arange(N_ENT) if cand is None else (cand if cand.ndim == 1 else cand[i // chunk])
        ids = ids[ids >= 0]
        s = S[i, ids]
        keep = np.ones(len(ids), bool)
        if filt is not None:
            keep = ~np.isin(ids, filt[1][filt[0][i, 0]:filt[0][i, 1]])
        if self_cand:
            k = i // chunk
            own = side[k * chunk:min(E, (k + 1) * chunk)]
            so = S[i, own].copy()
            so[i - k * chunk] = 0.0
            s, keep = np.concatenate([so, s]), np.concatenate([np.ones(len(own), bool), keep])
        out[i] = 1 + int((keep & ((s > p[i]) if strict else (s >= p[i]))).sum())
    return out


def tied_columns(p, S, i, cand=None):
    """the candidate columns of triple i whose score equals its positive score (the failure report of the device test)"""
    ids = np.arange(S.shape[1]) if cand is None else cand
    return np.nonzero((ids >= 0) & (S[i, np.maximum(ids, 0)] == p[i]))[0]


# ---- relation ranking -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rel_base(kind, model, d_e, n_rel):
    rng = np.random.RandomState(_seed("rel", kind, model, d_e, n_rel))
    c = Case()
    c.kind, c.model, c.n_rel = kind, model, n_rel
    c.d_e, c.d_r = dims(model, d_e)
    c.gamma, c.emb_init = GAMMA, 1.0
    c.ent = _grid(rng, (N_ENT, c.d_e), 1)        # {-1, 0, 1}: a narrow score range, so that 70 relations tie often enough
    c.rel = _grid(rng, (n_rel, c.d_r), 1)
    c.proj = _grid(rng, (n_rel, c.d_e * c.d_r), 1) if model == "TransR" else None
    if kind == "collapsed":
        c.rel = np.tile(_grid(rng, (1, c.d_r), 1, nonzero=True), (n_rel, 1))
        if c.proj is not None:
            c.proj = np.tile(c.proj[:1], (n_rel, 1))
        if model == "RotatE":        # a non-zero phase is not exact: phase 0 and identical entity rows, every score = gamma
            c.rel = np.zeros_like(c.rel)
            c.ent = np.tile(c.ent[:1], (N_ENT, 1))
    c.h, c.r, c.t = rng.randint(0, N_ENT, E), rng.randint(0, n_rel, E), rng.randint(0, N_ENT, E)
    return c


def rel_score_matrix(c, dtype=np.float64):
    """S [E, n_rel] in `dtype`: S[i, j] = s(h_i, j, t_i)"""
    S = np.empty((E, c.n_rel), dtype)
    for j in range(c.n_rel):
        S[:, j] = pos_scores(c, c.h, np.full(E, j, np.int64), c.t, dtype)
    return S


@functools.lru_cache(maxsize=None)
def rel_oracle_scores(kind, model, d_e, n_rel):
    c = _rel_base(kind, model, d_e, n_rel)
    S = rel_score_matrix(c)
    p = S[np.arange(E), c.r].copy()
    S.setflags(write=False)
    p.setflags(write=False)
    return p, S


@functools.lru_cache(maxsize=None)
def rel_inputs(kind, model, d_e, n_rel):
    """the relation-ranking case; known triples = the test triples and, for the first 40 of them, (h, j, t) for a relation j that
    ties with the true one (when there is one) and for one random relation"""
    b = _rel_base(kind, model, d_e, n_rel)
    c = Case()
    vars(c).update(vars(b))
    p, S = rel_oracle_scores(kind, model, d_e, n_rel)
    rng = np.random.RandomState(_seed("relknown", kind, model, d_e, n_rel))
    extra = []
    for i in range(40):
        tied = np.nonzero((S[i] == p[i]) & (np.arange(n_rel) != b.r[i]))[0]
        for j in ([int(tied[len(tied) // 2])] if len(tied) else []) + [int(rng.randint(0, n_rel))]:
            extra.append((b.h[i], j, b.t[i]))
    extra = np.array(extra, np.int64).reshape(-1, 3)
    c.kh, c.kr, c.kt = (np.concatenate([x, extra[:, k]]) for k, x in enumerate((b.h, b.r, b.t)))
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def relation_lists(kind, model, d_e, n_rel, filtered):
    """per test triple the ascending unique relation ids that do not count: its own relation, and filtered every relation j for
    which (h, j, t) is known - as (ranges [E, 2], ids), built here independently of eval.build_relation_filter"""
    c = rel_inputs(kind, model, d_e, n_rel)
    lists = []
    for i in range(E):
        own = np.array([c.r[i]], np.int64)
        lists.append(np.union1d(c.kr[(c.kh == c.h[i]) & (c.kt == c.t[i])], own).astype(np.int64) if filtered else own)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    rng, ids = np.stack([ptr[:-1], ptr[1:]], 1), np.concatenate(lists).astype(np.int64)
    rng.setflags(write=False)
    ids.setflags(write=False)
    return rng, ids


def rel_ranks_of(p, S, lists, strict=False):
    """[E] int64: 1 + #{relations j outside list_i : S[i, j] >= p[i]} (strict: >)"""
    out = np.zeros(E, np.int64)
    for i in range(E):
        keep = np.ones(S.shape[1], bool)
        keep[lists[1][lists[0][i, 0]:lists[0][i, 1]]] = False
        out[i] = 1 + int((keep & ((S[i] > p[i]) if strict else (S[i] >= p[i]))).sum())
    return out
