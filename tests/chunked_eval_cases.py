"""Shared inputs and expected ranks of the chunked-candidate ranking tests (test_chunked_eval_inputs.py on the CPU,
test_gpu_chunked_eval.py on the device): seeded tables, 90 test triples out of 4000 known ones, per-chunk candidate lists, and the
oracle's rank bounds.

Expected ranks come from oracle.kge_oracle.rank_eval's fp64 score matrix S, taken at the candidates' columns.  An fp32 score
within TOL of the positive score may fall on either side of `>=`, so the bar is lo <= rank <= hi with lo / hi the counts at
>= p + TOL and >= p - TOL (TOL = 1e-4: BASELINE.json's tolerance on fp32 scores, as in test_gpu_eval.py).

Free columns: a candidate column - other than the triple's own prepended column - that holds the triple's own true entity
scores exactly the positive score, a coin flip in fp32.  Unfiltered lists drawn with replacement have some; they widen hi - lo
by one each.  A ranking is AMBIGUOUS when hi - lo exceeds its free columns, and is compared exactly only when it is not
ambiguous and has no free column (lo == hi)."""
import functools

import numpy as np

from oracle import kge_oracle as O

TOL = 1e-4
N_ENT, N_REL, N_KNOWN, E = 300, 7, 4000, 90

# (model, hidden): the small widths of every model, the recipes' 400 and 100 (off the 32-wide k stage) for the two GEMM families
CASES = [("TransE_l1", 32), ("TransE_l2", 32), ("DistMult", 32), ("ComplEx", 16), ("RotatE", 16), ("SimplE", 16), ("RESCAL", 8),
         ("TransR", 16), ("TransE_l2", 400), ("DistMult", 400), ("TransE_l2", 100), ("DistMult", 100)]
CASE_IDS = ["%s_h%d" % c for c in CASES]
TRANSLATIONAL = ("TransE_l1", "TransE_l2", "RotatE")

# (chunk, n_cand): a ragged last chunk of 18; per-triple lists crossing a 128-candidate boundary; the default chunk; one chunk
# against all 300 entities
CONFIGS = [(24, 40), (1, 130), (8, 40), (90, None)]
SELF_CONFIGS = [(24, 40), (8, None)]


def dims(model, hidden):
    if model in ("ComplEx", "SimplE"):
        return 2 * hidden, 2 * hidden
    if model == "RotatE":
        return 2 * hidden, hidden
    if model == "RESCAL":
        return hidden, hidden * hidden
    return hidden, hidden


class Case(object):
    pass


@functools.lru_cache(maxsize=None)
def inputs(model, hidden):
    """tables uniform(-1, 1) (TransR's projection x 0.3), known triples with uniform ids, the first 90 as test triples.  gamma is
    8, except for the translational models: the median positive distance, so that positive scores of both signs occur (the zeroed
    own column of --neg_deg_sample_eval is then seen counting and not counting); RotatE's phase depends on emb_init =
    (gamma + 2) / hidden, so its median is taken again after gamma changed."""
    rng = np.random.RandomState(5)
    c = Case()
    c.model, c.hidden = model, hidden
    c.kh, c.kr, c.kt = rng.randint(0, N_ENT, N_KNOWN), rng.randint(0, N_REL, N_KNOWN), rng.randint(0, N_ENT, N_KNOWN)
    c.h, c.r, c.t = c.kh[:E].copy(), c.kr[:E].copy(), c.kt[:E].copy()
    d_e, d_r = dims(model, hidden)
    c.ent = rng.uniform(-1, 1, (N_ENT, d_e)).astype(np.float32)
    c.rel = rng.uniform(-1, 1, (N_REL, d_r)).astype(np.float32)
    c.proj = (rng.uniform(-1, 1, (N_REL, d_e * d_r)) * 0.3).astype(np.float32) if model == "TransR" else None
    c.ent64, c.rel64 = c.ent.astype(np.float64), c.rel.astype(np.float64)
    c.proj64 = c.proj.astype(np.float64) if c.proj is not None else None
    c.gamma = 8.0
    if model in TRANSLATIONAL:
        for _ in range(3 if model == "RotatE" else 1):
            p0 = O.score_pos(model, c.ent64[c.h], c.rel64[c.r], c.ent64[c.t], 0.0, (c.gamma + 2.0) / hidden)
            c.gamma = float(np.float32(np.median(-p0)))
    c.emb_init = (c.gamma + 2.0) / hidden
    return c


@functools.lru_cache(maxsize=None)
def oracle_scores(model, hidden, neg_head):
    """(p [E], S [E, n_ent]) in fp64; computed once per case and side, never modified"""
    c = inputs(model, hidden)
    _, p, S = O.rank_eval(model, c.ent64, c.rel64, c.h, c.r, c.t, neg_head, c.gamma, c.emb_init, proj=c.proj64)
    p, S = np.asarray(p, np.float64), np.asarray(S, np.float64)
    p.setflags(write=False)
    S.setflags(write=False)
    return p, S


@functools.lru_cache(maxsize=None)
def candidates(chunk, n_cand, n_triples=E):
    """[n_chunks, n_cand] ids drawn with replacement (repeats, and the triples' own entities among them), three slots per list -1"""
    if n_cand is None:
        return None
    n_chunks = (n_triples + chunk - 1) // chunk
    rng = np.random.RandomState(1000 * chunk + n_cand)
    cand = rng.randint(0, N_ENT, (n_chunks, n_cand)).astype(np.int64)
    for k in range(n_chunks):
        cand[k, rng.choice(n_cand, 3, replace=False)] = -1
    cand.setflags(write=False)
    return cand


@functools.lru_cache(maxsize=None)
def filter_lists(model, hidden, neg_head):
    """per test triple the ascending unique entity ids whose corruption is a known triple, as (ranges [E, 2], ids) - the layout of
    eval.build_filter, built here independently of it"""
    c = inputs(model, hidden)
    lists = []
    for i in range(E):
        if neg_head:
            m = (c.kt == c.t[i]) & (c.kr == c.r[i])
            lists.append(np.unique(c.kh[m]))
        else:
            m = (c.kh == c.h[i]) & (c.kr == c.r[i])
            lists.append(np.unique(c.kt[m]))
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return np.stack([ptr[:-1], ptr[1:]], 1), np.concatenate(lists).astype(np.int64)


def expected(model, hidden, neg_head, chunk, cand, filtered=False, self_cand=False, own="zero"):
    """(lo, hi, free, p): rank bounds and free-column counts of every test triple.  cand: [n_chunks, n] / None (all entities).
    own (self_cand only): "zero" = the triple's own prepended column scores 0.0 (the protocol); "always" / "never": it counts
    always / never (the two wrong behaviours the GPU test tells apart from the right one)."""
    c = inputs(model, hidden)
    p, S = oracle_scores(model, hidden, neg_head)
    frng, fids = filter_lists(model, hidden, neg_head)
    side = c.h if neg_head else c.t
    lo, hi, free = (np.zeros(E, np.int64) for _ in range(3))
    for i in range(E):
        k = i // chunk
        ids = cand[k] if cand is not None else np.arange(N_ENT)
        ids = ids[ids >= 0]
        s = S[i, ids]
        keep = np.ones(len(ids), bool)
        if filtered:
            keep = ~np.isin(ids, fids[frng[i, 0]:frng[i, 1]])
        is_true = ids == side[i]
        if self_cand:
            own_ids = side[k * chunk:min(E, (k + 1) * chunk)]
            so = S[i, own_ids].copy()
            ko = np.ones(len(own_ids), bool)
            to = own_ids == side[i]
            me = i - k * chunk
            to[me] = False
            if own == "zero":
                so[me] = 0.0
            elif own == "always":
                so[me] = np.inf
            else:
                ko[me] = False
            s, keep, is_true = np.concatenate([so, s]), np.concatenate([ko, keep]), np.concatenate([to, is_true])
        lo[i] = 1 + int((keep & (s >= p[i] + TOL)).sum())
        hi[i] = 1 + int((keep & (s >= p[i] - TOL)).sum())
        free[i] = int((keep & is_true).sum())
    return lo, hi, free, p
