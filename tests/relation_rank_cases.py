"""Shared inputs and expected ranks of the relation-ranking tests (test_relation_rank_inputs.py on the CPU,
test_gpu_relation_rank.py on the device): seeded tables, 90 test triples out of 3000 known ones over 60 entities, the relation
lists of every test triple, and rank bounds from an fp64 score matrix.

The protocol (include/kge_hip.h, kge_rank_rel_eval; the reference has no relation ranking): test triple i = (h, r, t) is ranked
against all n_rel relations,
    rank_i = 1 + #{j : j not in list_i, s(h, j, t) >= s(h, r, t)},
list_i = {r} (raw) or {r} united with the relations j for which (h, j, t) is a known triple (filtered).  The own relation never
counts.  S[i, j] comes from oracle.kge_oracle.score_pos on (ent[h_i], rel[j], ent[t_i]) in fp64 (TransR, which score_pos does not
take: gamma - |(h - t) P_j + c_j|_1 in numpy).  An fp32 score within TOL of the positive score may fall on either side of `>=`,
so the bar is lo <= rank <= hi with lo / hi the counts at >= p + TOL and >= p - TOL over the columns that count (TOL = 1e-4, the
project's tolerance on fp32 scores, as in chunked_eval_cases.py), and equality wherever lo == hi.

Sixty entities make (head, tail) pairs repeat among the 3000 known triples, so the filtered lists carry extra relations."""
import functools

import numpy as np

from oracle import kge_oracle as O

TOL = 1e-4
N_ENT, N_KNOWN, E = 60, 3000, 90
N_RELS = (7, 130)        # fewer columns than one 16-wide MFMA block; a list crossing the 128-column tile
EB = 64                  # the second batch is a ragged 26 rows

# (model, hidden, d_e override): the small widths of every model; the recipes' 400; 100 (off the 32-wide k stage); RotatE 200;
# 30 (not a multiple of 4: the scalar / pairwise route); RESCAL 12 (d^2 = 144, off the stage); TransR with d_e != d_r
SHAPES = [("TransE_l1", 32, None), ("TransE_l2", 32, None), ("DistMult", 32, None), ("ComplEx", 16, None), ("RotatE", 16, None),
          ("SimplE", 16, None), ("RESCAL", 8, None), ("TransR", 16, None), ("TransE_l2", 400, None), ("DistMult", 100, None),
          ("RotatE", 200, None), ("DistMult", 30, None), ("RESCAL", 12, None), ("TransR", 16, 24)]
CASES = [(m, hd, de, n) for (m, hd, de) in SHAPES for n in N_RELS]
CASE_IDS = ["%s_h%d%s_r%d" % (m, hd, "_de%d" % de if de else "", n) for (m, hd, de, n) in CASES]
# the models with both routes (fp32-MFMA tiles / pairwise score block); the others have one
TWO_ROUTES = ("TransE_l2", "DistMult", "ComplEx", "SimplE", "RESCAL")


def dims(model, hidden, de=None):
    if model in ("ComplEx", "SimplE"):
        return 2 * hidden, 2 * hidden
    if model == "RotatE":
        return 2 * hidden, hidden
    if model == "RESCAL":
        return hidden, hidden * hidden
    return (de or hidden), hidden


class Case(object):
    pass


@functools.lru_cache(maxsize=None)
def inputs(model, hidden, de, n_rel):
    """known triples with uniform ids (the first 90 are the test triples), then tables uniform(-1, 1) in float32 (TransR's
    projection x 0.3); gamma = 8, emb_init = (gamma + 2) / hidden"""
    rng = np.random.RandomState(5)
    c = Case()
    c.model, c.hidden, c.n_rel = model, hidden, n_rel
    c.kh, c.kr, c.kt = rng.randint(0, N_ENT, N_KNOWN), rng.randint(0, n_rel, N_KNOWN), rng.randint(0, N_ENT, N_KNOWN)
    c.h, c.r, c.t = c.kh[:E].copy(), c.kr[:E].copy(), c.kt[:E].copy()
    c.d_e, c.d_r = dims(model, hidden, de)
    c.ent = rng.uniform(-1, 1, (N_ENT, c.d_e)).astype(np.float32)
    c.rel = rng.uniform(-1, 1, (n_rel, c.d_r)).astype(np.float32)
    c.proj = (rng.uniform(-1, 1, (n_rel, c.d_e * c.d_r)) * 0.3).astype(np.float32) if model == "TransR" else None
    c.gamma = 8.0
    c.emb_init = (c.gamma + 2.0) / hidden
    for x in (c.kh, c.kr, c.kt, c.h, c.r, c.t, c.ent, c.rel) + ((c.proj,) if c.proj is not None else ()):
        x.setflags(write=False)
    return c


def score_matrix(c, dtype, rel=None):
    """S [E, n_rel] in `dtype`: S[i, j] = s(h_i, j, t_i).  rel: another relation table in the place of c.rel."""
    ent = c.ent.astype(dtype)
    rel = (c.rel if rel is None else rel).astype(dtype)
    hh, tt = ent[c.h], ent[c.t]
    S = np.empty((E, rel.shape[0]), dtype)
    if c.model == "TransR":
        u = hh - tt
        for j in range(rel.shape[0]):
            P = c.proj[j].astype(dtype).reshape(c.d_e, c.d_r)
            S[:, j] = dtype(c.gamma) - np.abs(u @ P + rel[j]).sum(-1)
        return S
    for j in range(rel.shape[0]):
        S[:, j] = O.score_pos(c.model, hh, np.broadcast_to(rel[j], (E, rel.shape[1])), tt, dtype(c.gamma), c.emb_init)
    return S


@functools.lru_cache(maxsize=None)
def oracle_scores(model, hidden, de, n_rel):
    """(p [E], S [E, n_rel]) in fp64; computed once per case, never modified"""
    c = inputs(model, hidden, de, n_rel)
    S = score_matrix(c, np.float64)
    p = S[np.arange(E), c.r].copy()
    S.setflags(write=False)
    p.setflags(write=False)
    return p, S


@functools.lru_cache(maxsize=None)
def relation_lists(n_rel, filtered):
    """per test triple the ascending unique relation ids that do not count, as (ranges [E, 2], ids) - built here independently
    of eval.build_relation_filter (the ids of the triples do not depend on the model)"""
    c = inputs("DistMult", 32, None, n_rel)
    lists = []
    for i in range(E):
        own = np.array([c.r[i]], np.int64)
        if filtered:
            m = (c.kh == c.h[i]) & (c.kt == c.t[i])
            lists.append(np.union1d(c.kr[m], own).astype(np.int64))
        else:
            lists.append(own)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    rng, ids = np.stack([ptr[:-1], ptr[1:]], 1), np.concatenate(lists).astype(np.int64)
    rng.setflags(write=False)
    ids.setflags(write=False)
    return rng, ids


def bounds(c, S, p, filtered):
    """(lo, hi) of every test triple from a score matrix S and positive scores p"""
    frng, fids = relation_lists(c.n_rel, filtered)
    lo, hi = np.zeros(E, np.int64), np.zeros(E, np.int64)
    for i in range(E):
        keep = np.ones(S.shape[1], bool)
        keep[fids[frng[i, 0]:frng[i, 1]]] = False
        lo[i] = 1 + int((keep & (S[i] >= p[i] + TOL)).sum())
        hi[i] = 1 + int((keep & (S[i] >= p[i] - TOL)).sum())
    return lo, hi


def expected(model, hidden, de, n_rel, filtered):
    """(lo, hi, p): the rank bounds and fp64 positive scores of a case"""
    c = inputs(model, hidden, de, n_rel)
    p, S = oracle_scores(model, hidden, de, n_rel)
    lo, hi = bounds(c, S, p, filtered)
    return lo, hi, p


def ranks_of(c, S, p, filtered):
    """the protocol applied to a score matrix as it stands (the fp32 evaluation of the CPU guard)"""
    frng, fids = relation_lists(c.n_rel, filtered)
    out = np.zeros(E, np.int64)
    for i in range(E):
        keep = np.ones(S.shape[1], bool)
        keep[fids[frng[i, 0]:frng[i, 1]]] = False
        out[i] = 1 + int((keep & (S[i] >= p[i])).sum())
    return out
