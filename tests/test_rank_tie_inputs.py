"""CPU guard of the exact-tie ranking tests: proves that the inputs of rank_tie_cases.py are what test_gpu_rank_ties.py relies on.

  * exactness: fp32 scores summed forward, reversed and in blocks of 4 (an MFMA's k) and 32 (an LDS stage) - TransE_l2 in the direct
    and in the |a|^2 + |b|^2 - 2 a.b form - equal the fp64 scores after a cast, so an fp32 kernel has no rounding to hide behind;
  * discriminating power: ranks counted with `>` instead of `>=` differ on at least half of the triples of every case (on all of a
    collapsed case), so the wrong comparison cannot pass;
  * the saturated, zero-relation, filter-list and candidate-list properties the case table promises.

Equality of scores is numeric (-0.0 == +0.0): the sign of a zero sum does depend on the order, which is the point of the zero_rel
cases - the device must rank the two zeros as equal."""
import numpy as np
import pytest

import rank_tie_cases as T
from oracle import kge_oracle as O

ORDERS = ("forward", "reversed", "blocks4", "blocks32")
EXACT_CASES = [c for c in T.CASES if c[0] != "collapsed"]
EXACT_IDS = ["%s-%s-%d" % c for c in EXACT_CASES]
f32 = np.float32


def _seq(parts):
    acc = parts[0]
    for x in parts[1:]:
        acc = acc + x
    return acc


def _osum(X, order):
    """float32 sum over the last axis of X, one addition at a time in the given order"""
    assert X.dtype == f32
    cols = [X[..., k] for k in range(X.shape[-1])]
    if order == "forward":
        return _seq(cols)
    if order == "reversed":
        return _seq(cols[::-1])
    b = {"blocks4": 4, "blocks32": 32}[order]
    return _seq([_seq(cols[k:k + b]) for k in range(0, len(cols), b)])


def scores32(c, neg_head, order, form="direct"):
    """[E, N_ENT] candidate scores computed in float32 throughout, the k sum in `order` (TransE_l2: also d^2)"""
    ent, rel = c.ent, c.rel
    g = f32(c.gamma)
    if c.model == "TransR":
        P = c.proj[c.r].reshape(T.E, c.d_e, c.d_r)
        x = np.einsum("ab,abc->ac", ent[c.t if neg_head else c.h], P)
        q = x - rel[c.r]
        cp = np.einsum("jd,ide->ije", ent, P)
        assert q.dtype == f32 and cp.dtype == f32
        return g - _osum(np.abs(cp - q[:, None, :]), order), None
    a = O.pos_side(c.model, neg_head, ent[c.t if neg_head else c.h], rel[c.r], c.emb_init)
    assert a.dtype == f32
    if c.model == "TransE_l1":
        return g - _osum(np.abs(a[:, None, :] - ent[None]), order), None
    if c.model == "TransE_l2":
        if form == "direct":
            d2 = _osum((a[:, None, :] - ent[None]) ** 2, order)
        else:
            d2 = (_osum(a * a, order)[:, None] + _osum(ent * ent, order)[None]) - f32(2) * _osum(a[:, None, :] * ent[None], order)
        return g - np.sqrt(np.maximum(d2, f32(1e-30))), d2
    s = _osum(a[:, None, :] * ent[None], order)
    if c.model == "SimplE":
        s = np.clip(f32(0.5) * s, -f32(O.SIMPLE_CLAMP), f32(O.SIMPLE_CLAMP))
    return s, None


@pytest.mark.parametrize("kind,model,d_e", EXACT_CASES, ids=EXACT_IDS)
def test_fp32_scores_equal_fp64_in_every_summation_order(kind, model, d_e):
    c = T.inputs(kind, model, d_e)
    for x in (c.ent, c.rel) + ((c.proj,) if c.proj is not None else ()):
        assert x.dtype == f32 and np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 4
    assert c.gamma == int(c.gamma) and c.gamma >= 1
    for neg_head in (False, True):
        p, S = T.oracle_scores(kind, model, d_e, neg_head)
        p32 = T.pos_scores(c, c.h, c.r, c.t, f32)
        assert p32.dtype == f32
        if model == "TransE_l2":
            d2 = T.l2_d2(c, neg_head)
            assert np.array_equal(d2, np.rint(d2)) and d2.max() < 2 ** 20
            assert np.array_equal(p32, T.pos32(c, p))
            # the reference's form (sqrt(.)^2 of the norms, oracle.kge_oracle.score_neg) is the same score up to fp64 rounding
            _, _, Sref = O.rank_eval(model, c.ent.astype(np.float64), c.rel.astype(np.float64), c.h, c.r, c.t, neg_head, c.gamma,
                                     c.emb_init)
            assert np.abs(Sref - S).max() < 1e-6
        else:
            assert np.array_equal(p32.astype(np.float64), p)
        for order in ORDERS:
            for form in (("direct", "expand") if model == "TransE_l2" else ("direct",)):
                S32, d32 = scores32(c, neg_head, order, form)
                assert S32.dtype == f32
                if model == "TransE_l2":
                    assert np.array_equal(d32.astype(np.float64), d2), (neg_head, order, form)
                    want = f32(c.gamma) - np.sqrt(np.maximum(d2.astype(f32), f32(1e-30)))
                    assert np.array_equal(S32, want)
                    # ... and fp32 ranks the pairs as fp64 does: >= between any candidate and the positive score
                    assert np.array_equal(S32 >= p32[:, None], S >= p[:, None])
                else:
                    assert np.array_equal(S32.astype(np.float64), S), (neg_head, order, form)


@pytest.mark.parametrize("kind,model,d_e", [c for c in T.CASES if c[1] == "TransE_l2"],
                         ids=["%s-%s-%d" % c for c in T.CASES if c[1] == "TransE_l2"])
def test_l2_score_is_injective_on_the_integers_it_meets(kind, model, d_e):
    """gamma - sqrtf(d^2) in IEEE fp32 is strictly decreasing over every integer d^2 up to the largest of the case, and the kernels'
    floor of 1e-30 under the root leaves d^2 = 0 at exactly gamma: equal d^2 <=> equal scores, on either side of the comparison"""
    c = T.inputs(kind, model, d_e)
    top = int(max(T.l2_d2(c, nh).max() for nh in (False, True)))
    s = f32(c.gamma) - np.sqrt(np.arange(top + 1, dtype=f32))
    assert s.dtype == f32 and np.all(np.diff(s) < 0)
    assert f32(c.gamma) - np.sqrt(f32(1e-30)) == f32(c.gamma)


def _all_rank_pairs(kind, model, d_e):
    """(name, >= ranks, > ranks) of every candidate set / filter combination the device test ranks with"""
    c = T.inputs(kind, model, d_e)
    out = []
    for neg_head in (False, True):
        p, S = T.oracle_scores(kind, model, d_e, neg_head)
        filt = T.filter_lists(kind, model, d_e, neg_head)
        sets = [("all", None, None)] + [("list%d" % n, T.cand_list(n), None) for n in T.LIST_LENS] + \
               [("chunk-all", None, T.CHUNK), ("chunk-lists", T.chunk_lists(), T.CHUNK)]
        for name, cand, chunk in sets:
            for f in (None, filt):
                a, b = (T.ranks_of(c, p, S, neg_head, cand, f, chunk, strict=st) for st in (False, True))
                out.append(("%s/%s/%s" % ("head" if neg_head else "tail", name, "filtered" if f else "raw"), a, b))
    return out


@pytest.mark.parametrize("kind,model,d_e", T.CASES, ids=T.CASE_IDS)
def test_a_strict_comparison_changes_at_least_half_of_the_ranks(kind, model, d_e):
    c = T.inputs(kind, model, d_e)
    for name, ge, gt in _all_rank_pairs(kind, model, d_e):
        differ = int((ge != gt).sum())
        print("%s-%s-%d %-28s ranks that differ between >= and >: %3d of %d" % (kind, model, d_e, name, differ, T.E))
        assert np.all(ge >= gt)
        if name.endswith("/all/filtered") or name.endswith("/all/raw"):
            assert differ * 2 >= T.E, name
        if kind == "collapsed":
            assert differ == T.E, name
    if kind != "collapsed":
        return
    # every candidate ties: raw rank 1 + n_cand, filtered rank 1 + n_cand - |filt_i ∩ cand|
    for neg_head in (False, True):
        p, S = T.oracle_scores(kind, model, d_e, neg_head)
        assert np.all(S == p[:, None])
        frng, fids = T.filter_lists(kind, model, d_e, neg_head)
        for cand in (None,) + tuple(T.cand_list(n) for n in T.LIST_LENS):
            ids = np.arange(T.N_ENT) if cand is None else cand
            assert np.all(T.ranks_of(c, p, S, neg_head, cand) == 1 + len(ids))
            hit = np.array([np.isin(ids, fids[frng[i, 0]:frng[i, 1]]).sum() for i in range(T.E)])
            assert np.array_equal(T.ranks_of(c, p, S, neg_head, cand, (frng, fids)), 1 + len(ids) - hit)


@pytest.mark.parametrize("model,d_e", T.SATURATED)
def test_saturated_cases_sit_on_the_clamp(model, d_e):
    for neg_head in (False, True):
        p, S = T.oracle_scores("saturated", model, d_e, neg_head)
        frac = float((np.abs(S) == O.SIMPLE_CLAMP).mean())
        print("saturated-%s-%d %s: clamped pairs %.3f (+20: %.3f, -20: %.3f), clamped positives %d of %d"
              % (model, d_e, "head" if neg_head else "tail", frac, (S == O.SIMPLE_CLAMP).mean(), (S == -O.SIMPLE_CLAMP).mean(),
                 (np.abs(p) == O.SIMPLE_CLAMP).sum(), T.E))
        assert 0.30 <= frac <= 0.95
        assert (S == O.SIMPLE_CLAMP).mean() > 0.1 and (S == -O.SIMPLE_CLAMP).mean() > 0.1
        assert (np.abs(p) == O.SIMPLE_CLAMP).sum() * 2 >= T.E


@pytest.mark.parametrize("model,d_e", T.ZERO_REL)
def test_zero_relation_cases_hold_both_zeros(model, d_e):
    c = T.inputs("zero_rel", model, d_e)
    zero = c.r < 2
    assert zero.sum() * 3 >= T.E and (~zero).sum() * 3 >= T.E
    assert not np.signbit(c.rel[0]).any() and np.signbit(c.rel[1]).all() and not c.rel[:2].any()
    neg = pos = 0
    for neg_head in (False, True):
        p, S = T.oracle_scores("zero_rel", model, d_e, neg_head)
        assert not S[zero].any() and not p[zero].any()              # every score of those triples is a zero: all tie
        for order in ORDERS:
            z = scores32(c, neg_head, order)[0][zero]
            neg, pos = neg + int(np.signbit(z).sum()), pos + int((~np.signbit(z)).sum())
    print("zero_rel-%s-%d: fp32 zero scores with the sign bit set %d, clear %d" % (model, d_e, neg, pos))
    assert neg > 0 and pos > 0


@pytest.mark.parametrize("kind,model,d_e", T.CASES, ids=T.CASE_IDS)
def test_filter_lists_hold_tied_columns(kind, model, d_e):
    c = T.inputs(kind, model, d_e)
    for neg_head in (False, True):
        p, S = T.oracle_scores(kind, model, d_e, neg_head)
        frng, fids = T.filter_lists(kind, model, d_e, neg_head)
        side = c.h if neg_head else c.t
        n = frng[:, 1] - frng[:, 0]
        tied = 0
        for i in range(T.E):
            ids = fids[frng[i, 0]:frng[i, 1]]
            assert side[i] in ids                                   # the test triples are known triples
            assert np.array_equal(ids, np.unique(ids))
            tied += int(((S[i, ids] == p[i]) & (ids != side[i])).any())
        print("%s-%s-%d %s: lists with more than the own entity %d, with a tied entity other than the own %d"
              % (kind, model, d_e, "head" if neg_head else "tail", (n > 1).sum(), tied))
        assert (n > 0).sum() * 4 >= T.E and (n > 1).sum() * 4 >= T.E
        assert tied >= 3


def test_candidate_lists_hold_repeats_and_pads():
    for n in T.LIST_LENS:
        cand = T.cand_list(n)
        assert len(cand) == n and len(np.unique(cand)) < n and cand.min() >= 0 and cand.max() < T.N_ENT
    lists = T.chunk_lists()
    assert lists.shape == ((T.E + T.CHUNK - 1) // T.CHUNK, T.CHUNK_LIST) and T.E % T.CHUNK not in (0, T.CHUNK)
    for row in lists:
        live = row[row >= 0]
        assert (row == -1).sum() == 3 and len(np.unique(live)) < len(live)
    assert T.SHARD_CUTS[0] == 0 and T.SHARD_CUTS[-1] == T.N_ENT and 1 in np.diff(T.SHARD_CUTS) and 0 in np.diff(T.SHARD_CUTS)


@pytest.mark.parametrize("model,d_e", T.GRID, ids=["%s-%d" % c for c in T.GRID])
def test_several_positive_scores_are_exactly_zero(model, d_e):
    """--neg_deg_sample_eval scores the triple's own column exactly 0.0: the grid cases hold positive scores that tie with it, and
    the `>` count differs from the `>=` count on exactly those (and on ties elsewhere)"""
    c = T.inputs("grid", model, d_e)
    for neg_head in (False, True):
        p, S = T.oracle_scores("grid", model, d_e, neg_head)
        assert (p == 0.0).sum() >= 3, (p == 0.0).sum()
        for cand in (None, T.chunk_lists()):
            ge, gt = (T.ranks_of(c, p, S, neg_head, cand, None, T.CHUNK, self_cand=True, strict=st) for st in (False, True))
            assert np.all(ge[p == 0.0] > gt[p == 0.0])


@pytest.mark.parametrize("kind,model,d_e,n_rel", T.REL_CASES, ids=T.REL_CASE_IDS)
def test_relation_ranking_cases(kind, model, d_e, n_rel):
    c = T.rel_inputs(kind, model, d_e, n_rel)
    p, S = T.rel_oracle_scores(kind, model, d_e, n_rel)
    S32 = T.rel_score_matrix(c, f32)
    assert S32.dtype == f32
    if model == "TransE_l2":
        d2 = np.rint((c.gamma - S) ** 2)
        assert np.abs((c.gamma - S) ** 2 - d2).max() < 1e-9
        assert np.array_equal(S32, f32(c.gamma) - np.sqrt(d2.astype(f32)))
        assert np.array_equal(S32 >= S32[np.arange(T.E), c.r][:, None], S >= p[:, None])
        s = f32(c.gamma) - np.sqrt(np.arange(int(d2.max()) + 1, dtype=f32))
        assert np.all(np.diff(s) < 0)
    elif model != "RotatE":
        assert np.array_equal(S32.astype(np.float64), S)
    else:
        assert np.all(S == c.gamma) and np.all(S32 == f32(c.gamma))
    for filtered in (False, True):
        lists = T.relation_lists(kind, model, d_e, n_rel, filtered)
        ge, gt = T.rel_ranks_of(p, S, lists), T.rel_ranks_of(p, S, lists, strict=True)
        n = lists[0][:, 1] - lists[0][:, 0]
        differ = int((ge != gt).sum())
        print("rel %s-%s-%d-r%d %s: ranks that differ between >= and >: %d of %d; lists beyond the own relation %d"
              % (kind, model, d_e, n_rel, "filtered" if filtered else "raw", differ, T.E, (n > 1).sum()))
        if kind == "collapsed":
            assert np.array_equal(ge, 1 + n_rel - n) and np.all(gt == 1)
            assert differ == T.E
        else:
            assert differ * 2 >= T.E
        if filtered:
            assert (n > 1).sum() * 4 >= T.E
