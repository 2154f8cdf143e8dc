"""CPU guard of the relation-ranking case table (relation_rank_cases.py): the bounds must pin almost every ranking, an fp32
evaluation of the same formulas must land inside them, the filtered lists must really carry relations beyond the triples' own,
and most true relations must not already rank first - otherwise the GPU test (test_gpu_relation_rank.py) would show little.
If a changed generator breaks one of these, change the seed, not the bar."""
import numpy as np
import pytest

import relation_rank_cases as RC


@pytest.mark.parametrize("model,hidden,de,n_rel", RC.CASES, ids=RC.CASE_IDS)
def test_bounds_pin_the_rankings_and_fp32_lands_inside(model, hidden, de, n_rel):
    c = RC.inputs(model, hidden, de, n_rel)
    S32 = RC.score_matrix(c, np.float32)
    p32 = S32[np.arange(RC.E), c.r]
    p64, S64 = RC.oracle_scores(model, hidden, de, n_rel)
    print("largest fp32 score error %.2e" % np.abs(S32.astype(np.float64) - S64).max())
    ambiguous = 0
    for filtered in (False, True):
        lo, hi, _ = RC.expected(model, hidden, de, n_rel, filtered)
        ambiguous += int((lo != hi).sum())
        got = RC.ranks_of(c, S32, p32, filtered)
        assert np.all((lo <= got) & (got <= hi)), (filtered, np.nonzero((got < lo) | (got > hi))[0][:8])
        assert (lo > 1).sum() * 2 >= RC.E, (filtered, int((lo > 1).sum()))
    print("ambiguous rankings: %d of %d" % (ambiguous, 2 * RC.E))
    assert ambiguous <= 0.05 * 2 * RC.E, ambiguous


@pytest.mark.parametrize("n_rel", RC.N_RELS)
def test_filtered_lists_carry_relations_beyond_the_own(n_rel):
    c = RC.inputs("DistMult", 32, None, n_rel)
    frng, fids = RC.relation_lists(n_rel, True)
    rrng, rids = RC.relation_lists(n_rel, False)
    assert np.array_equal(rids, c.r) and np.array_equal(rrng[:, 1] - rrng[:, 0], np.ones(RC.E, np.int64))
    extra = 0
    for i in range(RC.E):
        ids = fids[frng[i, 0]:frng[i, 1]]
        assert c.r[i] in ids and np.all(np.diff(ids) > 0)
        extra += len(ids) - 1
    print("listed relations beyond the own: %d" % extra)
    assert extra >= 20, extra
