"""CPU guard of test_gpu_chunked_eval.py (oracle only): the shared inputs of chunked_eval_cases.py pin almost every ranking, so the
GPU test cannot hide a wrong kernel behind its tolerance band, and the --neg_deg_sample_eval cases exercise the zeroed own column
both ways."""
import numpy as np
import pytest

import chunked_eval_cases as CC


@pytest.mark.parametrize("model,hidden", CC.CASES, ids=CC.CASE_IDS)
def test_few_rankings_are_ambiguous(model, hidden):
    """per case and (chunk, candidates) configuration: at most 10 % of the rankings (both sides) have a band wider than their free
    columns explain - filtered and raw, and with the own entities prepended.  Measured with these inputs: at most 11 of 180 (6.1 %),
    filtered and raw alike, and 7 of 90 (7.8 %) with own entities - both TransE_l2 at width 400 against all 300 entities, where the
    distances crowd around their mean.  10 % is no room for a wrong kernel."""
    for chunk, n_cand in CC.CONFIGS:
        cand = CC.candidates(chunk, n_cand)
        for filtered in (True, False):
            amb = tot = 0
            for neg_head in (False, True):
                lo, hi, free, _ = CC.expected(model, hidden, neg_head, chunk, cand, filtered=filtered)
                if filtered:
                    assert free.sum() == 0                # the true entity is in its own filter list
                amb += int((hi - lo > free).sum())
                tot += len(lo)
            assert amb <= 0.10 * tot, (chunk, n_cand, filtered, amb, tot)
    for chunk, n_cand in CC.SELF_CONFIGS:
        cand = CC.candidates(chunk, n_cand)
        for neg_head in (False, True):
            lo, hi, free, _ = CC.expected(model, hidden, neg_head, chunk, cand, self_cand=True)
            amb = int((hi - lo > free).sum())
            assert amb <= 0.10 * len(lo), (chunk, n_cand, neg_head, amb)


@pytest.mark.parametrize("model,hidden", CC.CASES, ids=CC.CASE_IDS)
def test_own_column_is_seen_counting_and_not_counting(model, hidden):
    """the zeroed own column counts iff 0 >= p: no positive score within 10 TOL of 0, and both signs among the 90 triples - and
    among the pinned rankings (lo == hi) of each side the right rank differs from `own column always counts` for a positive p and
    from `never counts` for a negative one.  (Against all entities every list holds the triple's true entity, a free column, so
    nearly all pinned rankings come from the sampled lists: the two configurations are taken together.)"""
    for neg_head in (False, True):
        p, _ = CC.oracle_scores(model, hidden, neg_head)
        assert np.abs(p).min() > 10 * CC.TOL
        assert (p > 0).any() and (p < 0).any(), ((p > 0).sum(), (p < 0).sum())
        seen_pos = seen_neg = 0
        for chunk, n_cand in CC.SELF_CONFIGS:
            cand = CC.candidates(chunk, n_cand)
            lo, hi, free, _ = CC.expected(model, hidden, neg_head, chunk, cand, self_cand=True)
            always = CC.expected(model, hidden, neg_head, chunk, cand, self_cand=True, own="always")[0]
            never = CC.expected(model, hidden, neg_head, chunk, cand, self_cand=True, own="never")[0]
            exact = lo == hi
            seen_pos += int((lo[exact & (p > 0)] != always[exact & (p > 0)]).sum())
            seen_neg += int((lo[exact & (p < 0)] != never[exact & (p < 0)]).sum())
        assert seen_pos > 0 and seen_neg > 0, (neg_head, seen_pos, seen_neg)


def test_inputs_have_the_shapes_the_gpu_test_relies_on():
    assert CC.candidates(24, 40).shape == (4, 40) and CC.E % 24 == 18          # ragged last chunk
    c = CC.candidates(1, 130)
    assert c.shape == (90, 130) and np.all((c < 0).sum(1) == 3)                # three empty slots per list
    assert any(len(np.unique(row[row >= 0])) < (row >= 0).sum() for row in CC.candidates(8, 40))      # repeats
    inp = CC.inputs("TransE_l2", 32)
    hit = sum(int(np.isin(inp.t[k * 24:(k + 1) * 24], CC.candidates(24, 40)[k]).sum()) for k in range(4))
    assert hit > 0                                                             # a triple's own entity among its candidates
    frng, fids = CC.filter_lists("TransE_l2", 32, False)
    for i in range(CC.E):
        ids = fids[frng[i, 0]:frng[i, 1]]
        assert inp.t[i] in ids and np.all(np.diff(ids) > 0)
