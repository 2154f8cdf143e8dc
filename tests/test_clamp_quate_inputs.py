"""The float64 statement of clamp_quate_cases.py checked on its own: the SimplE cases exercise the clamp on both sides and keep every
raw score decidably away from the bound, and the stated gradients are the central differences of the stated loss."""
import numpy as np
import pytest

import clamp_quate_cases as Q

SIMPLE = [c for c in Q.CASES if c.model == 'SimplE']


def _raw(c):
    tables, (hi, ri, ti, w), known = Q.inputs(c)
    return Q.forward(c, tables[0].astype(np.float64), tables[2].astype(np.float64), hi, ri, ti, np.ones(c.B), known)[5:]


@pytest.mark.parametrize("c", SIMPLE, ids=lambda c: c.name)
def test_simple_cases_reach_both_bounds_and_keep_the_margin(c):
    R, rp = _raw(c)
    assert (R < -Q.CLAMP).any() and (np.abs(R) < Q.CLAMP).any() and (R > Q.CLAMP).any()
    assert np.abs(np.abs(R) - Q.CLAMP).min() > Q.MARGIN and np.abs(np.abs(rp) - Q.CLAMP).min() > Q.MARGIN


def test_a_clamped_positive_occurs():
    assert any((np.abs(_raw(c)[1]) > Q.CLAMP).any() for c in SIMPLE)


@pytest.mark.parametrize("model,crit,neg_head", [(m, k, s) for m in ('SimplE', 'QuatE') for k in ('ova', 'kva') for s in (False, True)])
def test_stated_gradients_are_central_differences(model, crit, neg_head):      # (tiny shape; SimplE: saturated scores, none near the bound)
    c = Q._c(model, crit, neg_head, 9, 3, 8, 'weights')
    tables, (hi, ri, ti, w), known = Q.inputs(c)
    ent, rel, w = tables[0].astype(np.float64), tables[2].astype(np.float64), w.astype(np.float64)
    _, _, a, g, dp, R, _ = Q.forward(c, ent, rel, hi, ri, ti, w, known)
    assert model != 'SimplE' or ((np.abs(R) > Q.CLAMP).any() and (np.abs(R) < Q.CLAMP).any())
    y = ent[hi if neg_head else ti]
    _, gx, gr = Q.edge(model, neg_head, ent[hi], rel[ri], ent[ti], g @ ent + dp[:, None] * y)
    G_ent, G_rel = g.T @ a, np.zeros_like(rel)
    np.add.at(G_ent, ti if neg_head else hi, gx)
    np.add.at(G_ent, hi if neg_head else ti, dp[:, None] * a)
    np.add.at(G_rel, ri, gr)
    rng, h = np.random.RandomState(1), 1e-6
    for X, G in ((ent, G_ent), (rel, G_rel)):
        for _ in range(12):
            i, j = rng.randint(X.shape[0]), rng.randint(X.shape[1])
            keep, L = X[i, j], []
            for d in (h, -h):
                X[i, j] = keep + d
                L.append(Q.forward(c, ent, rel, hi, ri, ti, w, known)[0])
            X[i, j] = keep
            assert abs((L[0] - L[1]) / (2 * h) - G[i, j]) <= 1e-6 * max(1.0, abs(G[i, j])), (i, j, (L[0] - L[1]) / (2 * h), G[i, j])
