"""The TuckER statement and case table of tucker_cases.py, without a device: the gradients against central differences, the values
the table must cover, and a float32 restatement whose error is a usable tolerance on every case."""
import numpy as np
import pytest

import tucker_cases as T


@pytest.mark.parametrize("crit", ["ova", "kva"])
@pytest.mark.parametrize("neg_head", [False, True])
def test_gradients_match_central_differences(crit, neg_head):
    c = T._c(crit, neg_head, 9, 5, 4, 4)
    tables, (hi, ri, ti, _), known = T.inputs(c)
    ent, rel, W = (np.array(tables[k], np.float64) for k in (0, 2, 4))
    xi, yi = (ti, hi) if neg_head else (hi, ti)
    x, y, r = ent[xi], ent[yi], rel[ri]
    w = np.ones(c.B)

    def loss(x, y, r, W):                                        # the gathered rows as free variables: the candidates stay fixed
        a = T.operand(neg_head, x, r, W)
        return T.loss_and_g(c, a, (a * y).sum(1), ent, hi, ri, ti, w, known)[0]
    a = T.operand(neg_head, x, r, W)
    _, g, dp = T.loss_and_g(c, a, (a * y).sum(1), ent, hi, ri, ti, w, known)
    u = g @ ent + dp[:, None] * y
    gx, gr, gw = T.edge_grads(neg_head, x, r, W, u)
    for k, (arr, grad) in enumerate(((x, gx), (y, dp[:, None] * a), (r, gr), (W, gw))):
        num = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            args = [x, y, r, W]
            lo, hi_ = arr.copy(), arr.copy()
            lo[idx] -= 1e-6
            hi_[idx] += 1e-6
            args[k] = hi_
            up = loss(*args)
            args[k] = lo
            num[idx] = (up - loss(*args)) / 2e-6
        assert np.abs(num - grad).max() <= 1e-8 + 1e-6 * np.abs(grad).max(), k


def test_the_table_covers_every_listed_value():
    for crit in ("ova", "kva"):
        for neg_head in (False, True):
            cs = [c for c in T.CASES if c.crit == crit and c.neg_head == neg_head]
            assert {c.d_e for c in cs} >= {4, 36, 64, 68, 260} and {c.d_r for c in cs} >= {4, 12, 36}
            assert {c.B for c in cs} >= {16, 128, 136} and {c.n_ent for c in cs} >= {63, 129, 300}
    for kind in ("weights", "dups", "big"):
        assert {c.crit for c in T.CASES if c.kind == kind} == {"ova", "kva"}
    assert all(c.reg_coef > 0 for c in T.CASES if c.kind == "weights")
    parts = {-(-c.d_r // max(1, -(-256 // c.d_e))) for c in T.CASES}      # tk_geom at B <= 256: ceil(256 / d_e) values of l per part
    assert parts >= {1, 2, 5}


@pytest.mark.parametrize("c", T.CASES, ids=lambda c: c.name)
def test_the_float32_restatement_errs_and_stays_finite(c):
    tables, batch, known = T.inputs(c)
    ref, f32 = T.step(c, tables, batch, known), T.step(c, tables, batch, known, np.float32)
    for q, r in ref.items():
        err = np.abs(np.asarray(f32[q], np.float64) - r).max()
        assert np.isfinite(err) and err > 0, q
