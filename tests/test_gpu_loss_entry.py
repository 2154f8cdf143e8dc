"""kge_loss_fwd_bwd alone (LossGenerator.get_total_loss and its gradient, models/pytorch/loss.py:69-98) against the float64
oracle on the SAME float32 scores: every instance boundary of launch_loss (kge_rowwise.hip: one / two / four / eight score
columns per lane, the generic kernel above 512), batches below and above KGE_ACC_SLOTS, the four genres, -adv with adversarial
temperatures 0.5 / 1 / 2, edge importance, the pairwise forms - on scores that put every criterion in both regimes:
saturated rows (|s| up to 40: the loss stays finite, the gradients match) and, for Hinge, scores exactly on the kink
(n = -margin, p = margin, pairwise p - n = margin: the reference zeroes only loss < 0, so the gradient at v == 0 is kept).

The expectation follows the exact value of BCE on saturated scores (softplus), not the -100 log clamp of torch's BCELoss
('BCE on saturated scores')."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from oracle import kge_oracle as O
from test_gpu_parity import DEV, _close, grad_tol

pytestmark = pytest.mark.gpu


def _acc_slots():
    """KGE_ACC_SLOTS as the kernels see it (include/kge_hip.h, included by kge_common.hpp)"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define\s+KGE_ACC_SLOTS\s+(\d+)", open(os.path.join(root, "include", "kge_hip.h")).read())
    return int(m.group(1))


ACC_SLOTS = _acc_slots()
NS = [1, 4, 63, 64, 65, 128, 129, 256, 257, 512, 513, 700]          # launch_loss: <= 64 | <= 128 | <= 256 | <= 512 | generic
BS = [37, ACC_SLOTS + 5]


def _configs(full):
    """(genre, adv, adv_temp, pairwise, margin, weighted)"""
    out = []
    for genre in O.LOSSES:
        margins = (1.0, 2.0) if genre == "Hinge" else (1.0,)
        for margin in margins:
            for weighted in (False, True):
                for adv, T in ((False, 1.0), (True, 0.5), (True, 1.0), (True, 2.0)):
                    out.append((genre, adv, T, False, margin, weighted))
                if genre in ("Hinge", "Logistic"):
                    out.append((genre, False, 1.0, True, margin, weighted))
    if not full:
        # the large batch: every genre, every temperature, the pairwise forms and edge importance once each (the arithmetic per
        # row does not depend on B; what changes above KGE_ACC_SLOTS is the grid and the slot a row's sums go to)
        keep = {("Logsigmoid", True, 2.0, False, 1.0, True), ("Logistic", False, 1.0, False, 1.0, False),
                ("Logistic", False, 1.0, True, 1.0, True), ("Hinge", True, 0.5, False, 1.0, True),
                ("Hinge", False, 1.0, True, 2.0, False), ("Hinge", False, 1.0, False, 2.0, False),
                ("BCE", True, 1.0, False, 1.0, True), ("BCE", False, 1.0, False, 1.0, False)}
        out = [c for c in out if c in keep]
        assert len(out) == len(keep)
    return out


def _scores(rng, B, N, margin):
    """float32 scores: N(0, 3) body (both sides of every kink, the sigmoid's bend), rows 0-3 saturated (uniform in +-40, row 0 at
    the ends), row 5's negatives exactly at -margin, positive 6 exactly at margin, row 7 with p - n = margin for every n."""
    pos = (rng.randn(B) * 3).astype(np.float32)
    neg = (rng.randn(B, N) * 3).astype(np.float32)
    neg[0:4] = rng.uniform(-40, 40, size=(4, N)).astype(np.float32)
    pos[0:4] = np.float32([40.0, -40.0, 37.5, -33.25])
    neg[0, ::2] = 40.0
    neg[0, 1::2] = -40.0
    neg[5, :] = -margin
    pos[6] = margin
    pos[7] = 0.5
    neg[7, :] = 0.5 - margin
    return pos, neg


def _entry(pos, neg, w, genre, adv, T, pairwise, margin):
    from dglke_amd import _lib
    B, N = neg.shape
    p, n = torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV)
    wt = torch.from_numpy(w).to(DEV) if w is not None else None
    loss3 = torch.full((3,), float("nan"), device=DEV)
    dpos, dneg = torch.full_like(p, float("nan")), torch.full_like(n, float("nan"))
    wsb = (2 * B + 64) * 4 + 1024
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().kge_loss_fwd_bwd(_lib.LOSS_IDS[genre], int(adv), float(T), int(pairwise), float(margin), _lib.ptr(p),
                                           _lib.ptr(n), _lib.ptr(wt) if wt is not None else None, B, N, _lib.ptr(loss3),
                                           _lib.ptr(dpos), _lib.ptr(dneg), _lib.ptr(ws), wsb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return loss3.cpu().numpy(), dpos.cpu().numpy(), dneg.cpu().numpy()


@pytest.mark.parametrize("B", BS, ids=lambda b: "B%d" % b)
@pytest.mark.parametrize("N", NS, ids=lambda n: "N%d" % n)
def test_loss_entry_matches_float64_oracle(N, B):
    assert BS[0] < ACC_SLOTS < BS[1]
    rng = np.random.RandomState(100 * N + (B % 97))
    w_all = rng.uniform(0.5, 1.5, size=B).astype(np.float32)
    for genre, adv, T, pairwise, margin, weighted in _configs(full=B < ACC_SLOTS):
        pos, neg = _scores(rng, B, N, margin)
        w = w_all if weighted else None
        tag = "B%d N%d %s adv=%s T=%g pairwise=%s margin=%g w=%s" % (B, N, genre, adv, T, pairwise, margin, weighted)
        loss3, dpos, dneg = _entry(pos, neg, w, genre, adv, T, pairwise, margin)
        (pl, nl, loss), dp64, dn64 = O.loss_fwd_bwd(pos.astype(np.float64), neg.astype(np.float64),
                                                    None if w is None else w.astype(np.float64), genre, adv, T, pairwise, margin)
        assert np.isfinite(loss) and np.isfinite(dp64).all() and np.isfinite(dn64).all(), tag + ": the float64 expectation is not finite"
        if pairwise:
            assert np.isnan(loss3[0]) and np.isnan(loss3[1]), tag + ": the pairwise loss has no positive / negative part"
            _close(loss3[2], loss, 1e-4, 1e-5, tag + " loss")
            # the one discontinuity: a pair whose float32 p - n rounds onto the kink from the inactive side keeps its gradient in
            # float32 and has none in float64.  Found from the two activity masks, capped, excluded element-wise.
            act32 = (np.float32(margin) - (pos[:, None] - neg)) >= 0
            act64 = (margin - (pos.astype(np.float64)[:, None] - neg.astype(np.float64))) >= 0
            flip = act32 != act64
            assert flip.sum() <= 1e-4 * flip.size, tag + ": %d hinge flips" % flip.sum()
            if genre == "Hinge" and flip.any():
                dneg = np.where(flip, dn64, dneg)
                dpos = np.where(flip.any(1), dp64, dpos)
        else:
            _close(loss3, [pl, nl, loss], 1e-4, 1e-5, tag + " loss3")
        _close(dpos, dp64, 3e-4, grad_tol(dp64), tag + " dpos")
        _close(dneg, dn64, 3e-4, grad_tol(dn64), tag + " dneg")
        if genre == "Hinge":
            # v == 0 keeps its gradient (loss.py zeroes only loss < 0): the rows placed exactly on the kink
            if pairwise:
                assert np.all(dneg[7] > 0) and dpos[7] < 0, tag + ": pairwise hinge lost its gradient at p - n == margin"
                np.testing.assert_allclose(dneg[7], dn64[7], rtol=3e-4, atol=0, err_msg=tag)
            else:
                assert np.all(dneg[5] > 0), tag + ": hinge lost the negative-side gradient at n == -margin"
                assert dpos[6] < 0, tag + ": hinge lost the positive-side gradient at p == margin"
                assert dn64[5].min() > 0 and dp64[6] < 0          # (the oracle keeps it too: pinned to the reference by the goldens)


def test_loss_entry_rejects_illegal_combinations():
    from dglke_amd import _lib
    pos, neg = np.zeros(4, np.float32), np.zeros((4, 3), np.float32)
    with pytest.raises(_lib.KgeError):
        _entry(pos, neg, None, "Hinge", True, 1.0, True, 1.0)          # pairwise and adversarial
    with pytest.raises(_lib.KgeError):
        _entry(pos, neg, None, "BCE", False, 1.0, True, 1.0)           # BCE has no pairwise form (loss.py:58-61)
