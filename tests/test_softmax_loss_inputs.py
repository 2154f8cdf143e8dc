"""CPU guard of the Softmax loss tests (tests/softmax_loss_cases.py): the float64 statement against torch's cross_entropy and
autograd, every case of the tables does what it is listed for, and the refusals of the genre with -adv / -pw in the C ABI (no
GPU: argument errors are reported before any launch), in LossGenerator and in dglke_train's command line."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import loss_option_cases as L
import softmax_loss_cases as S
from oracle import kge_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib
    return _lib


# --------------------------------------------------------------------------------------------------------------------------
# the statement
# --------------------------------------------------------------------------------------------------------------------------
def _torch_statement(pos, neg, w):
    p = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    n = torch.tensor(neg, dtype=torch.float64, requires_grad=True)
    logits = torch.cat([p[:, None], n], 1)
    l = torch.nn.functional.cross_entropy(logits, torch.zeros(len(pos), dtype=torch.int64), reduction="none")
    wv = torch.ones(len(pos), dtype=torch.float64) if w is None else torch.tensor(w, dtype=torch.float64)
    loss = (wv * l).sum() / len(pos)
    loss.backward()
    return float(loss), p.grad.numpy(), n.grad.numpy()


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("B,N", [(1, 1), (7, 5), (7, 65), (130, 200), (7, 600)])
def test_statement_equals_torch_cross_entropy_and_autograd(B, N, weights):
    pos, neg, w = S.op_inputs(B, N, weights)
    pos, neg = pos.astype(np.float64), neg.astype(np.float64)
    (a, b, loss), dpos, dneg = S.softmax_fwd_bwd(pos, neg, None if w is None else w.astype(np.float64))
    assert np.isnan(a) and np.isnan(b)
    tl, tp, tn = _torch_statement(pos, neg, w)
    assert abs(loss - tl) <= 1e-12 * max(abs(tl), 1.0)
    # dL/dp: torch forms it as softmax - 1, which cancels where the positive dominates: absolute bound at the size of that rounding
    assert np.abs(dpos - tp).max() <= 1e-15 and np.abs(dneg - tn).max() <= 1e-15
    assert np.allclose(dneg, tn, rtol=1e-10, atol=0.0)
    assert np.all(dpos <= 0) and np.all(dneg >= 0)
    # the gradient of a row sums to zero: dL/dp = -sum_j dL/dn_j
    assert np.allclose(dpos, -dneg.sum(1), rtol=1e-12, atol=0.0)


def test_hard_rows_keep_their_digits_in_the_statement():
    """a dominating positive: loss and dL/dp are ~N exp(-60), not 0 and not rounding residue"""
    pos, neg, _ = S.op_inputs(7, 65, False)
    k = S.HARD.index("positive+60")
    (_, _, _), dpos, dneg = S.softmax_fwd_bwd(pos.astype(np.float64), neg.astype(np.float64))
    want = np.exp(neg[k].astype(np.float64) - float(pos[k])).sum() / 7
    assert 0 < -dpos[k] and abs(-dpos[k] / want - 1) < 1e-12 and want < 1e-20
    k = S.HARD.index("negative+60")
    assert abs(dneg[k].sum() * 7 - 1) < 1e-12 and dneg[k, 65 // 2] * 7 >= 1 - 1e-12


def test_hook_sends_only_softmax_to_the_statement(monkeypatch):
    S.hook(monkeypatch)
    rng = np.random.RandomState(0)
    pos, neg = rng.normal(size=6), rng.normal(size=(6, 9))
    for genre, kw in (("Logsigmoid", dict(adv=True)), ("Hinge", dict(pairwise=True)), ("BCE", {})):
        got, want = O.loss_fwd_bwd(pos, neg, None, genre, **kw), S._ORIGINAL(pos, neg, None, genre, **kw)
        assert all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(got[1:], want[1:]))
        assert np.array_equal(np.asarray(got[0], np.float64), np.asarray(want[0], np.float64), equal_nan=True)
    (_, _, loss), _, _ = O.loss_fwd_bwd(pos, neg, None, "Softmax")
    assert loss == S.softmax_fwd_bwd(pos, neg)[0][2]
    with pytest.raises(ValueError):
        S._ORIGINAL(pos, neg, None, "Softmax")                 # without the hook the oracle does not know the genre


# --------------------------------------------------------------------------------------------------------------------------
# the case tables
# --------------------------------------------------------------------------------------------------------------------------
def test_op_shapes_land_on_the_instances_named():
    seen = set()
    for N, aligned, inst in S.OP_SHAPES:
        assert S.loss_instance(N, aligned) == inst, (N, aligned)
        seen.add(inst)
    assert seen == {"strided NPER 1", "strided NPER 2", "strided NPER 4", "strided NPER 8", "one pack", "two packs", "streaming"}
    for B in S.OP_B:
        for N, _, _ in S.OP_SHAPES:
            pos, neg, w = S.op_inputs(B, N, True)
            assert pos.shape == (B,) and neg.shape == (B, N) and w.shape == (B,)
            assert B == 1 or np.ptp(w) > 0.3, "constant weights"
            assert np.isfinite(pos).all() and np.isfinite(neg).all()
    # the six hard rows are all walked at B = 1 too
    assert {S.HARD[i % len(S.HARD)] for i in range(len(S.OP_SHAPES))} == set(S.HARD)


@pytest.mark.parametrize("c", S.STEP_CASES, ids=lambda c: c["id"])
def test_step_case_does_what_it_is_listed_for(c, monkeypatch):
    S.hook(monkeypatch)
    assert c["genre"] == "Softmax" and not c["adv"] and not c["pairwise"]
    assert S.loss_instance(S.step_N(c), True) == S.STEP_INSTANCE[c["shape"]]
    ent, rel, proj = L.tables(c)
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    p64 = None if proj is None else proj.astype(np.float64)
    es, rs = np.zeros(len(ent)), np.zeros(len(rel))
    ps = None if proj is None else np.zeros(len(proj))
    bts = L.batches(c)
    if c["impts"]:
        assert all(np.ptp(bt["w"]) > 0.5 for bt in bts), "constant weights"
    for step, bt in enumerate(bts, 1):            # before the first step, and after it
        ent0, rel0 = e64.copy(), r64.copy()
        out = L.oracle_step(c, e64, es, r64, rs, p64, ps, bt)
        pos, neg = out["pos_score"], out["neg_score"].reshape(c["B"], -1)
        assert neg.shape[1] == S.step_N(c)
        if c["neg_deg"]:        # the diagonal sits inside the row, at score 0
            i = np.arange(c["B"])
            assert np.all(neg[i, i % c["chunk"]] == 0.0) and np.count_nonzero(neg == 0.0) == c["B"]
        share, gmax = S.row_stats(pos, neg)
        assert share >= 0.25, "%s step %d: a negative leads in %.0f %% of the rows only" % (c["id"], step, 100 * share)
        assert gmax >= 0.05, "%s step %d: the positive dominates every row (largest dL/dn * B = %.3g)" % (c["id"], step, gmax)
        assert np.isnan(out["log"][0]) and np.isnan(out["log"][1]) and np.isfinite(out["log"][2]) and out["log"][2] > 0
        if c["reg_coef"] > 0:
            assert L.reg_share(c, out, ent0, rel0, bt) >= 0.01, "the regulariser does not show in the gradients"
    assert any(c["reg_coef"] > 0 for c in S.STEP_CASES)


@pytest.mark.parametrize("cid", S.KNOWN_IDS)
def test_known_cases_keep_negatives_in_the_lead(cid, monkeypatch):
    import known_negative_cases as KN
    S.hook(monkeypatch)
    c = S.known_case(cid)
    bts, K, _ = KN.build(c)
    ent, rel, proj = L.tables(c)
    for bt in bts:
        known = KN.known_matrix(K, bt, c["chunk"], c["N"])
        out = KN.masked_forward_backward(c, ent.astype(np.float64), rel.astype(np.float64), None, bt, known)
        neg = out["neg_score"].reshape(c["B"], -1)
        assert np.all(out["dneg"][known] == 0.0) and known[0].all() and not known[1].any()
        assert out["log"][2] > 0 and np.isnan(out["log"][0])
        rows = ~known.all(1)
        share, gmax = S.row_stats(out["pos_score"][rows], neg[rows])
        assert share >= 0.25 and gmax >= 0.05
        # row 0: every column known - the row's loss is log(1 + 0) = 0 and its positive gets no gradient, exactly
        (_, _, _), dpos, _ = S.softmax_fwd_bwd(out["pos_score"], neg)
        assert dpos[0] == 0.0


# --------------------------------------------------------------------------------------------------------------------------
# the refusals
# --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_softmax_with_adv_or_pairwise_without_a_gpu():
    lib = _lib()
    h = lib.lib()
    assert lib.LOSS_IDS["Softmax"] == S.GENRE_ID and h.kge_abi_version() == 8
    one = 1                                                       # (a non-NULL pointer that is never dereferenced)

    def loss(genre, adv, pw):
        return h.kge_loss_fwd_bwd(genre, adv, 1.0, pw, 1.0, None, None, None, 4, 3, None, None, None, None, 0, None)

    hp, tb, b = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch()
    hp.model, hp.d_e, hp.d_r = lib.MODEL_IDS["DistMult"], 8, 8
    b.B, b.C, b.chunk, b.N = 4, 1, 4, 3

    def step(genre, adv, pw):
        hp.loss_genre, hp.adv, hp.pairwise = genre, adv, pw
        return h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20, None)

    for call in (loss, step):
        assert call(4, 1, 0) == -1 and b"Softmax" in h.kge_last_error() and b"adversarial" in h.kge_last_error()
        assert call(4, 0, 1) == -1 and b"Softmax" in h.kge_last_error() and b"pairwise" in h.kge_last_error()
        assert call(5, 0, 0) == -1 and b"unknown loss genre 5" in h.kge_last_error()
        assert call(-1, 0, 0) == -1 and b"unknown loss genre" in h.kge_last_error()
        # accepted: the next check speaks (null score arrays / null tables)
        assert call(4, 0, 0) == -1 and b"Softmax" not in h.kge_last_error() and b"genre" not in h.kge_last_error()
        assert call(2, 0, 1) == -1 and b"genre" not in h.kge_last_error() and b"pairwise" not in h.kge_last_error()


def test_loss_generator_and_cli_refuse_the_same_combinations(tmp_path):
    _lib()
    from dglke_amd import train as T
    from dglke_amd._lib import KgeError
    from dglke_amd.loss import LossGenerator
    g = LossGenerator(None, "Softmax")
    assert g.loss_genre == "Softmax" and not g.pairwise and not g.neg_adversarial_sampling
    with pytest.raises(ValueError, match="Softmax loss cannot be adversarial sampled"):
        LossGenerator(None, "Softmax", neg_adversarial_sampling=True)
    with pytest.raises(ValueError, match="Softmax loss cannot be applied to pairwise loss function"):
        LossGenerator(None, "Softmax", pairwise=True)
    with pytest.raises(ValueError, match="not support"):
        LossGenerator(None, "softmax")
    base = ["--model_name", "DistMult", "--dataset", "toy", "--data_path", str(tmp_path / "none"), "--save_path", str(tmp_path / "ckpts"),
            "--gpu", "0", "--loss_genre", "Softmax"]
    assert T.ArgParser().parse_args(base).loss_genre == "Softmax"
    for flag, word in (("-adv", "-adv"), ("-pw", "-pw")):
        with pytest.raises(KgeError, match="Softmax cannot be combined with " + word):
            T.main(base + [flag])
    assert not os.path.exists(str(tmp_path / "ckpts")), "refused before anything is loaded or created"
    with pytest.raises(SystemExit):
        T.ArgParser().parse_args(base[:-1] + ["softmax"])
