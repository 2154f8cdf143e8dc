"""Input guard of the per-op C-ABI tests (CPU): every case of tests/modular_op_cases.py through the oracle in float32 and in
float64.  Asserted from the reference alone, before any GPU run:
  * the float32 oracle (the reference's own formulation and precision) meets the suite's tolerances against the float64 oracle
    at every case - so a kernel that misses them is wrong, not the bound.  The one exception is measured here: the planted
    coincident pair of TransE_l2, whose float32 |a|^2 + |b|^2 - 2 a.b distance is cancellation noise;
  * the rows excluded for TransE_l1's sign(a - b) and at the edge of SimplE's clamp stay under ROW_CAP of every compared array;
  * the clamp cases put 1 - 50 % of their pairs into the clamp, the plain SimplE cases none;
  * the torch float64 formulas the GPU file evaluates on the device equal the oracle's;
  * the inputs of the small ops hold what their tests claim (duplicates, exact ties, masked candidates, exact zeros).
"""
import numpy as np
import pytest

import modular_op_cases as M
from loss_option_cases import ROW_CAP
from oracle import kge_oracle as O


def _distinct(cases):
    """one case per set of inputs: the kernel-path flags do not change the reference"""
    seen, out = set(), []
    for c in cases:
        k = (c["model"], c["C"], c["chunk"], c["N"], c["d_e"], c["kind"])
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def check_neg_case(c):
    for neg_head in (False, True):
        tag = "%s neg_head=%d" % (c["id"], neg_head)
        inp = M.neg_inputs(c, neg_head)
        grads = not c["fwd_only"]
        r64 = M.oracle_neg(c, neg_head, inp, np.float64, grads)
        r32 = M.oracle_neg(c, neg_head, inp, np.float32, grads)
        assert r32["score"].dtype == np.float32 and r64["score"].dtype == np.float64
        assert all(np.isfinite(v).all() for v in list(r32.values()) + list(r64.values())), tag
        slots, edges = M.neg_exclusions(c, neg_head, inp)
        M.check_neg_caps(c, slots, edges, tag)
        if c["model"] == "SimplE":
            share = M.clamp_stats(c, M.simple_raw(c, neg_head, inp))[0]
            if c["kind"] == "clamp":
                assert 0.01 <= share <= 0.5, "%s: %.3f of the pairs are clamped" % (tag, share)
                hit = np.abs(M.simple_raw(c, neg_head, inp)) > M.CLAMP + M.CLAMP_BAND
                assert (np.abs(r64["score"][hit]) == M.CLAMP).all()
                W = inp["W"].astype(np.float64)          # ... and a clamped pair carries no gradient: the rows of a chunk whose
                for ci in range(c["C"]):                 # every pair is clamped would be zero - checked on the pair level instead:
                    a = O.pos_side("SimplE", neg_head, inp["x"].astype(np.float64), inp["r"].astype(np.float64))
                    g_a, _ = O.score_neg_bwd("SimplE", a[ci * c["chunk"]:(ci + 1) * c["chunk"]], inp["nb"][ci * c["N"]:(ci + 1) * c["N"]].astype(np.float64),
                                             (W[ci] * hit[ci])[None], 1, c["chunk"], c["N"], c["gamma"])
                    assert not g_a.any(), tag + ": the oracle lets a clamped pair carry gradient"
            else:
                assert share == 0.0, "%s: a plain SimplE case reaches the clamp" % tag
        errs = M.neg_errors(c, r32, r64, slots, edges, ref32=r32 if c["kind"] == "coincident" else None)
        for k, (ratio, err, _) in errs.items():
            assert ratio <= 1.0, "%s %s: the float32 oracle is %.2f bounds (%.3e) from the float64 oracle" % (tag, k, ratio, err)
        if c["kind"] == "coincident":
            ci, i, j = M.COINCIDENT
            a64 = O.pos_side(c["model"], neg_head, inp["x"].astype(np.float64), inp["r"].astype(np.float64))
            assert np.array_equal(a64[ci * c["chunk"] + i], inp["nb"][ci * c["N"] + j].astype(np.float64)), tag + ": the pair does not coincide"
            assert r64["score"][ci, i, j] == pytest.approx(c["gamma"], abs=1e-12)
    return errs


@pytest.mark.parametrize("c", _distinct(M.NEG_CASES), ids=lambda c: c["id"])
def test_score_neg_case_inputs_stay_inside_the_caps_and_tolerances(c):
    check_neg_case(c)


@pytest.mark.parametrize("seed", range(M.FUZZ_N))
def test_score_neg_fuzz_inputs_stay_inside_the_caps_and_tolerances(seed):
    check_neg_case(M.neg_fuzz_case(seed))


def test_score_neg_cases_cover_what_the_issue_lists():
    cs = M.NEG_CASES
    paths = {c["path"] for c in cs}
    for p in ("fwd_gemm+bwd_gemm", "fwd_bcast+bwd_bcast", "fwd_pair32+bwd_pair32", "fwd_bcast+bwd_lc_shared", "fwd_bcast+bwd_bcast_two_pass",
              "fwd_gemm+bwd_bcast_beyond_maxk", "fwd_gemm", "fwd_bcast"):
        assert p in paths, p
    assert {c["model"] for c in cs} == set(M.MODELS)
    for m in M.MODELS:
        mine = [c for c in cs if c["model"] == m]
        assert {0, M.FORCE_PAIRWISE if m in M.MATRIX_MODELS else M.TWO_PASS_PAIR} <= {c["flags"] for c in mine}, m
        assert any(c["chunk"] == 1 for c in mine) and any(c["N"] == 1 for c in mine) and {4, 36, 30, 18} <= {c["d_e"] for c in mine}, m
        assert m == "RESCAL" or any(c["d_e"] == 2048 for c in mine), m
    for m in ("TransE_l2", "DistMult"):
        assert {(8, 2048), (8, 2049), (2049, 8)} <= {(c["chunk"], c["N"]) for c in cs if c["model"] == m and c["d_e"] == 64}
    assert {c["model"] for c in M.NEG_CASES if c["fwd_only"] and c["chunk"] == 64} == {"TransE_l2", "DistMult", "ComplEx", "RotatE"}
    assert {c["model"] for c in M.NEG_CASES if c["fwd_only"] and c["chunk"] == 1000} == {"TransE_l2", "DistMult", "ComplEx"}
    fz = [M.neg_fuzz_case(s) for s in range(24)]
    assert {c["model"] for c in fz} == set(M.MODELS) and len({c["flags"] for c in fz}) == 3 and len({c["path"] for c in fz}) >= 5


@pytest.mark.parametrize("neg_head", [False, True])
@pytest.mark.parametrize("model", M.MODELS)
def test_torch_reference_equals_the_oracle(model, neg_head):
    """the float64 torch formulas of modular_op_cases.torch_neg (what the GPU file evaluates on the device) against the pinned
    oracle, blocks smaller than a chunk included"""
    for kind in ("plain", "clamp"):
        if kind == "clamp" and model != "SimplE":
            continue
        c = M.neg_case(model, 2, 9, 11, 16, scale=M.simple_clamp_scale(16) if kind == "clamp" else 0.7, kind=kind)
        inp = M.neg_inputs(c, neg_head)
        want = M.oracle_neg(c, neg_head, inp, np.float64, elems=3 * 11 * 16)
        got = M.torch_neg(c, neg_head, inp, "cpu", elems=4 * 11 * 16)
        for k in ("score", "gx", "gr", "gn"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-10, atol=1e-11 * max(1.0, np.abs(want[k]).max()), err_msg="%s %s" % (model, k))


# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", M.POS_CASES, ids=lambda c: c["id"])
def test_score_pos_case_inputs_stay_inside_the_caps_and_tolerances(c):
    for B in c["Bs"]:
        tag = "%s B=%d" % (c["id"], B)
        inp = M.pos_inputs(c, B)
        r64, r32 = M.oracle_pos(c, inp, np.float64), M.oracle_pos(c, inp, np.float32)
        edges = M.pos_exclusions(c, inp)
        M.check_row_cap(edges, B, tag)
        if c["model"] == "SimplE":
            share = float((np.abs(M.simple_pos_raw(inp)) > M.CLAMP).mean())
            if c["kind"] != "clamp":
                assert share == 0.0, tag
            elif B >= 1000:
                assert 0.01 <= share <= 0.5, "%s: %.3f of the edges are clamped" % (tag, share)
        ratio, err, _ = M.worst(r32["score"], r64["score"], M.score_bound(r64["score"]))
        assert ratio <= 1.0, "%s score: float32 oracle %.2f bounds (%.3e) off" % (tag, ratio, err)
        for k in ("gh", "gr", "gt"):
            ratio, err, _ = M.worst(M.masked(r32[k], r64[k], edges), r64[k], M.grad_bound(r64[k]))
            assert ratio <= 1.0, "%s %s: float32 oracle %.2f bounds (%.3e) off" % (tag, k, ratio, err)


def test_score_pos_cases_cover_what_the_issue_lists():
    assert {c["model"] for c in M.POS_CASES} == set(M.MODELS)
    for m in M.MODELS:
        mine = [c for c in M.POS_CASES if c["model"] == m]
        assert {4, 36, 30, 18} <= {c["d_e"] for c in mine} and any(set(c["Bs"]) == set(M.POS_B) for c in mine), m
    assert sum(c["kind"] == "clamp" for c in M.POS_CASES) >= 2


# --------------------------------------------------------------------------------------------------------------------------
def test_small_op_inputs_hold_what_their_tests_claim():
    for n, dim in M.PNORM_SHAPES:
        x = M.pnorm_input(n, dim, zeros=True)
        assert (x == 0).any() and (x != 0).any() or x.size == 1
        for p in (1, 2, 3, 4):
            assert not M.pnorm_ref(x, p)[1][x == 0].any()
    for C, chunk, Np in M.MASK_SHAPES:
        x = np.random.RandomState(0).rand(C, chunk, Np).astype(np.float32) + 1.0
        y = M.mask_diag_ref(x, C, chunk, Np)
        assert int((y != x).sum()) == C * min(chunk, Np) and all(y[ci, i, i] == 0 for ci in range(C) for i in range(min(chunk, Np)))
    assert any((C * chunk) % 256 for C, chunk, _ in M.MASK_SHAPES)
    assert {np.sign(chunk - Np) for _, chunk, Np in M.MASK_SHAPES} == {-1, 0, 1}
    for kind, rows, n_idx, dim in M.GATHER_CASES:
        _, idx, g = M.gather_input(kind, rows, n_idx, dim)
        cnt = np.bincount(idx, minlength=rows)
        assert (cnt.max() == 1 and n_idx == 3000) if kind == "distinct" else (rows == 5 and n_idx == 4096 and cnt.min() > 500)
        ref, bound = M.scatter_add_ref(rows, idx, g)
        assert (bound[cnt > 0] > 0).all() and np.abs(ref).max() > 1.0 or kind == "distinct"
    for dim in M.ADAGRAD_DIMS:
        for dup in (False, True):
            _, _, idx, grad = M.adagrad_input(dim, dup)
            cnt = np.bincount(idx)
            assert len(idx) == 3000 and grad.shape == (3000, dim) and ((cnt.max() > 50 and (cnt == 2).any()) if dup else cnt.max() == 1)
    for E, N in M.RANK_SHAPES:
        for wb in (False, True):
            neg, pos, bias = M.rank_input(E, N, wb)
            ranks = M.rank_ref(neg, pos, bias)
            assert (neg == pos[:, None]).any(), "no exact tie"
            assert (neg[0] >= pos[0]).all() and ranks[0] == 1 + (N if bias is None else int((bias[0] != -1).sum()))
            if E > 1:
                assert ranks[-1] == 1 and (neg[1] == pos[1]).all()
                assert bias is None or ((bias == -1) & (neg >= pos[:, None])).any()


def test_dropin_recipe_inputs_stay_inside_the_l1_cap():
    """TransE_l1 at the recipe's shape, both steps of the oracle: the rows fed by a sign-ambiguous element are <= ROW_CAP of every
    array the drop-in test compares"""
    import loss_option_cases as L
    from test_gpu_parity import _l1_ambiguous
    c = L.case("dropin-l1", "l1", reg_coef=dict(M.DROPIN)["l1"])
    ent, rel, _ = L.tables(c)
    e64, r64, es, rs = ent.astype(np.float64), rel.astype(np.float64), np.zeros(len(ent)), np.zeros(len(rel))
    for bt in L.batches(c):
        amb = _l1_ambiguous(bt, e64, r64, c["chunk"], c["N"], tau=M.dropin_l1_tau(e64, r64))
        for what, rows, total in (("g_neg", amb["slots"], len(bt["neg"])), ("g_rel", amb["edges"], c["B"]), ("g_pos_ent", amb["pos_local"], len(bt["nid"])),
                                  ("entity table", amb["ent"], c["n_ent"]), ("relation table", amb["rel"], c["n_rel"])):
            assert len(rows) <= ROW_CAP * total, "%s: %d of %d rows excluded" % (what, len(rows), total)
        L.oracle_step(c, e64, es, r64, rs, None, None, bt)
