"""CPU guard of the PairRE tests (tests/pairre_cases.py): the float64 statement against torch.autograd on the same formulas and its
identities, the sign-ambiguity cap of every case, the cases of the tables do what they are listed for, the integer-grid ranking
inputs are exact in float32 and hold ties, and the refusals - widths and flag combinations on the command lines, dimensions,
workspaces and the closed entries in the C ABI (no GPU: argument errors are reported before any launch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import pairre_cases as Q

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
def _t_unit(x):
    return x / torch.sqrt((x * x).sum(-1, keepdim=True))


@pytest.mark.parametrize("d_e", [2, 6, 36])
@pytest.mark.parametrize("neg_head", [False, True])
def test_statement_gradients_equal_autograd(d_e, neg_head):
    """score, the chunked score and the full adjoint (through the normalisations) in float64, to 1e-10, away from the kinks"""
    C_, chunk, N = 2, 5, 7
    rng = np.random.RandomState(d_e + neg_head)
    u = lambda *s: rng.uniform(-1, 1, s)
    inp = dict(x=u(C_ * chunk, d_e), y=u(C_ * chunk, d_e), r=u(C_ * chunk, 2 * d_e), nb=u(C_ * N, d_e), W=u(C_, chunk, N), dp=u(C_ * chunk))
    ref = Q.op_reference(inp, C_, chunk, N, neg_head)
    assert not ref["amb_e"].any() and not ref["amb_p"].any(), "away from the kinks"
    x, y, r, nb = (torch.tensor(inp[k], dtype=torch.float64, requires_grad=True) for k in ("x", "y", "r", "nb"))
    h, t = (y, x) if neg_head else (x, y)
    pos = Q.GAMMA - (_t_unit(h) * r[:, :d_e] - _t_unit(t) * r[:, d_e:]).abs().sum(-1)
    assert np.abs(pos.detach().numpy() - ref["pos"]).max() < 1e-10
    (pos * torch.tensor(inp["dp"])).sum().backward()
    for got, want in ((h.grad, ref["gh"]), (r.grad, ref["grp"]), (t.grad, ref["gt"])):
        assert np.abs(got.numpy() - want).max() < 1e-10
    for v in (x, y, r):
        v.grad = None
    a, w = (_t_unit(x) * r[:, d_e:], r[:, :d_e]) if neg_head else (_t_unit(x) * r[:, :d_e], r[:, d_e:])
    nu = _t_unit(nb).reshape(C_, 1, N, d_e)
    s = Q.GAMMA - (a.reshape(C_, chunk, 1, d_e) - w.reshape(C_, chunk, 1, d_e) * nu).abs().sum(-1)
    assert np.abs(s.detach().numpy() - ref["score"]).max() < 1e-10
    (s * torch.tensor(inp["W"])).sum().backward()
    for got, want in ((x.grad, ref["gx"]), (r.grad, ref["gr"]), (nb.grad, ref["gn"])):
        assert np.abs(got.numpy() - want).max() < 1e-10


def test_both_chunked_forms_are_the_score_with_the_candidate_substituted():
    rng = np.random.RandomState(5)
    B, N, d = 6, 9, 10
    h, t, nb = (rng.uniform(-1, 1, (k, d)) for k in (B, B, N))
    r = rng.uniform(-1, 1, (B, 2 * d))
    for neg_head in (False, True):
        a, w = Q.pair(neg_head, t if neg_head else h, r)
        S = Q.score_neg(a, w, nb, 1, B, N)[0]
        for j in range(N):
            cand = np.repeat(nb[j:j + 1], B, 0)
            direct = Q.score(cand, r, t) if neg_head else Q.score(h, r, cand)
            assert np.abs(S[:, j] - direct).max() < 1e-12
        # the true entity in the corrupted slot gives the positive score
        own = Q.score_neg(a, w, h if neg_head else t, 1, B, B)[0]
        assert np.abs(np.diag(own) - Q.score(h, r, t)).max() < 1e-12


def test_scores_do_not_change_with_the_scale_of_any_entity_row():
    rng = np.random.RandomState(6)
    B, N, d = 5, 7, 12
    h, t, nb = (rng.uniform(-1, 1, (k, d)) for k in (B, B, N))
    r = rng.uniform(-1, 1, (B, 2 * d))
    sc = lambda k: rng.uniform(0.1, 10.0, (k, 1))
    assert np.abs(Q.score(h * sc(B), r, t * sc(B)) - Q.score(h, r, t)).max() < 1e-12
    a, w = Q.pair(False, h, r)
    a2, w2 = Q.pair(False, h * sc(B), r)
    assert np.abs(Q.score_neg(a2, w2, nb * sc(N), 1, B, N) - Q.score_neg(a, w, nb, 1, B, N)).max() < 1e-12
    assert np.abs(Q.norm(Q.unit(h)) - 1).max() < 1e-12
    # the gradient of a scale-invariant function is orthogonal to the row
    gh, _, gt = Q.score_bwd(h, r, t, np.ones(B))
    assert np.abs((gh * h).sum(-1)).max() < 1e-12 and np.abs((gt * t).sum(-1)).max() < 1e-12


def test_zero_entity_row_scores_through_zero_and_gets_no_gradient():
    inp = Q.op_inputs(6, 2, 5, 33, False)
    assert not inp["x"][1].any() and not inp["y"][2].any() and not inp["nb"][3].any() and inp["x"][0].all()
    for neg_head in (False, True):
        inp = Q.op_inputs(6, 2, 5, 33, neg_head)
        ref = Q.op_reference(inp, 2, 5, 33, neg_head)
        assert all(np.isfinite(v).all() for v in ref.values())
        assert not ref["gx"][1].any() and not ref["gn"][3].any()
        gown, gother = (ref["gt"], ref["gh"]) if neg_head else (ref["gh"], ref["gt"])
        assert not gown[1].any() and not gother[2].any() and gown[0].any()
        x, r = inp["x"].astype(np.float64), inp["r"].astype(np.float64)
        a, w = Q.pair(neg_head, x, r)
        assert not a[1].any(), "x^ = 0 where |x| = 0"
        # ... and the score of edge 1 is gamma - sum |w n^|, of candidate 3 gamma - sum |a|
        s = ref["score"]
        nu = Q.unit(inp["nb"].astype(np.float64))
        assert abs(s[0, 1, 0] - (Q.GAMMA - np.abs(w[1] * nu[0]).sum())) < 1e-12 and abs(s[0, 0, 3] - (Q.GAMMA - np.abs(a[0]).sum())) < 1e-12
    # in the step the zero row's gradient is the regulariser's alone: a zero row has none
    c = dict(Q.STEP_CASES[-1])
    ent, rel = (x.astype(np.float64) for x in Q.step_tables(32))
    bt = Q.step_batches(c)[0]
    ent[bt["nid"][0]] = 0.0
    out = Q.forward_backward(c, ent, rel, bt)
    assert not out["g_pos_ent"][0].any() and out["g_pos_ent"][1].any()


# --------------------------------------------------------------------------------------------------------------------------
# the case tables
# --------------------------------------------------------------------------------------------------------------------------
def test_op_cases_cover_the_tile_edges_and_keep_the_ambiguity_cap():
    assert [d % 4 for d in Q.OP_WIDTHS] == [2, 2, 2, 0, 0, 0] and 32 in Q.OP_WIDTHS and 200 in Q.OP_WIDTHS and min(Q.OP_WIDTHS) < 4
    assert any(chunk < 32 < N for _, chunk, N in Q.OP_SHAPES) and any(N < 32 < chunk for _, chunk, N in Q.OP_SHAPES)
    assert (1, 32, 32) in Q.OP_SHAPES and any(C_ > 1 for C_, _, _ in Q.OP_SHAPES)
    worst_loss, worst_tau = 0.0, 0.0
    for d_e in Q.OP_WIDTHS:
        for C_, chunk, N in Q.OP_SHAPES:
            for neg_head in (False, True):
                inp = Q.op_inputs(d_e, C_, chunk, N, neg_head)
                ref = Q.op_reference(inp, C_, chunk, N, neg_head)
                for k in ("amb_e", "amb_n", "amb_p"):
                    lost = ref[k].mean()
                    worst_loss = max(worst_loss, lost)
                    assert lost <= Q.ROW_CAP and not ref[k].all(), "D%d C%d c%d N%d neg_head=%d: %s loses %.1f%% of its rows" % (
                        d_e, C_, chunk, N, neg_head, k, 100 * lost)
                # the float32 evaluation of u stays inside tau
                x32, r32, nb32 = inp["x"], inp["r"], inp["nb"]
                a32, w32 = Q.pair(neg_head, x32, r32)
                assert a32.dtype == np.float32
                u32, _ = Q._diff(a32, w32, nb32, C_, chunk, N)
                a64, w64 = Q.pair(neg_head, x32.astype(np.float64), r32.astype(np.float64))
                worst_tau = max(worst_tau, Q.tau_share(a64, w64, nb32.astype(np.float64), C_, chunk, N, u32.astype(np.float64)))
    assert worst_tau < 0.5, "a float32 numpy evaluation of a - w n^ is off by %.2f tau" % worst_tau


def test_step_cases_do_what_they_are_listed_for():
    _lib()
    from dglke_amd import plan
    ids = [c["id"] for c in Q.STEP_CASES]
    assert len(set(ids)) == len(ids)
    assert {(c["genre"], c["adv"], c["pairwise"]) for c in Q.STEP_CASES} >= {
        ("Logsigmoid", False, False), ("Logsigmoid", True, False), ("Logistic", False, False), ("Hinge", False, False),
        ("Hinge", False, True), ("BCE", False, False), ("Softmax", False, False)}
    assert {c["reg_norm"] for c in Q.STEP_CASES if c["reg_coef"] > 0} == {1, 2, 3}
    assert any(c["neg_deg"] for c in Q.STEP_CASES) and any(c["impts"] for c in Q.STEP_CASES)
    for d_e in Q.STEP_WIDTHS:
        ent, rel = Q.step_tables(d_e)
        assert rel.shape[1] == 2 * d_e
        for c in Q.STEP_CASES:
            bts = Q.step_batches(c)
            assert [bt["neg_head"] for bt in bts] == [False, True], "tail then head corruption"
            for bt in bts:
                p = plan.build_plan(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], bt["w"])
                # owner-computes lists longer than one: an entity with several positive ends and negative slots, a relation with several edges
                assert np.diff(p["ue_pos_ptr"]).max() > 1 and np.diff(p["ue_neg_ptr"]).max() > 1 and np.diff(p["ur_ptr"]).max() > 1
                out = Q.forward_backward(c, ent.astype(np.float64), rel.astype(np.float64), bt)
                assert not out["amb"], "D%d %s: a sign-ambiguous element in a step input" % (d_e, c["id"])
                assert np.isfinite(out["log"][2]) and out["log"][2] > 0
                for k in ("g_pos_ent", "g_neg", "g_rel"):
                    assert np.isfinite(out[k]).all() and np.abs(out[k]).max() > 1e-4, (c["id"], k)
                if c["neg_deg"]:
                    n = out["neg_score"].reshape(c["B"], -1)
                    assert n.shape[1] == c["chunk"] + c["N"] and np.all(n[np.arange(c["B"]), np.arange(c["B"]) % c["chunk"]] == 0.0)
                if c["reg_coef"] > 0:
                    plain = Q.forward_backward(dict(c, reg_coef=0.0), ent.astype(np.float64), rel.astype(np.float64), bt)
                    share = np.abs(out["g_rel"] - plain["g_rel"]).max() / np.abs(out["g_rel"]).max()
                    assert share >= 0.01, "%s: the regulariser does not show in the gradients (%.3g)" % (c["id"], share)
                if c["genre"] == "Hinge" and c["pairwise"]:
                    act = c["margin"] - (out["pos_score"][:, None] - out["neg_score"].reshape(c["B"], -1))
                    assert 0.02 < (act > 0).mean() < 0.98, "the hinge is active for some pairs and not for others"


def test_planted_known_pairs_take_their_columns_out():
    c = Q.STEP_CASES[1]
    ent, rel = Q.step_tables(32)
    for bt in Q.step_batches(c):
        K, known = Q.planted_known(bt, c["chunk"], c["N"])
        assert known[0, 3] and known[c["chunk"], c["N"] - 1] and 2 <= known.sum() < known.size // 4
        out = Q.forward_backward(c, ent.astype(np.float64), rel.astype(np.float64), bt, known)
        plain = Q.forward_backward(c, ent.astype(np.float64), rel.astype(np.float64), bt)
        assert np.all(out["neg_score"].reshape(known.shape)[known] == Q.KNOWN_SCORE)
        assert np.abs(out["g_neg"] - plain["g_neg"]).max() > 1e-6, "the planted pairs carried gradient"


# --------------------------------------------------------------------------------------------------------------------------
# the integer-grid ranking inputs
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d_e", Q.TIE_CASES, ids=["n%d-D%d" % c for c in Q.TIE_CASES])
def test_grid_inputs_are_exact_in_float32_and_hold_ties(n, d_e, wide_e=None, chunk=None):
    c = Q.tie_inputs(n, d_e) if wide_e is None else Q.tie_inputs(n, d_e, wide_e)      # (the several-tile sizes)
    assert np.all((c.ent != 0).sum(1) == 4) and set(np.unique(c.ent).tolist()) == {-1.0, 0.0, 1.0}
    assert np.all(Q.norm(c.ent) == 2.0)
    eu = Q.unit(c.ent)
    assert eu.dtype == np.float32 and set(np.unique(eu).tolist()) == {-0.5, 0.0, 0.5}, "float32 normalisation is exact"
    assert np.array_equal(c.rel, np.rint(c.rel)) and c.rel.min() == -2 and c.rel.max() == 2 and Q.TIE_GAMMA == int(Q.TIE_GAMMA)
    E = len(c.h)
    filt_ties = 0
    for neg_head in (False, True):
        p, S = Q.tie_scores(c, c.h, c.r, c.t, neg_head)
        assert np.array_equal(2 * S, np.rint(2 * S)) and np.abs(S).max() < 2 ** 20, "scores are small multiples of 1/2"
        p32, S32 = Q.tie_scores(c, c.h, c.r, c.t, neg_head, np.float32)
        assert p32.dtype == np.float32 and np.array_equal(p32.astype(np.float64), p) and np.array_equal(S32.astype(np.float64), S)
        for s32 in Q.f32_scores_two_orders(c, c.h, c.r, c.t, neg_head):
            assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), S), "a float32 summation order is not exact"
        own = c.h if neg_head else c.t
        assert np.array_equal(S[np.arange(E), own], p)
        m = S == p[:, None]
        m[np.arange(E), own] = False
        assert m.any(1).sum() * 10 >= E, "fewer than one row in ten has a candidate that ties its positive (neg_head=%d)" % neg_head
        lists = Q.filter_lists(c, neg_head)
        raw, filt = Q.ranks_of(p, S), Q.ranks_of(p, S, lists)
        assert np.any(raw != Q.ranks_of(p, S, strict=True) + 1), "`>=` and `>` must differ by more than the own column"
        for i in range(E):
            ids = lists[1][lists[0][i, 0]:lists[0][i, 1]]
            assert own[i] in ids
            filt_ties += int(((S[i, ids] == p[i]) & (ids != own[i])).sum())
        assert np.all(filt <= raw - 1)
        cand = Q.tie_candidates(n) if wide_e is None else Q.tie_candidates(n, wide_e, chunk)
        assert (cand == -1).sum(1).min() == 2 and cand.max() < n
        listed, selfc = (Q.chunked_ranks_of(c, p, S, neg_head, cand, sc, chunk) for sc in (False, True))
        assert listed.max() > 1 and np.any(selfc != listed)
    assert filt_ties >= 1, "no tie on the filtered side"


def test_interface_reference_is_the_statement_on_every_triple():
    ent, rel = Q.interface_tables()
    S = Q.all_scores(ent, rel)
    assert S.shape == (Q.IF_ENT, Q.IF_REL, Q.IF_ENT)
    e, r = ent.astype(np.float64), rel.astype(np.float64)
    for hh, rr, tt in ((3, 2, 5), (0, 0, 0), (39, 5, 17)):
        assert abs(S[hh, rr, tt] - Q.score(e[hh:hh + 1], r[rr:rr + 1], e[tt:tt + 1], Q.IF_GAMMA)[0]) < 1e-12


# --------------------------------------------------------------------------------------------------------------------------
# the refusals
# --------------------------------------------------------------------------------------------------------------------------
def test_c_abi_takes_model_10_and_refuses_bad_dimensions_without_a_gpu():
    lib = _lib()
    h = lib.lib()
    assert lib.MODEL_IDS["PairRE"] == Q.MODEL_ID == 10 and lib.MODEL_IDS["QuatE"] == 8 and h.kge_abi_version() == 8
    assert 9 not in lib.MODEL_IDS.values()
    one = 1                                                       # (a non-NULL pointer that is never dereferenced)
    for d_e, d_r in ((8, 8), (8, 4), (0, 0), (6, 13)):
        rc = h.kge_score_pos(10, one, one, one, 2, d_e, d_r, 1.0, 1.0, one, None)
        assert rc == -1 and b"PairRE" in h.kge_last_error(), (d_e, d_r)
    rc = h.kge_score_pos(10, None, None, None, 2, 6, 12, 1.0, 1.0, None, None)     # accepted: the next check speaks
    assert rc == -1 and b"PairRE" not in h.kge_last_error() and b"kge_score_pos" in h.kge_last_error()
    for bad in (9, 11):
        rc = h.kge_score_pos(bad, one, one, one, 2, 4, 8, 1.0, 1.0, one, None)
        assert rc == -1 and b"unknown model" in h.kge_last_error()
    rc = h.kge_topk_select(10, 0, one, 5, one, 2, one, one, one, 1, 8, 8, 0.0, 1.0, None, 5, one, 1, 1, 3, one, one, one, 1 << 20, None)
    assert rc == -1 and b"do not fit model 10" in h.kge_last_error()
    rc = h.kge_topk_select(9, 0, one, 5, one, 2, one, one, one, 1, 8, 16, 0.0, 1.0, None, 5, one, 1, 1, 3, one, one, one, 1 << 20, None)
    assert rc == -1 and b"unknown score function 9" in h.kge_last_error()
    assert h.kge_rank_rel_workspace_bytes(10, 4, 10, 8, 16) == 0


def test_workspaces_one_byte_short_are_refused_before_any_launch():
    lib = _lib()
    h = lib.lib()
    one = 1
    WS = -2                                                       # KGE_ERR_WORKSPACE
    # the per-op entries: w, Gw and the candidate norms lie behind the entries every model has
    need = h.kge_score_neg_workspace_bytes(10, 2, 8, 24, 32)
    assert need > h.kge_score_neg_workspace_bytes(2, 2, 8, 24, 32)              # (DistMult: the common entries alone)
    assert h.kge_score_neg_fwd(10, 0, one, one, one, 2, 8, 24, 32, 64, 1.0, 1.0, one, one, need - 1, 0, None) == WS
    assert h.kge_score_neg_bwd(10, 0, one, one, one, None, one, 2, 8, 24, 32, 64, 1.0, 1.0, one, one, one, one, need - 1, 0, None) == WS
    # the step
    hp, tb, b = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch()
    hp.model, hp.d_e, hp.d_r = 10, 8, 16
    b.B, b.C, b.chunk, b.N, b.UE, b.UR = 4, 1, 4, 3, 5, 2
    need = h.kge_step_workspace_bytes(C.byref(hp), 4, 1, 4, 3, 5, 2)
    hp0 = lib.KgeHParams()
    hp0.model, hp0.d_e, hp0.d_r = 2, 8, 8
    assert need > h.kge_step_workspace_bytes(C.byref(hp0), 4, 1, 4, 3, 5, 2)
    tb.ent = tb.ent_state = tb.rel = tb.rel_state = one
    for f in ("h_gid", "t_gid", "rel_ids", "neg_ids", "ue_id", "ue_pos_ptr", "ue_pos_adj", "ue_neg_ptr", "ue_neg_slot", "ur_id", "ur_ptr",
              "ur_edge", "ue_rec", "ur_rec"):
        setattr(b, f, one)
    assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, one, need - 1, None) == WS
    assert b"workspace too small" in h.kge_last_error()
    # ranking: the pair lives in the A and RV entries, the norms in the bsq entry - the size function is the one of every model
    need = h.kge_rank_workspace_bytes(4, 10, 8)
    rc = h.kge_rank_eval(10, 0, one, 10, one, 3, one, one, one, 4, 8, 16, 1.0, 1.0, None, 0, None, None, 4, one, None, one, need - 1, 0, None)
    assert rc == WS
    # chunked ranking: one more entry of norms per list position
    need = h.kge_rank_chunked_workspace_bytes(10, 8, 4, 10, 1, 8, 16)
    assert need > h.kge_rank_chunked_workspace_bytes(2, 8, 4, 10, 1, 8, 8)
    rc = h.kge_rank_eval_chunked(10, 0, one, 10, one, 3, None, one, one, one, 8, 8, 16, 1.0, 1.0, 4, None, 0, 0, 1, None, None, one, None,
                                 one, h.kge_rank_chunked_workspace_bytes(10, 4, 4, 10, 1, 8, 16) - 1, 0, None)
    assert rc == WS
    # top-K: the header formula, rows 2 d_e wide
    need = lib.topk_workspace_bytes(10, 64, 10, 32, 3)
    assert need == h.kge_topk_workspace_bytes(64, 10, 64, 3) > h.kge_topk_workspace_bytes(64, 10, 32, 3)
    assert lib.topk_workspace_bytes(0, 64, 10, 32, 3) == h.kge_topk_workspace_bytes(64, 10, 32, 3)
    rc = h.kge_topk_select(10, 0, one, 10, one, 3, one, one, one, 64, 32, 64, 0.0, 1.0, one, 10, one, 1, 1, 3, one, one, one, need - 1, None)
    assert rc == WS and b"workspace too small" in h.kge_last_error()


def test_closed_entries_refuse_pairre_before_any_launch():
    lib = _lib()
    h = lib.lib()
    one = 1
    hp, tb, b, sh, em, job = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch(), lib.KgeShards(), lib.KgeEmit(), lib.KgeSamplerJob()
    hp.model, hp.d_e, hp.d_r = 10, 8, 16
    b.B, b.C, b.chunk, b.N = 4, 1, 4, 3

    def named(entry):
        return b"PairRE" in h.kge_last_error() and entry in h.kge_last_error()
    assert h.kge_step_sharded(C.byref(hp), C.byref(sh), C.byref(b), None, one, 1 << 20, None) == -1 and named(b"kge_step_sharded")
    assert h.kge_step_grads(C.byref(hp), C.byref(tb), C.byref(b), None, C.byref(em), one, 1 << 20, None) == -1 and named(b"kge_step_grads")
    pipe = C.c_void_p()
    assert h.kge_pipe_create(C.byref(pipe)) == 0
    assert h.kge_step_async(pipe, C.byref(hp), C.byref(tb), C.byref(b), None, None, one, 1 << 20, None) == -1 and named(b"kge_step_async")
    h.kge_pipe_destroy(pipe)
    assert h.kge_step_fused_sampling(C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20, C.byref(job), None) == -1
    assert named(b"kge_step_fused_sampling")
    rc = h.kge_rank_eval_split(10, 0, one, 5, one, 5, one, 2, None, one, one, one, 1, 8, 16, 0.0, 1.0, None, 0, None, None, 1, one, None,
                               one, 1 << 20, 0, None)
    assert rc == -1 and named(b"kge_rank_eval_split")
    rc = h.kge_rank_rel_eval(10, one, 5, one, 10, None, one, one, one, 4, 8, 16, 0.0, 1.0, one, one, 4, one, None, one, 1 << 20, 0, None)
    assert rc == -1 and named(b"kge_rank_rel_eval")
    # the strict step takes the id: the next check speaks (null tables)
    assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20, None) == -1
    assert b"PairRE" not in h.kge_last_error() and b"unknown model" not in h.kge_last_error()


def test_command_lines_refuse_widths_and_flag_combinations(tmp_path):
    _lib()
    from dglke_amd import eval_cli, train as T
    from dglke_amd._lib import KgeError
    base = ["--model_name", "PairRE", "--dataset", "toy", "--data_path", str(tmp_path / "none"), "--save_path", str(tmp_path / "ckpts"),
            "--gpu", "0"]
    assert T.ArgParser().parse_args(base).model_name == "PairRE"
    for extra, word in (([], "-dr without -de"), (["-de"], "-dr without -de"), (["-de", "-dr"], "-dr without -de"),
                        (["-dr", "--async_update", "--async_update_pipeline"], "one-step-stale pipeline"),
                        (["-dr", "--async_update", "--async_update_rel"], "one-step-stale pipeline"),
                        (["-dr", "--eval_relation"], "no relation ranking")):
        with pytest.raises(KgeError, match="PairRE.*" + word):
            T.main(base + extra)
    with pytest.raises(KgeError, match="PairRE is not available on more than one GPU"):
        T.main(base[:-1] + ["0", "0", "-dr"])
    assert not os.path.exists(str(tmp_path / "ckpts")), "refused before anything is loaded or created"
    ev = ["--model_name", "PairRE", "--dataset", "toy", "--data_path", str(tmp_path / "none"), "--model_path", str(tmp_path), "--gpu", "0"]
    with pytest.raises(KgeError, match="PairRE.*-dr without -de"):
        eval_cli.main(ev)
    with pytest.raises(KgeError, match="PairRE.*-dr without -de"):
        eval_cli.main(ev + ["-de", "-dr"])
    with pytest.raises(KgeError, match="PairRE is not available on sharded tables"):
        eval_cli.main(ev[:-1] + ["0", "0", "-dr"])
    with pytest.raises(KgeError, match="PairRE.*no relation ranking"):
        eval_cli.main(ev + ["-dr", "--eval_relation"])
    with pytest.raises(SystemExit):
        T.ArgParser().parse_args(["--model_name", "Pairre"])


def test_python_layers_check_the_widths_before_touching_a_device():
    lib = _lib()
    from dglke_amd import ke_model, score_fun
    from dglke_amd.train import check_model_widths
    assert score_fun.PairREScore.model_name == "PairRE" and score_fun.PairREScore(7.0).gamma == 7.0 and lib.model_id("PairRE") == 10
    assert issubclass(ke_model.PairREModel, ke_model.KGEModel) and ke_model.PairREModel(0, 5.0)._gamma == 5.0
    check_model_widths("PairRE", 32, False, True)
    check_model_widths("DistMult", 32, True, False)
    with pytest.raises(lib.KgeError, match="PairRE.*-dr without -de"):
        check_model_widths("PairRE", 32, True, True)
