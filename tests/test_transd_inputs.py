"""CPU guard of the TransD tests (tests/transd_cases.py): the float64 statement against torch.autograd on the defining formulas and
its identities (the matrix form, the reduction to TransE_l2), the conditions on the inputs of every case - distance share, no
cancellation-residual rows, |c_j| of order 1 - with nothing excluded, the Adam ambiguity cap, the integer-grid ranking inputs with
every intermediate of both forms an integer below 2^24, and the refusals - widths and flag combinations on the command lines,
dimensions, workspaces and the closed entries in the C ABI (no GPU: argument errors are reported before any launch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import adam_cases as A
import transd_cases as Q

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
def _t_proj(xrow, rp, k):
    x, xp = xrow[..., :k], xrow[..., k:]
    return x + (xp * x).sum(-1, keepdim=True) * rp


@pytest.mark.parametrize("k", [4, 8, 36])
@pytest.mark.parametrize("neg_head", [False, True])
def test_statement_gradients_equal_autograd(k, neg_head):
    """score, the chunked score in its direct form and the full adjoint - the issue's Ga, Grho, Gc, Gn, Gm formulas, then the
    adjoints of the two projections - against torch.autograd on the DEFINITION, in float64; the matrix form against the direct form.
    The issue measured 6e-14 for the form and 4e-15 for the gradients: the bounds here are 1e-12 and 1e-12"""
    C_, chunk, N = 2, 5, 7
    rng = np.random.RandomState(k + neg_head)
    u = lambda *s: rng.uniform(-1, 1, s)
    inp = dict(x=u(C_ * chunk, 2 * k), y=u(C_ * chunk, 2 * k), r=u(C_ * chunk, 2 * k), nb=u(C_ * N, 2 * k), W=u(C_, chunk, N), dp=u(C_ * chunk))
    inp["r"][3, k:] = 0.0
    ref = Q.op_reference(inp, C_, chunk, N, neg_head)
    x, y, r, nb = (torch.tensor(inp[n_], dtype=torch.float64, requires_grad=True) for n_ in ("x", "y", "r", "nb"))
    h, t = (y, x) if neg_head else (x, y)
    pos = Q.GAMMA - (_t_proj(h, r[:, k:], k) + r[:, :k] - _t_proj(t, r[:, k:], k)).norm(dim=-1)
    assert np.abs(pos.detach().numpy() - ref["pos"]).max() < 1e-12
    (pos * torch.tensor(inp["dp"])).sum().backward()
    for got, want in ((h.grad, ref["gh"]), (r.grad, ref["grp"]), (t.grad, ref["gt"])):
        assert np.abs(got.numpy() - want).max() < 1e-12
    for v in (x, y, r):
        v.grad = None
    # the chunked score by its DEFINITION: the score of the triple with the candidate row substituted on the corrupted side
    X_ = x.reshape(C_, chunk, 1, 2 * k).expand(C_, chunk, N, 2 * k)
    R_ = r.reshape(C_, chunk, 1, 2 * k).expand(C_, chunk, N, 2 * k)
    N_ = nb.reshape(C_, 1, N, 2 * k).expand(C_, chunk, N, 2 * k)
    hh, tt = (N_, X_) if neg_head else (X_, N_)
    s = Q.GAMMA - (_t_proj(hh, R_[..., k:], k) + R_[..., :k] - _t_proj(tt, R_[..., k:], k)).norm(dim=-1)
    assert np.abs(s.detach().numpy() - ref["score"]).max() < 1e-12
    (s * torch.tensor(inp["W"])).sum().backward()
    for got, want in ((x.grad, ref["gx"]), (r.grad, ref["gr"]), (nb.grad, ref["gn"])):
        assert np.abs(got.numpy() - want).max() < 1e-12
    assert np.abs(ref["gn"][:, k:]).max() > 1e-3 and np.abs(ref["gx"][:, k:]).max() > 1e-3, "both halves of a row take gradient"
    a, rho = Q.pair(neg_head, inp["x"], inp["r"])
    d2 = Q.dist2_matrix(a, rho, inp["nb"], C_, chunk, N)
    assert np.abs(d2 - Q.dist_neg(a, rho, inp["nb"], C_, chunk, N) ** 2).max() < 1e-12 * max(1.0, np.abs(d2).max())


def test_both_chunked_forms_are_the_score_with_the_candidate_substituted():
    rng = np.random.RandomState(5)
    B, N, d = 6, 9, 24
    h, t, nb, r = (rng.uniform(-1, 1, (n_, d)) for n_ in (B, B, N, B))
    for neg_head in (False, True):
        a, rho = Q.pair(neg_head, t if neg_head else h, r)
        S = Q.score_neg(a, rho, nb, 1, B, N)[0]
        for j in range(N):
            cand = np.repeat(nb[j:j + 1], B, 0)
            direct = Q.score(cand, r, t) if neg_head else Q.score(h, r, cand)
            assert np.abs(S[:, j] - direct).max() < 1e-12
        # the true entity in the corrupted slot gives the positive score
        own = Q.score_neg(a, rho, h if neg_head else t, 1, B, B)[0]
        assert np.abs(np.diag(own) - Q.score(h, r, t)).max() < 1e-12


def test_matrix_form_equals_the_direct_form():
    """alpha + beta + c^2 sigma - 2 p + 2 c (q - u) is the squared distance, on every per-op input"""
    for k in Q.OP_WIDTHS:
        for neg_head in (False, True):
            C_, chunk, N = Q.OP_SHAPES[0]
            inp = Q.op_inputs(k, C_, chunk, N, neg_head)
            a, rho = Q.pair(neg_head, inp["x"].astype(np.float64), inp["r"].astype(np.float64))
            nb = inp["nb"].astype(np.float64)
            d2 = Q.dist2_matrix(a, rho, nb, C_, chunk, N)
            assert np.abs(d2 - Q.dist_neg(a, rho, nb, C_, chunk, N) ** 2).max() < 1e-12 * max(1.0, np.abs(d2).max())
            assert np.abs(Q.score_neg_matrix(a, rho, nb, C_, chunk, N) - Q.score_neg(a, rho, nb, C_, chunk, N)).max() < 1e-12


@pytest.mark.parametrize("which", ["r_p", "e_p"])
def test_zero_mapping_vectors_are_transe_l2_on_the_first_halves(which):
    """r_p == 0, or every e_p == 0: both projections are the identity and the statement is the oracle's TransE_l2 on the first
    halves - scores and gradients; the zero halves that stay out of the score take no gradient"""
    from oracle import kge_oracle as O
    rng = np.random.RandomState(8)
    B, N, k = 6, 9, 12
    h, t, nb, r = (rng.uniform(-1, 1, (n_, 2 * k)) for n_ in (B, B, N, B))
    if which == "r_p":
        r[:, k:] = 0.0
    else:
        h[:, k:] = t[:, k:] = nb[:, k:] = 0.0
    h1, t1, n1, r1 = h[:, :k], t[:, :k], nb[:, :k], r[:, :k]
    assert np.abs(Q.score(h, r, t) - O.score_pos("TransE_l2", h1, r1, t1, Q.GAMMA, 1.0)).max() < 1e-12
    gh, gr, gt = Q.score_bwd(h, r, t, np.ones(B))
    e = h1 + r1 - t1
    ge = -e / np.sqrt((e * e).sum(-1, keepdims=True))
    assert np.abs(gh[:, :k] - ge).max() < 1e-12 and np.abs(gt[:, :k] + ge).max() < 1e-12 and np.abs(gr[:, :k] - ge).max() < 1e-12
    for neg_head in (False, True):
        x = t if neg_head else h
        a, rho = Q.pair(neg_head, x, r)
        assert np.abs(a - (x[:, :k] - r1 if neg_head else x[:, :k] + r1)).max() == 0
        S = Q.score_neg(a, rho, nb, 1, B, N)
        assert np.abs(S[0] - (Q.GAMMA - np.sqrt(((a[:, None, :] - n1[None]) ** 2).sum(-1)))).max() < 1e-12
        G = rng.uniform(-1, 1, (1, B, N))
        ga, grho, gn = Q.score_neg_bwd(a, rho, nb, G, 1, B, N)
        diff = a[:, None, :] - n1[None]
        gd = -G[0][..., None] * diff / np.sqrt((diff ** 2).sum(-1))[..., None]
        assert np.abs(ga - gd.sum(1)).max() < 1e-12 and np.abs(gn[:, :k] + gd.sum(0)).max() < 1e-12
        gx, gr2 = Q.pair_bwd(neg_head, x, r, ga, grho)
        assert np.abs(gx[:, :k] - ga).max() < 1e-12 and np.abs(gr2[:, :k] - (-ga if neg_head else ga)).max() < 1e-12
        if which == "r_p":          # the entities' mapping vectors are multiplied by r_p = 0: no gradient; r_p itself takes one
            assert not gx[:, k:].any() and not gn[:, k:].any() and gr2[:, k:].any()
        else:                       # e_p = 0 and x_p . x = 0: r_p takes none from the projections (c_j = 0 and u-terms vanish with it)
            assert np.abs(gr2[:, k:] - grho).max() == 0


# --------------------------------------------------------------------------------------------------------------------------
# the case tables
# --------------------------------------------------------------------------------------------------------------------------
def test_op_cases_cover_the_tile_edges_and_keep_the_input_conditions():
    import transh_cases as TH
    assert all(k % 4 == 0 for k in Q.OP_WIDTHS) and set(Q.OP_WIDTHS) >= {4, 8, 36, 64, 260}
    assert Q.OP_SHAPES == TH.OP_SHAPES and Q.DIST_SHARE == TH.DIST_SHARE == 0.05
    assert any(chunk <= 16 < 2 * chunk and chunk % 16 for _, chunk, _ in Q.OP_SHAPES)
    least, cmax = 1.0, 0.0
    for k in Q.OP_WIDTHS:
        for C_, chunk, N in Q.OP_SHAPES:
            for neg_head in (False, True):
                inp = Q.op_inputs(k, C_, chunk, N, neg_head)
                assert all(inp[n_].shape[1] == 2 * k for n_ in ("x", "y", "r", "nb"))
                assert not inp["r"][1, k:].any() and inp["r"][1, :k].all() and not inp["x"][2, k:].any() and not inp["nb"][3, k:].any()
                assert not inp["nb"][4].any()
                ref = Q.op_reference(inp, C_, chunk, N, neg_head)
                assert all(np.isfinite(v).all() for v in ref.values())
                least, cmax = min(least, ref["share"]), max(cmax, ref["cmax"])
                tag = "k%d C%d c%d N%d neg_head=%d" % (k, C_, chunk, N, neg_head)
                assert ref["share"] >= Q.DIST_SHARE, "%s: a distance at %.3f of sqrt(alpha + beta + c^2 sigma)" % (tag, ref["share"])
                assert ref["cmax"] <= Q.C_MAX, "%s: |c_j| reaches %.2f" % (tag, ref["cmax"])
                for g in ("gx", "gn", "gh", "gt"):
                    assert np.abs(ref[g][:, :k]).max() > 1e-4 and np.abs(ref[g][:, k:]).max() > 1e-4, (tag, g)
    assert least >= Q.DIST_SHARE and 0.5 < cmax <= Q.C_MAX, "|c_j| is of order 1 (largest %.2f)" % cmax


def test_step_cases_do_what_they_are_listed_for():
    _lib()
    import pairre_cases as PR
    from dglke_amd import plan
    assert [c["id"] for c in Q.STEP_CASES] == [c["id"] for c in PR.STEP_CASES] and Q.STEP_CASES == PR.STEP_CASES
    assert {(c["genre"], c["adv"], c["pairwise"]) for c in Q.STEP_CASES} >= {
        ("Logsigmoid", False, False), ("Logsigmoid", True, False), ("Logistic", False, False), ("Hinge", False, False),
        ("Hinge", False, True), ("BCE", False, False), ("Softmax", False, False)}
    assert {c["reg_norm"] for c in Q.STEP_CASES if c["reg_coef"] > 0} == {1, 2, 3}
    assert any(c["neg_deg"] for c in Q.STEP_CASES) and any(c["impts"] for c in Q.STEP_CASES)
    for k in Q.STEP_WIDTHS:
        assert k % 4 == 0
        for zero_p in (False, True):
            ent, rel = Q.step_tables(k, zero_p)
            assert ent.shape[1] == rel.shape[1] == 2 * k and np.abs(Q.c_of(ent)).max() <= Q.C_MAX
            assert (not ent[:, k:].any() and not rel[:, k:].any()) == zero_p
            for c in Q.STEP_CASES if not zero_p else Q.STEP_CASES[1:2]:
                bts = Q.step_batches(c)
                assert [bt["neg_head"] for bt in bts] == [False, True], "tail then head corruption"
                for bt in bts:
                    p = plan.build_plan(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], bt["w"])
                    # owner-computes lists longer than one: an entity with several positive ends and negative slots, a relation with several edges
                    assert np.diff(p["ue_pos_ptr"]).max() > 1 and np.diff(p["ue_neg_ptr"]).max() > 1 and np.diff(p["ur_ptr"]).max() > 1
                    out = Q.forward_backward(c, ent.astype(np.float64), rel.astype(np.float64), bt)
                    tag = "k%d %s %s" % (k, c["id"], "head" if bt["neg_head"] else "tail")
                    assert out["share"] >= Q.DIST_SHARE, "%s: a distance at %.3f of sqrt(alpha + beta + c^2 sigma)" % (tag, out["share"])
                    assert Q.residual_rows(out) == 0, "%s: a gradient row that is a cancellation residual" % tag
                    assert out["cmax"] <= Q.C_MAX, tag
                    assert np.isfinite(out["log"][2]) and out["log"][2] > 0
                    for g in ("g_pos_ent", "g_neg", "g_rel"):
                        assert np.isfinite(out[g]).all() and np.abs(out[g]).max() > 1e-4, (tag, g)
                        if zero_p:
                            assert not out[g][:, k:].any() and out[g][:, :k].any(), tag + ": the zero halves take no gradient"
                        else:
                            assert np.abs(out[g][:, k:]).max() > 1e-4, (tag, g)
                    if c["neg_deg"]:
                        n = out["neg_score"].reshape(c["B"], -1)
                        assert n.shape[1] == c["chunk"] + c["N"] and np.all(n[np.arange(c["B"]), np.arange(c["B"]) % c["chunk"]] == 0.0)
                    if c["reg_coef"] > 0:
                        plain = Q.forward_backward(dict(c, reg_coef=0.0), ent.astype(np.float64), rel.astype(np.float64), bt)
                        share = np.abs(out["g_rel"] - plain["g_rel"]).max() / np.abs(out["g_rel"]).max()
                        assert share >= 0.01, "%s: the regulariser does not show in the gradients (%.3g)" % (tag, share)
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


def test_adam_case_keeps_the_conditions_and_the_ambiguity_cap():
    """four steps of adam_cases.step on this file's gradients: at most AMBIGUITY_CAP of any compared array falls under the sign rule"""
    c = Q.ADAM_CASE
    assert c["model"] == Q.MODEL and A.widths(c) == (16, 16)
    ent, rel = A.tables(c)
    st = A.zero_state(c, ent, rel)
    amb = dict(ent=np.zeros(ent.shape, bool), rel=np.zeros(rel.shape, bool))
    for bt in A.batches(c):
        with Q.adam_gradients():
            info = A.step(c, st, bt)
        assert info["out"]["share"] >= Q.DIST_SHARE and info["out"]["cmax"] <= Q.C_MAX
        for tab in ("ent", "rel"):
            amb[tab] |= A.ambiguous(info[tab][0], info[tab][1], amb[tab].shape[0])
    assert A.gradients.__module__ == "adam_cases", "the hook is gone after the block"
    for tab in ("ent", "rel"):
        assert amb[tab].mean() <= A.AMBIGUITY_CAP, "%s: %.4f of the elements are ambiguous" % (tab, amb[tab].mean())


# --------------------------------------------------------------------------------------------------------------------------
# the integer-grid ranking inputs
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", Q.TIE_CASES, ids=["n%d-k%d" % c for c in Q.TIE_CASES])
def test_grid_inputs_are_exact_in_float32_and_hold_ties(n, k, wide_e=None, chunk=None):
    assert {c[0] for c in Q.TIE_CASES} == {5, 129, 300} and {c[1] for c in Q.TIE_CASES} == {4, 36}
    c = Q.tie_inputs(n, k) if wide_e is None else Q.tie_inputs(n, k, wide_e)      # (the several-tile sizes)
    chunk = Q.TIE_CHUNK if chunk is None else chunk
    assert np.array_equal(c.ent, np.rint(c.ent)) and np.abs(c.ent).max() <= 2 and np.array_equal(c.rel, np.rint(c.rel))
    assert not c.ent[0, k:].any() and not c.rel[0, k:].any() and c.ent[1:, k:].any() and c.rel[1:, k:].any()
    assert Q.TIE_GAMMA == int(Q.TIE_GAMMA)
    E = len(c.h)
    assert E == Q.tie_E(n)
    ties = filt_ties = 0
    for neg_head in (False, True):
        # every intermediate of both forms, c_j^2 sigma_i included, is an integer below 2^24: float32 is exact in any order
        inter = Q.tie_intermediates(c, c.h, c.r, c.t, neg_head)
        assert np.array_equal(inter, np.rint(inter)) and np.abs(inter).max() < 2 ** 24, "largest intermediate %g" % np.abs(inter).max()
        p, S = Q.tie_scores(c, c.h, c.r, c.t, neg_head)
        d2 = (Q.TIE_GAMMA - S) ** 2
        assert np.abs(d2 - np.rint(d2)).max() < 1e-9 and d2.max() < 2 ** 12, "squared distances are small integers"
        # the float32 statement: every squared distance is exact, so both float32 forms give the SAME bits (one correctly rounded root
        # of the same number), equal float64 scores stay equal and distinct ones stay distinct - the float32 ranks are the float64 ranks
        p32, S32 = Q.tie_scores(c, c.h, c.r, c.t, neg_head, np.float32)
        assert p32.dtype == np.float32 and S32.dtype == np.float32
        for s32 in Q.f32_scores_two_forms(c, c.h, c.r, c.t, neg_head):
            assert s32.dtype == np.float32 and np.array_equal(s32, S32), "a float32 form is not exact"
        for i in range(E):
            assert len(np.unique(S32[i])) == len(np.unique(S[i])) and np.array_equal(np.argsort(-S32[i], kind="stable"), np.argsort(-S[i], kind="stable"))
            assert np.array_equal(S32[i] >= p32[i], S[i] >= p[i]) and np.array_equal(S32[i] == p32[i], S[i] == p[i])
        assert np.array_equal(Q.ranks_of(p32, S32), Q.ranks_of(p, S))
        own = c.h if neg_head else c.t
        assert np.array_equal(S[np.arange(E), own], p)
        m = S == p[:, None]
        m[np.arange(E), own] = False
        ties += int(m.any(1).sum())
        lists = Q.filter_lists(c, neg_head)
        raw, filt = Q.ranks_of(p, S), Q.ranks_of(p, S, lists)
        for i in range(E):
            ids = lists[1][lists[0][i, 0]:lists[0][i, 1]]
            assert own[i] in ids
            filt_ties += int(((S[i, ids] == p[i]) & (ids != own[i])).sum())
        assert np.all(filt <= raw - 1)
        cand = Q.tie_candidates(n, E, chunk)
        assert (cand == -1).sum(1).min() == 2 and cand.max() < n
        listed, selfc = (Q.chunked_ranks_of(c, p, S, neg_head, cand, sc, chunk) for sc in (False, True))
        assert listed.max() > 1 and np.any(selfc != listed)
        if n > 5:
            assert m.any(1).sum() * 10 >= E, "fewer than one row in ten has a candidate that ties its positive (neg_head=%d)" % neg_head
            assert np.any(raw != Q.ranks_of(p, S, strict=True) + 1), "`>=` and `>` must differ by more than the own column"
    if n > 5:
        assert filt_ties >= 1, "no tie on the filtered side"


def test_interface_reference_is_the_statement_on_every_triple():
    ent, rel = Q.interface_tables()
    S = Q.all_scores(ent, rel)
    assert S.shape == (Q.IF_ENT, Q.IF_REL, Q.IF_ENT) and ent.shape[1] == rel.shape[1] == Q.IF_D
    e, r = ent.astype(np.float64), rel.astype(np.float64)
    for hh, rr, tt in ((3, 2, 5), (0, 0, 0), (39, 5, 17)):
        assert abs(S[hh, rr, tt] - Q.score(e[hh:hh + 1], r[rr:rr + 1], e[tt:tt + 1], Q.IF_GAMMA)[0]) < 1e-12


# --------------------------------------------------------------------------------------------------------------------------
# the refusals
# --------------------------------------------------------------------------------------------------------------------------
def test_c_abi_takes_model_14_and_refuses_bad_dimensions_without_a_gpu():
    lib = _lib()
    h = lib.lib()
    assert lib.MODEL_IDS["TransD"] == Q.MODEL_ID == 14 and lib.MODEL_IDS["TransH"] == 12 and h.kge_abi_version() == 8
    assert not {9, 11, 13, 15} & set(lib.MODEL_IDS.values())
    one = 1                                                       # (a non-NULL pointer that is never dereferenced)
    for d_e, d_r in ((8, 16), (16, 8), (0, 0), (12, 12), (4, 4), (20, 20)):      # d_e != d_r; d_e no multiple of 8; d_e < 8
        rc = h.kge_score_pos(14, one, one, one, 2, d_e, d_r, 1.0, 1.0, one, None)
        assert rc == -1 and b"TransD" in h.kge_last_error(), (d_e, d_r)
    rc = h.kge_score_pos(14, None, None, None, 2, 16, 16, 1.0, 1.0, None, None)     # accepted: the next check speaks
    assert rc == -1 and b"TransD" not in h.kge_last_error() and b"kge_score_pos" in h.kge_last_error()
    for bad in (9, 11, 13, 15):
        rc = h.kge_score_pos(bad, one, one, one, 2, 8, 8, 1.0, 1.0, one, None)
        assert rc == -1 and b"unknown model" in h.kge_last_error(), bad
        hp, tb, b = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch()
        hp.model, hp.d_e, hp.d_r = bad, 8, 8
        b.B, b.C, b.chunk, b.N = 4, 1, 4, 3
        assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20, None) == -1
        assert b"unknown model" in h.kge_last_error(), bad
        rc = h.kge_rank_eval(bad, 0, one, 10, one, 3, one, one, one, 4, 8, 8, 1.0, 1.0, None, 0, None, None, 4, one, None, one, 1 << 20, 0, None)
        assert rc == -1 and b"unknown model" in h.kge_last_error(), bad
    for d_e, d_r in ((8, 16), (12, 12)):
        rc = h.kge_topk_select(14, 0, one, 5, one, 2, one, one, one, 1, d_e, d_r, 0.0, 1.0, None, 5, one, 1, 1, 3, one, one, one, 1 << 20, None)
        assert rc == -1 and b"TransD" in h.kge_last_error()
    for bad in (13, 15):
        rc = h.kge_topk_select(bad, 0, one, 5, one, 2, one, one, one, 1, 8, 8, 0.0, 1.0, None, 5, one, 1, 1, 3, one, one, one, 1 << 20, None)
        assert rc == -1 and ("unknown score function %d" % bad).encode() in h.kge_last_error()
    assert h.kge_rank_rel_workspace_bytes(14, 4, 10, 16, 16) == 0


def test_workspaces_one_byte_short_are_refused_before_any_launch():
    lib = _lib()
    h = lib.lib()
    one = 1
    WS = -2                                                       # KGE_ERR_WORKSPACE
    # the per-op entries: the stacked operand, the candidates' first halves, the product blocks and the row / column terms lie behind
    # the entries every model has
    need = h.kge_score_neg_workspace_bytes(14, 2, 8, 24, 32)
    assert need > h.kge_score_neg_workspace_bytes(2, 2, 8, 24, 32)              # (DistMult: the common entries alone)
    assert h.kge_score_neg_fwd(14, 0, one, one, one, 2, 8, 24, 32, 32, 1.0, 1.0, one, one, need - 1, 0, None) == WS
    assert h.kge_score_neg_bwd(14, 0, one, one, one, None, one, 2, 8, 24, 32, 32, 1.0, 1.0, one, one, one, one, need - 1, 0, None) == WS
    # the step
    hp, tb, b = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch()
    hp.model, hp.d_e, hp.d_r = 14, 16, 16
    b.B, b.C, b.chunk, b.N, b.UE, b.UR = 4, 1, 4, 3, 5, 2
    need = h.kge_step_workspace_bytes(C.byref(hp), 4, 1, 4, 3, 5, 2)
    hp0 = lib.KgeHParams()
    hp0.model, hp0.d_e, hp0.d_r = 2, 16, 16
    assert need > h.kge_step_workspace_bytes(C.byref(hp0), 4, 1, 4, 3, 5, 2)
    tb.ent = tb.ent_state = tb.rel = tb.rel_state = one
    for f in ("h_gid", "t_gid", "rel_ids", "neg_ids", "ue_id", "ue_pos_ptr", "ue_pos_adj", "ue_neg_ptr", "ue_neg_slot", "ur_id", "ur_ptr",
              "ur_edge", "ue_rec", "ur_rec"):
        setattr(b, f, one)
    assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, one, need - 1, None) == WS
    assert b"workspace too small" in h.kge_last_error()
    # ranking: two scalars per candidate in the entry of the candidate norms - the size of 2 * n_cand candidates
    need = h.kge_rank_workspace_bytes(4, lib.rank_ws_cands(14, 10), 16)
    assert lib.rank_ws_cands(14, 10) == 20 and lib.rank_ws_cands(12, 10) == 10 and need > h.kge_rank_workspace_bytes(4, 10, 16)
    rc = h.kge_rank_eval(14, 0, one, 10, one, 3, one, one, one, 4, 16, 16, 1.0, 1.0, None, 0, None, None, 4, one, None, one, need - 1, 0, None)
    assert rc == WS
    # chunked ranking: the stacked operand, the scalars and first halves per list position and the product block
    need = h.kge_rank_chunked_workspace_bytes(14, 8, 4, 10, 1, 16, 16)
    assert need > h.kge_rank_chunked_workspace_bytes(2, 8, 4, 10, 1, 16, 16)
    rc = h.kge_rank_eval_chunked(14, 0, one, 10, one, 3, None, one, one, one, 8, 16, 16, 1.0, 1.0, 4, None, 0, 0, 1, None, None, one, None,
                                 one, h.kge_rank_chunked_workspace_bytes(14, 4, 4, 10, 1, 16, 16) - 1, 0, None)
    assert rc == WS
    # top-K: the header formula - rows d_e + 2 wide, 2 * n_cand candidates
    need = lib.topk_workspace_bytes(14, 64, 10, 32, 3)
    assert need == h.kge_topk_workspace_bytes(64, 20, 34, 3)
    assert lib.topk_workspace_bytes(14, 64, 100, 32, 3) == h.kge_topk_workspace_bytes(64, 200, 34, 3) > h.kge_topk_workspace_bytes(64, 100, 34, 3)
    assert lib.topk_workspace_bytes(12, 64, 10, 32, 3) == h.kge_topk_workspace_bytes(64, 10, 65, 3)
    rc = h.kge_topk_select(14, 0, one, 10, one, 3, one, one, one, 64, 32, 32, 0.0, 1.0, one, 10, one, 1, 1, 3, one, one, one, need - 1, None)
    assert rc == WS and b"workspace too small" in h.kge_last_error()


def test_closed_entries_refuse_transd_before_any_launch():
    lib = _lib()
    h = lib.lib()
    one = 1
    hp, tb, b, sh, em, job = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch(), lib.KgeShards(), lib.KgeEmit(), lib.KgeSamplerJob()
    hp.model, hp.d_e, hp.d_r = 14, 16, 16
    b.B, b.C, b.chunk, b.N = 4, 1, 4, 3

    def named(entry):
        return b"TransD" in h.kge_last_error() and entry in h.kge_last_error()
    assert h.kge_step_sharded(C.byref(hp), C.byref(sh), C.byref(b), None, one, 1 << 20, None) == -1 and named(b"kge_step_sharded")
    assert h.kge_step_grads(C.byref(hp), C.byref(tb), C.byref(b), None, C.byref(em), one, 1 << 20, None) == -1 and named(b"kge_step_grads")
    pipe = C.c_void_p()
    assert h.kge_pipe_create(C.byref(pipe)) == 0
    assert h.kge_step_async(pipe, C.byref(hp), C.byref(tb), C.byref(b), None, None, one, 1 << 20, None) == -1 and named(b"kge_step_async")
    h.kge_pipe_destroy(pipe)
    assert h.kge_step_fused_sampling(C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20, C.byref(job), None) == -1
    assert named(b"kge_step_fused_sampling")
    rc = h.kge_rank_eval_split(14, 0, one, 5, one, 5, one, 2, None, one, one, one, 1, 16, 16, 0.0, 1.0, None, 0, None, None, 1, one, None,
                               one, 1 << 20, 0, None)
    assert rc == -1 and named(b"kge_rank_eval_split")
    rc = h.kge_rank_rel_eval(14, one, 5, one, 10, None, one, one, one, 4, 16, 16, 0.0, 1.0, one, one, 4, one, None, one, 1 << 20, 0, None)
    assert rc == -1 and named(b"kge_rank_rel_eval")
    # the strict step takes the id: the next check speaks (null tables)
    assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20, None) == -1
    assert b"TransD" not in h.kge_last_error() and b"unknown model" not in h.kge_last_error()


def test_command_lines_refuse_widths_and_flag_combinations(tmp_path):
    _lib()
    from dglke_amd import eval_cli, train as T
    from dglke_amd._lib import KgeError
    base = ["--model_name", "TransD", "--dataset", "toy", "--data_path", str(tmp_path / "none"), "--save_path", str(tmp_path / "ckpts"),
            "--gpu", "0"]
    assert T.ArgParser().parse_args(base).model_name == "TransD"
    for extra, word in (([], "pass -de and -dr.*no -de, no -dr"), (["-de"], "pass -de and -dr.* -de, no -dr"),
                        (["-dr"], "pass -de and -dr.*no -de, -dr"),
                        (["-de", "-dr", "--hidden_dim", "30"], "--hidden_dim must be a multiple of 4"),
                        (["-de", "-dr", "--async_update", "--async_update_pipeline"], "one-step-stale pipeline"),
                        (["-de", "-dr", "--async_update", "--async_update_rel"], "one-step-stale pipeline"),
                        (["-de", "-dr", "--eval_relation"], "no relation ranking")):
        with pytest.raises(KgeError, match="TransD.*" + word):
            T.main(base + extra)
    with pytest.raises(KgeError, match="TransD is not available on more than one GPU"):
        T.main(base[:-1] + ["0", "0", "-de", "-dr"])
    assert not os.path.exists(str(tmp_path / "ckpts")), "refused before anything is loaded or created"
    ev = ["--model_name", "TransD", "--dataset", "toy", "--data_path", str(tmp_path / "none"), "--model_path", str(tmp_path), "--gpu", "0"]
    with pytest.raises(KgeError, match="TransD.*pass -de and -dr"):
        eval_cli.main(ev)
    with pytest.raises(KgeError, match="TransD.*pass -de and -dr"):
        eval_cli.main(ev + ["-dr"])
    with pytest.raises(KgeError, match="TransD.*multiple of 4"):
        eval_cli.main(ev + ["-de", "-dr", "--hidden_dim", "30"])
    with pytest.raises(KgeError, match="TransD is not available on sharded tables"):
        eval_cli.main(ev[:-1] + ["0", "0", "-de", "-dr"])
    with pytest.raises(KgeError, match="TransD.*no relation ranking"):
        eval_cli.main(ev + ["-de", "-dr", "--eval_relation"])
    with pytest.raises(SystemExit):
        T.ArgParser().parse_args(["--model_name", "Transd"])


def test_python_layers_check_the_widths_before_touching_a_device():
    lib = _lib()
    from dglke_amd import ke_model, score_fun
    from dglke_amd.train import check_model_widths
    assert score_fun.TransDScore.model_name == "TransD" and score_fun.TransDScore(7.0).gamma == 7.0 and lib.model_id("TransD") == 14
    assert issubclass(ke_model.TransDModel, ke_model.KGEModel) and ke_model.TransDModel(0, 5.0)._gamma == 5.0
    check_model_widths("TransD", 32, True, True)
    check_model_widths("DistMult", 30, True, False)
    with pytest.raises(lib.KgeError, match="TransD.*pass -de and -dr"):
        check_model_widths("TransD", 32, False, True)
    with pytest.raises(lib.KgeError, match="TransD.*multiple of 4"):
        check_model_widths("TransD", 30, True, True)
    assert lib.topk_row_width(14, 32) == 34 and lib.topk_row_width(12, 32) == 65 and lib.topk_row_width(1, 32) == 32
