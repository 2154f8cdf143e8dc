"""CPU guard of the TransH tests (tests/transh_cases.py): the float64 statement against torch.autograd on the defining formulas and
its identities, the distance condition and the Adam ambiguity cap of every case, the cases of the tables do what they are listed
for, the integer-grid ranking inputs are exact in float32 and hold ties, and the refusals - widths and flag combinations on the
command lines, dimensions, workspaces and the closed entries in the C ABI (no GPU: argument errors are reported before any
launch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import adam_cases as A
import transh_cases as Q

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
def _t_unit(w):
    ss = (w * w).sum(-1, keepdim=True)                    # (the root is taken of a positive number only: its derivative at 0 is not finite)
    return torch.where(ss > 0, w / torch.sqrt(torch.where(ss > 0, ss, torch.ones_like(ss))), torch.zeros_like(w))


def _t_proj(x, wu):
    return x - (wu * x).sum(-1, keepdim=True) * wu


@pytest.mark.parametrize("d_e", [4, 8, 36])
@pytest.mark.parametrize("neg_head", [False, True])
def test_statement_gradients_equal_autograd(d_e, neg_head):
    """score, the chunked score in its direct form and the full adjoint - the issue's Ga, Gw^, Gn formulas, then the projections and
    the normalisation - against torch.autograd on the DEFINITION, in float64, to 1e-10; one normal exactly zero"""
    C_, chunk, N = 2, 5, 7
    rng = np.random.RandomState(d_e + neg_head)
    u = lambda *s: rng.uniform(-1, 1, s)
    inp = dict(x=u(C_ * chunk, d_e), y=u(C_ * chunk, d_e), r=u(C_ * chunk, 2 * d_e), nb=u(C_ * N, d_e), W=u(C_, chunk, N), dp=u(C_ * chunk))
    inp["r"][3, d_e:] = 0.0
    ref = Q.op_reference(inp, C_, chunk, N, neg_head)
    assert ref["share"] > Q.DIST_SHARE, "away from the kink of the norm"
    x, y, r, nb = (torch.tensor(inp[k], dtype=torch.float64, requires_grad=True) for k in ("x", "y", "r", "nb"))
    h, t = (y, x) if neg_head else (x, y)
    wu = _t_unit(r[:, d_e:])
    pos = Q.GAMMA - (_t_proj(h, wu) + r[:, :d_e] - _t_proj(t, wu)).norm(dim=-1)
    assert np.abs(pos.detach().numpy() - ref["pos"]).max() < 1e-10
    (pos * torch.tensor(inp["dp"])).sum().backward()
    for got, want in ((h.grad, ref["gh"]), (r.grad, ref["grp"]), (t.grad, ref["gt"])):
        assert np.abs(got.numpy() - want).max() < 1e-10
    assert not ref["grp"][3, d_e:].any() and ref["grp"][3, :d_e].any(), "a zero normal gets no gradient, its translation does"
    for v in (x, y, r):
        v.grad = None
    wu = _t_unit(r[:, d_e:])
    a = _t_proj(x, wu) - r[:, :d_e] if neg_head else _t_proj(x, wu) + r[:, :d_e]
    A_, W_, N_ = a.reshape(C_, chunk, 1, d_e), wu.reshape(C_, chunk, 1, d_e), nb.reshape(C_, 1, N, d_e)
    s = Q.GAMMA - (A_ - N_ + (W_ * N_).sum(-1, keepdim=True) * W_).norm(dim=-1)
    assert np.abs(s.detach().numpy() - ref["score"]).max() < 1e-10
    (s * torch.tensor(inp["W"])).sum().backward()
    for got, want in ((x.grad, ref["gx"]), (r.grad, ref["gr"]), (nb.grad, ref["gn"])):
        assert np.abs(got.numpy() - want).max() < 1e-10
    assert not ref["gr"][3, d_e:].any()


def test_both_chunked_forms_are_the_score_with_the_candidate_substituted():
    rng = np.random.RandomState(5)
    B, N, d = 6, 9, 12
    h, t, nb = (rng.uniform(-1, 1, (k, d)) for k in (B, B, N))
    r = rng.uniform(-1, 1, (B, 2 * d))
    for neg_head in (False, True):
        a, wu = Q.pair(neg_head, t if neg_head else h, r)
        S = Q.score_neg(a, wu, nb, 1, B, N)[0]
        for j in range(N):
            cand = np.repeat(nb[j:j + 1], B, 0)
            direct = Q.score(cand, r, t) if neg_head else Q.score(h, r, cand)
            assert np.abs(S[:, j] - direct).max() < 1e-12
        # the true entity in the corrupted slot gives the positive score
        own = Q.score_neg(a, wu, h if neg_head else t, 1, B, B)[0]
        assert np.abs(np.diag(own) - Q.score(h, r, t)).max() < 1e-12


def test_matrix_form_equals_the_direct_form():
    """alpha + beta - 2 p + 2 c q - (2 - omega) q^2 is the squared distance, with unit normals and with zero ones (omega = 0)"""
    for d_e in Q.OP_WIDTHS:
        for neg_head in (False, True):
            C_, chunk, N = Q.OP_SHAPES[0]
            inp = Q.op_inputs(d_e, C_, chunk, N, neg_head)
            a, wu = Q.pair(neg_head, inp["x"].astype(np.float64), inp["r"].astype(np.float64))
            nb = inp["nb"].astype(np.float64)
            om = Q.matrix_terms(a, wu, nb, C_, chunk, N)[5]
            assert set(np.round(om.reshape(-1), 12).tolist()) == {0.0, 1.0}
            d2 = Q.dist2_matrix(a, wu, nb, C_, chunk, N)
            assert np.abs(d2 - Q.dist_neg(a, wu, nb, C_, chunk, N) ** 2).max() < 1e-12 * max(1.0, np.abs(d2).max())
            assert np.abs(Q.score_neg_matrix(a, wu, nb, C_, chunk, N) - Q.score_neg(a, wu, nb, C_, chunk, N)).max() < 1e-12


def test_zero_normal_is_transe_l2_on_the_translation():
    """w == 0: the projection is the identity and the statement is the oracle's TransE_l2 with relation d - scores and gradients"""
    from oracle import kge_oracle as O
    rng = np.random.RandomState(8)
    B, N, d = 6, 9, 12
    h, t, nb, dd = (rng.uniform(-1, 1, (k, d)) for k in (B, B, N, B))
    r = np.concatenate([dd, np.zeros((B, d))], -1)
    assert np.abs(Q.score(h, r, t) - (Q.GAMMA - np.sqrt(((h + dd - t) ** 2).sum(-1)))).max() < 1e-12
    assert np.abs(Q.score(h, r, t) - O.score_pos("TransE_l2", h, dd, t, Q.GAMMA, 1.0)).max() < 1e-12
    for neg_head in (False, True):
        x = t if neg_head else h
        a, wu = Q.pair(neg_head, x, r)
        assert not wu.any() and np.abs(a - (x - dd if neg_head else x + dd)).max() == 0
        S = Q.score_neg(a, wu, nb, 1, B, N)
        assert np.abs(S[0] - (Q.GAMMA - np.sqrt(((a[:, None, :] - nb[None]) ** 2).sum(-1)))).max() < 1e-12
        G = rng.uniform(-1, 1, (1, B, N))
        ga, gw, gn = Q.score_neg_bwd(a, wu, nb, G, 1, B, N)
        diff = a[:, None, :] - nb[None]
        gd = -G[0][..., None] * diff / np.sqrt((diff ** 2).sum(-1))[..., None]
        assert np.abs(ga - gd.sum(1)).max() < 1e-12 and np.abs(gn + gd.sum(0)).max() < 1e-12
        gx, gr = Q.pair_bwd(neg_head, x, r, ga, gw)
        assert np.abs(gx - ga).max() < 1e-12 and not gr[:, d:].any() and np.abs(gr[:, :d] - (-ga if neg_head else ga)).max() < 1e-12


def test_scores_depend_on_the_direction_of_the_normal_alone():
    rng = np.random.RandomState(6)
    B, N, d = 5, 7, 12
    h, t, nb = (rng.uniform(-1, 1, (k, d)) for k in (B, B, N))
    r = rng.uniform(-1, 1, (B, 2 * d))
    r2 = r.copy()
    r2[:, d:] *= rng.uniform(0.1, 10.0, (B, 1))
    assert np.abs(Q.score(h, r2, t) - Q.score(h, r, t)).max() < 1e-12
    for neg_head in (False, True):
        a, wu = Q.pair(neg_head, h, r)
        a2, wu2 = Q.pair(neg_head, h, r2)
        assert np.abs(Q.score_neg(a2, wu2, nb, 1, B, N) - Q.score_neg(a, wu, nb, 1, B, N)).max() < 1e-12
        # the gradient of a scale-invariant function is orthogonal to the row: Gw . w = 0
        ga, gw, _ = Q.score_neg_bwd(a, wu, nb, rng.uniform(-1, 1, (1, B, N)), 1, B, N)
        _, gr = Q.pair_bwd(neg_head, h, r, ga, gw)
        assert np.abs((gr[:, d:] * r[:, d:]).sum(-1)).max() < 1e-12 and np.abs(gr[:, d:]).max() > 1e-3
    _, grp, _ = Q.score_bwd(h, r, t, np.ones(B))
    assert np.abs((grp[:, d:] * r[:, d:]).sum(-1)).max() < 1e-12 and np.abs(grp[:, d:]).max() > 1e-3
    assert np.abs(Q.norm(Q.unit(r[:, d:])) - 1).max() < 1e-12


# --------------------------------------------------------------------------------------------------------------------------
# the case tables
# --------------------------------------------------------------------------------------------------------------------------
def test_op_cases_cover_the_tile_edges_and_keep_the_distance_condition():
    assert all(d % 4 == 0 for d in Q.OP_WIDTHS) and set(Q.OP_WIDTHS) >= {4, 8, 36, 64, 260}
    assert {(2, 5, 33), (2, 33, 5), (1, 32, 32)} <= set(Q.OP_SHAPES)
    # the forward tiles are 16 rows high, the backward's 16 rows (Ga | Gw^) and 16 values of the reduction (Gn)
    # (kge_neg_gemm.hip): a shape whose chunk stays inside one and whose stacked rows do not
    assert any(chunk <= 16 < 2 * chunk and chunk % 16 for _, chunk, _ in Q.OP_SHAPES)
    least = 1.0
    for d_e in Q.OP_WIDTHS:
        for C_, chunk, N in Q.OP_SHAPES:
            for neg_head in (False, True):
                inp = Q.op_inputs(d_e, C_, chunk, N, neg_head)
                assert not inp["r"][1, d_e:].any() and inp["r"][1, :d_e].all() and not inp["x"][2].any() and not inp["nb"][3].any()
                ref = Q.op_reference(inp, C_, chunk, N, neg_head)
                assert all(np.isfinite(v).all() for v in ref.values())
                least = min(least, ref["share"])
                assert ref["share"] >= Q.DIST_SHARE, "D%d C%d c%d N%d neg_head=%d: a distance at %.3f of sqrt(alpha + beta)" % (
                    d_e, C_, chunk, N, neg_head, ref["share"])
                assert not ref["gr"][1, d_e:].any() and not ref["grp"][1, d_e:].any() and ref["gr"][0, d_e:].any()
    assert least >= Q.DIST_SHARE


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
    for d_e in Q.STEP_WIDTHS:
        assert d_e % 4 == 0
        for zero_w in (False, True):
            ent, rel = Q.step_tables(d_e, zero_w)
            assert rel.shape[1] == 2 * d_e
            assert [not rel[k, d_e:].any() for k in range(Q.STEP_REL)] == [zero_w and k in Q.ZERO_W_RELS for k in range(Q.STEP_REL)]
            for c in Q.STEP_CASES if not zero_w else Q.STEP_CASES[1:2]:
                bts = Q.step_batches(c)
                assert [bt["neg_head"] for bt in bts] == [False, True], "tail then head corruption"
                for bt in bts:
                    p = plan.build_plan(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], bt["w"])
                    # owner-computes lists longer than one: an entity with several positive ends and negative slots, a relation with several edges
                    assert np.diff(p["ue_pos_ptr"]).max() > 1 and np.diff(p["ue_neg_ptr"]).max() > 1 and np.diff(p["ur_ptr"]).max() > 1
                    out = Q.forward_backward(c, ent.astype(np.float64), rel.astype(np.float64), bt)
                    assert out["share"] >= Q.DIST_SHARE, "D%d %s: a distance at %.3f of sqrt(alpha + beta)" % (d_e, c["id"], out["share"])
                    assert Q.residual_rows(out) == 0, "D%d %s: a gradient row that is a cancellation residual" % (d_e, c["id"])
                    assert np.isfinite(out["log"][2]) and out["log"][2] > 0
                    for k in ("g_pos_ent", "g_neg", "g_rel"):
                        assert np.isfinite(out[k]).all() and np.abs(out[k]).max() > 1e-4, (c["id"], k)
                    if zero_w:
                        zero = np.isin(bt["r"], Q.ZERO_W_RELS)
                        assert zero.any() and not out["g_rel"][zero][:, d_e:].any() and out["g_rel"][~zero][:, d_e:].any()
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


def test_adam_case_keeps_the_distance_condition_and_the_ambiguity_cap():
    """four steps of adam_cases.step on this file's gradients: at most AMBIGUITY_CAP of any compared array falls under the sign rule"""
    c = Q.ADAM_CASE
    assert c["model"] == Q.MODEL and A.widths(c) == (16, 32)
    ent, rel = A.tables(c)
    st = A.zero_state(c, ent, rel)
    amb = dict(ent=np.zeros(ent.shape, bool), rel=np.zeros(rel.shape, bool))
    for bt in A.batches(c):
        with Q.adam_gradients():
            info = A.step(c, st, bt)
        assert info["out"]["share"] >= Q.DIST_SHARE
        for tab in ("ent", "rel"):
            amb[tab] |= A.ambiguous(info[tab][0], info[tab][1], amb[tab].shape[0])
    assert A.gradients.__module__ == "adam_cases", "the hook is gone after the block"
    for tab in ("ent", "rel"):
        assert amb[tab].mean() <= A.AMBIGUITY_CAP, "%s: %.4f of the elements are ambiguous" % (tab, amb[tab].mean())


# --------------------------------------------------------------------------------------------------------------------------
# the integer-grid ranking inputs
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d_e", Q.TIE_CASES, ids=["n%d-D%d" % c for c in Q.TIE_CASES])
def test_grid_inputs_are_exact_in_float32_and_hold_ties(n, d_e, wide_e=None, chunk=None):
    import pairre_cases as PR
    assert Q.TIE_CASES == PR.TIE_CASES and (Q.TIE_E, Q.TIE_CHUNK) == (PR.TIE_E, PR.TIE_CHUNK)
    c = Q.tie_inputs(n, d_e) if wide_e is None else Q.tie_inputs(n, d_e, wide_e)      # (the several-tile sizes)
    w = c.rel[:, d_e:]
    assert np.all((w[1:] != 0).sum(1) == 4) and set(np.unique(w).tolist()) == {-1.0, 0.0, 1.0} and not w[0].any()
    wu = Q.unit(w)
    assert wu.dtype == np.float32 and set(np.unique(wu).tolist()) == {-0.5, 0.0, 0.5}, "float32 normalisation is exact"
    assert np.array_equal(c.ent, np.rint(c.ent)) and np.abs(c.ent).max() <= 2 and np.array_equal(c.rel, np.rint(c.rel))
    assert Q.TIE_GAMMA == int(Q.TIE_GAMMA)
    E = len(c.h)
    filt_ties = 0
    for neg_head in (False, True):
        p, S = Q.tie_scores(c, c.h, c.r, c.t, neg_head)
        d2 = (Q.TIE_GAMMA - S) ** 2
        assert np.abs(16 * d2 - np.rint(16 * d2)).max() < 1e-9 and d2.max() < 2 ** 10, "squared distances are small multiples of 1/16"
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
def test_c_abi_takes_model_12_and_refuses_bad_dimensions_without_a_gpu():
    lib = _lib()
    h = lib.lib()
    assert lib.MODEL_IDS["TransH"] == Q.MODEL_ID == 12 and lib.MODEL_IDS["PairRE"] == 10 and h.kge_abi_version() == 8
    assert 9 not in lib.MODEL_IDS.values() and 11 not in lib.MODEL_IDS.values()
    one = 1                                                       # (a non-NULL pointer that is never dereferenced)
    for d_e, d_r in ((8, 8), (8, 4), (0, 0), (6, 12), (2, 4), (10, 20)):      # d_r != 2 d_e; d_e no multiple of 4; d_e < 4
        rc = h.kge_score_pos(12, one, one, one, 2, d_e, d_r, 1.0, 1.0, one, None)
        assert rc == -1 and b"TransH" in h.kge_last_error(), (d_e, d_r)
    rc = h.kge_score_pos(12, None, None, None, 2, 8, 16, 1.0, 1.0, None, None)     # accepted: the next check speaks
    assert rc == -1 and b"TransH" not in h.kge_last_error() and b"kge_score_pos" in h.kge_last_error()
    for bad in (9, 11, 13):
        rc = h.kge_score_pos(bad, one, one, one, 2, 4, 8, 1.0, 1.0, one, None)
        assert rc == -1 and b"unknown model" in h.kge_last_error()
    for d_e, d_r in ((8, 8), (6, 12)):
        rc = h.kge_topk_select(12, 0, one, 5, one, 2, one, one, one, 1, d_e, d_r, 0.0, 1.0, None, 5, one, 1, 1, 3, one, one, one, 1 << 20, None)
        assert rc == -1 and b"TransH" in h.kge_last_error()
    rc = h.kge_topk_select(11, 0, one, 5, one, 2, one, one, one, 1, 8, 16, 0.0, 1.0, None, 5, one, 1, 1, 3, one, one, one, 1 << 20, None)
    assert rc == -1 and b"unknown score function 11" in h.kge_last_error()
    assert h.kge_rank_rel_workspace_bytes(12, 4, 10, 8, 16) == 0


def test_workspaces_one_byte_short_are_refused_before_any_launch():
    lib = _lib()
    h = lib.lib()
    one = 1
    WS = -2                                                       # KGE_ERR_WORKSPACE
    # the per-op entries: the stacked operand, the product blocks and the row / column terms lie behind the entries every model has
    need = h.kge_score_neg_workspace_bytes(12, 2, 8, 24, 32)
    assert need > h.kge_score_neg_workspace_bytes(2, 2, 8, 24, 32)              # (DistMult: the common entries alone)
    assert h.kge_score_neg_fwd(12, 0, one, one, one, 2, 8, 24, 32, 64, 1.0, 1.0, one, one, need - 1, 0, None) == WS
    assert h.kge_score_neg_bwd(12, 0, one, one, one, None, one, 2, 8, 24, 32, 64, 1.0, 1.0, one, one, one, one, need - 1, 0, None) == WS
    # the step
    hp, tb, b = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch()
    hp.model, hp.d_e, hp.d_r = 12, 8, 16
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
    # ranking: the pair lives in the A and RV entries, its statistics in asq and the TransR rows, the norms in the bsq entry - the size
    # function is the one of every model
    need = h.kge_rank_workspace_bytes(4, 10, 8)
    rc = h.kge_rank_eval(12, 0, one, 10, one, 3, one, one, one, 4, 8, 16, 1.0, 1.0, None, 0, None, None, 4, one, None, one, need - 1, 0, None)
    assert rc == WS
    # chunked ranking: the stacked operand, the norms per list position and the product block
    need = h.kge_rank_chunked_workspace_bytes(12, 8, 4, 10, 1, 8, 16)
    assert need > h.kge_rank_chunked_workspace_bytes(2, 8, 4, 10, 1, 8, 8)
    rc = h.kge_rank_eval_chunked(12, 0, one, 10, one, 3, None, one, one, one, 8, 8, 16, 1.0, 1.0, 4, None, 0, 0, 1, None, None, one, None,
                                 one, h.kge_rank_chunked_workspace_bytes(12, 4, 4, 10, 1, 8, 16) - 1, 0, None)
    assert rc == WS
    # top-K: the header formula, rows 2 d_e + 1 wide
    need = lib.topk_workspace_bytes(12, 64, 10, 32, 3)
    assert need == h.kge_topk_workspace_bytes(64, 10, 65, 3) > h.kge_topk_workspace_bytes(64, 10, 32, 3)
    assert lib.topk_workspace_bytes(10, 64, 10, 32, 3) == h.kge_topk_workspace_bytes(64, 10, 64, 3)
    rc = h.kge_topk_select(12, 0, one, 10, one, 3, one, one, one, 64, 32, 64, 0.0, 1.0, one, 10, one, 1, 1, 3, one, one, one, need - 1, None)
    assert rc == WS and b"workspace too small" in h.kge_last_error()


def test_closed_entries_refuse_transh_before_any_launch():
    lib = _lib()
    h = lib.lib()
    one = 1
    hp, tb, b, sh, em, job = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch(), lib.KgeShards(), lib.KgeEmit(), lib.KgeSamplerJob()
    hp.model, hp.d_e, hp.d_r = 12, 8, 16
    b.B, b.C, b.chunk, b.N = 4, 1, 4, 3

    def named(entry):
        return b"TransH" in h.kge_last_error() and entry in h.kge_last_error()
    assert h.kge_step_sharded(C.byref(hp), C.byref(sh), C.byref(b), None, one, 1 << 20, None) == -1 and named(b"kge_step_sharded")
    assert h.kge_step_grads(C.byref(hp), C.byref(tb), C.byref(b), None, C.byref(em), one, 1 << 20, None) == -1 and named(b"kge_step_grads")
    pipe = C.c_void_p()
    assert h.kge_pipe_create(C.byref(pipe)) == 0
    assert h.kge_step_async(pipe, C.byref(hp), C.byref(tb), C.byref(b), None, None, one, 1 << 20, None) == -1 and named(b"kge_step_async")
    h.kge_pipe_destroy(pipe)
    assert h.kge_step_fused_sampling(C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20, C.byref(job), None) == -1
    assert named(b"kge_step_fused_sampling")
    rc = h.kge_rank_eval_split(12, 0, one, 5, one, 5, one, 2, None, one, one, one, 1, 8, 16, 0.0, 1.0, None, 0, None, None, 1, one, None,
                               one, 1 << 20, 0, None)
    assert rc == -1 and named(b"kge_rank_eval_split")
    rc = h.kge_rank_rel_eval(12, one, 5, one, 10, None, one, one, one, 4, 8, 16, 0.0, 1.0, one, one, 4, one, None, one, 1 << 20, 0, None)
    assert rc == -1 and named(b"kge_rank_rel_eval")
    # the strict step takes the id: the next check speaks (null tables)
    assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20, None) == -1
    assert b"TransH" not in h.kge_last_error() and b"unknown model" not in h.kge_last_error()


def test_command_lines_refuse_widths_and_flag_combinations(tmp_path):
    _lib()
    from dglke_amd import eval_cli, train as T
    from dglke_amd._lib import KgeError
    base = ["--model_name", "TransH", "--dataset", "toy", "--data_path", str(tmp_path / "none"), "--save_path", str(tmp_path / "ckpts"),
            "--gpu", "0"]
    assert T.ArgParser().parse_args(base).model_name == "TransH"
    for extra, word in (([], "-dr without -de"), (["-de"], "-dr without -de"), (["-de", "-dr"], "-dr without -de"),
                        (["-dr", "--hidden_dim", "30"], "multiple of 4"),
                        (["-dr", "--async_update", "--async_update_pipeline"], "one-step-stale pipeline"),
                        (["-dr", "--async_update", "--async_update_rel"], "one-step-stale pipeline"),
                        (["-dr", "--eval_relation"], "no relation ranking")):
        with pytest.raises(KgeError, match="TransH.*" + word):
            T.main(base + extra)
    with pytest.raises(KgeError, match="TransH is not available on more than one GPU"):
        T.main(base[:-1] + ["0", "0", "-dr"])
    assert not os.path.exists(str(tmp_path / "ckpts")), "refused before anything is loaded or created"
    ev = ["--model_name", "TransH", "--dataset", "toy", "--data_path", str(tmp_path / "none"), "--model_path", str(tmp_path), "--gpu", "0"]
    with pytest.raises(KgeError, match="TransH.*-dr without -de"):
        eval_cli.main(ev)
    with pytest.raises(KgeError, match="TransH.*-dr without -de"):
        eval_cli.main(ev + ["-de", "-dr"])
    with pytest.raises(KgeError, match="TransH.*multiple of 4"):
        eval_cli.main(ev + ["-dr", "--hidden_dim", "30"])
    with pytest.raises(KgeError, match="TransH is not available on sharded tables"):
        eval_cli.main(ev[:-1] + ["0", "0", "-dr"])
    with pytest.raises(KgeError, match="TransH.*no relation ranking"):
        eval_cli.main(ev + ["-dr", "--eval_relation"])
    with pytest.raises(SystemExit):
        T.ArgParser().parse_args(["--model_name", "Transh"])


def test_python_layers_check_the_widths_before_touching_a_device():
    lib = _lib()
    from dglke_amd import ke_model, score_fun
    from dglke_amd.train import check_model_widths
    assert score_fun.TransHScore.model_name == "TransH" and score_fun.TransHScore(7.0).gamma == 7.0 and lib.model_id("TransH") == 12
    assert issubclass(ke_model.TransHModel, ke_model.KGEModel) and ke_model.TransHModel(0, 5.0)._gamma == 5.0
    check_model_widths("TransH", 32, False, True)
    check_model_widths("DistMult", 30, True, False)
    with pytest.raises(lib.KgeError, match="TransH.*-dr without -de"):
        check_model_widths("TransH", 32, True, True)
    with pytest.raises(lib.KgeError, match="TransH.*multiple of 4"):
        check_model_widths("TransH", 30, False, True)
    assert lib.topk_row_width(12, 32) == 65 and lib.topk_row_width(10, 32) == 64 and lib.topk_row_width(1, 32) == 32
