"""The inputs of tests/test_gpu_new_model_shapes.py (cases: tests/new_model_shape_cases.py), checked on the CPU from the float64
statements alone - a GPU comparison is only as good as these conditions:
  - every shape produces the tile, slab and route counts it is meant to, computed from the constants the kernels use;
  - update lists longer than one exist in every step (far beyond 64 entries in the heavy-list cases);
  - PairRE: sign ambiguity takes out at most pairre_cases.ROW_CAP of the rows of any compared array, nothing of the scores or
    loss terms, and nothing at all on the `separated` tables;
  - TransH, TransD: every distance share is at least DIST_SHARE and no gradient row is a cancellation residual (asserted for all
    four models: a row below 1e-6 of its array's largest component says nothing in any of them); TransD: |c_j| < C_MAX, and
    nothing at all is left out;
  - TransH, TransD: which side of own_bwd_products' condition max(2 chunk, N) <= GB_MAXK every case is on - the s7 shapes are the
    only ones beyond it, and s7c is the last one on the backward GEMM tiles;
  - hinge cases: no pair within KINK_SAFETY float32-statement score errors of the kink, and the float32 statement flips none;
  - where the float32 statement itself is over a bound of the suite (only shapes of `may_relax` may be) the factor the GPU file
    applies is the one measured here;
  - the integer-grid ranking tables of the several-tile sizes are float32-exact and hold ties (the assertions of the four models'
    own input tests, run at the new sizes); on the random ranking tables at least 90 % of the rank intervals are a single rank."""
import zlib

import numpy as np
import pytest

import new_model_shape_cases as S
import test_pairre_inputs as PRI
import test_quate_inputs as QEI
import test_transd_inputs as TDI
import test_transh_inputs as THI

_ID = lambda c: c["id"]


def test_case_tables_cover_what_the_issue_lists():
    ids = [c["id"] for c in S.BOUNDARY_CASES]
    assert len(set(ids)) == len(ids)
    for model in S.MODELS:
        mine = [c for c in S.BOUNDARY_CASES if c["model"] == model]
        stacked = model in ("TransH", "TransD")
        assert sorted(set(c["sid"] for c in mine)) == sorted(list(S.SHAPES) + (["s7a", "s7b", "s7c"] if stacked else []))
        assert len(mine) == {"QuatE": 26, "PairRE": 13, "TransH": 16, "TransD": 16}[model]
        for sid, (shape, n_ent, n_rel, opts) in list(S.SHAPES.items()) + (list(S.S7_SHAPES.items()) if stacked else []):
            got = [c for c in mine if c["sid"] == sid]
            assert sorted(set(c["oid"] for c in got)) == sorted(opts)
            want = S.QUATE_S6 if (sid == "s6" and model == "QuatE") else shape
            if model == "TransD":           # the last entry is the half-width k
                want = shape[:3] + (400 if sid == "s5" else 2 * shape[3],)
            assert S.case_shape(model, sid) == want
            assert all((c["C"], c["chunk"], c["N"], c["d_e"]) == want and c["B"] == want[0] * want[1] for c in got)
            assert all((c["n_ent"], c["n_rel"]) == (n_ent, n_rel) for c in got)
            assert all(sorted(c["flags"] for c in got if c["oid"] == o) == ([0, S.QE.FORCE_PAIRWISE] if model == "QuatE" else [0]) for o in opts)
    # the options mean what their ids say
    by = {c["id"]: c for c in S.BOUNDARY_CASES}
    c = by["PairRE-s3-neg-deg+reg3-f0"]
    assert c["neg_deg"] and c["adv"] and c["reg_coef"] > 0 and c["reg_norm"] == 3 and not c["impts"]
    c = by["TransH-s5-impts+reg3-f0"]
    assert c["impts"] and c["adv"] and c["reg_coef"] > 0 and c["reg_norm"] == 3 and not c["neg_deg"]
    c = by["QuatE-s1-hinge-pw-f1"]
    assert c["genre"] == "Hinge" and c["pairwise"] and c["flags"] == S.QE.FORCE_PAIRWISE
    assert by["PairRE-s4-bce-f0"]["genre"] == "BCE" and by["TransH-s4-softmax-f0"]["genre"] == S.QE.SM.GENRE
    c = by["TransD-s3-neg-deg+reg3-f0"]
    assert c["neg_deg"] and c["adv"] and c["reg_coef"] > 0 and c["reg_norm"] == 3 and not c["impts"] and c["d_e"] == 72
    c = by["TransD-s5-impts+reg3-f0"]
    assert c["impts"] and c["adv"] and c["reg_coef"] > 0 and c["reg_norm"] == 3 and not c["neg_deg"] and c["d_e"] == 400
    assert by["TransD-s1-hinge-pw-f0"]["genre"] == "Hinge" and by["TransD-s1-hinge-pw-f0"]["pairwise"]
    assert by["TransD-s4-bce-f0"]["genre"] == "BCE" and by["TransD-s4-softmax-f0"]["genre"] == S.QE.SM.GENRE
    assert [by["%s-s7a-logsigmoid-adv-f0" % m]["d_e"] for m in ("TransH", "TransD")] == [4, 8]
    assert S.S7_SHAPES["s7a"][0] == (1, 1032, 8, 4) and S.S7_SHAPES["s7b"][0] == (1, 8, 2049, 4) and S.S7_SHAPES["s7c"][0] == (1, 1024, 8, 4)
    assert S.rel_width("TransD", 72) == 72 and S.rel_width("TransH", 36) == 72 and S.engine_gamma("TransD") == S.TD.GAMMA
    assert (S.TD_CT, S.TD_CR, S.GB_MAXK, S.TILE_BK, S.STACK_TILE) == (32, 8, 2048, 32, 32)
    # transd_coef_kernel decodes a column-sum workgroup b as (chunk b / tct, column tile b % tct).  Where C == tct (s1: 3 and 3) the
    # two taken the other way round still visit every (chunk, tile) pair once, so cases with C > 1, tct > 1 and C != tct must exist
    td = [S.transd_tiles(c)["tct"] for c in S.BOUNDARY_CASES if c["model"] == "TransD"]
    tc = [c["C"] for c in S.BOUNDARY_CASES if c["model"] == "TransD"]
    assert {(3, 2), (2, 17)} <= {(C_, t) for C_, t in zip(tc, td) if C_ > 1 and t > 1 and C_ != t}, "s3 and s4"
    assert len(S.HEAVY_CASES) == 8 and all(not c["pairwise"] for c in S.HEAVY_CASES)


@pytest.mark.parametrize("c", S.BOUNDARY_CASES, ids=_ID)
def test_boundary_shapes_cross_what_they_name(c):
    """tile, slab and route counts from the kernels' constants (new_model_shape_cases.py quotes where each is read)"""
    sid, model = c["sid"], c["model"]
    d_r = S.rel_width(model, c["d_e"])
    Np = c["chunk"] + c["N"] if c["neg_deg"] else c["N"]
    if model in S.STACKED:
        # own_bwd_products: the backward GEMM tiles while max(2 chunk, N) <= GB_MAXK, the pairwise kernels beyond
        beyond = max(2 * c["chunk"], Np) > S.GB_MAXK
        assert S.bwd_route(c) == ("pair" if beyond else "gemm") == S.EXPECT_BWD.get(sid, "gemm")
        assert beyond == (sid in ("s7a", "s7b"))
        if sid == "s7a":
            assert 2 * c["chunk"] == 2064 > S.GB_MAXK >= c["chunk"] and Np <= S.GB_MAXK, "only the STACKED rows are beyond"
        if sid == "s7b":
            assert Np == S.GB_MAXK + 1 and 2 * c["chunk"] <= S.GB_MAXK
        if sid == "s7c":
            assert 2 * c["chunk"] == S.GB_MAXK and Np <= S.GB_MAXK and 2 * (c["chunk"] + 1) > S.GB_MAXK, "the last chunk on the tiles"
        if sid.startswith("s7"):
            assert c["d_e"] == (8 if model == "TransD" else 4), "the narrowest width"
    if model == "TransD":
        return _transd_shape_crosses_what_it_names(c, Np)
    assert S.tiles(c) == S.EXPECT_TILES.get((sid, model), S.EXPECT_TILES[sid])
    if sid.startswith("s7"):
        return
    if model == "QuatE":
        route = S.QE.neg_route(c["d_e"], c["flags"])
        assert route == S.EXPECT_ROUTES[(sid, c["flags"])]
        assert S.QE.vector_packs(c["d_e"]) == (sid in ("s4", "s5", "s6")), "s1, s2a, s2b and s3 take the scalar packs"
    if sid == "s1":
        ti, tj, tk = (S.tiles(c)[k] for k in ("ti", "tj", "tk"))
        assert min(ti, tj, tk) >= 2 and c["C"] > 1 and ti != tj, "pairre_fwd_kernel's decode: ti, tj > 1, unequal, several chunks"
        assert c["C"] * ti * tk == 18 and c["C"] * (ti + tj) * tk == 45, "pairre_bwd_kernel: row tiles before candidate tiles"
        assert (c["N"] + S.QS - 1) // S.QS == 3, "three rounds of the backward reduction over the candidates"
        assert (c["N"] + S.TH_CT - 1) // S.TH_CT == 3, "transh_coef_kernel: tct = 3"
        assert (c["d_e"] // 4) % 4 != 0
    if sid == "s3":
        assert c["neg_deg"] and Np == 48 and c["chunk"] % 16 != 0
    if sid == "s4":
        assert c["N"] > S.LOSS_REG_N and not c["neg_deg"], "the loss rows stream"
    if sid == "s5":
        assert c["d_e"] == 400 and d_r == (400 if model == "QuatE" else 800)
        assert model == "QuatE" or 512 < d_r <= S.UPDATE_REG_W, "four packs per lane in the register-resident update"
    if sid == "s6":
        assert max(c["d_e"], d_r) > S.UPDATE_REG_W, "beyond the register-resident update"
        assert model == "QuatE" or max(c["d_e"] - 4, S.rel_width(model, c["d_e"] - 4)) <= S.UPDATE_REG_W, "the narrowest such width"
    if sid == "s2a":
        assert c["d_e"] == 4 and c["chunk"] == 1 and c["N"] == 1 and c["C"] == 2


def _transd_shape_crosses_what_it_names(c, Np):
    """transd_coef_kernel's column-sum workgroups, the stacked operand's row tiles and the k-stages of the products"""
    sid, chunk, k = c["sid"], c["chunk"], c["d_e"] // 2
    assert c["d_e"] % 8 == 0 and k % 4 == 0
    t = S.transd_tiles(c)
    assert t == S.EXPECT_TRANSD[sid]
    # the row groups of a column-sum workgroup: group rg sums the rows rg, rg + TD_CR, ...
    per_group = [len(range(rg, chunk, S.TD_CR)) for rg in range(S.TD_CR)]
    assert (max(per_group), min(per_group)) == t["rows"] and sum(per_group) == chunk
    if sid == "s1":
        assert c["C"] == 3 and 2 * chunk == 80 and t["stack"] == 3 and 2 * chunk % S.STACK_TILE == 16, "three row tiles, the last of 16"
        assert chunk > S.STACK_TILE, "rho lies more than a row tile behind a"
        assert t["tct"] == 3 and Np % S.TD_CT == 8, "b / tct and b % tct with tct > 1; the j < N guard of a ragged last column tile"
        assert per_group == [5] * 8, "the strided row loop runs five times"
        assert t["kst"] == 3 and k % S.TILE_BK == 4
    if sid == "s2a":
        assert (c["C"], chunk, c["N"], k) == (2, 1, 1, 4)
    if sid == "s2b":
        assert per_group == [3, 2, 2, 2, 2, 2, 2, 2] and chunk % 2 == 1 and t["kst"] == 2 and k % S.TILE_BK == 4
    if sid == "s3":
        assert c["neg_deg"] and Np == 48 and t["tct"] == 2 and chunk % 16 != 0, "two column tiles over the in-batch and sampled rows"
    if sid == "s4":
        assert c["N"] > S.LOSS_REG_N and not c["neg_deg"] and t["tct"] == 17, "the loss rows stream"
    if sid == "s5":
        assert c["d_e"] == 400, "the recipe width"
        assert 256 < c["d_e"] <= 512, "two packs per lane in the register-resident update"
    if sid == "s6":
        assert c["d_e"] == 1032 > S.UPDATE_REG_W and c["d_e"] - 8 <= S.UPDATE_REG_W, "both tables beyond the register-resident update"


def test_all_three_quate_routes_occur():
    routes = set(S.QE.neg_route(c["d_e"], c["flags"]) for c in S.BOUNDARY_CASES if c["model"] == "QuatE")
    assert routes == {"gemm", "bcast", "pair32"}
    assert set(S.EXPECT_ROUTES.values()) == routes


def _check_conditions(c):
    bad, facts = S.conditions(c)
    assert not bad, "\n".join(bad)
    return facts


@pytest.mark.parametrize("c", S.BOUNDARY_CASES, ids=_ID)
def test_boundary_inputs_hold_their_conditions(c):
    facts = _check_conditions(c)
    assert all(f["lists"][0] >= 2 for f in facts), "no entity update list longer than one"
    if c["B"] > 1:
        assert all(f["lists"][1] >= 2 for f in facts), "no relation update list longer than one"
    if c["separated"]:
        assert all(f["ambiguous"] == 0 for f in facts)
    if c["model"] == "TransD":      # (conditions() asserts the residual rows, the traces, the kink clearance and the float32 flips)
        assert all(f["share"] >= S.TD.DIST_SHARE and f["cmax"] < S.TD.C_MAX for f in facts)
        assert all(f["ambiguous"] == 0 and not any(f["excluded"].values()) for f in facts), "TransD leaves out no rows"
        assert not S.bound_factors(c, 0) and not S.bound_factors(c, 1), "the float32 statement is inside every bound: no factor"
    # the float32 statement: within the suite's bounds everywhere but, possibly, at the shapes of `may_relax`
    for step in (0, 1):
        f32 = S.f32_statement_errors(c, step)
        assert set(f32) == set(S.QUANTITIES)
        fac = S.bound_factors(c, step)
        if not S.may_relax(c):
            assert not fac and all(v[0] <= 1.0 for v in f32.values()), {k: v for k, v in f32.items() if v[0] > 1.0}
        for k, v in fac.items():
            assert v == 3.0 * f32[k][0] > 3.0


@pytest.mark.parametrize("seed", range(S.FUZZ_N))
@pytest.mark.parametrize("model", S.MODELS)
def test_random_shapes_hold_their_conditions(model, seed):
    c = S.fuzz_case(model, seed)
    assert c["chunk"] in S.FUZZ_CHUNK and 1 <= c["C"] <= 4 and c["N"] in S.FUZZ_NEG
    if model == "TransD":
        assert c["d_e"] % 8 == 0 and c["d_e"] // 2 in S.FUZZ_WIDTH, "the draw is the half-width"
    else:
        assert c["d_e"] in S.FUZZ_WIDTH
    assert c["oid"] in [x["id"] for x in S.MOD[model].STEP_CASES] and c["flags"] in ((0, S.QE.FORCE_PAIRWISE) if model == "QuatE" else (0,))
    assert not S.may_relax(c)
    _check_conditions(c)


def test_random_shapes_draw_widely():
    cases = [S.fuzz_case(m, s) for m in S.MODELS for s in range(24)]
    assert len(set(c["chunk"] for c in cases)) == len(S.FUZZ_CHUNK) and len(set(c["N"] for c in cases)) == len(S.FUZZ_NEG)
    assert len(set(c["d_e"] for c in cases if c["model"] != "TransD")) == len(S.FUZZ_WIDTH) and set(c["C"] for c in cases) == {1, 2, 3, 4}
    td = [c for c in cases if c["model"] == "TransD"]
    assert len(set(c["d_e"] for c in td)) >= 6 and len(set(c["chunk"] for c in td)) >= 6 and len(set(c["N"] for c in td)) >= 6
    assert any(c["neg_deg"] for c in td) and any(c["pairwise"] for c in td) and any(c["impts"] for c in td)
    assert any(c["chunk"] > S.TD_CR and c["chunk"] % S.TD_CR for c in td) and any(c["N"] > S.TD_CT for c in td)
    assert 0.1 < np.mean([c["impts"] for c in cases]) < 0.5
    assert set(c["flags"] for c in cases if c["model"] == "QuatE") == {0, S.QE.FORCE_PAIRWISE}
    assert any(c["neg_deg"] for c in cases) and any(c["pairwise"] for c in cases)


def test_adding_a_model_leaves_the_other_models_draws_alone():
    """the draws of the first three models, pinned before TransD joined (crc32 of every drawn field of the default 24 seeds)"""
    pins = {"QuatE": 3169575462, "PairRE": 1015180402, "TransH": 798487333}
    for m, pin in pins.items():
        key = [(c["id"], c["C"], c["chunk"], c["N"], c["d_e"], c["oid"], c["impts"], c["flags"], c["n_ent"], c["n_rel"], c["seed"])
               for c in (S.fuzz_case(m, s) for s in range(24))]
        assert zlib.crc32(repr(key).encode()) == pin, m


@pytest.mark.parametrize("c", S.HEAVY_CASES, ids=_ID)
def test_heavy_lists_are_heavy_and_exclude_nothing(c):
    d_e = 104 if c["model"] == "TransD" else 100
    assert (c["B"], c["chunk"], c["N"], c["d_e"], c["n_ent"], c["n_rel"]) == (600, 100, 64, d_e, 3000, 11)
    assert c["chunk"] % 8 != 0
    facts = _check_conditions(c)
    for f in facts:
        assert min(f["lists"]) > 64, f["lists"]
        assert f["ambiguous"] == 0 and not any(f["excluded"].values()), "nothing may be left out of these cases"


# --------------------------------------------------------------------------------------------------------------------------
# ranking
# --------------------------------------------------------------------------------------------------------------------------
def test_ranking_sizes_cross_the_row_and_column_tiles():
    t = lambda x, T: (x + T - 1) // T
    assert t(S.RANK_N, S.RANK_COL_TILE) == 3 and S.RANK_N % S.RANK_COL_TILE == 44
    assert t(S.RANK_E, 128) == 2 and t(S.RANK_E, 64) == 3 and S.RANK_E % 64 == 22
    assert S.RANK_ROW_TILES == {"QuatE": 128, "PairRE": 128, "TransH": 64, "TransD": 64}
    assert S.RANK_BATCHES[0] == S.RANK_E and t(S.RANK_E, S.RANK_BATCHES[1]) == 3, "one call; three calls, two with e0 > 0"
    second = range(S.RANK_CHUNK, min(2 * S.RANK_CHUNK, S.RANK_E))
    assert second[0] // 128 != second[-1] // 128 and second[0] // 64 != second[-1] // 64, "the second chunk spans two row tiles"
    assert t(S.RANK_LIST, S.RANK_COL_TILE) == 2 and len(set(S.rank_list().tolist())) == S.RANK_LIST
    assert max(S.RANK_TOPK) == S.RANK_COL_TILE and min(S.RANK_TOPK) == 1


@pytest.mark.parametrize("model", S.MODELS)
@pytest.mark.parametrize("d_e", S.RANK_WIDTHS)
def test_wide_grid_tables_are_exact_in_float32_and_hold_ties(model, d_e):
    """the three models' own assertions (test_*_inputs.py) at 300 entities / 150 triples, and what the later Ranker batches need"""
    Q = S.MOD[model]
    if model == "QuatE":
        QEI.test_grid_inputs_are_exact_in_float32_and_hold_ties(S.RANK_N, d_e, wide_e=S.RANK_E)
    elif model == "TransD":         # (d_e is the half-width k here, as for transd_cases.tie_inputs)
        TDI.test_grid_inputs_are_exact_in_float32_and_hold_ties(S.RANK_N, d_e, wide_e=S.RANK_E, chunk=S.RANK_CHUNK)
    else:
        (PRI if model == "PairRE" else THI).test_grid_inputs_are_exact_in_float32_and_hold_ties(S.RANK_N, d_e, wide_e=S.RANK_E,
                                                                                                 chunk=S.RANK_CHUNK)
    c = Q.tie_inputs(S.RANK_N, d_e, S.RANK_E)
    width = 2 * d_e if model == "TransD" else d_e
    assert len(c.h) == S.RANK_E and c.d_e == width and c.ent.shape == (S.RANK_N, width) and c.rel.shape == (S.RANK_N, S.rel_width(model, width))
    cols = S.rank_list()
    for neg_head in (False, True):
        p, Sc = Q.tie_scores(c, c.h, c.r, c.t, neg_head)
        p32, S32 = Q.tie_scores(c, c.h, c.r, c.t, neg_head, np.float32)
        assert p32.dtype == np.float32 and S32.dtype == np.float32
        assert np.array_equal(S32 >= p32[:, None], Sc >= p[:, None]), "the float32 statement ranks as the float64 one"
        # ties beyond the first row tile of either kind, and in the rows of the later batches
        m = Sc == p[:, None]
        m[np.arange(S.RANK_E), c.h if neg_head else c.t] = False
        assert m[128:].any() and m[64:128].any(), "no tie in the rows of a later row tile"
        assert m[:, 128:256].any() and m[:, 256:].any(), "no tie in the columns of a later column tile"
        # the explicit list changes the ranks
        raw = Q.ranks_of(p, Sc)
        assert np.any((Sc[:, cols] >= p[:, None]).sum(1) + 1 != raw)
        # the ranks of the later rows differ from what the first row tile's rows would give them
        for bm in (64, 128):
            wrong = 1 + (Sc[np.arange(S.RANK_E) % bm] >= p[:, None]).sum(1)
            assert np.mean(wrong[bm:] != raw[bm:]) > 0.5, "reading the row tile as 0 would go unnoticed"
        lists = Q.filter_lists(c, neg_head)
        assert (lists[0][64:, 1] - lists[0][64:, 0]).min() >= 1 and np.any(Q.ranks_of(p, Sc, lists)[64:] != raw[64:])


@pytest.mark.parametrize("model", S.MODELS)
@pytest.mark.parametrize("d_e", S.RANK_WIDTHS)
def test_random_ranking_tables_give_single_rank_intervals(model, d_e):
    """>= 90 % of the intervals [lo, hi] hold one rank (the own column of a raw ranking set aside: its score IS the positive's), so
    the band cannot hide a wrong rank; raw, filtered and on the explicit list, both sides"""
    c = S.rank_random_inputs(model, d_e)
    tol = 1e-4                                             # tests/test_gpu_eval.py TOL
    if model == "TransD":
        assert c.ent.shape == c.rel.shape == (S.RANK_N, 2 * d_e) == (S.RANK_N, c.d_e) and np.abs(S.TD.c_of(c.ent)).max() < S.TD.C_MAX
    for neg_head in (False, True):
        p, Sc = S.rank_scores(model, c, neg_head)
        assert np.isfinite(Sc).all() and Sc.shape == (S.RANK_E, S.RANK_N)
        own = c.h if neg_head else c.t
        assert np.abs(Sc[np.arange(S.RANK_E), own] - p).max() < 1e-9, "the own column carries the positive's score"
        lists = S.PR.filter_lists(c, neg_head)
        assert (lists[0][:, 1] - lists[0][:, 0]).max() >= 3 and (lists[0][-30:, 1] - lists[0][-30:, 0]).min() >= 2
        for fl in (None, lists):
            for cols in (None, S.rank_list()):
                lo, hi, o = S.rank_band(c, p, Sc, neg_head, fl, cols, tol)
                assert np.all(lo <= hi) and (fl is None or not o.any())
                share = S.degenerate_share(lo, hi, o)
                assert share >= S.RANK_DEGENERATE, "%s d_e %d neg_head %d: only %.3f of the intervals are one rank" % (model, d_e, neg_head, share)
                assert len(set(lo.tolist())) > 20, "the ranks spread"
