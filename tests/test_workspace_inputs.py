"""CPU guard of tests/test_gpu_workspace_contract.py: the carve trace (kge_debug_carve) at every case's shape, and the helpers
that decide which bytes of a guarded buffer belong to no carved buffer (tests/workspace_cases.py)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import workspace_cases as W


def _h():
    import __graft_entry__ as G
    G.build()
    from dglke_amd import _lib
    return _lib.lib()


def _ids():
    from dglke_amd import _lib          # (importing the package does not load the library)
    return [i for i, _ in W.size_cases(None)]


@pytest.mark.parametrize("case", range(len(_ids())), ids=_ids())
def test_traced_layout_of_every_case(case):
    """with gap = 256: buffers ascending, disjoint, each followed by >= 256 bytes of nobody's, the last end + gap rounded up is
    the size function's value; with the setting off the size is today's and nothing is recorded"""
    h = _h()
    name, size = W.size_cases(h)[case]
    plain = size()
    assert plain > 0, name
    with W.Trace(h, W.GAP) as t:
        need = size()
        pairs = t.pairs()
    W.check_layout(pairs, need, W.GAP)
    assert size() == plain, name + ": the size with the setting switched off again"
    assert h.kge_debug_carve_count() == 0
    with W.Trace(h, 0) as t:                         # trace only: today's layout, byte for byte
        assert size() == plain
        p0 = t.pairs()
    W.check_layout(p0, plain, 0)
    assert [n for _, n in p0] == [n for _, n in pairs], name + ": the gap changed a buffer's size"
    m = W.free_mask(pairs, need)
    assert m[:W.GUARD].all() and m[-W.GUARD:].all() and m.sum() >= 2 * W.GUARD + W.GAP * len(pairs)


def test_cases_reach_the_instances_they_name():
    """host arithmetic behind the case table: the two `lc-parts` shapes carve GA in more than one part (their workspace shrinks by
    whole [B, d_e] blocks under KGE_FLAG_TWO_PASS_PAIR), and the top-K shapes have several segments"""
    h = _h()
    for c in W.STEP_CASES:
        if c["id"].endswith("lc-parts"):
            d_e, _ = W.step_dims(c)
            with W.Trace(h, 0) as t:
                W.step_size(h, c)
                ga = t.pairs()[10][1]                 # A Bn asq bsq P dP S PM PS PL GA
            assert ga % (4 * c["B"] * d_e) == 0 and ga // (4 * c["B"] * d_e) > 1, (c["id"], ga)
    for c in W.TOPK_CASES:
        d_e, _ = W.rank_dims(c)
        with W.Trace(h, 0) as t:
            h.kge_topk_workspace_bytes(c["rows"], c["n_cand"], d_e, c["K"])
            part = t.pairs()[3][1]                    # A an bn part
        assert part // (8 * c["rows"] * c["K"]) >= 2, (c["id"], part)


def _define(path, name):
    """the integer value of `#define name` in a file under dgl-ke_amd/csrc"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "dgl-ke_amd", "csrc", path)).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert m, (path, name)
    return int(m.group(1))


def test_selection_rules_behind_the_case_table():
    """the launchers' selection rules are not reachable from the host, so they are restated here on the constants read from the
    sources, and the case table is held to them:
      transr_use_wide / transr_wide_supported (kge_transr.hip, kge_transr_wide.hpp): widths divisible by 4 and <= TW_C, the id /
          weight tables of a workgroup within 16 KB;
      RESCAL_RB / RESCAL_RBN (kge_common.hpp): row blocks of a relation matrix;
      topk_fan, topk_seg_cap, topk_segments, merge_tree (kge_topk.hip): segments per row and merge rounds"""
    TW_C, TW_R = _define("kge_transr_wide.hpp", "TW_C"), _define("kge_transr_wide.hpp", "TW_R")

    def wide(c):
        De, Dr = W.step_dims(c)
        return De % 4 == 0 and Dr % 4 == 0 and De <= TW_C and Dr <= TW_C and c["N"] * 12 + TW_C * 4 <= 16 * 1024
    by_id = {c["id"]: c for c in W.STEP_CASES}
    assert all(wide(by_id[i]) for i in ("TransR-h36-N24", "TransR-36x20", "TransR-36x72")), "no case on the 128 x 208-tile kernels"
    assert not wide(by_id["TransR-18x36"]) and not wide(by_id["TransR-108x216"]), "no case on the 64 x 64 tiles"
    assert W.step_dims(by_id["TransR-18x36"])[0] % 4 != 0 and W.step_dims(by_id["TransR-108x216"])[1] > TW_C     # both reasons
    assert TW_R * 4 + 8 <= 16 * 1024                       # (one id per group at chunk = 8 <= the group cap: ipg = 1)
    RB, RBN = _define("kge_common.hpp", "RESCAL_RB"), _define("kge_common.hpp", "RESCAL_RBN")
    d = {i: W.step_dims(by_id[i])[0] for i in ("RESCAL-h20", "RESCAL-h12", "RESCAL-h18", "RESCAL-h36-N24")}
    assert d["RESCAL-h12"] < RBN < d["RESCAL-h20"] and d["RESCAL-h12"] > RB, d      # fewer / more rows than row blocks
    assert d["RESCAL-h18"] % RB != 0 and d["RESCAL-h20"] % RBN != 0 and d["RESCAL-h36-N24"] > 2 * RBN, d   # rows no multiple of the blocks
    MCAP, BM, BN = _define("kge_topk.hip", "TK_MCAP"), _define("kge_tile_gemm.hpp", "TILE_BM"), _define("kge_tile_gemm.hpp", "TILE_BN")
    MINT = _define("kge_topk.hip", "TK_MIN_TILES")
    fan = lambda K: max(1, MCAP // K - 1)

    def rounds(L, K):
        n = 0
        while True:
            L, n = (L + fan(K) - 1) // fan(K), n + 1
            if L == 1:
                return n

    def segments(rows, N, K):
        rb = max(1, (rows + BM - 1) // BM)
        cap = max(1, min(fan(K), (256 + rb - 1) // rb))
        nbn = (N + BN - 1) // BN
        s = max(1, min(nbn // MINT, cap))
        tps = (nbn + s - 1) // s
        return (nbn + tps - 1) // tps
    for c in W.TOPK_CASES:
        assert segments(c["rows"], c["n_cand"], c["K"]) >= 2, c["id"]
        # a group merges at least its rows' lists (times the segments where the launch merges those too): a lower bound
        assert rounds(c["rows"], c["K"]) >= 2, c["id"]
    assert {c["n_cand"]: segments(c["rows"], c["n_cand"], c["K"]) for c in W.TOPK_CASES} == {1100: 2, 2100: 4}
    for K in (1, 10, 128):
        got = sorted(rounds((n + K - 1) // K, K) for k_, n in W.TOPK_VECTOR if k_ == K and n > K)
        assert got[0] == 1 and got[-1] == 2, (K, got)


def test_selection_rules_of_quate_pairre_transh_behind_the_case_table():
    """restated from the sources, and the case table held to them:
      use_mfma / neg_mfma_supported (kge_api.hip, kge_neg_gemm.hip): of the three only QuatE has a matrix-core route (d_e % 4 == 0)
          next to its pairwise one, so only QuatE sees KGE_FLAG_FORCE_PAIRWISE - PairRE and TransH carve the same layout under it;
      quate_cases.neg_route / vector_packs: the broadcast kernels at d_e % 16 == 0, 16-byte packs where a quarter is a multiple of 4;
      TransH top-K (kge_topk.hip `mf`): the matrix-core tile at d_e % 4 == 0 and d_e >= TILE_BK, the VALU tile below;
      the 32-wide k stages / slabs (TILE_BK; pairre_cases.OP_WIDTHS): 36 leaves a partial one, 260 is past 256"""
    import quate_cases as QT
    h = _h()
    BK = _define("kge_tile_gemm.hpp", "TILE_BK")
    api = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-ke_amd", "csrc", "kge_neg_gemm.hip")).read()
    body = api[api.index("bool neg_mfma_supported("):api.index("bool neg_gemm_fused_loss_supported(")]
    assert "KGE_QUATE" in body and "KGE_PAIRRE" not in body and "KGE_TRANSH" not in body and "d_e % 4 == 0" in body
    topk = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-ke_amd", "csrc", "kge_topk.hip")).read()
    assert "const int mf = D % 4 == 0 && D >= TILE_BK;" in topk and "acc = mf ? ACC_TH : ACC_THV" in topk
    by_id = {c["id"]: c for c in W.MODEL_STEP_CASES}
    for m in W.NEW_MODELS:
        widths = sorted({c["d_e"] for c in W.MODEL_STEP_CASES if c["model"] == m})
        assert widths == [16, 36, 260], (m, widths)
        assert all(d % 4 == 0 for d in widths) and 16 < BK < 36 and 36 % BK != 0 and 260 > 256 and 260 % BK != 0
        tags = {c["id"].split("-", 2)[2] for c in W.MODEL_STEP_CASES if c["model"] == m}
        assert {"N24", "N21", "plain", "neg-deg", "softmax", "hinge-pw", "impts", "w16", "w260"} <= tags, (m, tags)
        assert ("f1" in tags) == (m == "QuatE"), (m, tags)
        for tag, key, val in (("neg-deg", "neg_deg", True), ("softmax", "genre", "Softmax"), ("hinge-pw", "pairwise", True), ("impts", "impts", True)):
            c = by_id["%s-D36-%s" % (m, tag)]
            assert c[key] == val and (tag != "hinge-pw" or c["genre"] == "Hinge"), c["id"]
        assert by_id["%s-D36-N21" % m]["N"] == 21 and not by_id["%s-D36-plain" % m]["outputs"]
    assert QT.neg_route(36, 0) == "gemm" and QT.neg_route(36, W.FORCE_PAIRWISE) == "pair32" and QT.neg_route(16, W.FORCE_PAIRWISE) == "bcast"
    assert QT.vector_packs(16) and not QT.vector_packs(36) and not QT.vector_packs(260)
    assert by_id["QuatE-D36-f1"]["flags"] == W.FORCE_PAIRWISE
    # the layout under the flag: PairRE's and TransH's are their flags = 0 layout, buffer for buffer
    for m in ("PairRE", "TransH"):
        c = by_id["%s-D36-N24" % m]
        lay = []
        for flags in (0, W.FORCE_PAIRWISE):
            with W.Trace(h, W.GAP) as t:
                need = W.model_step_size(h, c, flags=flags)
                lay.append((need, t.pairs()))
        assert lay[0] == lay[1], m
    # what the three models carve beyond the shared step buffers: PairRE three (PW, PGW, Pnrm), TransH eight, four of them stacked
    B, N, d = 40, 24, 36
    with W.Trace(h, 0) as t:
        W.model_step_size(h, by_id["QuatE-D36-N24"])
        nq = t.pairs()
    with W.Trace(h, 0) as t:
        W.model_step_size(h, by_id["PairRE-D36-N24"])
        np_ = t.pairs()
    with W.Trace(h, 0) as t:
        W.model_step_size(h, by_id["TransH-D36-N24"])
        nt = t.pairs()
    assert [n for _, n in np_[-3:]] == [4 * B * d, 4 * B * d, 4 * (B // 8) * N]
    assert [n for _, n in nt[-8:]] == [4 * 2 * B * d, 4 * B, 4 * 2 * B * N, 4 * 2 * B * N, 4 * B, 4 * B, 4 * (B // 8) * N, 4 * 2 * B * d]
    assert len(np_) - 3 == len(nt) - 8 and len(nq) <= len(np_) - 3 + 1


@pytest.mark.parametrize("c", W.MODEL_STEP_CASES + [W.DONOR_TRANSH], ids=lambda c: c["id"])
def test_model_step_cases_hold_the_conditions_of_their_statements(c):
    """every step of every QuatE / PairRE / TransH case - and the steps with the planted known pairs - on the float64 statement
    alone, from the fixed tables: no sign-ambiguous element (PairRE); every distance at least DIST_SHARE of sqrt(alpha + beta) and no
    gradient row a cancellation residual (TransH).  Nothing is excluded."""
    Q = W.model_cases(c["model"])
    ent, rel = W.model_tables(c)
    bts = W.model_batches(c)
    assert [bt["neg_head"] for bt in bts] == [False, True] and all(len(bt["h"]) == c["B"] and len(bt["neg"]) == c["B"] // c["chunk"] * c["N"] for bt in bts)
    assert all((bt["w"] is not None) == c["impts"] for bt in bts)
    for known in ((False, True) if c is W.MODEL_KNOWN_CASES.get(c["model"]) else (False,)):
        for bt in bts:
            e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
            kn = Q.planted_known(bt, c["chunk"], c["N"])[1] if known else None
            out = Q.step(c, e64, np.zeros(len(e64)), r64, np.zeros(len(r64)), bt, kn)
            W.model_conditions(c, out)
            assert all(np.isfinite(out[k]).all() for k in ("pos_score", "neg_score", "g_pos_ent", "g_neg", "g_rel")) and np.abs(out["g_neg"]).max() > 0
    # entities and relations repeat inside a batch and among the negatives: the update walks lists longer than one
    ids = lambda bt: np.concatenate([bt["h"], bt["t"], bt["neg"]])
    assert all(len(np.unique(ids(bt))) < len(ids(bt)) for bt in bts) and all(len(np.unique(bt["r"])) < c["B"] for bt in bts)


@pytest.mark.parametrize("c", W.MODEL_REL_CASES, ids=lambda c: c["id"])
def test_traced_layout_of_quate_relation_ranking(c):
    """kge_rank_rel_workspace_bytes does not answer for QuatE (a QuatE call takes the DistMult layout followed by the normalised
    relation table), so there is no size function to trace: the entry itself is, refused one byte short before any launch.  Its
    buffers are ascending, disjoint and gapped, the DistMult buffers first, and end at workspace_cases.rel_need - without the gap the
    bytes of _lib.rank_rel_workspace_bytes"""
    from dglke_amd import _lib
    h = _h()
    one, d = 1, c["d_e"]
    assert _lib.model_id("QuatE") == W.QUATE_ID and _lib.model_id("DistMult") == W.DISTMULT_ID
    for gap in (W.GAP, 0):
        with W.Trace(h, gap) as t:
            base = int(h.kge_rank_rel_workspace_bytes(W.DISTMULT_ID, W.RANK_EB, W.TIE_N, d, d))
            p0 = t.pairs()
            need = W.rel_need(h, W.QUATE_ID, W.RANK_EB, W.TIE_N, d, d, gap)
            t.reset()
            args = lambda n: (W.QUATE_ID, one, W.TIE_N, one, W.TIE_N, None, one, one, one, W.TIE_E, d, d, 0.0, 1.0, one, one, W.RANK_EB, one, None, one, n, 0, None)
            assert h.kge_rank_rel_eval(*args(need - 1)) == W.ERR_WORKSPACE
            p1 = t.pairs()
        W.check_layout(p1, need, gap)
        assert p1[:len(p0)] == p0 and len(p1) == len(p0) + 1 and p1[-1][1] == 4 * W.TIE_N * d and need > base
        if gap == 0:
            assert need == _lib.rank_rel_workspace_bytes(W.QUATE_ID, W.RANK_EB, W.TIE_N, d, d)
    assert W.WS_ENTRIES["kge_rank_rel_eval"].more([W.QUATE_ID]) == 1 and W.WS_ENTRIES["kge_rank_rel_eval"].more([W.DISTMULT_ID]) == 0


@pytest.mark.parametrize("cid", sorted({o["case"] for o in W.OPTIM_ADAM}))
def test_optim_cases_keep_the_ambiguity_cap(cid):
    """the steps the kge_step_optim cases run, on adam_cases.step in float64: the ambiguity rule takes out at most AMBIGUITY_CAP of
    either table; TransH keeps its distance condition; the table names the models, widths and options it says"""
    import adam_cases as A
    import transh_cases as TH
    from dglke_amd import _lib
    c = W.optim_case(cid)
    d_e, d_r = A.widths(c)
    assert d_e % 4 == 0 and d_r % 4 == 0 and max(d_e, d_r) <= _lib.ADAM_MAX_DIM
    ent, rel = A.tables(c)
    st = A.zero_state(c, ent, rel)
    amb = dict(ent=np.zeros(ent.shape, bool), rel=np.zeros(rel.shape, bool))
    for bt in A.batches(c, W.OPTIM_STEPS):
        known = A.known_pairs(c, bt)[0] if c["known"] else None
        with TH.adam_gradients():
            info = A.step(c, st, bt, known)
        if c["model"] == "TransH":
            assert info["out"]["share"] >= TH.DIST_SHARE
        for tab in ("ent", "rel"):
            amb[tab] |= A.ambiguous(info[tab][0], info[tab][1], amb[tab].shape[0])
            assert amb[tab].mean() <= A.AMBIGUITY_CAP, "%s: %.4f of %s is ambiguous" % (cid, amb[tab].mean(), tab)
        assert len(info["ent"][0]) < c["n_ent"], "no untouched entity row"


def test_optim_table_names_what_it_says():
    import adam_cases as A
    cases = {o["id"]: (W.optim_case(o["case"]), o["phases"]) for o in W.OPTIM_ADAM}
    assert {c["model"] for c, _ in cases.values()} >= {"TransE_l2", "TransE_l1", "DistMult", "ComplEx", "QuatE", "PairRE", "TransH"}
    assert any(max(A.widths(c)) > 512 for c, _ in cases.values()) and any(ph for _, ph in cases.values())
    assert any(c["known"] and not ph for c, ph in cases.values()) and any(c["known"] and ph for c, ph in cases.values())
    assert any(W.optim_case(i)["known"] for i in W.OPTIM_ADAGRAD) and not all(W.optim_case(i)["known"] for i in W.OPTIM_ADAGRAD)
    e = W.WS_ENTRIES["kge_step_optim"]
    assert (e.ws, e.phases, e.known) == (5, 7, 8)


@pytest.mark.parametrize("c", W.SAMPLING_CASES, ids=lambda c: c["id"])
def test_tail_scratch_layout(c):
    """the sampler job's tail scratch has a fixed layout (no allocator, so no trace and no gap): the six arrays of
    workspace_cases.tail_scratch_layout are ascending, disjoint, inside kge_sampler_tail_scratch_bytes and end exactly there; the key
    width the case names is the one the size function assumes; the batch fits the tail jobs' element cap"""
    h = _h()
    C_ = c["B"] // c["chunk"]
    need = int(h.kge_sampler_tail_scratch_bytes(c["B"], C_, c["N"], c["n_ent"]))
    arrays, total = W.tail_scratch_layout(c["B"], C_ * c["N"], c["n_ent"])
    assert total == need, (c["id"], total, need)
    end = 0
    for off, n in arrays:
        assert off % 32 == 0 and off >= end and n > 0
        end = off + n
    assert end <= need < end + 32
    assert (c["id"] == "k64") == (c["n_ent"] > 1 << (32 - W.SP_CODE_BITS))
    other = int(h.kge_sampler_tail_scratch_bytes(c["B"], C_, c["N"], 1 << 30 if c["id"] != "k64" else 1000))
    assert (other > need) == (c["id"] != "k64"), "64-bit keys take more room than 32-bit ones"
    assert 2 * c["B"] + C_ * c["N"] <= 4096
    if c["id"] == "k32-big-bucket":      # a bucket can hold more than 4 keys per thread of a 256-thread workgroup
        assert c["skewed"] and 2 * c["B"] + C_ * c["N"] > 1024


def test_setting_is_thread_local_and_goes_off():
    h = _h()
    plain = int(h.kge_topk_workspace_bytes(4, 1000, 32, 10))
    seen = {}
    with W.Trace(h, W.GAP) as t:
        here = int(h.kge_topk_workspace_bytes(4, 1000, 32, 10))

        def other():
            seen["size"] = int(h.kge_topk_workspace_bytes(4, 1000, 32, 10))
            seen["count"] = int(h.kge_debug_carve_count())
        th = threading.Thread(target=other)
        th.start()
        th.join()
        assert t.count() == 8
    assert here > plain and seen == dict(size=plain, count=0)
    assert int(h.kge_topk_workspace_bytes(4, 1000, 32, 10)) == plain and h.kge_debug_carve_count() == 0
    # more buffers than the trace holds: counted, not recorded
    buf = (C.c_int64 * 4)(*([-7] * 4))
    assert h.kge_debug_carve(C.cast(buf, C.c_void_p), 1, 0) == 0
    assert int(h.kge_topk_workspace_bytes(4, 1000, 32, 10)) == plain
    assert h.kge_debug_carve_count() == 8 and list(buf)[2:] == [-7, -7] and buf[0] == 0
    assert h.kge_debug_carve(None, 3, 0) == W.ERR_ARG          # a capacity without a trace: refused, the setting stays
    assert h.kge_debug_carve(None, 0, 0) == 0
    assert h.kge_debug_carve_count() == 0


def test_an_entry_and_its_size_function_agree_with_the_gap():
    """ws_bytes one below the gapped size is refused before any launch (no GPU needed: the check precedes them), the gapped size
    itself passes the check on an entry with nothing to do"""
    h = _h()
    one = 1
    with W.Trace(h, W.GAP):
        need = int(h.kge_topk_workspace_bytes(0, 1000, 0, 10))
        assert h.kge_topk_vector(one, 1000, 10, one, one, one, need - 1, None) == W.ERR_WORKSPACE
        nn = int(h.kge_score_neg_workspace_bytes(2, 2, 8, 24, 36))
        assert h.kge_score_neg_fwd(2, 0, one, one, one, 2, 8, 24, 36, 36, 8.0, 1.0, one, one, nn - 1, 0, None) == W.ERR_WORKSPACE
        assert h.kge_loss_fwd_bwd(0, 0, 1.0, 0, 1.0, one, one, None, 37, 21, one, one, one, one,
                                  W.WS_ENTRIES["kge_loss_fwd_bwd"].need(h, [0] * 8 + [37, 21, one], W.GAP) - 1, None) == W.ERR_WORKSPACE


def test_guard_and_gap_helpers_find_planted_stray_writes():
    pairs, gap = [(0, 100), (512, 256), (1024, 4)], 256
    need = W.al(1024 + 4 + gap)
    W.check_layout(pairs, need, gap)
    m = W.free_mask(pairs, need)
    assert m.sum() == 2 * W.GUARD + need - 360
    for value in (0, 0xFF):
        buf = np.full(W.GUARD + need + W.GUARD, value, np.uint8)
        buf[W.GUARD:W.GUARD + 100] = 7                           # the buffers themselves may hold anything
        buf[W.GUARD + 512:W.GUARD + 768] = 9
        assert len(W.stray_bytes(buf, m, value)) == 0
        for at, what in ((-1, "FRONT"), (100, "past the end of buffer 0"), (768, "past the end of buffer 1"), (1028, "past the end of buffer 2"),
                         (need - 1, "past the end of buffer 2"), (need, "BEHIND"), (need + W.GUARD - 1, "BEHIND")):
            b = buf.copy()
            b[W.GUARD + at] ^= 0x10
            s = W.stray_bytes(b, m, value)
            assert list(s) == [at] and what in W.describe_stray(s, pairs, need), (at, W.describe_stray(s, pairs, need))
    # the async workspace: the same layout in both halves
    m2 = W.free_mask(pairs, 2 * need, halves=2)
    assert not m2[W.GUARD + need + 512] and m2[W.GUARD + need + 100] and m2.sum() == 2 * W.GUARD + 2 * (need - 360)
    for bad in ([(0, 100), (256, 4)], [(0, 100), (512, 4), (512, 4)]):           # too close / overlapping
        with pytest.raises(AssertionError):
            W.check_layout(bad, W.al(bad[-1][0] + 4 + gap), gap)
    with pytest.raises(AssertionError):
        W.check_layout(pairs, need + 256, gap)
    with pytest.raises(AssertionError):
        W.free_mask([(0, need + 1)], need)
