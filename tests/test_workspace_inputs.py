"""CPU guard of tests/test_gpu_workspace_contract.py: the carve trace (kge_debug_carve) at every case's shape, and the helpers
that decide which bytes of a guarded buffer belong to no carved buffer (tests/workspace_cases.py)."""
import ctypes as C
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
