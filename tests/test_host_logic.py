"""CPU tests of the host logic: the batch plan, the C-ABI surface of libkge_hip.so (symbols only -
no compute without a GPU), the torch-CPU port used as cpu_baseline, the no-CPU-fallback rule."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from golden_util import golden_names, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    declared = set(re.findall(r"\b(kge_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(h, name), "libkge_hip.so does not export " + name
    assert declared == set(_lib.EXPORTED_SYMBOLS), (declared ^ set(_lib.EXPORTED_SYMBOLS))
    assert _lib.lib().kge_abi_version() == _lib.KGE_ABI_VERSION == 8


def test_argument_errors_are_reported_without_a_gpu():
    from dglke_amd import _lib
    h = _lib.lib()
    rc = h.kge_gather_rows(None, 0, 4, None, 0, None, None)
    assert rc == -1 and b"kge_gather_rows" in h.kge_last_error()
    rc = h.kge_score_pos(3, 1, 1, 1, 2, 6, 4, 1.0, 1.0, 1, None)   # ComplEx with d_r != d_e
    assert rc == -1 and b"ComplEx" in h.kge_last_error()
    rc = h.kge_score_pos(9, 1, 1, 1, 2, 4, 4, 1.0, 1.0, 1, None)
    assert rc == -1 and b"unknown model" in h.kge_last_error()


def test_product_has_no_cpu_fallback():
    from dglke_amd import _lib, ops
    from dglke_amd.engine import StepEngine
    with pytest.raises(_lib.KgeError):
        ops.gather_rows(torch.zeros(4, 4), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(_lib.KgeError):
        StepEngine("TransE_l2", 10, 2, 8, 12.0, 0.1, "cpu")
    # nothing in the product imports the oracle
    for dirpath, _, files in os.walk(os.path.join(ROOT, "dgl-ke_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def _check_plan(p):
    B, C, N = p["B"], p["C"], p["N"]
    ue = p["ue_id"]
    assert np.all(np.diff(ue) > 0)
    assert set(ue) == set(p["nid"]) | set(p["neg_ids"])
    # every edge end appears exactly once, under the right entity
    seen = np.zeros(2 * B, bool)
    for u in range(p["UE"]):
        for k in range(p["ue_pos_ptr"][u], p["ue_pos_ptr"][u + 1]):
            code = p["ue_pos_adj"][k]
            e, side = code >> 1, code & 1
            assert (p["t_gid"][e] if side else p["h_gid"][e]) == ue[u]
            assert not seen[code]
            seen[code] = True
        slots = p["ue_neg_slot"][p["ue_neg_ptr"][u]:p["ue_neg_ptr"][u + 1]]
        assert np.all(p["neg_ids"][slots] == ue[u]) and np.all(np.diff(slots) > 0)
    assert seen.all() and p["ue_neg_ptr"][-1] == C * N
    seen_e = np.zeros(B, bool)
    for u in range(p["UR"]):
        es = p["ur_edge"][p["ur_ptr"][u]:p["ur_ptr"][u + 1]]
        assert np.all(p["rel_ids"][es] == p["ur_id"][u]) and np.all(np.diff(es) > 0)
        seen_e[es] = True
    assert seen_e.all()
    assert np.array_equal(p["nid"][p["h_local"]], p["h_gid"])
    assert np.array_equal(p["nid"][p["t_local"]], p["t_gid"])


@pytest.mark.parametrize("n_ent,n_rel,B,N,chunk", [(50, 3, 16, 4, 4), (5, 1, 12, 3, 6), (14951, 1345, 1000, 200, 200)])
def test_plan_groups_every_row_once(n_ent, n_rel, B, N, chunk):
    from dglke_amd import plan
    rng = np.random.RandomState(0)
    h, t = rng.randint(0, n_ent, B), rng.randint(0, n_ent, B)
    r = rng.randint(0, n_rel, B)
    neg = rng.randint(0, n_ent, (B // chunk) * N)
    p = plan.build_plan(h, t, r, neg, chunk, N, True)
    _check_plan(p)
    with pytest.raises(ValueError):
        plan.build_plan(h[:-1], t[:-1], r[:-1], neg, chunk, N, True)     # ragged batch is rejected
    with pytest.raises(ValueError):
        plan.build_plan(h, t, r, neg[:-1], chunk, N, True)


def test_sampler_alternates_corruption_side_and_covers_epochs():
    """dataloader/sampler.py:853-859: step 1 corrupts tails, step 2 heads, ..."""
    from dglke_amd.dataloader import UniformChunkedSampler
    rng = np.random.RandomState(0)
    n = 100
    s = UniformChunkedSampler(rng.randint(0, 30, n), rng.randint(0, 4, n), rng.randint(0, 30, n), 30,
                              batch_size=16, neg_sample_size=4, device="cpu", seed=1)
    plans = s.next_plans(12)
    assert [p["neg_head"] for p in plans[:4]] == [0, 1, 0, 1]
    assert all(p["B"] == 16 and p["C"] == 4 and p["neg_ids"].shape[0] == 16 for p in plans)
    for p in plans:
        _check_plan(p)


@pytest.mark.parametrize("name", [n for n in golden_names(transr=False) if not any(
    k in n for k in ("logistic", "hinge", "bce", "impts"))])
def test_torch_port_matches_reference(name):
    """the cpu_baseline port reproduces the reference step (same torch ops)."""
    from oracle import torch_port
    z, case = load_golden(name)
    m = torch_port.TorchPort(case["model"], case["n_ent"], case["n_rel"], case["hidden"], case["gamma"],
                             case["lr"], case["de"], case["dr"], case["adv"], case["adv_temp"],
                             case["reg_coef"], case["reg_norm"])
    m.ent = torch.from_numpy(z["init_entity"].copy())
    m.rel = torch.from_numpy(z["init_relation"].copy())
    torch.set_num_threads(1)
    for s in range(1, case["steps"] + 1):
        p = "s%d_" % s
        pl = dict(nid=z[p + "nid"], rel_ids=z[p + "r"], neg_ids=z[p + "neg"], h_local=z[p + "h_local"],
                  t_local=z[p + "t_local"], C=case["B"] // case["chunk"], chunk=case["chunk"],
                  N=case["N"], neg_head=int(z[p + "neg_head"]))
        out = m.step(pl)
        np.testing.assert_allclose(out["neg_score"], z[p + "neg_score"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(out["g_neg"], z[p + "g_neg"], rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(out["log"][2], z[p + "log"][2], rtol=1e-5)
    np.testing.assert_allclose(m.ent.numpy(), z["final_entity"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(m.rel.numpy(), z["final_relation"], rtol=1e-4, atol=1e-5)


def test_dist_make_comm_without_gpu_is_the_c10d_wrapper_and_stream_override_nests():
    """dist.make_comm(): no GPU (or KGE_DIST_COMM=torch) -> the torch.distributed wrappers; _lib.use_stream() returns the
    previous override so that sections nest"""
    from dglke_amd import dist as kd, _lib
    import torch
    if not torch.cuda.is_available():
        assert isinstance(kd.make_comm(), kd.TorchComm)
    assert isinstance(kd.make_comm(kind="torch"), kd.TorchComm)
    assert _lib.use_stream(123) is None
    assert _lib.stream_ptr() == 123
    assert _lib.use_stream(456) == 123 and _lib.stream_ptr() == 456
    assert _lib.use_stream(None) == 456
    assert kd.default_cap(3000, 8, 1.5) % 64 == 0 and kd.default_cap(3000, 8, 1.5) >= 3000 * 1.5 / 8


def test_workspace_accounts_for_the_gradient_parts_of_the_shared_pair_backward():
    """kge_step_workspace_bytes (host arithmetic only): RotatE / TransE_l1 reserve room for GA in parts (the shared-pair backward
    splits a chunk's negatives over workgroups, kge_neg_bcast.hip neg_bwd_lc_splits) - exactly (parts - 1) more [B, d_e] blocks
    than with the two-pass kernels, a whole number of them and at most 7; the matrix-core models reserve none"""
    import ctypes as C
    from dglke_amd import _lib
    L = _lib.lib()

    def ws(model, d_e, d_r, B, Cn, chunk, N, flags):
        hp = _lib.KgeHParams()
        hp.model, hp.d_e, hp.d_r, hp.flags = _lib.model_id(model), d_e, d_r, flags
        hp.gamma, hp.lr, hp.adv_temp, hp.reg_norm = 12.0, 0.1, 1.0, 3
        return L.kge_step_workspace_bytes(C.byref(hp), B, Cn, chunk, N, 2 * B + Cn * N, B)
    for model, d_e, d_r, B, Cn, chunk, N in (("RotatE", 400, 200, 1024, 4, 256, 256), ("RotatE", 800, 400, 1024, 4, 256, 256),
                                           ("TransE_l1", 400, 400, 1000, 5, 200, 200)):
        full, two_pass = ws(model, d_e, d_r, B, Cn, chunk, N, 0), ws(model, d_e, d_r, B, Cn, chunk, N, _lib.FLAG_TWO_PASS_PAIR)
        extra = full - two_pass
        block = B * d_e * 4
        assert extra > 0 and extra % block == 0 and 1 <= extra // block <= 7, (model, extra, block)
    for model in ("TransE_l2", "DistMult", "ComplEx"):
        d_e = 400
        assert ws(model, d_e, d_e if model != "ComplEx" else d_e, 1000, 5, 200, 200, 0) == \
               ws(model, d_e, d_e if model != "ComplEx" else d_e, 1000, 5, 200, 200, _lib.FLAG_TWO_PASS_PAIR)


# (B, C, chunk, N, n_cand) -> model -> (d_e, d_r, kge_step_workspace_bytes at flags 0 / 1 / 16 / 32, kge_step_async_workspace_bytes at
# the same flags, kge_score_neg_workspace_bytes, kge_rank_workspace_bytes(B, n_cand, d_e)), with UE = 2 B + C N and UR = B.  The
# values are those of the library before each workspace got its single carve function (kge_api.hip carve_step / carve_neg /
# carve_rank): what callers allocate must not move.  Second shape: the FB15k recipes (bench.py WORKLOADS widths for RESCAL / TransR).
_WORKSPACE_BYTES = {
    (64, 4, 16, 16, 500): {
        "TransE_l1": (64, 64, (138496, 138496, 138496, 192768), (375296, 375296, 375296, 483840), 53760, 1211904),
        "TransE_l2": (64, 64, (122112, 122112, 122112, 160000), (342528, 342528, 342528, 418304), 37376, 1211904),
        "DistMult": (64, 64, (122112, 122112, 122112, 160000), (342528, 342528, 342528, 418304), 37376, 1211904),
        "ComplEx": (64, 64, (122112, 122112, 122112, 160000), (342528, 342528, 342528, 418304), 37376, 1211904),
        "RotatE": (64, 32, (130304, 130304, 130304, 184576), (342528, 342528, 342528, 451072), 53760, 1211904),
        "SimplE": (64, 64, (122112, 122112, 122112, 160000), (342528, 342528, 342528, 418304), 37376, 1211904),
        "RESCAL": (16, 256, (191488, 191488, 191488, 209408), (530432, 530432, 530432, 566272), 12800, 1187328),
        "TransR": (16, 24, (477184, 477184, 477184, 782848), (983040, 983040, 983040, 1594368), 12800, 1187328),
    },
    (1000, 5, 200, 200, 14951): {
        "TransE_l1": (400, 400, (23397376, 23397376, 20197376, 35545088), (56394752, 56394752, 49994752, 80690176), 12008192, 79456256),
        "TransE_l2": (400, 400, (12197376, 12197376, 12197376, 16345088), (33994752, 33994752, 33994752, 42290176), 4008192, 79456256),
        "DistMult": (400, 400, (12197376, 12197376, 12197376, 16345088), (33994752, 33994752, 33994752, 42290176), 4008192, 79456256),
        "ComplEx": (400, 400, (12197376, 12197376, 12197376, 16345088), (33994752, 33994752, 33994752, 42290176), 4008192, 79456256),
        "RotatE": (400, 200, (28997376, 28997376, 22597376, 44345088), (65994752, 65994752, 53194752, 96690176), 15208192, 79456256),
        "SimplE": (400, 400, (12197376, 12197376, 12197376, 16345088), (33994752, 33994752, 33994752, 42290176), 4008192, 79456256),
        "RESCAL": (500, 250000, (85186560, 85186560, 85186560, 92141824), (2178373632, 2178373632, 2178373632, 2192284160), 4808448, 80256512),
        "TransR": (200, 200, (265901824, 265901824, 265901824, 360473600), (536603648, 536603648, 536603648, 725747200), 2408192, 77856256),
    },
}


def test_workspace_sizes_are_the_recorded_ones():
    """the four *_workspace_bytes functions (host arithmetic only, no step call) over the eight models, flags {0, FORCE_PAIRWISE,
    TWO_PASS_PAIR, NEG_DEG_SAMPLE} and two shapes return the recorded byte counts exactly"""
    import ctypes as C
    from dglke_amd import _lib
    L = _lib.lib()
    flags = (0, _lib.FLAG_FORCE_PAIRWISE, _lib.FLAG_TWO_PASS_PAIR, _lib.FLAG_NEG_DEG_SAMPLE)
    assert flags == (0, 1, 16, 32)
    for (B, Cn, chunk, N, n_cand), models in _WORKSPACE_BYTES.items():
        assert len(models) == 8
        for model, (d_e, d_r, step, asy, score_neg, rank) in models.items():
            for k, fl in enumerate(flags):
                hp = _lib.KgeHParams()
                hp.model, hp.d_e, hp.d_r, hp.flags = _lib.model_id(model), d_e, d_r, fl
                hp.gamma, hp.lr, hp.adv_temp, hp.reg_norm = 12.0, 0.1, 1.0, 3
                args = (C.byref(hp), B, Cn, chunk, N, 2 * B + Cn * N, B)
                assert L.kge_step_workspace_bytes(*args) == step[k], (model, B, fl)
                assert L.kge_step_async_workspace_bytes(*args) == asy[k], (model, B, fl)
            assert L.kge_score_neg_workspace_bytes(_lib.model_id(model), Cn, chunk, N, d_e) == score_neg, (model, B)
            assert L.kge_rank_workspace_bytes(B, n_cand, d_e) == rank, (model, B)


def test_inline_assembly_wide_stores_carry_their_wait_states():
    """a 128-bit global store written as inline assembly must be followed by two wait states before its data registers may be
    overwritten (gfx940+ VMEM store-data hazard) - the compiler does not see inside the asm statement, so the statement itself
    carries the s_nop (kge_common.hpp st_wt<4>; found in round 3 when three such stores ran back to back)"""
    import re
    src_dir = os.path.join(ROOT, "dgl-ke_amd", "csrc")
    n = 0
    for f in os.listdir(src_dir):
        if not f.endswith((".hip", ".hpp")):
            continue
        for m in re.finditer(r'asm\s+volatile\(\s*"((?:[^"\\]|\\.)*)"', open(os.path.join(src_dir, f)).read()):
            text = m.group(1)
            if re.search(r"(global|flat|buffer)_store_dwordx[34]", text):
                n += 1
                assert "s_nop" in text, "%s: wide store without wait states: %s" % (f, text)
    assert n >= 1


def test_kernel_sources_have_one_build_configuration():
    """the kernel sources compile one way: the only macros a preprocessor conditional may test are the developer timeline's
    (kge_common.hpp).  A tuning probe or an A/B alternative lives in a working copy and a variant library (tools/build_variant.sh),
    not behind a -D in the shipped kernels."""
    src_dir = os.path.join(ROOT, "dgl-ke_amd", "csrc")
    tested, files = set(), [f for f in sorted(os.listdir(src_dir)) if f.endswith((".hip", ".hpp"))]
    assert files
    for f in files:
        text = open(os.path.join(src_dir, f)).read().replace("\\\n", " ")
        for m in re.finditer(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif)\b(.*)$", text, re.M):
            cond = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
            names = set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}
            assert names or m.group(1) in ("if", "elif"), "%s: %s" % (f, m.group(0))
            tested |= {(n, f) for n in names}
    extra = sorted((n, f) for n, f in tested if n not in ("KGE_TIMELINE", "KGE_TL_MARKS"))
    assert not extra, "conditional compilation on %s" % extra
    assert {n for n, _ in tested} == {"KGE_TIMELINE", "KGE_TL_MARKS"}      # (the scan does see conditionals)


def test_makefile_and_build_compile_the_same_sources():
    """csrc/Makefile's SRCS (which tools/build_variant*.sh follow) and __graft_entry__.SOURCES (which build() follows) name the
    same files, and every one of them exists: a variant library exports what dglke_amd/_lib.py binds"""
    import __graft_entry__
    src_dir = os.path.join(ROOT, "dgl-ke_amd", "csrc")
    lines = [m.group(1) for m in re.finditer(r"^SRCS[ \t]*=[ \t]*(.*)$", open(os.path.join(src_dir, "Makefile")).read(), re.M)]
    assert len(lines) == 1, lines
    srcs = lines[0].split()
    assert len(set(srcs)) == len(srcs) and set(srcs) == set(__graft_entry__.SOURCES)
    assert all(os.path.isfile(os.path.join(src_dir, s)) for s in srcs)


def _lc_balanced_map(ncol, ngr, P, nB):
    """Python statement of the block -> (column, part, groups) map of the shared-pair backward's balanced split
    (dgl-ke_amd/csrc/kge_neg_bcast.hip, neg_bwd_lc_kernel, NegArgs::lc_P): 1024 block ids, rounds of 256, odd rounds reversed,
    classes in descending part size."""
    nA = ncol - nB
    remB, remA = ngr % P, ngr % (P + 1)
    n1, n2, n3 = nB * remB, nB * (P - remB), nA * remA
    out = []
    for b in range(1024):
        k, rnd = b & 255, b >> 8
        t = (rnd << 8) + ((255 - k) if (rnd & 1) else k)
        if t < n1:
            col, j, nsp = t // remB, t % remB, P
        elif t < n1 + n2:
            t -= n1
            col, j, nsp = t // (P - remB), remB + t % (P - remB), P
        elif t < n1 + n2 + n3:
            t -= n1 + n2
            col, j, nsp = nB + t // remA, t % remA, P + 1
        else:
            t -= n1 + n2 + n3
            col, j, nsp = nB + t // (P + 1 - remA), remA + t % (P + 1 - remA), P + 1
        base, rem = ngr // nsp, ngr % nsp
        g_lo = j * base + min(j, rem)
        out.append((col, j, nsp, g_lo, g_lo + base + (1 if j < rem else 0)))
    return out


def test_balanced_split_map_covers_every_group_once_and_balances_the_cus():
    """every column's quad groups are covered exactly once by its P or P + 1 parts, and the four block ids that share a CU
    (k, k + 256, k + 512, k + 768) carry almost equal work - the property the dealing order exists for"""
    for ncol, ngr in [(224, 16), (416, 16), (208, 16), (320, 8), (192, 16), (832, 16), (325, 7), (513, 9), (1023, 4)]:
        P = 1024 // ncol
        nA = 1024 - ncol * P
        if nA == 0:
            continue
        nB = ncol - nA
        m = _lc_balanced_map(ncol, ngr, P, nB)
        cover = {}
        for col, j, nsp, lo, hi in m:
            assert 0 <= col < ncol and 0 <= j < nsp and nsp == (P if col < nB else P + 1)
            assert 0 <= lo <= hi <= ngr
            cover.setdefault(col, []).append((lo, hi, j))
        assert len(cover) == ncol
        for col, parts in cover.items():
            parts.sort()
            assert len(parts) == (P if col < nB else P + 1) and sorted(p[2] for p in parts) == list(range(len(parts)))
            assert parts[0][0] == 0 and parts[-1][1] == ngr
            assert all(parts[i][1] == parts[i + 1][0] for i in range(len(parts) - 1))
        per_cu = [sum(m[k + 256 * r][4] - m[k + 256 * r][3] for r in range(4)) for k in range(256)]
        sizes = sorted(hi - lo for _, _, _, lo, hi in m)
        assert max(per_cu) - min(per_cu) <= 2 * (sizes[-1] - sizes[0]), (ncol, ngr, min(per_cu), max(per_cu))


def test_device_filter_lists_equal_the_host_lists():
    """eval.build_filter_device (one composite key through torch.unique - runs on any torch device, here the CPU) returns the lists
    of eval.build_filter (np.lexsort): unique (key, entity) pairs in the same order, the same [left, right) range per test triple -
    duplicates among the known triples, test triples without any known match, both corruption sides; None when the composite
    key would not fit int64."""
    import numpy as np
    import torch
    from dglke_amd import eval as E
    rng = np.random.RandomState(3)
    n_ent, n_rel = 97, 7
    known = tuple(rng.randint(0, n, 4000) for n in (n_ent, n_rel, n_ent))           # many duplicates
    test = (np.concatenate([known[0][:300], rng.randint(0, n_ent, 50)]), np.concatenate([known[1][:300], rng.randint(0, n_rel, 50)]),
            np.concatenate([known[2][:300], rng.randint(0, n_ent, 50)]))
    for neg_head in (True, False):
        want = E.build_filter(known[0], known[1], known[2], test[0], test[1], test[2], neg_head, n_rel)
        got = E.build_filter_device(known, test, neg_head, n_rel, n_ent, torch.device("cpu"))
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.int64
        assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])
    # Freebase-sized id spaces (the composite key would overflow): two stable sorts give the same lists
    E._FORCE_TWO_KEY_SORT = True
    try:
        for neg_head in (True, False):
            want = E.build_filter(known[0], known[1], known[2], test[0], test[1], test[2], neg_head, n_rel)
            got = E.build_filter_device(known, test, neg_head, n_rel, n_ent, torch.device("cpu"))
            assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])
    finally:
        E._FORCE_TWO_KEY_SORT = False
    big = E.build_filter_device(tuple(np.asarray(x[:50]) for x in known), tuple(np.asarray(x[:5]) for x in test), True, 14824, 86054151,
                                torch.device("cpu"))
    assert big is not None and big[0].shape == (5, 2)
    assert E.build_filter_device(known, test, True, 1 << 40, 1 << 30, torch.device("cpu")) is None


# ---- dglke_train / dglke_eval driver: the step marks of the training loop and the evaluation setup ------------------------------

def test_step_marks_against_hand_written_lists():
    from dglke_amd.train import step_marks
    assert step_marks(1250, 500, 1000, True) == [500, 1000, 1250]
    assert step_marks(1250, 500, 1000, False) == [500, 1000, 1250]
    assert step_marks(1250, 500, 300, True) == [300, 500, 600, 900, 1000, 1200, 1250]
    assert step_marks(1250, 500, 300, False) == [500, 1000, 1250]           # --eval_interval counts with --valid only
    assert step_marks(400, 1000, 10000, True) == [400]
    # --force_sync_interval 150 where it applies (lanes on one GPU, several GPUs) and where it does not
    assert step_marks(600, 300, 10000, False, 150, True) == [150, 300, 450, 600]
    assert step_marks(500, 300, 10000, False, 150, True) == [150, 300, 450, 500]
    assert step_marks(600, 300, 10000, False, 150, False) == [300, 600]
    assert step_marks(600, 300, 10000, False, -1, True) == [300, 600]         # the flag's default: never


class _Splits(object):
    def __init__(self, n_entities, n_train, n_valid, n_test, seed=0):
        rng = np.random.RandomState(seed)
        self.n_entities, self.n_relations = n_entities, 7

        def trip(n):
            return None if n is None else (rng.randint(0, n_entities, n), rng.randint(0, 7, n), rng.randint(0, n_entities, n))
        self.train, self.valid, self.test = trip(n_train), trip(n_valid), trip(n_test)


def _eval_args(**kw):
    import argparse
    a = dict(model_name='TransE_l2', eval_percent=1, seed=5, eval_filter=True, batch_size_eval=16)
    a.update(kw)
    return argparse.Namespace(**a)


def test_eval_setup_batch():
    from dglke_amd._lib import KgeError
    from dglke_amd.eval import eval_setup
    fb = _Splits(14951, 100, 50, 59071)                     # FB15k's entity and test-triple counts
    assert eval_setup(fb, 'test', _eval_args())[2] == 4096
    assert eval_setup(fb, 'test', _eval_args(batch_size_eval=5000))[2] == 5000
    assert eval_setup(fb, 'test', _eval_args(model_name='TransR'))[2] == 64
    assert eval_setup(_Splits(14951, 100, 50, 3), 'test', _eval_args())[2] == 3
    assert eval_setup(_Splits(14951, 100, 50, 3), 'test', _eval_args(model_name='TransR'))[2] == 3
    # a [batch, entities] float32 score block stays within 2 GiB
    assert eval_setup(_Splits(1 << 20, 100, 50, 59071), 'test', _eval_args())[2] == 512
    with pytest.raises(KgeError, match="no valid split"):
        eval_setup(_Splits(100, 100, None, 10), 'valid', _eval_args())


def test_eval_setup_eval_percent_keeps_the_same_rows_of_triples_and_candidates():
    from dglke_amd.eval import eval_setup
    ds = _Splits(300, 1000, 200, 137)
    n = 137
    cand_h = np.arange(n * 4).reshape(n, 4)
    test, known, batch, cands = eval_setup(ds, 'test', _eval_args(eval_percent=0.1), [cand_h, None])
    keep = np.random.RandomState(5 + 17).permutation(n)[:max(1, int(0.1 * n))]
    assert len(keep) == 13 and batch == 13
    for got, full in zip(test, ds.test):
        assert np.array_equal(got, full[keep])
    assert np.array_equal(cands[0], cand_h[keep]) and cands[1] is None
    assert all(len(k) == 1000 + 200 + 137 for k in known)            # the known set is never subsampled
    # a share that rounds to nothing keeps one triple; the whole split comes back untouched, in order
    assert len(eval_setup(ds, 'test', _eval_args(eval_percent=0.001))[0][0]) == 1
    test, _, _, cands = eval_setup(ds, 'valid', _eval_args())
    assert cands is None and all(np.array_equal(a, b) for a, b in zip(test, ds.valid))


def test_eval_setup_known_set():
    from dglke_amd.eval import eval_setup
    ds = _Splits(300, 1000, 200, 137)
    known = eval_setup(ds, 'test', _eval_args())[1]
    for k in range(3):
        assert np.array_equal(known[k], np.concatenate([ds.train[k], ds.valid[k], ds.test[k]]))
    ds = _Splits(300, 1000, None, 137)                      # no valid split: the splits that exist
    known = eval_setup(ds, 'test', _eval_args())[1]
    for k in range(3):
        assert np.array_equal(known[k], np.concatenate([ds.train[k], ds.test[k]]))
    assert eval_setup(ds, 'test', _eval_args(eval_filter=False))[1] is None           # --no_eval_filter


def test_split_of_the_training_triples_and_its_refusal():
    """one trainer: every row in order; several: the random partition by --seed, or the rows a relation partition assigns; a share
    below one batch is refused whichever trainer it falls to (every rank computes the same partition and raises)"""
    import argparse
    import types
    from dglke_amd import train as T
    from dglke_amd._lib import KgeError
    ds = _Splits(300, 1001, 10, 10)

    def split(batch, *a, **k):
        t = types.SimpleNamespace(args=argparse.Namespace(batch_size=batch, seed=4), dataset=ds)
        return T._Trainer.split(t, *a, **k)
    (part,) = split(256, 1)
    assert np.array_equal(ds.train[0][part], ds.train[0])
    parts = split(256, 3)
    want = np.array_split(np.random.RandomState(4).permutation(1001), 3)
    assert len(parts) == 3 and all(np.array_equal(a, b) for a, b in zip(parts, want))
    edge_rank = (ds.train[1] >= 2).astype(np.int64)             # relations 0, 1 -> trainer 0
    parts = split(256, 2, edge_rank)
    assert np.array_equal(parts[0], np.nonzero(ds.train[1] < 2)[0]) and np.array_equal(parts[1], np.nonzero(ds.train[1] >= 2)[0])
    with pytest.raises(KgeError, match="--batch_size 400 is larger than a trainer's share of the training triples .1001 over 3 trainers."):
        split(400, 3)
    n0 = int((ds.train[1] < 2).sum())
    with pytest.raises(KgeError, match="trainer 0 gets %d training triples, fewer than --batch_size 400" % n0):
        split(400, 2, edge_rank, "relation partition: trainer %(trainer)d gets %(share)d training triples, fewer than --batch_size %(batch)d")
    assert len(split(1001, 1)) == 1
    with pytest.raises(KgeError):
        split(1002, 1)
