"""CPU guard of the stream contract (include/kge_hip.h, conventions): what can be read from the sources without a GPU.

  header and table agree        every prototype with a `void *stream` (or `void *..._stream`) is in stream_cases.STREAM_ENTRIES, takes
                                it LAST (the GPU proxy of tests/test_gpu_stream_contract.py reads it there), and has a case or a
                                reasoned exemption; every prototype with `void *ws, size_t ws_bytes` is in
                                workspace_cases.WS_ENTRIES with the position of `ws`;
  every launch names a stream   the fifth argument of every hipLaunchKernelGGL and the last of every hip*Async call in csrc/ is a
                                variable - never 0, nullptr or one of the runtime's own stream names;
  nothing synchronous           no blocking copy / memset, allocation or synchronisation call in csrc/ (outside the developer timeline
                                and the kge_ipc_* plumbing);
  no hidden state               no device-side variable and no mutable data at namespace scope.

The last test plants each violation into the text of a real source file and expects the scan to find exactly it: the scans are
regular expressions over C++, and one that went blind would pass for ever.
"""
import os
import re

import pytest

import stream_cases as S

FILES = S.source_files()
IDS = [os.path.basename(f) for f in FILES]


def _header():
    return open(S.HEADER).read()


def test_header_and_table_agree():
    protos = S.prototypes(_header())
    assert len(protos) > 60 and "kge_step_fused" in protos and "kge_abi_version" in protos, sorted(protos)
    streamed = S.stream_functions(protos)
    missing, stale = sorted(set(streamed) - set(S.STREAM_ENTRIES)), sorted(set(S.STREAM_ENTRIES) - set(streamed))
    assert not missing, "entry points with a stream and no case in stream_cases.STREAM_ENTRIES: %s" % missing
    assert not stale, "STREAM_ENTRIES names functions the header does not declare with a stream: %s" % stale
    for name, params in streamed.items():
        assert S.is_stream_param(params[-1]), "%s: the stream is not its last parameter (%s)" % (name, params[-1])
        assert sum(bool(re.search(S.STREAM_NAME, p)) for p in params) == 1, name
    for name in ("kge_step_optim", "kge_sample_batches_weighted", "kge_subsampling_weights"):     # spelled `void *hip_stream`
        assert name in streamed and streamed[name][-1].endswith("hip_stream"), name
    # what takes no stream: host-side helpers, the size functions, the hipIpc plumbing
    for name in ("kge_ipc_export", "kge_ipc_open", "kge_ipc_close", "kge_pipe_create", "kge_pipe_destroy", "kge_batch_from_slot",
                 "kge_batch_localized", "kge_step_workspace_bytes", "kge_known_mask_bytes"):
        assert name in protos and name not in streamed, name


def test_header_and_workspace_table_agree():
    """every prototype with the adjacent parameters `void *ws, size_t ws_bytes` is a key of workspace_cases.WS_ENTRIES and the
    reverse; Entry.ws is the position of `ws` in the prototype (the GPU proxy swaps the pair it finds there)"""
    import workspace_cases as W
    protos = S.prototypes(_header())
    takes = S.workspace_functions(protos)
    assert len(takes) >= 21 and takes["kge_step_fused"] == 4, sorted(takes)
    missing, stale = sorted(set(takes) - set(W.WS_ENTRIES)), sorted(set(W.WS_ENTRIES) - set(takes))
    assert not missing, "entry points with (ws, ws_bytes) and no entry in workspace_cases.WS_ENTRIES: %s" % missing
    assert not stale, "WS_ENTRIES names functions the header does not declare with (ws, ws_bytes): %s" % stale
    for name, at in sorted(takes.items()):
        assert W.WS_ENTRIES[name].ws == at, "%s: `ws` is parameter %d of the prototype, WS_ENTRIES says %d" % (name, at, W.WS_ENTRIES[name].ws)
    # a size function takes none; a planted prototype is found with its index
    assert "kge_step_workspace_bytes" in protos and "kge_step_workspace_bytes" not in takes
    more = S.prototypes(_header().replace("int kge_mask_diag(", "int kge_planted(int n, void *ws, size_t ws_bytes, void *stream);\nint kge_mask_diag(", 1))
    assert S.workspace_functions(more).get("kge_planted") == 1


def test_every_entry_has_a_case_or_an_exemption():
    exempt = [n for n, v in S.STREAM_ENTRIES.items() if isinstance(v, S.Exempt)]
    assert len(exempt) <= S.MAX_EXEMPT, exempt
    for n, v in S.STREAM_ENTRIES.items():
        if isinstance(v, S.Exempt):
            assert v.reason.strip() and "\n" not in v.reason, n
        else:
            assert v and all(isinstance(c, str) for c in v), n
    # every case the table names exists in the GPU file, and the GPU file's cases all stand in the table
    gpu = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_stream_contract.py")).read()
    defined = set(re.findall(r"^def test_(\w+)\(", gpu, re.M))
    named = {c for n in S.STREAM_ENTRIES for c in S.cases_of(n)}
    assert named <= defined, "cases without a test function: %s" % sorted(named - defined)
    assert set(re.findall(r"\b(?:_stream_case|_through)\(\s*\"(\w+)\"", gpu)) == named


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_every_launch_names_a_stream(path):
    raw = open(path).read()
    n, bad = S.launch_findings(S.product_text(path))
    assert n == raw.count("hipLaunchKernelGGL("), "%s: parsed %d of %d launches" % (path, n, raw.count("hipLaunchKernelGGL("))
    assert not bad, "%s: %s" % (os.path.basename(path), bad)


def test_the_launch_scan_saw_the_whole_library():
    total = sum(S.launch_findings(S.product_text(f))[0] for f in FILES)
    with_launches = [f for f in FILES if "hipLaunchKernelGGL(" in open(f).read()]
    assert total >= 185 and len(with_launches) >= 15, (total, len(with_launches))
    asyncs = sum(len(S.calls(S.product_text(f), r"hip\w+Async")) for f in FILES)
    assert asyncs >= 4, asyncs                            # the loss terms' and g0's copies, the two rank memsets


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_nothing_synchronous_or_allocating(path):
    bad = S.sync_findings(S.product_text(path))
    assert not bad, "%s: %s" % (os.path.basename(path), bad)


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_no_hidden_state(path):
    bad = S.state_findings(S.product_text(path))
    assert not bad, "%s: %s" % (os.path.basename(path), bad)


def test_the_named_exemptions_are_what_they_say():
    """the timeline block holds the one device-side variable and the one hipMemcpyToSymbol; the kge_ipc_* bodies hold hipIpc calls
    only; g_err and g_carve are seen as data and pass as thread_local"""
    common = open(os.path.join(S.CSRC, "kge_common.hpp")).read()
    cut, blocks = S.cut_timeline_blocks(S.blank_comments_and_strings(common))
    assert blocks == 2 and "kge_tl_buf" not in cut and "hipMemcpyToSymbol" not in cut and "check_launch" in cut
    kept = S.blank_comments_and_strings(common)
    assert [w for _, w, _ in S.state_findings(kept)] == ["device-side variable at namespace scope"]
    assert [c for _, c in S.sync_findings(kept)] == ["hipMemcpyToSymbol"]
    api = S.product_text(os.path.join(S.CSRC, "kge_api.hip"))
    bodies = S.function_bodies(api, r"kge_ipc_\w+")
    assert len(bodies) == 3
    for a, b in bodies:
        assert re.search(r"\bhipIpc\w+\(", api[a:b]) and not re.search(r"\bhip(Malloc|Free|Memcpy|Memset|\w+Synchronize)", api[a:b])
    data = [s for _, s in S.namespace_scope_statements(api) if S.is_data(s)]
    assert any("g_err" in s for s in data) and any("g_carve" in s for s in data), data
    assert all("thread_local" in s for s in data), data


def test_argument_splitter():
    t = S.blank_comments_and_strings("""
#define L(A_, B_) do { if (x) hipLaunchKernelGGL((k<A_, B_, true>), dim3(g, 1), b, f(a, b) /* , 0, */, s, KGE_H); \\
                       else hipLaunchKernelGGL((k<A_, B_, false>), g, b, lds, (hipStream_t)stream, p[1, 2], "a,b)"); } while (0)
hipLaunchKernelGGL(plain, g, b, 0,
                   st, a);
""")
    got = S.calls(t, "hipLaunchKernelGGL")
    assert [a[0] for _, a, _ in got] == ["(k<A_, B_, true>)", "(k<A_, B_, false>)", "plain"]
    assert [a[4] for _, a, _ in got] == ["s", "(hipStream_t)stream", "st"] and [len(a) for _, a, _ in got] == [6, 7, 6]
    assert [ln for _, _, ln in got] == [2, 3, 4]
    assert S.launch_findings(t) == (3, [])
    for ok in ("s", "stream", "(hipStream_t)stream", "( hipStream_t ) s_", "a"):
        assert S.stream_argument_ok(ok), ok
    for bad in ("0", "nullptr", "NULL", "hipStreamDefault", "hipStreamLegacy", "hipStreamPerThread", "(hipStream_t)0", "(hipStream_t)nullptr",
                "", "s + 1", "get()", "0u"):
        assert not S.stream_argument_ok(bad), bad


def _plant(path, after, text):
    raw = open(os.path.join(S.CSRC, path)).read()
    at = raw.index(after) + len(after)
    return raw[:at] + text + raw[at:]


def test_each_scan_finds_a_planted_violation():
    line = lambda raw, what: raw[:raw.index(what)].count("\n") + 1
    # a launch on the null stream: in plain code, inside a macro body, through a cast; an async copy without its stream
    raw = open(os.path.join(S.CSRC, "kge_known.hip")).read()
    m = re.search(r"hipLaunchKernelGGL\(", raw)
    args, end = S.split_args(raw, m.end() - 1)
    for null in ("0", "nullptr", "(hipStream_t)0", "hipStreamPerThread"):
        broken = raw[:m.end()] + ", ".join(args[:4] + [null] + args[5:]) + raw[end:]
        n, bad = S.launch_findings(S.product_text(broken, True))
        assert n == 1 and len(bad) == 1 and repr(null) in bad[0][1], (null, bad)
    raw = open(os.path.join(S.CSRC, "kge_rowwise.hip")).read()
    assert "g, b, 0, s, KGE_LOSS_H);" in raw
    broken = raw.replace("g, b, 0, s, KGE_LOSS_H);", "g, b, 0, 0, KGE_LOSS_H);", 1)
    n, bad = S.launch_findings(S.product_text(broken, True))
    assert n == raw.count("hipLaunchKernelGGL(") and len(bad) == 1 and bad[0][0] == line(broken, "g, b, 0, 0, KGE_LOSS_H);"), bad
    raw = open(os.path.join(S.CSRC, "kge_api.hip")).read()
    assert "hipMemcpyDeviceToDevice, s)" in raw
    _, bad = S.launch_findings(S.product_text(raw.replace("hipMemcpyDeviceToDevice, s)", "hipMemcpyDeviceToDevice, 0)", 1), True))
    assert len(bad) == 1 and bad[0][1].startswith("hipMemcpyAsync"), bad
    # a blocking memset, a synchronisation, an allocation - and the same words in a comment or a string, which are none
    marker = "using namespace kge;"
    for call in ("hipMemset(p, 0, n);", "hipMemsetD32(p, 1, n);", "hipDeviceSynchronize();", "hipStreamSynchronize(s);", "hipMalloc(&p, n);",
                 "hipMallocAsync(&p, n, s);", "hipFree(p);", "hipMemcpy(a, b, n, hipMemcpyDeviceToHost);", "hipEventSynchronize(e);"):
        broken = _plant("kge_route.hip", marker, "\nstatic inline void planted(void *p, size_t n) { %s }\n" % call)
        bad = S.sync_findings(S.product_text(broken, True))
        assert len(bad) == 1 and bad[0][1] == call.split("(")[0] and bad[0][0] == line(broken, "planted"), (call, bad)
    quiet = _plant("kge_route.hip", marker, "\n// hipMemset(p, 0, n) would block\nstatic const char *planted = \"hipMalloc(\";\n")
    assert S.sync_findings(S.product_text(quiet, True)) == []
    # hidden state: at file scope, inside the namespace, inside extern "C"; the forms that are none
    for decl, what in (("static int planted_count;", "mutable data"), ("static int planted_count = 0;", "mutable data"),
                       ("int planted_count;", "mutable data"), ("static float planted_tab[4] = {0, 1, 2, 3};", "mutable data"),
                       ("static struct { int a; void *p; } planted_count;", "mutable data"),
                       ("__device__ int planted_count;", "device-side"), ("static __device__ unsigned planted_count[2];", "device-side"),
                       ("__constant__ float planted_tab[4] = {0, 1, 2, 3};", "device-side")):
        for path, after in (("kge_route.hip", marker), ("kge_api.hip", "thread_local char g_err[512] = \"\";"), ("kge_route.hip", "extern \"C\" {")):
            broken = _plant(path, after, "\n%s\n" % decl)
            bad = S.state_findings(S.product_text(broken, True))
            assert len(bad) == 1 and bad[0][1].startswith(what) and "planted" in bad[0][2], (decl, path, bad)
    for fine in ("static const int planted_count = 3;", "static constexpr float planted_tab[2] = {0, 1};", "thread_local int planted_count = 0;",
                 "static int planted(int x);", "static inline int planted(int x) { static_assert(true, \"\"); return x; }",
                 "struct planted_t { int a; };", "typedef struct planted_s { int a; } planted_t;", "enum { PLANTED = 3 };",
                 "using planted_t = int;", "template <int N> struct planted_t { int a[N]; };"):
        assert S.state_findings(S.product_text(_plant("kge_route.hip", marker, "\n%s\n" % fine), True)) == [], fine
    # a prototype with a stream that the table does not know; one that takes its stream in the middle
    head = _header()
    more = head.replace("int kge_mask_diag(", "int kge_planted(float *x, void *stream);\nint kge_mask_diag(", 1)
    assert set(S.stream_functions(S.prototypes(more))) - set(S.STREAM_ENTRIES) == {"kge_planted"}
    for spelled in ("void *hip_stream", "void * side_stream", "void *stream"):
        more = head.replace("int kge_mask_diag(", "int kge_planted(float *x, %s);\nint kge_mask_diag(" % spelled, 1)
        assert set(S.stream_functions(S.prototypes(more))) - set(S.STREAM_ENTRIES) == {"kge_planted"}, spelled
    for none in ("void *streams", "int stream", "void *upstream", "const void *stream_of"):
        more = head.replace("int kge_mask_diag(", "int kge_planted(float *x, %s);\nint kge_mask_diag(" % none, 1)
        assert "kge_planted" not in S.stream_functions(S.prototypes(more)), none
    # a `stream` of the header renamed to `hip_stream` is still found, still last
    renamed = head.replace("int kge_mask_diag(float *x, int C, int chunk, int Np, void *stream);",
                           "int kge_mask_diag(float *x, int C, int chunk, int Np, void *hip_stream);", 1)
    assert renamed != head and S.is_stream_param(S.stream_functions(S.prototypes(renamed))["kge_mask_diag"][-1])
    moved = head.replace("int kge_mask_diag(float *x, int C, int chunk, int Np, void *stream);",
                         "int kge_mask_diag(float *x, void *stream, int C, int chunk, int Np);", 1)
    assert moved != head
    p = S.stream_functions(S.prototypes(moved))["kge_mask_diag"]
    assert not S.is_stream_param(p[-1])
