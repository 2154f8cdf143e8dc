"""The stream contract of include/kge_hip.h on the device: "no allocation, no host synchronisation and no global mutable state
inside; every call takes an explicit stream and only enqueues kernels on it, so calls can be captured into a hipGraph" - for EVERY
entry that takes a stream (tests/stream_cases.py STREAM_ENTRIES; what can be read from the sources: tests/test_stream_inputs.py).

Every case runs three times behind a proxy in front of the ctypes handle (StreamProbe, installed like the workspace-contract test's
Probe), which sees every call of an entry of STREAM_ENTRIES:

  default   on torch's default stream - on ROCm the null stream, where a launch that drops its stream argument, a blocking memset
            and a host read of device memory are all correct.  The result passes the float64 / numpy / golden comparison of the
            entry's own test (the runners ARE those tests' bodies, with their oracles and tolerances);
  side      the whole run under `with torch.cuda.stream(side)`, a non-blocking stream: the last argument of every call is
            side.cuda_stream - the Python callers (ops, Ranker, infer, known, dataloader, engine, dist.HipOps) follow the current
            stream;
  capture   also under the side stream, and every intercepted call is captured ALONE into a fresh graph (_lib.graph_capture),
            must return 0 inside the capture, the capture must close, and the graph is replayed once on the side stream and kept
            until the run's final synchronise.  Nothing executes at capture time: every output of the run comes from replays.  A
            capture fails for what the header forbids - a launch or copy on another stream, a synchronous runtime call, a host
            read of device memory, an allocation.  A call that returns non-zero is passed through (no replay).

The side and the capture result equal the default result bit for bit (no tolerance in this file: every entry is deterministic at
these shapes - the atomics of kge_adagrad_scatter / kge_scatter_add_rows run on unique indices here), and every case calls the
entries the table assigns to it.  What a runner does around the C call - uploads, reading results back, torch ops, the allocation of
outputs and workspaces, DeviceSampler.prepare_tail() (inside tail_jobs(): the proxy's capture is closed whenever Python runs) -
stays outside the capture: only the C call is captured.

The entries with a workspace run through the test functions of tests/test_gpu_workspace_contract.py themselves: each of them builds
its runner and hands it to that module's `_contract`, which is swapped for this file's three-mode contract for the duration of the
call (_through) - the cases, the float64 baselines and the read-back stay in one place.

Last: two StepEngines on two side streams with their calls interleaved from one thread (kge_step_phase, then a kge_step_async group)
equal the same engines run alone - "no global mutable state" at run time for the entries that carry state from call to call.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import modular_op_cases as M
import stream_cases as S
import test_gpu_workspace_contract as WC
import workspace_cases as W
from test_gpu_parity import DEV
from test_gpu_workspace_contract import _bits, _same        # noqa: F401 - the bit comparison of the workspace contract

pytestmark = pytest.mark.gpu

MODES = ("default", "side", "capture")
_STATE = {}
CALLED = {m: set() for m in MODES}          # mode -> entries that ran (capture: were replayed) with status 0, over the whole file


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """a lost GPU context fails every later call: end the session instead of running the rest of the file against it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU context is lost (%s): nothing more is run" % (e,), returncode=3)


# --------------------------------------------------------------------------------------------------------------------------
# the proxy
# --------------------------------------------------------------------------------------------------------------------------
class StreamProbe(object):
    """stands in for the ctypes handle (dglke_amd._lib._lib): every call of an entry of S.STREAM_ENTRIES is recorded, held to the
    stream of the mode and, in capture mode, captured alone and replayed"""

    def __init__(self, real, side):
        self.real, self.side = real, side
        self.mode = "default"
        self.calls, self.graphs = [], []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in S.STREAM_ENTRIES:
            return fn

        def call(*a):
            from dglke_amd import _lib
            self.calls.append(name)
            want = torch.cuda.default_stream() if self.mode == "default" else self.side
            assert torch.cuda.current_stream() == want, "%s: the run left the %s stream" % (name, self.mode)
            assert int(a[-1] or 0) == int(want.cuda_stream), "%s was given stream %r, the current stream is %r" % (name, a[-1], want.cuda_stream)
            if self.mode != "capture":
                rc = fn(*a)
                CALLED[self.mode].add(name) if rc == 0 else None
                return rc
            g = torch.cuda.CUDAGraph()
            with _lib.graph_capture(g, stream=self.side):
                rc = fn(*a)
            if rc != 0:
                return rc                                 # a refusal: nothing to replay, the caller sees the code
            g.replay()
            self.graphs.append(g)
            CALLED[self.mode].add(name)                   # (captured, closed and replayed)
            return rc
        return call


def _probe():
    from dglke_amd import _lib
    if "probe" not in _STATE:
        _STATE["probe"] = StreamProbe(_lib.lib(), torch.cuda.Stream())
    return _STATE["probe"]


@contextlib.contextmanager
def _installed(p, mode):
    from dglke_amd import _lib
    assert _lib._lib is p.real and torch.cuda.current_stream() == torch.cuda.default_stream()
    torch.cuda.synchronize()
    p.mode = mode
    _lib._lib = p
    try:
        with torch.cuda.stream(p.side) if mode != "default" else contextlib.nullcontext():
            yield p
    finally:
        _lib._lib = p.real
        torch.cuda.synchronize()
        del p.graphs[:]                                   # (kept until here: a replay may still have been running)
        p.mode = "default"


def _tensors(res):
    return {k: v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)) for k, v in res.items()}


def _stream_case(case, run, entries=None):
    """run(verify) -> {name: tensor or array}: default (with the baseline comparison), side, capture; returns the default result"""
    mine = S.entries_of(case)
    assert mine, "no entry of stream_cases.STREAM_ENTRIES names the case %r" % case
    entries = sorted(set(mine if entries is None else entries))
    assert set(entries) <= set(mine), (case, entries, mine)
    p = _probe()
    got = {}
    for mode in MODES:
        n0 = len(p.calls)
        with _installed(p, mode):
            got[mode] = _tensors(run(mode == "default"))
        seen = set(p.calls[n0:])
        assert set(entries) <= seen, "%s, %s: the case never called %s (called: %s)" % (case, mode, sorted(set(entries) - seen), sorted(seen))
    assert got["default"], case
    _same(got["default"], got["side"], "%s: on the side stream against the default stream" % case)
    _same(got["default"], got["capture"], "%s: every call captured and replayed against the default stream" % case)
    return got["default"]


@contextlib.contextmanager
def _through(case, entries=None):
    """a test function of test_gpu_workspace_contract.py called inside hands its runner to this file's contract instead of the
    workspace contract (same runner, same float64 baseline on the first run; `entries`: what that test expects to be called)"""
    saved, state = WC._contract, dict(WC._STATE)

    def contract(run, expected, donor=None, transh=True):
        return _stream_case(case, run, entries if entries is not None else [e for e in expected if e in S.entries_of(case)])
    WC._contract = contract
    try:
        yield
    finally:
        WC._contract = saved
        WC._STATE.clear()
        WC._STATE.update(state)


def _pick(cases, *ids):
    by_id = {c["id"]: c for c in cases}
    return [by_id[i] for i in ids]


# --------------------------------------------------------------------------------------------------------------------------
# the steps
# --------------------------------------------------------------------------------------------------------------------------
# one model each of the matrix-core, the pairwise and the relation-matrix launch sequences
STEPS = _pick(W.STEP_CASES, "TransE_l2-h36-N24", "RotatE-h36-N24", "TransR-36x72")
assert all(c in W.PHASE_CASES for c in STEPS)


@pytest.mark.parametrize("c", STEPS, ids=lambda c: c["id"])
def test_step_fused(c):
    with _through("step_fused"):
        WC.test_step_fused(c)
        _STATE[("fused", c["id"])] = WC._STATE[("fused", c["id"])]


def _phase_step(eng, b, want):
    """WC._phase_step with the engine's own workspace (there the workspace-contract proxy supplies one)"""
    from dglke_amd import _lib
    out = _lib.KgeStepOut()
    if want is not None:
        out.loss4 = _lib.ptr(eng.loss4)
        for k, t in want.items():
            setattr(out, k, _lib.ptr(t))
    out.loss_accum = _lib.ptr(eng.loss_accum)
    out.tickets = _lib.ptr(eng.tickets)
    ws = eng.workspace_for(b)
    for ph in (_lib.PHASE_GATHER, _lib.PHASE_FORWARD, _lib.PHASE_BACKWARD, _lib.PHASE_UPDATE):
        _lib.check(_lib.lib().kge_step_phase(C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(ws), eng._ws_bytes, ph,
                                             _lib.stream_ptr()))


@pytest.mark.parametrize("c", STEPS, ids=lambda c: c["id"])
def test_step_phase(c, monkeypatch):
    """the four phase groups, each captured on its own, against the fused step of the same case on the default stream"""
    monkeypatch.setattr(WC, "_phase_step", _phase_step)
    ref = _STATE.get(("fused", c["id"]))
    if ref is None:
        ref = _tensors(WC._run_steps(c, False))
        torch.cuda.synchronize()
    with _through("step_phase"):
        WC._STATE[("fused", c["id"])] = ref
        WC.test_step_phase_equals_the_fused_step(c)


@pytest.mark.parametrize("c", _pick(W.ASYNC_CASES, "TransE_l2-h36-N24", "TransE_l2-h36-N24-rel"), ids=lambda c: c["id"])
def test_step_async_group(c):
    """three steps and the flush: four graphs, the kge_pipe's host state carried from capture to capture; -rel: PREP of the next
    step rides on the backward launch"""
    with _through("step_async_group", ["kge_step_async", "kge_step_async_flush"]):
        WC.test_step_async_group(c)


def test_step_sharded():
    with _through("step_sharded"):
        WC.test_step_sharded_on_three_emulated_shards(WC.SHARDED[0])


def test_step_fused_known():
    with _through("step_fused_known"):
        WC.test_step_fused_known(24, None)


def test_step_phase_known():
    """StepEngine.step_timed with a known index attached: the four kge_step_phase_known groups (the mask launch heads FORWARD).
    Baseline: the tables and loss sums of kge_step_fused_known on the same batches, bit for bit ("calling the four phase groups in
    this order on one stream IS kge_step_fused"); that entry's float64 comparison is test_step_fused_known's"""
    import known_negative_cases as KN
    from test_gpu_known_negatives import _batch, _engine as known_engine, _index
    c = [x for x in KN.CASES if x["id"] == "l2-d32-n40"][0]
    bts, K, _ = KN.build(c)

    def steps(timed):
        eng = known_engine(c)
        eng.attach_known(_index(K, c["n_ent"], c["n_rel"]))
        for bt in bts:
            eng.step_timed(_batch(c, bt)) if timed else eng.step(_batch(c, bt))
        torch.cuda.synchronize()
        return {k: getattr(eng, k).clone() for k in ("ent", "ent_state", "rel", "rel_state", "loss_accum")}

    def run(verify):
        res = steps(True)
        if verify:
            _same(steps(False), res, "kge_step_phase_known against kge_step_fused_known")
        return res
    _stream_case("step_phase_known", run)


def test_known_neg_mask():
    """host-built plans, both corruption sides, N = 33 (two mask words per row); baseline: set membership, as in
    test_mask_kernel_equals_set_membership (test_gpu_known_negatives.py)"""
    from dglke_amd import plan
    from test_gpu_known_negatives import MASK_ENT, MASK_REL, _index, _known_struct, _mask_bits, _mask_graph, _membership
    K = _mask_graph()
    B, chunk, N = 24, 8, 33
    rng = np.random.RandomState(5)
    sides = []
    for neg_head in (False, True):
        sel = rng.randint(0, len(K[0]), size=B)
        h, r, t = K[0][sel].copy(), K[1][sel].copy(), K[2][sel].copy()
        neg = rng.randint(0, MASK_ENT, size=(B // chunk) * N).astype(np.int64)
        h[0], r[0] = 0, 0
        sides.append((neg_head, h, r, t, neg, _membership(K, h, r, t, neg, neg_head, chunk, N)))
    assert sum(int(s[5].sum()) for s in sides) > 0

    def run(verify):
        idx = _index(K, MASK_ENT, MASK_REL)
        k = _known_struct(idx)
        res = {}
        for neg_head, h, r, t, neg, want in sides:
            b = plan.make_batch(h, t, r, neg, chunk, N, neg_head, DEV)
            got, spill = _mask_bits(b.c, k, B, N)
            if verify:
                assert np.array_equal(got, want) and not spill.any(), neg_head
            res["mask %d" % neg_head], res["spill %d" % neg_head] = got, spill
        return res
    _stream_case("known_neg_mask", run)


def test_step_fused_sampling():
    """the sampler launch (kge_sample_batches) and the steps that carry the tail jobs; tail_jobs() calls prepare_tail() between two
    intercepted calls, outside any capture"""
    with _through("step_fused_sampling", ["kge_step_fused_sampling", "kge_sample_batches"]):
        WC.test_step_fused_sampling(W.SAMPLING_CASES[0])


@pytest.mark.parametrize("k", [0, 1], ids=["dense", "packed"])
def test_step_grads(k):
    c, lay = WC._grads_cases()[k].values
    assert lay == ("dense", "packed")[k]
    with _through("step_grads"):
        WC.test_step_grads(c, lay)


# ---- QuatE, PairRE, TransH through the workspace-contract cases: one case per (entry, model) ----
MODEL_STEPS = list(W.MODEL_PHASE_CASES)              # the -D36-N24 case of each model


@pytest.mark.parametrize("c", MODEL_STEPS, ids=lambda c: c["id"])
def test_step_fused_of_quate_pairre_transh(c):
    with _through("step_fused"):
        WC.test_step_fused_of_quate_pairre_transh(c)
        _STATE[("fused", c["id"])] = WC._STATE[("fused", c["id"])]


@pytest.mark.parametrize("c", MODEL_STEPS, ids=lambda c: c["id"])
def test_step_phase_of_quate_pairre_transh(c, monkeypatch):
    monkeypatch.setattr(WC, "_phase_step", _phase_step)
    ref = _STATE.get(("fused", c["id"]))
    if ref is None:
        ref = _tensors(WC._run_model_steps(c, False))
        torch.cuda.synchronize()
    with _through("step_phase"):
        WC._STATE[("fused", c["id"])] = ref
        WC.test_step_phase_of_quate_pairre_transh_equals_the_fused_step(c)


@pytest.mark.parametrize("model", W.NEW_MODELS)
def test_step_fused_known_of_quate_pairre_transh(model):
    """kge_step_fused_known, then the four kge_step_phase_known groups (step_timed), each in the three modes"""
    with _through("step_fused_known"):
        WC.test_step_fused_known(24, model)


@pytest.mark.parametrize("model", W.NEW_MODELS)
def test_step_phase_known_of_quate_pairre_transh(model):
    c = W.MODEL_KNOWN_CASES[model]
    _stream_case("step_phase_known", lambda verify: WC._run_model_steps(c, False, "phase", known=True))


def test_step_optim_adam():
    """Adam through kge_step_optim: a plain case, TransH, a width above 512, and with a known index the whole step and then its
    four phase groups as four captures"""
    by_id = {o["id"]: o for o in W.OPTIM_ADAM}
    with _through("step_optim_adam"):
        for i in ("TransE_l2-w16", "TransH-w16", "DistMult-w516", "l2-known", "l2-known-phases"):
            WC.test_step_optim_adam(by_id[i])


def test_step_optim_adagrad():
    """kind = KGE_OPT_ADAGRAD through kge_step_optim, with a known index (the fused entry it is compared with runs in the modes too)"""
    with _through("step_optim_adagrad"):
        WC.test_step_optim_adagrad_kind_is_the_existing_step("l2-known")
        WC.test_step_optim_adagrad_kind_is_the_existing_step("TransE_l1-w16")


def test_subsampling_weights():
    """dataloader.subsampling_weights on the table's graph; bound: test_weights_match_the_float64_statement (test_gpu_subsampling.py)"""
    import subsampling_cases as SC
    from dglke_amd.dataloader import subsampling_weights
    h, r, t = SC.graph()
    ref = SC.weights64(h, r, t, SC.N_REL)

    def run(verify):
        w = subsampling_weights(h, r, t, SC.N_ENT, SC.N_REL, DEV)
        torch.cuda.current_stream().synchronize()
        if verify:
            got = w.cpu().numpy().astype(np.float64)
            assert (np.abs(got - ref) / ref).max() <= 4 * 2.0 ** -24
        return dict(weights=w)
    _stream_case("subsampling_weights", run)


def test_sample_batches_weighted():
    """two launches of a weighted DeviceSampler (the second crosses an epoch boundary): every slot whole - ids, plan, counts and the
    weights behind the plan - and the device state.  Baseline: test_weighted_sampler_carries_the_weights_and_changes_nothing_else
    (test_gpu_subsampling.py) - every array the unweighted sampler's, edge_w the weights of the slot's triples bit for bit"""
    import subsampling_cases as SC
    from dglke_amd.dataloader import DeviceSampler
    B, N, n_train, n_ent, n_slots = 64, 16, 163, 500, 3
    h, r, t, w = SC.unique_triples(n_train, n_ent)
    weight_of = dict(zip(zip(h.tolist(), r.tolist(), t.tolist()), w.tolist()))

    def run(verify):
        smp = DeviceSampler(h, r, t, n_ent, B, N, DEV, n_slots=n_slots, seed=2, edge_importance=w)
        plain = DeviceSampler(h, r, t, n_ent, B, N, DEV, n_slots=n_slots, seed=2) if verify else None
        res = {}
        for launch in range(2):
            smp.sample(n_slots)
            torch.cuda.current_stream().synchronize()
            res["slots %d" % launch], res["state %d" % launch] = smp.slots.clone(), smp.state.clone()
            if verify:
                plain.sample(n_slots)
                torch.cuda.current_stream().synchronize()
                assert torch.equal(plain.state, smp.state)
                for k in range(n_slots):
                    a, b = plain.slot_arrays(k), smp.slot_arrays(k)
                    UE, UR = int(a["counts"][0]), int(a["counts"][1])
                    assert np.array_equal(a["counts"], b["counts"])
                    for name, n in (("h_gid", B), ("t_gid", B), ("rel_ids", B), ("neg_ids", smp.C * N), ("ue_id", UE), ("ur_id", UR),
                                    ("ue_pos_ptr", UE + 1), ("ue_neg_ptr", UE + 1), ("ur_ptr", UR + 1), ("ue_rec", 8 * UE), ("ur_rec", 8 * UR)):
                        assert np.array_equal(a[name][:n], b[name][:n]), (launch, k, name)
                    want = np.array([weight_of[x] for x in zip(b["h_gid"].tolist(), b["rel_ids"].tolist(), b["t_gid"].tolist())], np.float32)
                    assert np.array_equal(b["edge_w"].view(np.int32), want.view(np.int32)), (launch, k)
        return res
    _stream_case("sample_batches_weighted", run)


def test_reduce_loss():
    """StepEngine.read_loss_sums after two steps.  Baseline: the float64 sums of the 4 x 4096 slots within 4096 * 2^-24 * sum |x| (a
    fixed-order float32 sum at most that deep), and the slots zeroed"""
    from dglke_amd import _lib, plan
    c = STEPS[0]
    bts = W.step_batches(c)

    def run(verify):
        eng = WC._engine(c)
        for bt in bts:
            eng.step(plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV))
        acc = eng.loss_accum.clone()
        sums = np.array(eng.read_loss_sums(zero=True), np.float32)
        if verify:
            a64 = acc.cpu().numpy().astype(np.float64).reshape(4, _lib.ACC_SLOTS)
            assert np.abs(a64).sum() > 0
            assert np.all(np.abs(sums - a64.sum(1)) <= _lib.ACC_SLOTS * 2.0 ** -24 * np.abs(a64).sum(1)), (sums, a64.sum(1))
            assert not bool(eng.loss_accum.any())
        return dict(accum=acc, sums=sums, after=eng.loss_accum.clone())
    _stream_case("reduce_loss", run)


# --------------------------------------------------------------------------------------------------------------------------
# the per-op entries (runners: the bodies of tests/test_gpu_modular_ops.py, test_gpu_transr.py, test_gpu_loss_entry.py)
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in W.NEG_CASES if c["flags"] == 0 and (c["model"], c["d_e"]) in (("TransE_l2", 36), ("RotatE", 48))],
                         ids=lambda c: c["id"])
def test_score_neg(c):
    with _through("score_neg"):
        WC.test_score_neg_fwd_bwd(c)


@pytest.mark.parametrize("c", _pick(W.MODEL_NEG_CASES, "QuatE-D36-C2-c8-N24-f0", "PairRE-D36-C2-c5-N33-f0", "TransH-D36-C1-c12-N20-f0"), ids=lambda c: c["id"])
def test_score_neg_of_quate_pairre_transh(c):
    with _through("score_neg"):
        WC.test_score_neg_fwd_bwd_of_quate_pairre_transh(c)


@pytest.mark.parametrize("c", _pick(M.POS_CASES, "DistMult-D36", "RotatE-D48", "RESCAL-D18"), ids=lambda c: c["id"])
def test_score_pos(c):
    from test_gpu_modular_ops import run_pos_case
    _stream_case("score_pos", lambda verify: run_pos_case(c, Bs=(37,)))


def test_loss_fwd_bwd():
    with _through("loss_fwd_bwd"):
        WC.test_loss_fwd_bwd(("Logsigmoid", True, 1.0, False, 1.0, True))


def test_pnorm_pow():
    from test_gpu_modular_ops import run_pnorm_case
    _stream_case("pnorm_pow", lambda verify: run_pnorm_case(3, True, shapes=[(3000, 30), (None, 777)]))


def test_mask_diag():
    from test_gpu_modular_ops import run_mask_diag_case
    _stream_case("mask_diag", lambda verify: run_mask_diag_case(M.MASK_SHAPES[0]))


def test_gather_and_scatter_rows():
    """distinct indices: the float atomics of kge_scatter_add_rows add one term per element, in no order"""
    from test_gpu_modular_ops import run_gather_case
    case = M.GATHER_CASES[1]
    assert case[0] == "distinct"
    _stream_case("gather_and_scatter_rows", lambda verify: run_gather_case(case))


def test_adagrad_scatter():
    """unique indices (with duplicates the atomics' order, and so the last bit, is free)"""
    from test_gpu_modular_ops import run_adagrad_scatter_case
    _stream_case("adagrad_scatter", lambda verify: run_adagrad_scatter_case(30, False))


def test_rank_from_scores():
    from test_gpu_modular_ops import run_rank_case
    _stream_case("rank_from_scores", lambda verify: run_rank_case((1000, 65), True))


def test_transr_projections():
    from test_gpu_transr import run_projection_ops_case
    _stream_case("transr_projections", lambda verify: run_projection_ops_case(3, 33, 70, 64, 40))


# --------------------------------------------------------------------------------------------------------------------------
# ranking, top-K, inference
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _pick(W.RANK_CASES, "DistMult-h32-n130-filt", "TransE_l1-h32-n40-raw", "TransR-h16-n40-filt"), ids=lambda c: c["id"])
def test_rank_eval_ex(c):
    with _through("rank_eval_ex"):
        WC.test_rank_eval_ex(c)


@pytest.mark.parametrize("c", _pick(W.MODEL_RANK_CASES, "QuatE-D36-filt", "PairRE-D36-raw", "TransH-D16-filt"), ids=lambda c: c["id"])
def test_rank_eval_ex_of_quate_pairre_transh(c):
    with _through("rank_eval_ex"):
        WC.test_rank_eval_ex_of_quate_pairre_transh(c)


@pytest.mark.parametrize("c", _pick(W.MODEL_CHUNKED_CASES, "QuatE-D36-lists", "PairRE-D36-self", "TransH-D36-all"), ids=lambda c: c["id"])
def test_rank_eval_chunked_of_quate_pairre_transh(c):
    with _through("rank_eval_chunked"):
        WC.test_rank_eval_chunked_of_quate_pairre_transh(c)


def test_rank_rel_eval_of_quate():
    with _through("rank_rel_eval"):
        WC.test_rank_rel_eval_of_quate(W.MODEL_REL_CASES[1])


@pytest.mark.parametrize("filtered", [False, True], ids=["select", "filtered"])
@pytest.mark.parametrize("c", _pick(W.MODEL_TOPK_CASES, "QuatE-D36-K10-g1", "PairRE-D36-K128-g9", "TransH-D16-K10-g1", "TransH-D36-K128-g9"), ids=lambda c: c["id"])
def test_topk_select_of_quate_pairre_transh(c, filtered):
    with _through("topk_select"):
        WC.test_topk_select_of_quate_pairre_transh(c, filtered)


def test_rank_eval_split_and_plain():
    """kge_rank_eval on every entity and kge_rank_eval_split with the candidates in a second table, called directly as in the
    workspace-contract test of the same name (there its proxy supplies the workspace); bounds: chunked_eval_cases.expected"""
    import chunked_eval_cases as CC
    from dglke_amd import _lib
    c = W.RANK_CASES[0]
    k, rk = WC._cc_ranker(c, batch=W.RANK_EB)
    ent, rel = rk.ent, rk.rel
    h, r, t = (WC._dev(x) for x in (k.h, k.r, k.t))
    lo_hi = CC.expected(c["model"], c["hidden"], False, CC.E, None)

    def run(verify):
        res = {}
        ws = torch.empty(int(_lib.lib().kge_rank_workspace_bytes(W.RANK_EB, CC.N_ENT, ent.shape[1])), dtype=torch.uint8, device=DEV)
        for name in ("kge_rank_eval", "kge_rank_eval_split"):
            ranks = torch.zeros(CC.E, dtype=torch.int32, device=DEV)
            head = (rk.model, 0, _lib.ptr(ent), CC.N_ENT) + ((_lib.ptr(ent), CC.N_ENT) if name.endswith("split") else ())
            mid = (_lib.ptr(rel), CC.N_REL) + ((None,) if name.endswith("split") else ())
            _lib.check(getattr(_lib.lib(), name)(*(head + mid + (_lib.ptr(h), _lib.ptr(r), _lib.ptr(t), CC.E, ent.shape[1], rel.shape[1], k.gamma,
                                                                   k.emb_init, None, CC.N_ENT, None, None, W.RANK_EB, _lib.ptr(ranks), None,
                                                                   _lib.ptr(ws), ws.numel(), 0, _lib.stream_ptr()))))
            if verify:
                WC._in_band(ranks.cpu().numpy(), lo_hi[0], lo_hi[1], lo_hi[2], name)
            res[name] = ranks
        return res
    _stream_case("rank_eval_split_and_plain", run)


@pytest.mark.parametrize("c", _pick(W.CHUNKED_CASES, "DistMult-h32-lists", "RotatE-h16-self"), ids=lambda c: c["id"])
def test_rank_eval_chunked(c):
    with _through("rank_eval_chunked"):
        WC.test_rank_eval_chunked(c)


@pytest.mark.parametrize("c", _pick(W.REL_CASES, "TransE_l2-h32-r130", "RotatE-h16-r7"), ids=lambda c: c["id"])
def test_rank_rel_eval(c):
    with _through("rank_rel_eval"):
        WC.test_rank_rel_eval(c)


@pytest.mark.parametrize("filtered", [False, True], ids=["select", "filtered"])
def test_topk_select(filtered):
    c, = _pick(W.TOPK_CASES, "DistMult-h36-K10-batch_head")
    with _through("topk_select"):
        WC.test_topk_select(c, filtered)


def test_topk_vector():
    with _through("topk_vector"):
        WC.test_topk_vector(10, 5000, "shuffled")


def test_sim_pairwise():
    """EmbSimInfer.topK(pair_ws=True): kge_sim_pairwise, then the top-K of its scores; float64 similarities and acceptance rule of
    test_emb_sim_fp64 (test_gpu_infer.py)"""
    from dglke_amd.infer import EmbSimInfer
    from test_gpu_infer import accept, exact_sim
    rng = np.random.RandomState(7)
    emb = rng.uniform(-1, 1, (300, 36)).astype(np.float32)
    pl, pr = rng.randint(0, 300, 100), rng.permutation(300)[:100]

    def run(verify):
        res = {}
        for sim in ("cosine", "l2", "ext_jaccard"):
            m = EmbSimInfer.from_tensor(0, torch.from_numpy(emb), sim)
            (hl, tl, sl), = m.topK(pl, pr, pair_ws=True, k=10)
            if verify:
                Sp = exact_sim(sim, emb, pl, pr).diagonal().cpu().numpy()
                ex = {}
                for i in range(100):
                    ex.setdefault((int(pl[i]), int(pr[i])), []).append(float(Sp[i]))
                accept(ex, list(zip(hl.tolist(), tl.tolist())), [float(x) for x in sl], 10, None)
            res.update({sim + " h": hl, sim + " t": tl, sim + " s": sl})
        return res
    _stream_case("sim_pairwise", run)


def test_triples_known():
    """KnownIndex.known against a Python set, as in test_triples_known_kernel_and_embed_sim (test_gpu_link_predict.py)"""
    from dglke_amd.known import KnownIndex
    rng = np.random.RandomState(71)
    NE, R = 500, 7
    kh, kr, kt = rng.randint(0, NE, 3000), rng.choice([0, 1, 2, 4, 5, 6], 3000), rng.randint(0, NE, 3000)
    kh[:4], kr[:4], kt[:4] = [0, 0, NE - 1, NE - 1], [0, 6, 0, 6], [0, NE - 1, 0, NE - 1]
    known = set(zip(kh.tolist(), kr.tolist(), kt.tolist()))
    qh, qr, qt = (np.concatenate([a[:1500], b]) for a, b in zip((kh, kr, kt), (rng.randint(0, NE, 1500), rng.randint(0, R, 1500), rng.randint(0, NE, 1500))))
    want = [x in known for x in zip(qh.tolist(), qr.tolist(), qt.tolist())]

    def run(verify):
        ix = KnownIndex((kh, kr, kt), NE, R, DEV)
        got = ix.known(*(torch.as_tensor(x, device=DEV) for x in (qh, qr, qt)))
        if verify:
            assert got.dtype == torch.uint8 and got.cpu().numpy().astype(bool).tolist() == want
        return dict(known=got)
    _stream_case("triples_known", run)


# --------------------------------------------------------------------------------------------------------------------------
# the owner side and the routing of the range-sharded step (runners: the bodies of tests/test_gpu_dist.py and
# test_gpu_emit_messages.py, single process)
# --------------------------------------------------------------------------------------------------------------------------
def test_adagrad_apply_rows_and_packed():
    import time
    import test_gpu_emit_messages as EM
    from test_gpu_emit_messages import run_apply_packed_case
    from test_gpu_modular_ops import run_adagrad_apply_rows_case
    EM.T0.append(time.time()) if not EM.T0 else None         # (its error report's clock, started by that file's own fixture)

    def run(verify):
        res = {"rows " + k: v for k, v in run_adagrad_apply_rows_case(30).items()}
        for inside in (False, True):
            res.update({"packed %d %s" % (inside, k): v for k, v in run_apply_packed_case(30, 2, inside).items()})
        return res
    _stream_case("adagrad_apply_rows_and_packed", run)


def test_adagrad_apply_merged():
    """three sources, messages with and without their ids inside, and the pair launch"""
    from test_gpu_dist import run_apply_merged_case
    _stream_case("adagrad_apply_merged", lambda verify: run_apply_merged_case(3, 100, 64, 120))


def test_route():
    """kge_route_build on host-built plans; kge_route_fill, kge_route_build and kge_route_build_group on sampler slots with
    DistEngine.ensure_capacity reading the fill in between; kge_gather_rows_req"""
    from test_gpu_dist import run_gather_rows_req_case, run_route_build_case, run_route_fill_case

    def run(verify):
        res = {"build " + k: v for k, v in run_route_build_case().items()}
        res.update({"fill " + k: v for k, v in run_route_fill_case().items()})
        res.update({"req " + k: v for k, v in run_gather_rows_req_case().items()})
        return res
    _stream_case("route", run)


def test_gather_rows_sharded():
    """ShardedTables.gather over three emulated shards with a ragged last one; baseline: the rows of the full table, bit for bit
    (test_emulated_shards_equal_single_table, test_gpu_p2p.py)"""
    from dglke_amd import p2p
    n_ent, n_rel, d = 1000, 23, 36
    rng = np.random.RandomState(3)
    ent, rel = rng.randn(n_ent, d).astype(np.float32), rng.randn(n_rel, d).astype(np.float32)
    ids = np.concatenate([[0, n_ent - 1, n_ent // 2, 1], rng.randint(0, n_ent, 300)]).astype(np.int64)

    def run(verify):
        tabs = p2p.ShardedTables(n_ent, n_rel, d, d, DEV, emulate=3)
        tabs.load_full(torch.from_numpy(ent).to(DEV), torch.from_numpy(rel).to(DEV))
        got = tabs.gather("ent", torch.from_numpy(ids).to(DEV))
        if verify:
            assert np.array_equal(got.cpu().numpy(), ent[ids])
        return dict(rows=got)
    _stream_case("gather_rows_sharded", run)


# --------------------------------------------------------------------------------------------------------------------------
# test support
# --------------------------------------------------------------------------------------------------------------------------
def test_debug_epoch_order():
    """kge_debug_epoch_order for a graph of 2^32 + 15 triples, shuffled and not; baseline: the Python-integer statement, as in
    test_epoch_order_of_any_graph_size_equals_the_statement (test_gpu_sampler_statement.py)"""
    from test_gpu_sampler_statement import epoch_order, order_statement
    n = (1 << 32) + 15
    positions = [0, 1, n - 2, n - 1] + [int(x) % n for x in np.random.RandomState(4).randint(0, 1 << 62, 300, dtype=np.int64)]
    epochs, pos = [ep for ep in (0, 1, 9, 1 << 40) for _ in positions], positions * 4

    def run(verify):
        res = {}
        for shuffled in (True, False):
            got = epoch_order(n, 3, shuffled, epochs, pos)
            if verify:
                assert np.array_equal(got.cpu().numpy().view(np.uint64), order_statement(n, 3, shuffled, epochs, pos)), shuffled
            res["shuffled %d" % shuffled] = got
        return res
    _stream_case("debug_epoch_order", run)


# --------------------------------------------------------------------------------------------------------------------------
# two engines, two streams
# --------------------------------------------------------------------------------------------------------------------------
def _tables_of(eng):
    return {k: getattr(eng, k).clone() for k in ("ent", "ent_state", "rel", "rel_state", "loss_accum", "tickets")}


def test_two_engines_two_streams():
    """two StepEngines of one TransE_l2 case on different batches - each with its own tables, workspace, tickets, loss_accum and
    kge_pipe - on two side streams, their calls interleaved from one thread: A's PHASE_GATHER, B's PHASE_GATHER, A's FORWARD ...;
    then a three-step kge_step_async group with the flush, step by step.  Each engine's tables, Adagrad state and loss sums equal,
    bit for bit, what the same engine gives when it runs alone"""
    from dglke_amd import _lib, plan
    c, = _pick(W.ASYNC_CASES, "TransE_l2-h36-N24-rel")
    bts = W.step_batches(c, 6)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    PHASES = (_lib.PHASE_GATHER, _lib.PHASE_FORWARD, _lib.PHASE_BACKWARD, _lib.PHASE_UPDATE)

    def build(k):
        with torch.cuda.stream(streams[k]):
            eng = WC._engine(c)
            mine = [plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV) for bt in bts[3 * k:3 * k + 3]]
        return eng, mine

    def phase(k, eng, b, ph):
        with torch.cuda.stream(streams[k]):
            out = _lib.KgeStepOut()
            out.loss_accum, out.tickets = _lib.ptr(eng.loss_accum), _lib.ptr(eng.tickets)
            assert _lib.stream_ptr() == streams[k].cuda_stream
            _lib.check(_lib.lib().kge_step_phase(C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(eng.workspace_for(b)),
                                                 eng._ws_bytes, ph, _lib.stream_ptr()))

    def async_step(k, eng, mine, s):
        with torch.cuda.stream(streams[k]):
            if s < len(mine):
                eng.step_async(mine[s], next_batch=mine[s + 1] if s + 1 < len(mine) else None)
            else:
                eng.flush_async()

    def run(order):
        """order: the (engine, step, part) sequence of the calls"""
        engs = [build(0), build(1)]
        torch.cuda.synchronize()
        for k, s, ph in order("phase"):
            phase(k, engs[k][0], engs[k][1][s], ph)
        torch.cuda.synchronize()
        mid = [_tables_of(e) for e, _ in engs]
        for k, s, _ in order("async"):
            async_step(k, engs[k][0], engs[k][1], s)
        torch.cuda.synchronize()
        assert engs[0][0]._pipe.value != engs[1][0]._pipe.value
        return mid, [_tables_of(e) for e, _ in engs]

    def alone(kind):
        return [(k, s, ph) for k in (0, 1) for s in range(3 if kind == "phase" else 4) for ph in (PHASES if kind == "phase" else (None,))]

    def interleaved(kind):
        return [(k, s, ph) for s in range(3 if kind == "phase" else 4) for ph in (PHASES if kind == "phase" else (None,)) for k in (0, 1)]
    mid0, end0 = run(alone)
    mid1, end1 = run(interleaved)
    for k in (0, 1):
        _same(mid0[k], mid1[k], "engine %d, kge_step_phase interleaved with the other engine's" % k)
        _same(end0[k], end1[k], "engine %d, kge_step_async interleaved with the other engine's" % k)
    assert not torch.equal(mid0[0]["ent"], mid0[1]["ent"]) and not torch.equal(mid0[0]["ent"], end0[0]["ent"])    # they trained, on different batches


# --------------------------------------------------------------------------------------------------------------------------
# the proxy itself, and the table
# --------------------------------------------------------------------------------------------------------------------------
def test_the_proxy_holds_a_call_to_its_stream_and_passes_a_refusal_through():
    """a call that names another stream than the mode's fails in the proxy BEFORE it reaches the library; a call the library
    refuses (KGE_ERR_ARG before any launch) comes back with its code from inside the capture, is not replayed and not counted"""
    from dglke_amd import _lib
    p = _probe()
    x = torch.ones(2, 3, 3, device=DEV)
    other = torch.cuda.Stream()
    before = {m: set(CALLED[m]) for m in MODES}
    for mode in ("side", "capture"):
        with _installed(p, mode):
            for wrong in (0, None, other.cuda_stream):
                with pytest.raises(AssertionError, match="kge_mask_diag was given stream"):
                    _lib.lib().kge_mask_diag(_lib.ptr(x), 2, 3, 3, wrong)
            with torch.cuda.stream(other), pytest.raises(AssertionError, match="the run left the"):
                _lib.lib().kge_mask_diag(_lib.ptr(x), 2, 3, 3, other.cuda_stream)
            n = len(p.graphs)
            assert _lib.lib().kge_mask_diag(None, 2, 3, 3, _lib.stream_ptr()) == -1 and len(p.graphs) == n
    with _installed(p, "default"):
        with pytest.raises(AssertionError, match="kge_mask_diag was given stream"):
            _lib.lib().kge_mask_diag(_lib.ptr(x), 2, 3, 3, p.side.cuda_stream)
    assert bool((x == 1).all()), "a call the proxy stopped reached the library"
    assert {m: set(CALLED[m]) for m in MODES} == before


def test_every_entry_ran_in_all_three_modes():
    """over the proxy's call log of the whole file (run it whole: a selection of cases leaves entries out)"""
    due = {n for n in S.STREAM_ENTRIES if S.cases_of(n)}
    for mode in MODES:
        assert due <= CALLED[mode], "never called in mode %r: %s" % (mode, sorted(due - CALLED[mode]))
