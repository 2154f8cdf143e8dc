"""The two contracts of include/kge_hip.h for every entry TransD (KGE_TRANSD = 14) runs through:

  workspace  "ws_bytes of the size function is enough, its contents on entry do not matter, nothing outside the carved buffers is
             written": every call gets a guarded buffer [GUARD | need | GUARD] with ws_bytes = need exactly, carved with a gap behind
             every buffer (kge_debug_carve), filled with 0x00, with 0xFF and with random bytes; the three results are equal bit for
             bit, the free bytes - guards, gaps, padding - still hold the fill, and need - 1 bytes are refused with
             KGE_ERR_WORKSPACE and nothing written;
  stream     "every call takes an explicit stream and only enqueues kernels on it": every case on the default stream, on a side
             stream, and with every call captured alone into a graph that is replayed - all three bit for bit the same.

The helpers of tests/workspace_cases.py (Trace, free_mask, describe_stray, Entry) and the stream proxy of
tests/test_gpu_stream_contract.py take the model as they are.  The workspace proxy is this file's own: ranking and top-K of TransD
are sized for 2 * n_cand candidates (two scalars per candidate, _lib.rank_ws_cands), which the size table of workspace_cases.py
does not know.  Cases, inputs and the float64 baselines are those of tests/transd_cases.py; the first run of every case is held to
them with the suite's tolerances."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import adam_cases as A
import stream_cases as S
import transd_cases as Q
import workspace_cases as W
from test_gpu_parity import DEV
from test_gpu_transd import _batch, _dev, _engine

pytestmark = pytest.mark.gpu

ARENA_BYTES = 32 << 20
_STATE = {}


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """a lost GPU context fails every later call: end the session instead of running the rest of the file against it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU context is lost (%s): nothing more is run" % (e,), returncode=3)


def _entries():
    """workspace_cases.WS_ENTRIES with the sizes of the entries whose TransD workspace is the one of 2 * n_cand candidates"""
    from dglke_amd import _lib
    e = {n: W.WS_ENTRIES[n] for n in ("kge_step_fused", "kge_step_fused_known", "kge_step_phase", "kge_step_phase_known", "kge_step_optim",
                                      "kge_score_neg_fwd", "kge_score_neg_bwd", "kge_rank_eval_chunked")}
    e["kge_rank_eval_ex"] = W.Entry(22, lambda h, a, gap: int(h.kge_rank_workspace_bytes(a[19], _lib.rank_ws_cands(a[0], a[16]), a[11])))
    topk = lambda h, a, gap: int(h.kge_topk_workspace_bytes(a[9], _lib.rank_ws_cands(a[0], a[15]), _lib.topk_row_width(a[0], a[10]), a[19]))
    e["kge_topk_select"] = W.Entry(22, topk)
    e["kge_topk_select_filtered"] = W.Entry(22, topk)
    return e


class Probe(object):
    """stands in for the ctypes handle (dglke_amd._lib._lib): every call of a workspace entry gets the guarded buffer"""

    def __init__(self, real, arena, arena2):
        self.real, self.arena, self.arena2 = real, arena, arena2
        self.fill, self.short = 0, False             # fill: 0 / 0xFF / "random"
        self.entries = _entries()
        self.trace = W.Trace(real, W.GAP)
        self.calls = []

    def _poison(self, buf):
        if self.fill == "random":
            buf.copy_(torch.randint(0, 256, (buf.numel(),), dtype=torch.uint8, device=buf.device))
        else:
            buf.fill_(self.fill)

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        e = self.entries.get(name)
        if e is None:
            assert name not in W.WS_ENTRIES, name + ": a workspace entry this file does not guard"
            return fn

        def call(*a):
            from dglke_amd import _lib
            a = list(a)
            self.trace.reset()
            need = e.need(self.real, a, W.GAP)
            k = self.trace.count()
            region = W.GUARD + need + W.GUARD
            assert 0 < need and region <= self.arena.numel(), (name, need)
            later_phase = e.phases is not None and not (int(a[e.phases]) & _lib.PHASE_GATHER)     # (the phases of a step share it)
            if not later_phase:
                self._poison(self.arena[:region])
                self.before = self.arena[:region].clone()
            a[e.ws], a[e.ws + 1] = self.arena.data_ptr() + W.GUARD, need - 1 if self.short else need
            mask_need = 0
            if e.known is not None and a[e.known] is not None:         # the known-pair mask: exactly kge_known_mask_bytes, guarded
                b = W._obj(a[e.ws - 2])
                mask_need = int(self.real.kge_known_mask_bytes(b.B, b.N))
                if not later_phase:
                    self.arena2[:2 * W.GUARD + mask_need].fill_(0x5A)
                a[e.known + 1], a[e.known + 2] = self.arena2.data_ptr() + W.GUARD, mask_need
            self.trace.reset()
            rc = fn(*a)
            pairs = self.trace.pairs(last=k or None) if self.trace.count() >= max(k, 1) else []
            self.trace.reset()
            self.calls.append(name)
            torch.cuda.synchronize()
            if self.short:
                assert rc == W.ERR_WORKSPACE, "%s with ws_bytes = need - 1 returned %d" % (name, rc)
                assert torch.equal(self.arena[:region], self.before), name + ": refused, but the buffer was written"
                return rc
            assert rc == 0, "%s returned %d: %s" % (name, rc, self.real.kge_last_error())
            assert pairs, name + ": no buffer carved"
            W.check_layout(pairs, need, W.GAP)
            m = torch.from_numpy(W.free_mask(pairs, need)).to(DEV)
            bad = (self.arena[:region] != self.before) & m
            if bool(bad.any()):
                off = np.nonzero(bad.cpu().numpy())[0] - W.GUARD
                pytest.fail("%s, fill %r: %s" % (name, self.fill, W.describe_stray(off, pairs, need)))
            if mask_need:
                g = self.arena2[:2 * W.GUARD + mask_need]
                assert bool((torch.cat([g[:W.GUARD], g[W.GUARD + mask_need:]]) == 0x5A).all()), name + ": written outside the known-pair mask"
            return rc
        return call


def _probe():
    from dglke_amd import _lib
    if "probe" not in _STATE:
        _STATE["probe"] = Probe(_lib.lib(), torch.zeros(ARENA_BYTES, dtype=torch.uint8, device=DEV),
                                torch.zeros(1 << 20, dtype=torch.uint8, device=DEV))
    return _STATE["probe"]


@contextlib.contextmanager
def _installed(p, fill, short=False):
    from dglke_amd import _lib
    assert _lib._lib is p.real
    p.fill, p.short = fill, short
    p.trace.reset()
    _lib._lib = p
    try:
        yield p
    finally:
        _lib._lib = p.real
        assert p.real.kge_debug_carve(None, 0, 0) == 0


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in sorted(a):
        assert a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), \
            "%s: %s differs in %d of %d elements" % (what, k, int((_bits(a[k]) != _bits(b[k])).sum()), a[k].numel())


# --------------------------------------------------------------------------------------------------------------------------
# the cases: run(verify) -> {name: tensor}; verify: hold the result to the float64 statement
# --------------------------------------------------------------------------------------------------------------------------
K_STEP = 36                 # a partial k-stage
STEP_CASE = Q.STEP_CASES[1]
ND_CASE = [c for c in Q.STEP_CASES if c["neg_deg"]][0]


def _named(eng, extra=()):
    torch.cuda.synchronize()
    out = {n: t.detach().clone() for n, t in eng.named_tensors().items()}
    out["loss_sums"] = torch.tensor(np.array(eng.read_loss_sums(), np.float32))
    out.update(extra)
    return out


def _step_runner(c, entry, known=False):
    def run(verify):
        from dglke_amd import _lib
        from dglke_amd.known import KnownIndex
        eng = _engine(c, K_STEP)
        extra = {}
        for s_, bt in enumerate(Q.step_batches(c)):
            b = _batch(c, bt)
            kn = None
            if known:
                K, kn = Q.planted_known(bt, c["chunk"], c["N"])
                eng.attach_known(KnownIndex(K, c["n_ent"], c["n_rel"], DEV))
            f64 = [x.detach().cpu().numpy().astype(np.float64) for x in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)]
            if entry == "fused":
                want = eng.alloc_outputs(b)
                eng.step(b, want)
                extra.update({"%s%d" % (n_, s_): t.detach().clone() for n_, t in want.items() if isinstance(t, torch.Tensor)})
            elif known:
                eng.step_timed(b)
            else:
                ws = eng.workspace_for(b)
                out = _lib.KgeStepOut()
                out.loss_accum = _lib.ptr(eng.loss_accum)
                a = (C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(ws), eng._ws_bytes)
                for ph in (_lib.PHASE_GATHER, _lib.PHASE_FORWARD, _lib.PHASE_BACKWARD, _lib.PHASE_UPDATE):
                    _lib.check(_lib.lib().kge_step_phase(*a, ph, _lib.stream_ptr()))
            torch.cuda.synchronize()
            if verify:
                ref = Q.step(c, f64[0], f64[1], f64[2], f64[3], bt, kn)
                assert ref["share"] >= Q.DIST_SHARE and Q.residual_rows(ref) == 0
                for got, want64, what in ((eng.ent, f64[0], "entity rows"), (eng.rel, f64[2], "relation rows"),
                                          (eng.ent_state, f64[1], "entity state"), (eng.rel_state, f64[3], "relation state")):
                    ratio, err, bound = Q.worst(got.detach().cpu().numpy().astype(np.float64), want64, Q.grad_bound(want64))
                    assert ratio <= 1.0, "%s step %d %s: error %.3e, bound %.3e" % (c["id"], s_, what, err, bound)
        return _named(eng, extra)
    return run


def _adam_runner():
    def run(verify):
        from test_gpu_adam import _batch as a_batch, _engine as a_engine, _f64 as a_f64, _state as a_state
        c = Q.ADAM_CASE
        ent, rel = A.tables(c)
        eng = a_engine(c)
        eng.load_tables(ent, rel)
        for bt in A.batches(c)[:2]:
            before = a_state(eng)
            eng.step(a_batch(c, bt))
            if verify:
                ref = a_f64(before)
                with Q.adam_gradients():
                    A.step(c, ref, bt)
                after = a_state(eng)
                ratio, err, bound = Q.worst(after["ent"].astype(np.float64), ref["ent"], Q.grad_bound(ref["ent"]))
                assert ratio <= 1.0, "Adam entity rows: error %.3e, bound %.3e" % (err, bound)
        return _named(eng)
    return run


NEG_SHAPE = (1, 12, 20)     # the stacked 24 rows cross a tile boundary that 12 rows do not


def _neg_runner(neg_head):
    def run(verify):
        from dglke_amd import ops
        C_, chunk, N = NEG_SHAPE
        inp = Q.op_inputs(K_STEP, C_, chunk, N, neg_head)
        x, y, r, nb = (_dev(inp[n_], True) for n_ in ("x", "y", "r", "nb"))
        h, t = (y, x) if neg_head else (x, y)
        pos = ops.score_pos(Q.MODEL, h, r, t, Q.GAMMA)
        (pos * _dev(inp["dp"])).sum().backward()
        res = dict(pos=pos.detach().clone(), gh=h.grad.clone(), grp=r.grad.clone(), gt=t.grad.clone())
        x.grad = y.grad = r.grad = None
        s = ops.score_neg(Q.MODEL, neg_head, x, r, nb, C_, chunk, N, Q.GAMMA, emb_init=1.0)
        (s * _dev(inp["W"])).sum().backward()
        res.update(score=s.detach().clone(), gx=x.grad.clone(), gr=r.grad.clone(), gn=nb.grad.clone())
        torch.cuda.synchronize()
        if verify:
            ref = Q.op_reference(inp, C_, chunk, N, neg_head)
            for q in ("pos", "score") + Q.OP_GRADS:
                bound = Q.score_bound(ref[q]) if q in ("pos", "score") else Q.grad_bound(ref[q])
                ratio, err, b_ = Q.worst(res[q].cpu().numpy(), ref[q], bound)
                assert ratio <= 1.0, "%s: error %.3e, bound %.3e" % (q, err, b_)
        return res
    return run


TIE = (129, 36)             # two column tiles, the second of one column; the MFMA instances


def _rank_runner(chunked):
    def run(verify):
        from dglke_amd import eval as kev
        c = Q.tie_inputs(*TIE)
        ent, rel = _dev(c.ent), _dev(c.rel)
        E = len(c.h)
        rk = kev.Ranker(Q.MODEL, ent, rel, Q.TIE_GAMMA, 1.0, batch=16)
        res = {}
        for neg_head in (False, True):
            p, S_ = Q.tie_scores(c, c.h, c.r, c.t, neg_head)
            lists = Q.filter_lists(c, neg_head)
            fl = (_dev(lists[0]), _dev(lists[1]))
            if not chunked:
                got, pos = rk.ranks(c.h, c.r, c.t, neg_head, filt=fl, want_pos_score=True)
                want = Q.ranks_of(p, S_, lists)
            else:
                cand = Q.tie_candidates(TIE[0], E, Q.TIE_CHUNK)
                got, pos = rk.chunked_ranks(c.h, c.r, c.t, neg_head, Q.TIE_CHUNK, cand=_dev(cand), self_cand=True, want_pos_score=True)
                want = Q.chunked_ranks_of(c, p, S_, neg_head, cand, True, Q.TIE_CHUNK)
            torch.cuda.synchronize()
            if verify:
                assert np.array_equal(got.cpu().numpy().astype(np.int64), want), "ranks differ from the float64 ranks (neg_head=%d)" % neg_head
            res["ranks%d" % neg_head], res["pos%d" % neg_head] = got.clone(), pos.clone()
        return res
    return run


def _topk_runner(filtered):
    def run(verify):
        from dglke_amd import _lib
        n, k = TIE
        c = Q.tie_inputs(n, k)
        d_e, E, K = 2 * k, len(c.h), 128
        ent, rel = _dev(c.ent), _dev(c.rel)
        h, r, t, cd = _dev(c.h), _dev(c.r), _dev(c.t), torch.arange(n, dtype=torch.int64, device=DEV)
        res = {}
        for side in (0, 1):
            res_s = torch.zeros(E, K, dtype=torch.float32, device=DEV)
            res_o = torch.full((E, K), -1, dtype=torch.int64, device=DEV)
            base = torch.zeros(E, dtype=torch.int64, device=DEV)
            ws = torch.empty(_lib.topk_workspace_bytes(Q.MODEL_ID, E, n, d_e, K), dtype=torch.uint8, device=DEV)
            a = (Q.MODEL_ID, side, _lib.ptr(ent), n, _lib.ptr(rel), n, _lib.ptr(h), _lib.ptr(r), _lib.ptr(t), E, d_e, d_e, Q.TIE_GAMMA,
                 1.0, _lib.ptr(cd), n, _lib.ptr(base), 1, 1, K, _lib.ptr(res_s), _lib.ptr(res_o), _lib.ptr(ws), ws.numel())
            frng, fids = Q.filter_lists(c, bool(side))
            if filtered:
                fr, fi = _dev(frng.reshape(-1)), _dev(fids)
                _lib.check(_lib.lib().kge_topk_select_filtered(*a, _lib.ptr(fr), _lib.ptr(fi), _lib.stream_ptr()))
            else:
                _lib.check(_lib.lib().kge_topk_select(*a, _lib.stream_ptr()))
            torch.cuda.synchronize()
            if verify:
                _, S_ = Q.tie_scores(c, c.h, c.r, c.t, bool(side))
                go = res_o.cpu().numpy()
                for i in range(E):
                    keep = np.ones(n, bool)
                    if filtered:
                        keep[fids[frng[i, 0]:frng[i, 1]]] = False
                    ids = np.nonzero(keep)[0]
                    order = ids[np.argsort(-S_[i, ids], kind="stable")][:K]
                    assert np.array_equal(go[i, :len(order)], order), "top-K order of row %d, side %d" % (i, side)
            res["score%d" % side], res["order%d" % side] = res_s.clone(), res_o.clone()
        return res
    return run


# (id, runner, the entries the case must call)
CASES = [
    ("step_fused", _step_runner(STEP_CASE, "fused"), ["kge_step_fused"]),
    ("step_fused_neg_deg", _step_runner(ND_CASE, "fused"), ["kge_step_fused"]),
    ("step_fused_softmax", _step_runner([c for c in Q.STEP_CASES if c["genre"] == "Softmax"][0], "fused"), ["kge_step_fused"]),
    ("step_phase", _step_runner(STEP_CASE, "phase"), ["kge_step_phase"]),
    ("step_fused_known", _step_runner(STEP_CASE, "fused", known=True), ["kge_step_fused_known"]),
    ("step_phase_known", _step_runner(STEP_CASE, "phase", known=True), ["kge_step_phase_known"]),
    ("step_optim_adam", _adam_runner(), ["kge_step_optim"]),
    ("score_neg_tail", _neg_runner(False), ["kge_score_neg_fwd", "kge_score_neg_bwd"]),
    ("score_neg_head", _neg_runner(True), ["kge_score_neg_fwd", "kge_score_neg_bwd"]),
    ("rank_eval_ex", _rank_runner(False), ["kge_rank_eval_ex"]),
    ("rank_eval_chunked", _rank_runner(True), ["kge_rank_eval_chunked"]),
    ("topk_select", _topk_runner(False), ["kge_topk_select"]),
    ("topk_select_filtered", _topk_runner(True), ["kge_topk_select_filtered"]),
]
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("cid", IDS)
def test_workspace_contents_are_ignored_and_bounds_kept_to_the_byte(cid):
    _, run, entries = CASES[IDS.index(cid)]
    p = _probe()
    n0 = len(p.calls)
    with _installed(p, 0):
        r0 = run(True)
    seen = set(p.calls[n0:])
    assert set(entries) <= seen, "the case never called %s (called: %s)" % (sorted(set(entries) - seen), sorted(seen))
    with _installed(p, 0xFF):
        r1 = run(False)
    with _installed(p, "random"):
        r2 = run(False)
    _same(r0, r1, "0xFF-filled workspace against the zero-filled one")
    _same(r0, r2, "randomly filled workspace against the zero-filled one")


@pytest.mark.parametrize("cid", IDS)
def test_a_workspace_one_byte_short_is_refused_and_nothing_written(cid):
    from dglke_amd import _lib
    _, run, entries = CASES[IDS.index(cid)]
    p = _probe()
    n0 = len(p.calls)
    with _installed(p, 0xFF, short=True):
        with pytest.raises(_lib.KgeError, match="workspace too small"):       # (the proxy's own assertions are not KgeErrors)
            run(False)
    assert set(p.calls[n0:]) & set(entries), "no guarded entry was reached"


@pytest.mark.parametrize("cid", IDS)
def test_default_stream_side_stream_and_captured_replay_agree(cid):
    import test_gpu_stream_contract as SC
    _, run, entries = CASES[IDS.index(cid)]
    stream_entries = sorted(set(entries) | ({"kge_score_pos", "kge_score_pos_bwd"} if cid.startswith("score_neg") else set()))
    assert set(stream_entries) <= set(S.STREAM_ENTRIES), sorted(set(stream_entries) - set(S.STREAM_ENTRIES))
    p = SC._probe()
    got = {}
    for mode in SC.MODES:
        n0 = len(p.calls)
        with SC._installed(p, mode):
            got[mode] = {n_: v.clone() for n_, v in run(mode == "default").items()}
        seen = set(p.calls[n0:])
        assert set(stream_entries) <= seen, "%s, %s: the case never called %s" % (cid, mode, sorted(set(stream_entries) - seen))
    _same(got["default"], got["side"], "%s: on the side stream against the default stream" % cid)
    _same(got["default"], got["capture"], "%s: every call captured and replayed against the default stream" % cid)
