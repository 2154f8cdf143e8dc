"""The workspace contract of include/kge_hip.h on the device: every entry point that takes (ws, ws_bytes) runs on a guarded
buffer [4096 guard | need | 4096 guard] with ws_bytes = need EXACTLY, carved with a 256-byte gap behind every buffer
(kge_debug_carve), three times: the buffer filled with zero bytes, with 0xFF bytes (NaN as float, -1 as int32 / int64), and
dirty - whatever a step of another model and a larger shape left there (a ComplEx step; then once more behind a larger TransH step).

  contents ignored   every output, table, Adagrad state and rank array is bit for bit the same across the three fills;
  baseline right     the zero-fill result passes the float64 comparison of the entry's own test (helpers, oracle and tolerances
                     imported from those tests: a kernel that needs zeros is right on zeros and wrong on 0xFF);
  bounds kept        after the zero and the 0xFF run every byte that belongs to no carved buffer - gaps, padding, both guards -
                     still holds the fill value (checked after EVERY call of the entry);
  too small          ws_bytes = need - 1 is KGE_ERR_WORKSPACE with the buffer and the sentinel-filled outputs untouched;
  refused            an entry that does not serve a model (QuatE / PairRE / TransH outside the strict step, single-table ranking and
                     top-K) answers KGE_ERR_ARG with every byte of the filled region - the workspace body included - and every
                     sentinel-filled output untouched.

QuatE, PairRE and TransH run on the cases, float64 statements, bounds and input conditions of their own case modules (quate_cases.py,
pairre_cases.py, transh_cases.py) at this file's shapes; what they carve beyond the shared buffers - PairRE's PW, PGW and Pnrm, QuatE's
normalised relation table behind the DistMult layout of kge_rank_rel_eval, TransH's eight buffers (four of them stacked 2 B rows high),
its doubled A and TPQ of the chunked ranking - holds floats only: no integer buffer is added to the list below.  kge_step_optim runs
under the same proxy (Adam: adam_cases.py's statement; Adagrad kind: bit-equal to kge_step_fused / kge_step_fused_known).

The library calls go through the callers the other tests use (StepEngine, dglke_amd.ops, Ranker, dglke_amd.infer): a proxy in
front of the ctypes handle (Probe) swaps the (ws, ws_bytes) pair of every call for the guarded buffer.  Fills happen where the
contract allows them: before every call, except that the phases of one kge_step_phase step and the steps of one kge_step_async
group (up to the flush) share their workspace - filled before PHASE_GATHER / before the group only.  tickets, loss_accum and the
engine's other caller-zeroed words are never filled.

No entry is compared with a tolerance across fills: all are deterministic at these sizes (two zero-fill runs agree).

Integer-typed workspace buffers and the launch that writes all of each before any read (a -1 read as an id is an address):
  carve_step iota [2B + C N]   launch_gather3_sharded writes ids 0 .. 2B + C N - 1 next to the dense rows Xd (sharded TransR /
                               RESCAL only: the first launch of PREP; on local tables the buffer is never read)
  carve_step ndids [C N']      launch_nd_ids writes every [own | sampled] id (TransR with NEG_DEG_SAMPLE: first launch of PREP)
  carve_step Z (sign bytes)    transr_fwd kernels write every (edge, negative, column) sign before the backward reads them
  carve_chunked ids [nch x n]  chunk_ids_kernel (kge_rank_chunk.hip) writes every column of every chunk of the block (an empty
                               slot as row 0: scored, never counted) before the score-block kernels gather through it
  top-K part [rows x S x K]    topk_select_kernel: every (row block, segment) workgroup first sets its rows' K packed entries to
                               0 (= empty), then merges into them; topk_unpack_kernel reads exactly rows x S x K of them, S =
                               the launch's segment count (the carve holds room for the segment CAP)
  top-K o0 / o1                topk_unpack_kernel writes o0[0 .. rows S K); each merge round writes G x nout x K entries of the
                               half it targets and the next round reads exactly those
  carve_rank, carve_rank_rel   no integer buffers (comparison masks are written by the tile epilogue before the count kernel)
None of them is read before it is written; the reading found one contract bug elsewhere: kge_loss_fwd_bwd checked the room for its
staged loss terms AFTER the loss launch (fixed: refused before any launch), and its header asked for 2 B floats where the
256-byte-aligned carve needs more; kge_pnorm_pow answered a short workspace with KGE_ERR_ARG (now KGE_ERR_WORKSPACE).

The sampler job's tail scratch (kge_step_fused_sampling; csrc/kge_sampler_common.hpp tail_scratch, a fixed layout without the
allocator: guards only, no gaps) is all integers.  Who writes what before whom (csrc/kge_sampler_tail.hpp):
  hdr[0..12)   bucket counts: phase 1, workgroups 0 - 2 write the four words of their source each; read by phase 2
  ekeys        phase 1 deals counted keys to [bucket][part + rank]; phase 2 reads exactly the counted ones of each part
  rkeys [B]    phase 1, workgroup 3; read by the relation plan of phase 2
  esort, hdr[12..24)   phase 2 writes the n sorted keys and the totals of every bucket; read by phase 3 (an empty bucket's key 0
               is loaded and never used)
  escan, ust   big-bucket instance of phase 3 only: written, fenced and read back inside the workgroup
A key read from there becomes an index into the slot only after these writes.  Phase 3 of job k runs under the FIRST launch of the
step that carries job k + 1 (the group's last job: under its own update launch), next to that job's phase 1, which writes other
words: the jobs of a group share the scratch like the steps of an async group, so it is filled before job 0 only - a fill before
every step would erase the header and sorted keys the design carries across (the header said "one job"; corrected).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import chunked_eval_cases as CC
import modular_op_cases as M
import relation_rank_cases as RC
import workspace_cases as W
from oracle import kge_oracle as O
from test_gpu_parity import DEV, _close, _l1_ambiguous, _masked, grad_tol

pytestmark = pytest.mark.gpu

ARENA_BYTES = 96 << 20
SENT = float.fromhex("0x1.5a5a5ap+100")      # outputs start as this value: an element a kernel leaves unwritten shows
_STATE = {}


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
class Probe(object):
    """stands in for the ctypes handle (dglke_amd._lib._lib): every call of an entry of W.WS_ENTRIES gets the guarded buffer"""

    def __init__(self, real, arena, arena2):
        self.real, self.arena, self.arena2 = real, arena, arena2
        self.fill = None              # 0 / 0xFF: fill before, check after; None: leave the buffer as it is (dirty), no check
        self.short = False            # hand over need - 1 bytes
        self.refuse = False           # the call must be refused with KGE_ERR_ARG, every byte of the region still the fill
        self.async_open = False
        self.trace = W.Trace(real, W.GAP)
        self.calls, self.masks = [], {}
        assert arena.data_ptr() % 256 == 0 and arena2.data_ptr() % 256 == 0

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name == "kge_step_async_flush":
            def flush(*a):
                self.async_open = False
                return fn(*a)
            return flush
        e = W.WS_ENTRIES.get(name)
        if e is None:
            return fn

        def call(*a):
            from dglke_amd import _lib
            a = list(a)
            self.trace.reset()
            need = e.need(self.real, a, W.GAP)
            k = self.trace.count() + (e.more(a) if e.more else 0)
            if self.refuse and need <= 0:                              # (a size function may refuse the model too)
                need = 1 << 20
            region = W.GUARD + need + W.GUARD
            assert 0 < need and region <= self.arena.numel(), (name, need)
            # (the phase groups of one step share the workspace and the pair mask: filled before the call that has PHASE_GATHER)
            later_phase = e.phases is not None and not (int(a[e.phases]) & _lib.PHASE_GATHER)
            shared = later_phase or (name == "kge_step_async" and self.async_open)
            if self.fill is not None and not shared:
                self.arena[:region].fill_(self.fill)
            a[e.ws], a[e.ws + 1] = self.arena.data_ptr() + W.GUARD, need - 1 if self.short else need
            mask_need = 0
            if e.known is not None and a[e.known] is not None:         # the known-pair mask: exactly kge_known_mask_bytes, guarded
                b = W._obj(a[e.ws - 2])                                # (the batch stands two in front of `ws` in all of them)
                mask_need = int(self.real.kge_known_mask_bytes(b.B, b.N))
                if self.fill is not None and not later_phase:
                    self.arena2[:2 * W.GUARD + mask_need].fill_(self.fill)
                a[e.known + 1], a[e.known + 2] = self.arena2.data_ptr() + W.GUARD, mask_need
            if name == "kge_step_fused_sampling":                      # the job's tail scratch: exactly its size function, guarded
                job = W._obj(a[6])
                mask_need = int(self.real.kge_sampler_tail_scratch_bytes(job.B, job.C, job.N, job.n_ent))
                assert 2 * W.GUARD + mask_need <= self.arena2.numel()
                if self.fill is not None and job.k == 0:               # (the jobs of a group share it: see the module docstring)
                    self.arena2[:2 * W.GUARD + mask_need].fill_(self.fill)
                job.scratch, job.scratch_bytes = self.arena2.data_ptr() + W.GUARD, mask_need
            self.trace.reset()
            rc = fn(*a)
            n = self.trace.count()
            pairs = e.explicit(a) if e.explicit else self.trace.pairs(last=k or None) if n >= max(k, 1) else []
            self.trace.reset()
            if name == "kge_step_async" and rc == 0:
                self.async_open = True
            self.calls.append((name, need, len(pairs)))
            if self.refuse:
                torch.cuda.synchronize()
                assert rc == W.ERR_ARG, "%s returned %d, not KGE_ERR_ARG" % (name, rc)
                assert bool((self.arena[:region] == self.fill).all()), name + ": refused, but the region was written"
                assert not mask_need or bool((self.arena2[:2 * W.GUARD + mask_need] == self.fill).all()), name + ": refused, but its second buffer was written"
            elif self.short:
                torch.cuda.synchronize()
                assert rc == W.ERR_WORKSPACE, "%s with ws_bytes = need - 1 returned %d" % (name, rc)
                assert bool((self.arena[:region] == self.fill).all()), name + ": refused, but the buffer was written"
            elif self.fill is not None and rc == 0:
                torch.cuda.synchronize()
                self.check(name, pairs, need, e.halves)
                if mask_need:
                    g = self.arena2[:2 * W.GUARD + mask_need]
                    bad = torch.cat([g[:W.GUARD], g[W.GUARD + mask_need:]]) != self.fill
                    assert not bool(bad.any()), "%s: %d bytes written outside the %s" % (
                        name, int(bad.sum()), "sampler job's tail scratch" if name.endswith("_sampling") else "known-pair mask")
            return rc
        return call

    def check(self, name, pairs, need, halves):
        assert pairs, name + ": no buffer carved"
        key = (need, tuple(pairs), halves)
        if key not in self.masks:
            if len(self.masks) > 8:
                self.masks.clear()
            self.masks[key] = torch.from_numpy(W.free_mask(pairs, need, halves)).to(DEV)
        m = self.masks[key]
        bad = (self.arena[:m.numel()] != self.fill) & m
        if bool(bad.any()):
            off = np.nonzero(bad.cpu().numpy())[0] - W.GUARD
            pytest.fail("%s, fill 0x%02X: %s" % (name, self.fill, W.describe_stray(off, pairs, need)))


def _probe():
    from dglke_amd import _lib
    if "probe" not in _STATE:
        real = _lib.lib()
        _STATE["probe"] = Probe(real, torch.zeros(ARENA_BYTES, dtype=torch.uint8, device=DEV), torch.zeros(1 << 20, dtype=torch.uint8, device=DEV))
    return _STATE["probe"]


@contextlib.contextmanager
def _installed(p, fill, short=False, refuse=False):
    from dglke_amd import _lib
    assert _lib._lib is p.real
    p.fill, p.short, p.refuse, p.async_open = fill, short, refuse, False
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


def _contract(run, entries, donor=None, transh=True):
    """run(verify) -> {name: tensor}.  Zero fill (with the float64 baseline), 0xFF fill, dirty fill - and, transh: dirty once more
    behind the larger TransH step (every case that is not TransH's own); returns the zero-fill result"""
    p = _probe()
    n0 = len(p.calls)
    with _installed(p, 0):
        r0 = run(True)
    seen = {c[0] for c in p.calls[n0:]}
    assert set(entries) <= seen, "the case never called %s (called: %s)" % (sorted(set(entries) - seen), sorted(seen))
    with _installed(p, 0xFF):
        r1 = run(False)
    with _installed(p, None):
        (donor or _donor)(W.DONOR)
        r2 = run(False)
        if transh:
            _transh_donor()
            r3 = run(False)
    _same(r0, r1, "0xFF-filled workspace against the zero-filled one")
    _same(r0, r2, "dirty workspace against the zero-filled one")
    if transh:
        _same(r0, r3, "workspace left by the TransH step against the zero-filled one")
    return r0


# --------------------------------------------------------------------------------------------------------------------------
# the step
# --------------------------------------------------------------------------------------------------------------------------
def _dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dt is None else t.to(dt)


def _engine(c):
    from dglke_amd.engine import StepEngine
    ent, rel, proj = W.step_tables(c)
    tabs = [_dev(ent), torch.zeros(len(ent), device=DEV), _dev(rel), torch.zeros(len(rel), device=DEV)]
    if proj is not None:
        tabs += [_dev(proj), torch.zeros(len(rel), device=DEV)]
    eng = StepEngine(c["model"], c["n_ent"], c["n_rel"], c["hidden"], c["gamma"], c["lr"], DEV, c["de"], c["dr"], c["adv"], 1.0,
                     c["reg"], 3, loss_genre=c.get("genre", "Logsigmoid"), flags=c["flags"], tables=tuple(tabs))
    eng.d_e, eng.d_r = W.step_dims(c)
    eng.hp.d_r = eng.d_r
    assert tuple(eng.rel.shape) == (c["n_rel"], eng.d_r) and eng.hp.d_e == eng.d_e
    return eng


def _config(c):
    cfg = O.Config(c["model"], c["gamma"], c["hidden"], c["lr"], adv=c["adv"], adv_temp=1.0, reg_coef=c["reg"], reg_norm=3,
                   loss_genre=c.get("genre", "Logsigmoid"), double_ent=c["de"], double_rel=c["dr"], neg_deg=bool(c["flags"] & 32))
    cfg.ent_dim, cfg.rel_dim = W.step_dims(c)
    return cfg


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _tables64(eng):
    out = [_f64(eng.ent), _f64(eng.ent_state), _f64(eng.rel), _f64(eng.rel_state)]
    return out + ([_f64(eng.proj), _f64(eng.proj_state)] if eng.proj is not None else [])


@contextlib.contextmanager
def _softmax_oracle():
    """the oracle's loss with the Softmax genre of tests/softmax_loss_cases.py (every other genre: the oracle's own)"""
    import softmax_loss_cases as SM
    saved = O.loss_fwd_bwd
    O.loss_fwd_bwd = SM.hooked_loss_fwd_bwd
    try:
        yield
    finally:
        O.loss_fwd_bwd = saved


def _verify_step(c, cfg, bt, b, want, l4, eng, pre, tag):
    """one step against the float64 oracle restarted from the tables the step started from: the comparisons and tolerances of
    test_fused_step_matches_oracle_at_config_shapes (test_gpu_parity.py) and, for RESCAL / TransR, of
    test_matrix_models_random_shapes_match_oracle (test_gpu_rescal.py) with its exclusions of rows that have no digits"""
    chunk, N, lr = c["chunk"], c["N"], c["lr"]
    matrix = c["model"] in ("RESCAL", "TransR")
    ent64, es64, rel64, rs64 = pre[:4]
    ent0, rs0 = ent64.copy(), rs64.copy()
    negrows = ent64[bt["neg"]].copy()
    amb = dict(slots=[], edges=[], pos_local=[], ent=[], rel=[])
    if c["model"] == "TransE_l1" and not (c["flags"] & 32):
        amb = _l1_ambiguous(bt, ent64, rel64, chunk, N)
        assert len(amb["ent"]) <= 3 and len(amb["rel"]) <= 2, amb
    if c["model"] == "TransR":
        pj64, ps64 = pre[4], pre[5]
        ps0 = ps64.copy()
        out = O.transr_train_step(cfg, ent64, es64, rel64, rs64, pj64, ps64, bt["nid"], bt["h_local"], bt["t_local"], bt["r"], bt["neg"],
                                  bt["neg_head"], chunk, N)
    else:
        with _softmax_oracle():
            out = O.train_step(cfg, ent64, es64, rel64, rs64, bt["nid"], bt["h_local"], bt["t_local"], bt["r"], bt["neg"], bt["neg_head"], chunk, N)
    if want is not None:
        _close(want["pos_score"].cpu(), out["pos_score"], 1e-4, 1e-4, tag + " pos_score")
        _close(want["neg_score"].cpu(), out["neg_score"], 1e-4, 2e-4 if matrix else 1e-4, tag + " neg_score")
        if c.get("genre") == "Softmax":      # (no positive / negative part: test_gpu_softmax_loss.py run_case)
            assert np.isnan(l4[0]) and np.isnan(l4[1]) and np.isnan(out["log"][0]) and np.isnan(out["log"][1]), tag
            _close(l4[2], out["log"][2], 1e-4, 1e-5, tag + " loss")
        else:
            _close(l4[:3], out["log"][:3], 1e-4, 1e-5, tag + " loss")
        _close(l4[3], out["log"][3], 1e-3, 1e-7, tag + " reg")
        gn = want["g_neg"].cpu().numpy()
        if c["flags"] & 32:          # the sampled rows of every chunk's N' block; their regulariser is added by the update kernel
            gn = gn.reshape(-1, chunk + N, gn.shape[1])[:, chunk:].reshape(-1, gn.shape[1])
            if c["reg"] > 0:
                gn = gn + O.reg_grad(negrows, c["reg"], 3)
        sel = np.searchsorted(b.p["ue_id"], bt["nid"])
        _close(_masked(want["g_pos_ent"].cpu().numpy()[sel], out["g_pos_ent"], amb["pos_local"]), out["g_pos_ent"], 3e-4,
               grad_tol(out["g_pos_ent"]), tag + " g_pos_ent")
        _close(_masked(gn, out["g_neg"], amb["slots"]), out["g_neg"], 3e-4, grad_tol(out["g_neg"]), tag + " g_neg")
        _close(_masked(want["g_rel"].cpu(), out["g_rel"], amb["edges"]), out["g_rel"], 3e-4, grad_tol(out["g_rel"]), tag + " g_rel")
    _close(_masked(eng.rel_state.cpu(), rs64, amb["rel"]), rs64, 2e-3, 1e-9, tag + " rel state")
    if not matrix:
        _close(_masked(eng.ent_state.cpu(), es64, amb["ent"]), es64, 2e-3, 1e-9, tag + " ent state")
        _close(_masked(eng.ent.cpu(), ent64, amb["ent"]), ent64, 1e-4, 1e-3 * lr, tag + " entity rows")
        _close(_masked(eng.rel.cpu(), rel64, amb["rel"]), rel64, 1e-4, 1e-3 * lr, tag + " relation rows")
        return

    def weak_rows(inc, ids):
        tr = np.unique(ids)
        return tr[inc[tr] < 1e-4 * np.median(inc[tr])]
    dead_r = weak_rows(rs64 - rs0, bt["r"])
    assert len(dead_r) <= 2, (tag, dead_r)
    _close(_masked(eng.rel.cpu(), rel64, dead_r), rel64, 1e-4, 5e-3 * lr, tag + " relation rows")
    starved = np.zeros(0, np.int64)
    if c["model"] == "TransR":
        _close(eng.proj_state.cpu(), ps64, 2e-3, 1e-9, tag + " projection state")
        dead = weak_rows(ps64 - ps0, bt["r"])
        assert len(dead) <= 2, (tag, dead)
        _close(_masked(eng.proj.cpu(), pj64, dead), pj64, 1e-4, 5e-3 * lr, tag + " projection rows")
        starved = np.unique(bt["h"][bt["h"] == bt["t"]])
    touched = set(bt["nid"].tolist()) | set(bt["neg"].tolist())
    assert len(starved) <= max(2, len(touched) // 10), (tag, len(starved))
    _close(_masked(eng.ent.cpu(), ent64, starved), ent64, 1e-4, 5e-3 * lr, tag + " entity rows")
    rest = sorted(set(range(c["n_ent"])) - touched)
    assert np.array_equal(_f64(eng.ent)[rest], ent0[rest]), tag + ": an untouched entity row moved"


def _outputs(eng, b, c):
    if not c["outputs"]:
        return None
    want = eng.alloc_outputs(b)
    for t in want.values():
        t.fill_(SENT)
    return want


def _collect(res, eng, s, want):
    if want is not None:
        for k, t in want.items():
            res["s%d %s" % (s, k)] = t.clone()
        res["s%d loss4" % s] = eng.loss4.clone()
    if s == "end":
        for k in ("ent", "ent_state", "rel", "rel_state", "proj", "proj_state"):
            if getattr(eng, k) is not None:
                res[k] = getattr(eng, k).clone()
        res["loss_accum"] = eng.loss_accum.clone()
        res["tickets"] = eng.tickets.clone()


def _phase_step(eng, b, want):
    """engine.step's argument block through the four kge_step_phase calls"""
    from dglke_amd import _lib
    out = _lib.KgeStepOut()
    if want is not None:
        out.loss4 = _lib.ptr(eng.loss4)
        for k, t in want.items():
            setattr(out, k, _lib.ptr(t))
    out.loss_accum = _lib.ptr(eng.loss_accum)
    out.tickets = _lib.ptr(eng.tickets)
    for ph in (_lib.PHASE_GATHER, _lib.PHASE_FORWARD, _lib.PHASE_BACKWARD, _lib.PHASE_UPDATE):
        _lib.check(_lib.lib().kge_step_phase(C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), 0, 0, ph, _lib.stream_ptr()))


def _run_steps(c, verify, entry="fused"):
    """two steps (tail- then head-corrupted) of a step case from its seeded tables; every output, then the tables"""
    from dglke_amd import plan
    eng = _engine(c)
    cfg = _config(c) if verify else None
    res = {}
    for s, bt in enumerate(W.step_batches(c), 1):
        b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV)
        want = _outputs(eng, b, c)
        pre = _tables64(eng) if verify else None
        if entry == "fused":
            eng.step(b, want)
        else:
            _phase_step(eng, b, want)
        torch.cuda.synchronize()
        _collect(res, eng, s, want)
        if verify:
            _verify_step(c, cfg, bt, b, want, eng.read_loss(), eng, pre, "%s step %d" % (c["id"], s))
    _collect(res, eng, "end", None)
    assert not bool(eng.tickets.any()), "the step did not return its tickets to zero"
    return res


def _donor(d):
    """a step of another model at a larger shape, on the same buffer: what the dirty fill leaves behind"""
    from dglke_amd import plan
    eng = _engine(d)
    bt = W.step_batches(d, 1)[0]
    eng.step(plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], d["chunk"], d["N"], bt["neg_head"], DEV))
    torch.cuda.synchronize()


def _step_donor(c):
    return (lambda _d: _donor(W.DONOR_ALT)) if c["model"] == "ComplEx" else None


@pytest.mark.parametrize("c", W.STEP_CASES, ids=lambda c: c["id"])
def test_step_fused(c):
    r = _contract(lambda verify: _run_steps(c, verify), ["kge_step_fused"], _step_donor(c))
    _STATE[("fused", c["id"])] = r


@pytest.mark.parametrize("c", W.PHASE_CASES, ids=lambda c: c["id"])
def test_step_phase_equals_the_fused_step(c):
    """filled before PHASE_GATHER only (the four phase groups share the workspace by design)"""
    ref = _STATE.get(("fused", c["id"]))
    if ref is None:
        p = _probe()
        with _installed(p, 0):
            ref = _run_steps(c, False)
    r = _contract(lambda verify: _run_steps(c, False, "phase"), ["kge_step_phase"], _step_donor(c))
    _same(ref, r, "kge_step_phase against kge_step_fused")


# ---- QuatE, PairRE, TransH (cases: W.MODEL_STEP_CASES; engines, comparisons and bounds: the models' own GPU tests) ----
def _model_test(model):
    import importlib
    return importlib.import_module({"QuatE": "test_gpu_quate", "PairRE": "test_gpu_pairre", "TransH": "test_gpu_transh"}[model])


def _model_engine(c):
    with W.model_shapes(c):
        eng = _model_test(c["model"])._engine(c, c["d_e"], c["flags"])
    assert tuple(eng.ent.shape) == (c["n_ent"], c["d_e"]) and tuple(eng.rel.shape) == (c["n_rel"], W.model_d_r(c["model"], c["d_e"]))
    return eng


def _run_model_steps(c, verify, entry="fused", known=False):
    """one step per corruption side, each from the fixed tables (the statements' conditions are asserted for exactly these inputs in
    test_workspace_inputs.py).  entry: fused / phase (with known: kge_step_fused_known / kge_step_phase_known through step_timed)"""
    from dglke_amd.known import KnownIndex
    T, Q = _model_test(c["model"]), W.model_cases(c["model"])
    res = {}
    for s, bt in enumerate(W.model_batches(c), 1):
        eng = _model_engine(c)
        kn = None
        if known:
            K, kn = Q.planted_known(bt, c["chunk"], c["N"])
            assert kn.any() and not kn.all()
            eng.attach_known(KnownIndex(K, c["n_ent"], c["n_rel"], DEV))
        b = T._batch(c, bt)
        want = _outputs(eng, b, c) if entry == "fused" or not known else None
        pre = _tables64(eng) if verify else None
        if entry == "fused":
            eng.step(b, want)
        elif known:
            eng.step_timed(b)
        else:
            _phase_step(eng, b, want)
        torch.cuda.synchronize()
        _collect(res, eng, s, want)
        _collect(res, eng, "end", None)
        res.update({"s%d %s" % (s, k): res.pop(k) for k in ("ent", "ent_state", "rel", "rel_state", "loss_accum", "tickets")})
        assert not bool(eng.tickets.any()), "the step did not return its tickets to zero"
        if verify:
            ent64, es64, rel64, rs64 = pre
            ent0 = ent64.copy()
            out = Q.step(c, ent64, es64, rel64, rs64, bt, kn)
            W.model_conditions(c, out)
            tag = "%s step %d%s" % (c["id"], s, " known" if known else "")
            if want is not None:
                errs = T._compare_step(c, eng, b, bt, want, out, (ent64, es64, rel64, rs64, ent0), tag, known=kn)
            else:
                errs = dict(ent_rows=Q.worst(_f64(eng.ent), ent64, Q.grad_bound(ent64)), rel_rows=Q.worst(_f64(eng.rel), rel64, Q.grad_bound(rel64)),
                            ent_state=Q.worst(_f64(eng.ent_state), es64, Q.grad_bound(es64)),
                            rel_state=Q.worst(_f64(eng.rel_state), rs64, Q.grad_bound(rs64)))
            T._check(errs, tag)
            assert not np.array_equal(_f64(eng.ent), ent0), tag + ": the step did not move the entity table"
    return res


def _transh_donor():
    """the second dirty fill: a larger TransH step (eight more buffers, four of them stacked) on the same buffer"""
    d = W.DONOR_TRANSH
    eng = _model_engine(d)
    eng.step(_model_test("TransH")._batch(d, W.model_batches(d, 1)[0]))
    torch.cuda.synchronize()


def _not_transh(c):
    """(the ComplEx donor alone stays for TransH's own cases)"""
    return c["model"] != "TransH"


@pytest.mark.parametrize("c", W.MODEL_STEP_CASES, ids=lambda c: c["id"])
def test_step_fused_of_quate_pairre_transh(c):
    r = _contract(lambda verify: _run_model_steps(c, verify), ["kge_step_fused"], transh=_not_transh(c))
    _STATE[("fused", c["id"])] = r


@pytest.mark.parametrize("c", W.MODEL_PHASE_CASES, ids=lambda c: c["id"])
def test_step_phase_of_quate_pairre_transh_equals_the_fused_step(c):
    """the four phase groups share one fill; bit-equal to the fused step"""
    ref = _STATE.get(("fused", c["id"]))
    if ref is None:
        p = _probe()
        with _installed(p, 0):
            ref = _run_model_steps(c, False)
    r = _contract(lambda verify: _run_model_steps(c, False, "phase"), ["kge_step_phase"], transh=_not_transh(c))
    _same(ref, r, "kge_step_phase against kge_step_fused")


# ---- kge_step_optim (cases: W.OPTIM_ADAM / W.OPTIM_ADAGRAD; engines, state and comparison: tests/test_gpu_adam.py) ----
def _state_tensors(st, s):
    return {"s%d %s" % (s, k): torch.from_numpy(np.ascontiguousarray(v)) for k, v in st.items()}


def _run_optim_adam(o, verify):
    """W.OPTIM_STEPS Adam steps through StepEngine.step (phases: step_timed, the four phase groups as four calls); tables, counts,
    both moment tables and the loss sums after every step.  Baseline: adam_cases.step under its ambiguity rule and cap, as in
    test_four_steps_match_the_statement (which also asserts the rows the step does not touch unchanged)"""
    import adam_cases as A
    import test_gpu_adam as TA
    import transh_cases as TH
    from dglke_amd.known import KnownIndex
    c = W.optim_case(o["case"])
    ent, rel = A.tables(c)
    eng = TA._engine(c)
    eng.load_tables(ent, rel)
    amb = dict(ent=np.zeros(ent.shape, bool), rel=np.zeros(rel.shape, bool))
    res = {}
    for s, bt in enumerate(A.batches(c, W.OPTIM_STEPS), 1):
        known = None
        if c["known"]:
            known, K = A.known_pairs(c, bt)
            eng.attach_known(KnownIndex(K, c["n_ent"], c["n_rel"], DEV))
        before = TA._state(eng)
        b = TA._batch(c, bt)
        eng.step_timed(b) if o["phases"] else eng.step(b)
        after = TA._state(eng)
        res.update(_state_tensors(after, s))
        res["s%d loss_accum" % s] = eng.loss_accum.clone()
        if verify:
            ref = TA._f64(before)
            with TH.adam_gradients():
                info = A.step(c, ref, bt, known)
            for tab in ("ent", "rel"):
                amb[tab] |= A.ambiguous(info[tab][0], info[tab][1], amb[tab].shape[0])
                assert amb[tab].mean() <= A.AMBIGUITY_CAP, "%s step %d: %.4f of %s is ambiguous" % (o["id"], s, amb[tab].mean(), tab)
            for k, (ratio, err, bound) in TA._compare_step(o["id"], before, after, ref, info, amb, s).items():
                assert ratio <= 1.0, "%s step %d %s: %.2f bounds off (error %.3e, bound %.3e)" % (o["id"], s, k, ratio, err, bound)
            assert not np.array_equal(before["ent"], after["ent"]) and after["ent_mom"].any() and after["rel_mom"].any()
    return res


@pytest.mark.parametrize("o", W.OPTIM_ADAM, ids=lambda o: o["id"])
def test_step_optim_adam(o):
    """-phases: filled before the call with PHASE_GATHER only; with a known index the pair mask stands in its own guarded buffer"""
    r = _contract(lambda verify: _run_optim_adam(o, verify), ["kge_step_optim"], transh=_not_transh(W.optim_case(o["case"])))
    if o["phases"]:
        ref = _STATE.get(("optim", o["case"]))
        if ref is None:
            with _installed(_probe(), 0):
                ref = _run_optim_adam(dict(o, phases=False), False)
        _same(ref, r, "the four phase groups of kge_step_optim against the whole step")
    else:
        _STATE[("optim", o["case"])] = r


def _run_optim_adagrad(cid, through_optim):
    """the body of test_adagrad_kind_is_the_existing_step_bit_for_bit (test_gpu_adam.py): an Adagrad engine stepped through
    kge_step_fused / kge_step_fused_known, or through kge_step_optim with kind = KGE_OPT_ADAGRAD"""
    import adam_cases as A
    import test_gpu_adam as TA
    from dglke_amd import _lib
    from dglke_amd.known import KnownIndex
    c = W.optim_case(cid)
    ent, rel = A.tables(c)
    eng = TA._engine(c, "Adagrad")
    eng.load_tables(ent, rel)
    opt = _lib.KgeOptim()
    opt.kind = _lib.OPT_ADAGRAD
    res = {}
    for s, bt in enumerate(A.batches(c, W.OPTIM_STEPS), 1):
        b = TA._batch(c, bt)
        if c["known"]:
            eng.attach_known(KnownIndex(A.known_pairs(c, bt)[1], c["n_ent"], c["n_rel"], DEV))
        if not through_optim:
            eng.step(b)
        elif c["known"]:
            km = eng.known_mask_for(b)
            assert TA._optim_call(eng, opt, b, known=C.byref(eng._known[0]), mask=_lib.ptr(km), mask_bytes=eng._kmask_bytes) == 0
        else:
            assert TA._optim_call(eng, opt, b) == 0
        res.update(_state_tensors(TA._state(eng), s))
        res["s%d loss_accum" % s] = eng.loss_accum.clone()
    assert not np.array_equal(res["s%d ent" % W.OPTIM_STEPS].numpy(), ent)
    return res


@pytest.mark.parametrize("cid", W.OPTIM_ADAGRAD)
def test_step_optim_adagrad_kind_is_the_existing_step(cid):
    """on the same guarded buffer kge_step_optim with kind = KGE_OPT_ADAGRAD is kge_step_fused (with an index: kge_step_fused_known)
    bit for bit - whose float64 comparison is test_step_fused's"""
    fused = "kge_step_fused_known" if W.optim_case(cid)["known"] else "kge_step_fused"
    ref = _contract(lambda verify: _run_optim_adagrad(cid, False), [fused])
    r = _contract(lambda verify: _run_optim_adagrad(cid, True), ["kge_step_optim"])
    _same(ref, r, "kge_step_optim (Adagrad kind) against " + fused)


def _run_async(c, verify):
    """a group of three steps and the flush; the pipeline's float64 statement and tolerances: test_gpu_async.py"""
    from dglke_amd import plan
    eng = _engine(c)
    bts = W.step_batches(c, 3)
    batches = [plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV) for bt in bts]
    pre = _tables64(eng)
    eng.steps_async(batches)
    torch.cuda.synchronize()
    res = {}
    _collect(res, eng, "end", None)
    if verify:
        for bt in bts:
            bt.update(chunk=c["chunk"], N=c["N"])
        e64, es, r64, rs = pre
        O.train_steps_async(_config(c), e64, es, r64, rs, bts, defer_rel=bool(c["flags"] & 64))
        _close(eng.ent_state.cpu(), es, 2e-3, 1e-9, c["id"] + " entity state")
        _close(eng.rel_state.cpu(), rs, 2e-3, 1e-9, c["id"] + " relation state")
        _close(eng.ent.cpu(), e64, 1e-4, 1e-2 * c["lr"], c["id"] + " entity table")
        _close(eng.rel.cpu(), r64, 1e-4, 1e-2 * c["lr"], c["id"] + " relation table")
    return res


@pytest.mark.parametrize("c", W.ASYNC_CASES, ids=lambda c: c["id"])
def test_step_async_group(c):
    """filled before the group only: the two halves carry the pending update from step to step"""
    _contract(lambda verify: _run_async(c, verify), ["kge_step_async"], _step_donor(c))


SHARDED = [c for c in W.STEP_CASES if c["id"] in ("TransE_l2-h36-N24", "TransE_l2-h36-N24-f32", "TransR-36x72", "RESCAL-h20")]


@pytest.mark.parametrize("c", SHARDED, ids=lambda c: c["id"])
def test_step_sharded_on_three_emulated_shards(c):
    """kge_step_sharded; TransR / RESCAL with the relation-side tables local (rel_local: the dense rows Xd and the identity ids
    iota).  Baseline as in test_gpu_p2p.py: every table bit-identical to the single-table step on the same batches"""
    from dglke_amd import p2p, plan
    from dglke_amd.engine import StepEngine
    d_e, d_r = W.step_dims(c)
    matrix = c["model"] in ("TransR", "RESCAL")
    bts = W.step_batches(c)

    def batches():
        return [plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV) for bt in bts]
    ref = _engine(c)
    for b in batches():
        ref.step(b)
    torch.cuda.synchronize()

    def run(verify):
        src = _engine(c)
        tabs = p2p.ShardedTables(c["n_ent"], c["n_rel"], d_e, d_r, DEV, emulate=3, rel_local=matrix,
                                 proj_dim=d_e * d_r if c["model"] == "TransR" else 0)
        tabs.load_full(src.ent, src.rel, **(dict(proj=src.proj) if matrix else {}))
        eng = StepEngine(c["model"], c["n_ent"], c["n_rel"], c["hidden"], c["gamma"], c["lr"], DEV, c["de"], c["dr"], c["adv"], 1.0,
                         c["reg"], 3, flags=c["flags"], shards=tabs)
        for b in batches():
            eng.step(b)
        torch.cuda.synchronize()
        res = {k: tabs.full(k).clone() for k in ("ent", "ent_state", "rel", "rel_state")}
        if c["model"] == "TransR":
            res.update(proj=tabs.proj_tab.clone(), proj_state=tabs.proj_state_tab.clone())
        res["loss_accum"] = eng.loss_accum.clone()
        if verify:
            for k in res:
                assert torch.equal(res[k], getattr(ref, k)), "%s differs between the sharded and the single-table step" % k
        return res
    _contract(run, ["kge_step_sharded"], _step_donor(c))


@pytest.mark.parametrize("N,model", [(24, None), (40, None)] + [(24, m) for m in W.NEW_MODELS], ids=["24", "40"] + ["%s-24" % m for m in W.NEW_MODELS])
def test_step_fused_known(N, model):
    """the pair mask at exactly kge_known_mask_bytes in a guarded buffer of its own (0xFF = every pair known: a word the mask kernel
    skips changes the loss); N = 24 / 40: one / two words per row.  Case, float64 statement and tolerances:
    known_negative_cases.py / test_step_with_known_index_matches_float64_statement.  QuatE / PairRE / TransH: their -D36-N24 case
    with the planted pairs of their own known-index test; then the same step as its four kge_step_phase_known groups
    (StepEngine.step_timed), bit-equal in tables and loss sums"""
    if model is not None:
        c = W.MODEL_KNOWN_CASES[model]
        r = _contract(lambda verify: _run_model_steps(c, verify, "fused", known=True), ["kge_step_fused_known"], transh=_not_transh(c))
        t = _contract(lambda verify: _run_model_steps(c, False, "phase", known=True), ["kge_step_phase_known"], transh=_not_transh(c))
        _same({k: v for k, v in r.items() if k in t}, t, "kge_step_phase_known against kge_step_fused_known")
        return
    import known_negative_cases as KN
    from test_gpu_known_negatives import _batch, _engine as known_engine, _index
    c = dict([x for x in KN.CASES if x["id"] == "l2-d32-n40"][0], N=N)
    bts, K, _ = KN.build(c)

    def run(verify):
        eng = known_engine(c)
        eng.attach_known(_index(K, c["n_ent"], c["n_rel"]))
        res = {}
        for s, bt in enumerate(bts, 1):
            pre = [_f64(x) for x in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)]
            b = _batch(c, bt)
            want = eng.alloc_outputs(b)
            eng.step(b, want)
            torch.cuda.synchronize()
            _collect(res, eng, s, want)
            if verify:
                known = KN.known_matrix(K, bt, c["chunk"], c["N"])
                assert known.any() and not known.all()
                out = KN.masked_step(c, pre[0], pre[1], pre[2], pre[3], None, None, bt, known)
                tag = "known N=%d step %d" % (N, s)
                _close(want["pos_score"].cpu(), out["pos_score"], 1e-4, 1e-4, tag + " pos_score")
                _close(want["neg_score"].cpu(), out["neg_score"], 1e-4, 1e-4, tag + " neg_score")
                l4 = eng.read_loss()
                _close(l4[:3], out["log"][:3], 1e-4, 1e-5, tag + " loss")
                _close(want["g_neg"].cpu(), out["g_neg"], 3e-4, grad_tol(out["g_neg"]), tag + " g_neg")
                _close(want["g_rel"].cpu(), out["g_rel"], 3e-4, grad_tol(out["g_rel"]), tag + " g_rel")
                _close(eng.ent_state.cpu(), pre[1], 2e-3, 1e-9, tag + " ent state")
                _close(eng.ent.cpu(), pre[0], 1e-4, c["rows"] * c["lr"], tag + " entity rows")
                _close(eng.rel.cpu(), pre[2], 1e-4, c["rows"] * c["lr"], tag + " relation rows")
        _collect(res, eng, "end", None)
        return res
    _contract(run, ["kge_step_fused_known"])


@pytest.mark.parametrize("c", W.SAMPLING_CASES, ids=lambda c: c["id"])
def test_step_fused_sampling(c):
    """two groups of three jobs (the second crosses the epoch boundary) on the steps' launches; the tail scratch at exactly
    kge_sampler_tail_scratch_bytes between guards, filled before a group's first job.  Baseline as in
    test_sampler_tail_on_the_step_launches_builds_the_same_batches / test_sampler_tail_64bit_keys (test_gpu_sampler.py): every array
    of every slot and the device state equal, bit for bit, what the stand-alone sampler launch builds from the same state"""
    from dglke_amd.dataloader import DeviceSampler
    from dglke_amd.engine import StepEngine
    n_ent, n_rel, B, N, chunk, tab = c["n_ent"], c["n_rel"], c["B"], c["N"], c["chunk"], c["table_ent"]
    rng = np.random.RandomState(11)
    n_train, G, Cn = 7 * B + 5, 3, (B // chunk) * N
    if c["skewed"]:                                          # 85 % of the edge ends in the lowest 2 % of the id range
        hot = lambda n: np.where(rng.rand(n) < 0.85, rng.randint(0, max(2, n_ent // 50), n), rng.randint(0, n_ent, n))
        h, t = hot(n_train), hot(n_train)
    else:
        h, t = rng.randint(0, n_ent, n_train), rng.randint(0, n_ent, n_train)
    r = rng.randint(0, n_rel, n_train)
    de = c["model"] == "ComplEx"

    def run(verify):
        torch.manual_seed(1)
        eng = StepEngine(c["model"], tab or n_ent, n_rel, 32, 12.0, 0.1, DEV, de, de, True, 1.0, 1e-6, 3)
        smp_a = DeviceSampler(h, r, t, n_ent, B, N, DEV, n_slots=2 * G, neg_chunk_size=chunk, seed=3)      # stand-alone launches
        smp_b = DeviceSampler(h, r, t, n_ent, B, N, DEV, n_slots=2 * G, neg_chunk_size=chunk, seed=3)      # tail jobs
        carrier = DeviceSampler(h % tab, r, t % tab, tab, B, N, DEV, n_slots=G, neg_chunk_size=chunk, seed=1) if tab else None
        smp_a.sample(G, slot0=0)
        cur = smp_b.sample(G, slot0=0)
        res, half = {}, 0
        for grp in range(2):
            if carrier is not None:
                cur = carrier.sample(G)
            smp_a.sample(G, slot0=(half ^ 1) * G)
            jobs, nxt = smp_b.tail_jobs(G, slot0=(half ^ 1) * G)
            for k in range(G):
                eng.step(cur[k], sample_job=jobs[k])
            torch.cuda.synchronize()
            for k in range(G):
                a, b = smp_a.slot_arrays((half ^ 1) * G + k), smp_b.slot_arrays((half ^ 1) * G + k)
                res["g%d b%d counts" % (grp, k)] = torch.from_numpy(np.ascontiguousarray(b["counts"]))
                if verify:
                    assert np.array_equal(a["counts"], b["counts"]), (grp, k, a["counts"], b["counts"])
                UE, UR = int(b["counts"][0]), int(b["counts"][1])
                assert 0 < UE <= 2 * B + Cn and 0 < UR <= B, (grp, k, UE, UR)
                for name, n in (("h_gid", B), ("t_gid", B), ("rel_ids", B), ("neg_ids", Cn), ("ue_id", UE), ("ur_id", UR),
                                ("ue_pos_ptr", UE + 1), ("ue_pos_adj", 2 * B), ("ue_neg_ptr", UE + 1), ("ue_neg_slot", Cn),
                                ("ur_ptr", UR + 1), ("ur_edge", B), ("ue_rec", 8 * UE), ("ur_rec", 8 * UR)):
                    res["g%d b%d %s" % (grp, k, name)] = torch.from_numpy(np.ascontiguousarray(b[name][:n]))
                    if verify:
                        assert np.array_equal(a[name][:n], b[name][:n]), "group %d batch %d: %s differs" % (grp, k, name)
            res["g%d state" % grp] = smp_b.state[:2].clone()
            if verify:
                assert torch.equal(smp_a.state[:2], smp_b.state[:2]), "device state"
            cur, half = nxt, half ^ 1
        _collect(res, eng, "end", None)
        return res
    _contract(run, ["kge_step_fused_sampling"])


@pytest.mark.parametrize("B,N", [(20, 4), (64, 16)], ids=["B20-N4", "B64-N16"])
def test_weighted_sampler_slots_to_the_byte(B, N):
    """kge_sample_batches_weighted writes B weights behind each slot's plan: n_slots slots of exactly
    kge_sampler_slot_bytes_weighted bytes between two 4096-byte guards, filled with zero bytes and with 0xFF bytes.  The guards stay;
    ids, plan, counts and the state are the unweighted launch's; the weights are weights[e] bit for bit; the bytes between the end of
    the B weights and the end of the slot (the weights' 32-byte round-up: 16 bytes at B = 20, none at B = 64) are UNTOUCHED - they
    still hold the fill"""
    import subsampling_cases as SC
    from dglke_amd import _lib
    from dglke_amd.dataloader import DeviceSampler
    n_train, n_ent, n_slots = 163, 40, 3
    h, r, t, w = SC.unique_triples(n_train, n_ent)
    weight_of = dict(zip(zip(h.tolist(), r.tolist(), t.tolist()), w.tolist()))
    L = _lib.lib()
    plain = DeviceSampler(h, r, t, n_ent, B, N, DEV, n_slots=n_slots, seed=3)
    plain.sample()
    torch.cuda.synchronize()
    results = []
    for fill in (0x00, 0xFF):
        smp = DeviceSampler(h, r, t, n_ent, B, N, DEV, n_slots=n_slots, seed=3, edge_importance=w)
        sb = int(L.kge_sampler_slot_bytes_weighted(B, smp.C, N))
        assert sb == smp.slot_bytes == plain.slot_bytes + SC.al32(4 * B)
        buf = torch.full((2 * W.GUARD + n_slots * sb,), fill, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 256 == 0
        _lib.check(L.kge_sample_batches_weighted(_lib.ptr(smp.H), _lib.ptr(smp.R), _lib.ptr(smp.T), _lib.ptr(smp.perm) if smp.perm is not None else None,
                                                 _lib.ptr(smp.W), smp.n_train, n_ent, B, smp.C, smp.chunk, N, smp.seed, _lib.ptr(smp.state),
                                                 buf.data_ptr() + W.GUARD, sb, n_slots, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((buf[:W.GUARD] == fill).all()) and bool((buf[W.GUARD + n_slots * sb:] == fill).all()), "fill 0x%02X: a guard was written" % fill
        assert torch.equal(smp.state, plain.state), "device state"
        smp.slots.copy_(buf[W.GUARD:W.GUARD + n_slots * sb])
        slots = []
        for k in range(n_slots):
            a, b = plain.slot_arrays(k), smp.slot_arrays(k)
            UE, UR = int(a["counts"][0]), int(a["counts"][1])
            CN = smp.C * N
            for name, n in (("h_gid", B), ("t_gid", B), ("rel_ids", B), ("neg_ids", CN), ("ue_id", UE), ("ur_id", UR), ("ue_pos_ptr", UE + 1),
                            ("ue_pos_adj", 2 * B), ("ue_neg_ptr", UE + 1), ("ue_neg_slot", CN), ("ur_ptr", UR + 1), ("ur_edge", B),
                            ("ue_rec", 8 * UE), ("ur_rec", 8 * UR), ("counts", 4)):
                assert np.array_equal(a[name][:n], b[name][:n]), "fill 0x%02X slot %d: %s differs from the unweighted launch's" % (fill, k, name)
            want = np.array([weight_of[x] for x in zip(b["h_gid"].tolist(), b["rel_ids"].tolist(), b["t_gid"].tolist())], np.float32)
            assert np.array_equal(b["edge_w"].view(np.int32), want.view(np.int32)), "fill 0x%02X slot %d: edge_w" % (fill, k)
            tail = buf[W.GUARD + k * sb + plain.slot_bytes + 4 * B:W.GUARD + (k + 1) * sb]
            assert tail.numel() == SC.al32(4 * B) - 4 * B and bool((tail == fill).all()), "fill 0x%02X slot %d: bytes behind the weights written" % (fill, k)
            slots.append({n_: b[n_][:m] for n_, m in (("h_gid", B), ("neg_ids", CN), ("ue_id", UE), ("edge_w", B))})
        results.append(slots)
    for k in range(n_slots):
        for name in results[0][k]:
            assert np.array_equal(results[0][k][name], results[1][k][name]), (k, name)


def _grads_cases():
    """cases of emit_message_cases.py (host-planned), one per update instance family, in the two-trace (dense) and the packed
    layout; the relation-matrix models apply their relation trace in place (dense_rel_inplace)"""
    import emit_message_cases as E
    out = []
    for prefix, lays in (("TransE_l2-D16-nh0", ("dense", "packed")), ("TransE_l2-D16-nd-", ("dense", "packed")),
                         ("DistMult-D16-nh1", ("dense", "packed")), ("RotatE-D16-", ("dense", "packed")), ("TransE_l2-D30-", ("dense",)),
                         ("TransR-D32-", ("dense_rel_inplace",)), ("RESCAL-D16-", ("dense_rel_inplace",))):
        hit = [c for c in E.CASES if c["id"].startswith(prefix) and not c["device_plan"]]
        assert len(hit) == 1, (prefix, [c["id"] for c in hit])
        assert all(lay in E.layouts_of(hit[0]) for lay in lays) and ("packed" not in lays or E.packed_supported(hit[0])), prefix
        out += [pytest.param(hit[0], lay, id="%s-%s" % (hit[0]["id"], lay)) for lay in lays]
    return out


@pytest.mark.parametrize("c,lay", _grads_cases())
def test_step_grads(c, lay):
    """kge_step_grads with two-trace and packed messages.  Case, float64 statement, bounds and the reading of the layouts (every
    word a layout does not name still the sentinel): emit_message_cases.py / test_messages_match_the_float64_statement"""
    import emit_message_cases as E
    from dglke_amd import plan
    from test_gpu_emit_messages import _check, _layout, _read
    from test_gpu_loss_options import _engine as emit_engine
    bt = E.host_ids(c)
    b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV, bt["w"])
    ent, rel, proj = E.tables(c)
    ref = E.messages(c, ent, rel, proj, bt)
    excl = E.exclusions(c, ent, rel, bt)
    Np = c["N"] + (c["chunk"] if c["neg_deg"] else 0)
    tag = "%s %s" % (c["id"], lay)

    def run(verify):
        eng = emit_engine(c, c["flags"])
        em, bufs, route = _layout(c, lay, b, ref)
        want = dict(pos_score=torch.full((c["B"],), SENT, device=DEV), neg_score=torch.full((b.C, c["chunk"], Np), SENT, device=DEV))
        eng.step(b, want, emit=em)
        torch.cuda.synchronize()
        if verify:
            got = _read(c, lay, b, ref, bufs, route, tag)
            assert all(np.isfinite(v).all() for v in got.values()), tag + ": non-finite message"
            _check(E.message_errors(got, ref, excl), tag)
        res = {k: v.clone() for k, v in bufs.items()}
        res.update(pos_score=want["pos_score"].clone(), neg_score=want["neg_score"].clone())
        _collect(res, eng, "end", None)
        return res
    _contract(run, ["kge_step_grads"])


def test_step_refuses_a_workspace_one_byte_short():
    """fused, phase and async: KGE_ERR_WORKSPACE, the 0xFF-filled buffer, the sentinel-filled outputs and the tables untouched"""
    from dglke_amd import _lib, plan
    c = W.STEP_CASES[1]
    bt = W.step_batches(c, 1)[0]
    p = _probe()
    for entry in ("fused", "phase", "async"):
        eng = _engine(c)
        b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV)
        want = _outputs(eng, b, c)
        before = _tables64(eng)
        with _installed(p, 0xFF, short=True):
            with pytest.raises(_lib.KgeError, match="workspace too small"):
                eng.step(b, want) if entry == "fused" else _phase_step(eng, b, want) if entry == "phase" else eng.step_async(b, want)
        torch.cuda.synchronize()
        assert all(bool((t == SENT).all()) for t in want.values()), entry
        assert all(np.array_equal(x, y) for x, y in zip(before, _tables64(eng))), entry


def _refusal_cases():
    out = [(e, m) for e in ("kge_step_async", "kge_step_grads", "kge_step_sharded", "kge_rank_eval_split") for m in W.NEW_MODELS]
    return out + [(e, m) for e in ("kge_step_fused_sampling", "kge_rank_rel_eval") for m in ("PairRE", "TransH")]


@pytest.mark.parametrize("entry,model", _refusal_cases(), ids=["%s-%s" % x for x in _refusal_cases()])
def test_entries_refuse_the_models_they_do_not_serve(entry, model):
    """KGE_ERR_ARG before any launch: every byte of the 0xFF-filled guarded region - the workspace body included - still the fill,
    every sentinel-filled output still the sentinel, the tables unmoved (the proxy asserts the status and the region)"""
    from dglke_amd import _lib
    c = W.MODEL_KNOWN_CASES[model]
    T = _model_test(model)
    eng = _model_engine(c)
    bt = W.model_batches(c, 1)[0]
    b = T._batch(c, bt)
    want = _outputs(eng, b, c)
    eng.loss4.fill_(SENT)
    out = _lib.KgeStepOut()
    out.loss4, out.loss_accum, out.tickets = _lib.ptr(eng.loss4), _lib.ptr(eng.loss_accum), _lib.ptr(eng.tickets)
    for k, t in want.items():
        setattr(out, k, _lib.ptr(t))
    UE, d_e, d_r = b.UE, c["d_e"], W.model_d_r(model, c["d_e"])
    bufs = [torch.full((UE, d_e), SENT, device=DEV), torch.full((UE,), SENT, device=DEV), torch.full((UE, d_e), SENT, device=DEV),
            torch.full((UE,), SENT, device=DEV)]
    ranks, pos = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV), torch.full((4,), SENT, device=DEV)
    scratch = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=DEV)
    before = [x.clone() for x in (eng.ent, eng.ent_state, eng.rel, eng.rel_state, eng.loss_accum, eng.tickets)]
    h, r, t = (_dev(bt[k][:4]) for k in ("h", "r", "t"))
    mid, gamma = _lib.model_id(model), W.model_gamma(model)
    p = _probe()
    n0 = len(p.calls)
    with _installed(p, 0xFF, refuse=True):
        L = _lib.lib()
        if entry == "kge_step_async":
            with pytest.raises(_lib.KgeError, match="kge_step_async.*" + model):
                eng.step_async(b, want)
        elif entry == "kge_step_grads":
            em = _lib.KgeEmit()
            em.g0, em.gs0, em.g1, em.gs1 = (x.data_ptr() for x in bufs)
            with pytest.raises(_lib.KgeError, match="kge_step_grads.*" + model):
                eng.step(b, want, emit=em)
        elif entry == "kge_step_sharded":
            rc = L.kge_step_sharded(C.byref(eng.hp), C.byref(_lib.KgeShards()), C.byref(b.c), C.byref(out), 0, 0, _lib.stream_ptr())
        elif entry == "kge_step_fused_sampling":
            job = _lib.KgeSamplerJob()
            ids = torch.zeros(64, dtype=torch.int64, device=DEV)
            job.heads = job.rels = job.tails = _lib.ptr(ids)
            job.state = job.slot = _lib.ptr(scratch)
            job.n_train, job.n_ent, job.B, job.C, job.chunk, job.N = 64, c["n_ent"], c["B"], c["B"] // c["chunk"], c["chunk"], c["N"]
            rc = L.kge_step_fused_sampling(C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), 0, 0, C.byref(job), _lib.stream_ptr())
        elif entry == "kge_rank_eval_split":
            rc = L.kge_rank_eval_split(mid, 0, _lib.ptr(eng.ent), c["n_ent"], _lib.ptr(eng.ent), c["n_ent"], _lib.ptr(eng.rel), c["n_rel"], None,
                                       _lib.ptr(h), _lib.ptr(r), _lib.ptr(t), 4, d_e, d_r, gamma, 1.0, None, c["n_ent"], None, None, 4,
                                       _lib.ptr(ranks), _lib.ptr(pos), 0, 0, 0, _lib.stream_ptr())
        else:
            frng = torch.tensor([[0, 1]] * 4, dtype=torch.int64, device=DEV)
            fids = torch.zeros(1, dtype=torch.int64, device=DEV)
            rc = L.kge_rank_rel_eval(mid, _lib.ptr(eng.ent), c["n_ent"], _lib.ptr(eng.rel), c["n_rel"], None, _lib.ptr(h), _lib.ptr(r), _lib.ptr(t),
                                     4, d_e, d_r, gamma, 1.0, _lib.ptr(frng), _lib.ptr(fids), 4, _lib.ptr(ranks), _lib.ptr(pos), 0, 0, 0,
                                     _lib.stream_ptr())
        msg = L.kge_last_error().decode()
    torch.cuda.synchronize()
    assert [x[0] for x in p.calls[n0:]] == [entry], p.calls[n0:]
    assert entry in msg and model in msg, msg
    assert all(bool((x == SENT).all()) for x in list(want.values()) + bufs + [eng.loss4, pos]), "a refused call wrote an output"
    assert bool((ranks == 0x5A5A5A5A).all()) and bool((scratch == 0x5A).all())
    for x, y in zip(before, (eng.ent, eng.ent_state, eng.rel, eng.rel_state, eng.loss_accum, eng.tickets)):
        assert torch.equal(x, y), "a refused call moved a table"


# --------------------------------------------------------------------------------------------------------------------------
# the modular ops
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.NEG_CASES, ids=lambda c: c["id"])
def test_score_neg_fwd_bwd(c):
    """through dglke_amd.ops like test_gpu_modular_ops.py, its float64 reference, exclusions and bounds"""
    from test_gpu_modular_ops import _run_neg

    def run(verify):
        res = {}
        for neg_head in (False, True):
            inp = M.neg_inputs(c, neg_head)
            got = _run_neg(c, inp, neg_head)
            if verify:
                slots, edges = M.neg_exclusions(c, neg_head, inp)
                M.check_neg_caps(c, slots, edges, c["id"])
                errs = M.neg_errors(c, got, M.oracle_neg(c, neg_head, inp), slots, edges)
                for k, (ratio, err, bound) in errs.items():
                    assert ratio <= 1.0, "%s neg_head=%d %s: error %.3e, bound %.3e" % (c["id"], neg_head, k, err, bound)
            res.update({"%s %d" % (k, neg_head): torch.from_numpy(v) for k, v in got.items()})
        return res
    _contract(run, ["kge_score_neg_fwd", "kge_score_neg_bwd"])


@pytest.mark.parametrize("config", [("Logsigmoid", True, 1.0, False, 1.0, True), ("Hinge", False, 1.0, True, 2.0, False),
                                    ("BCE", False, 1.0, False, 1.0, False), ("Softmax", False, 1.0, False, 1.0, True)],
                         ids=lambda k: "%s-adv%d-pw%d" % (k[0], k[1], k[3]))
def test_loss_fwd_bwd(config):
    """B = 37; scores, oracle call and tolerances of test_gpu_loss_entry.py (its _entry passes a roomier buffer: replaced here)"""
    from test_gpu_loss_entry import _entry, _scores
    genre, adv, T, pairwise, margin, weighted = config
    rng = np.random.RandomState(3)
    pos, neg = _scores(rng, W.LOSS_B, W.LOSS_N, margin)
    w = rng.uniform(0.5, 1.5, size=W.LOSS_B).astype(np.float32) if weighted else None

    def run(verify):
        loss3, dpos, dneg = _entry(pos, neg, w, genre, adv, T, pairwise, margin)
        if verify:
            with _softmax_oracle():          # (Softmax: the statement and tolerances of test_loss_op_matches_float64, test_gpu_softmax_loss.py)
                (pl, nl, loss), dp64, dn64 = O.loss_fwd_bwd(pos.astype(np.float64), neg.astype(np.float64),
                                                            None if w is None else w.astype(np.float64), genre, adv, T, pairwise, margin)
            if genre == "Softmax":
                assert np.isnan(loss3[0]) and np.isnan(loss3[1])
                _close(loss3[2], loss, 1e-4, 1e-5, "loss")
            elif pairwise:
                assert np.isnan(loss3[0]) and np.isnan(loss3[1])
                _close(loss3[2], loss, 1e-4, 1e-5, "loss")
                flip = ((np.float32(margin) - (pos[:, None] - neg)) >= 0) != ((margin - (pos.astype(np.float64)[:, None] - neg.astype(np.float64))) >= 0)
                assert not flip.any()
            else:
                _close(loss3, [pl, nl, loss], 1e-4, 1e-5, "loss3")
            _close(dpos, dp64, 3e-4, grad_tol(dp64), "dpos")
            _close(dneg, dn64, 3e-4, grad_tol(dn64), "dneg")
        return dict(loss3=torch.from_numpy(loss3), dpos=torch.from_numpy(dpos), dneg=torch.from_numpy(dneg))
    _contract(run, ["kge_loss_fwd_bwd"])


@pytest.mark.parametrize("p", [1, 2, 3])
def test_pnorm_pow(p):
    """value bound of test_pnorm_pow_value_and_gradient (test_gpu_modular_ops.py): n * dim * 2^-24 * sum |x|^p"""
    from dglke_amd import ops

    def run(verify):
        res = {}
        for n, dim in W.PNORM_SHAPES:
            x = M.pnorm_input(n, dim)
            y = ops.pnorm_pow(_dev(x), p)
            if verify:
                val, _ = M.pnorm_ref(x, p)
                assert abs(y.item() - val) <= x.size * 2.0 ** -24 * val, (n, dim, y.item(), val)
            res["n%d dim%d" % (n, dim)] = y.detach().clone().reshape(1)
        return res
    _contract(run, ["kge_pnorm_pow"])


@pytest.mark.parametrize("c", W.MODEL_NEG_CASES, ids=lambda c: c["id"])
def test_score_neg_fwd_bwd_of_quate_pairre_transh(c):
    """through dglke_amd.ops on the models' own op inputs, both corruption sides; float64 reference, bounds and (PairRE) the rows
    its sign-ambiguity rule takes out under its cap: quate_cases / pairre_cases / transh_cases op_reference, as in their
    test_per_op_entries_match_float64"""
    from dglke_amd import ops
    Q, T = W.model_cases(c["model"]), _model_test(c["model"])
    C_, chunk, N = c["shape"]
    gamma = W.model_gamma(c["model"])

    def run(verify):
        res = {}
        for neg_head in (False, True):
            inp = Q.op_inputs(c["d_e"], C_, chunk, N, neg_head)
            x, r, nb = (_dev(inp[k]).requires_grad_() for k in ("x", "r", "nb"))
            kw = dict(flags=c["flags"]) if c["flags"] else {}
            s = ops.score_neg(c["model"], neg_head, x, r, nb, C_, chunk, N, gamma, emb_init=1.0, **kw)
            (s * _dev(inp["W"])).sum().backward()
            torch.cuda.synchronize()
            got = dict(score=s.detach().cpu().numpy(), gx=x.grad.cpu().numpy(), gr=r.grad.cpu().numpy(), gn=nb.grad.cpu().numpy())
            if verify:
                tag = "%s neg_head=%d" % (c["id"], neg_head)
                assert all(np.isfinite(v).all() for v in got.values()), tag + ": non-finite output"
                ref = Q.op_reference(inp, C_, chunk, N, neg_head)
                if c["model"] == "TransH":
                    assert ref["share"] >= Q.DIST_SHARE, tag
                errs = {}
                for k in got:
                    bound = Q.score_bound(ref[k]) if k == "score" else Q.grad_bound(ref[k])
                    if c["model"] == "PairRE" and k in Q.OP_ROWS:
                        keep = ~ref[Q.OP_ROWS[k]]
                        assert keep.mean() >= 1 - Q.ROW_CAP and keep.any(), tag
                        errs[k] = Q.worst(got[k][keep], ref[k][keep], bound[keep])
                    else:
                        errs[k] = Q.worst(got[k], ref[k], bound)
                T._check(errs, tag)
            res.update({"%s %d" % (k, neg_head): torch.from_numpy(v) for k, v in got.items()})
        return res
    _contract(run, ["kge_score_neg_fwd", "kge_score_neg_bwd"], transh=_not_transh(c))


def test_modular_ops_refuse_a_workspace_one_byte_short():
    from dglke_amd import _lib, ops
    from test_gpu_loss_entry import _entry, _scores
    from test_gpu_modular_ops import _run_neg
    p = _probe()
    c = W.NEG_CASES[4]
    with _installed(p, 0xFF, short=True):
        with pytest.raises(_lib.KgeError, match="workspace too small"):
            _run_neg(c, M.neg_inputs(c, False), False)
        pos, neg = _scores(np.random.RandomState(3), W.LOSS_B, W.LOSS_N, 1.0)
        with pytest.raises(_lib.KgeError, match="workspace too small"):
            _entry(pos, neg, None, "Logsigmoid", False, 1.0, False, 1.0)
        with pytest.raises(_lib.KgeError, match="workspace too small"):
            ops.pnorm_pow(_dev(M.pnorm_input(37, 30)), 2)


# --------------------------------------------------------------------------------------------------------------------------
# ranking
# --------------------------------------------------------------------------------------------------------------------------
def _cc_ranker(c, batch=1024):
    from dglke_amd import eval as kev
    k = CC.inputs(c["model"], c["hidden"])
    return k, kev.Ranker(c["model"], _dev(k.ent), _dev(k.rel), k.gamma, k.emb_init, batch=batch, proj=_dev(k.proj) if k.proj is not None else None)


def _column_lists(cand, filt):
    """kge_rank_eval's lists hold candidate COLUMNS: the positions in `cand` of the entities of an entity-id list pair"""
    frng, fids = filt
    cols = [np.nonzero(np.isin(cand, fids[a:b]))[0] for a, b in frng]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in cols])]).astype(np.int64)
    return np.stack([ptr[:-1], ptr[1:]], 1), np.concatenate(cols).astype(np.int64)


def _in_band(got, lo, hi, free, what):
    assert np.all((lo <= got) & (got <= hi)), (what, np.nonzero((got < lo) | (got > hi))[0][:8], lo[:8], got[:8], hi[:8])
    exact = (lo == hi) & (free == 0)
    assert np.array_equal(got[exact], lo[exact]), what


@pytest.mark.parametrize("c", W.RANK_CASES, ids=lambda c: c["id"])
def test_rank_eval_ex(c):
    """Ranker.ranks with Eb = 32 over 90 triples (three passes over the same buffers), both sides; the bounds are
    chunked_eval_cases.expected with one list shared by all triples (the oracle's fp64 score matrix at the candidates' columns)"""
    k, rk = _cc_ranker(c, batch=W.RANK_EB)
    cand = np.random.RandomState(c["n_cand"]).choice(CC.N_ENT, c["n_cand"], replace=False).astype(np.int64)

    def run(verify):
        res = {}
        for neg_head in (False, True):
            filt = _column_lists(cand, CC.filter_lists(c["model"], c["hidden"], neg_head)) if c["filt"] else None
            ranks, pos = rk.ranks(k.h, k.r, k.t, neg_head, filt, cand=cand, want_pos_score=True)
            if verify:
                lo, hi, free, p = CC.expected(c["model"], c["hidden"], neg_head, CC.E, cand[None, :], filtered=c["filt"])
                _in_band(ranks.cpu().numpy(), lo, hi, free, (c["id"], neg_head))
                assert np.abs(pos.cpu().numpy() - p).max() <= 1e-4
            res["ranks %d" % neg_head], res["pos %d" % neg_head] = ranks.clone(), pos.clone()
        return res
    _contract(run, ["kge_rank_eval_ex"])


def test_rank_eval_split_and_plain():
    """kge_rank_eval_split with the candidates in a second table, kge_rank_eval on every entity: ranks equal to kge_rank_eval_ex's"""
    from dglke_amd import _lib
    c = W.RANK_CASES[0]
    k, rk = _cc_ranker(c, batch=W.RANK_EB)
    ent, rel = rk.ent, rk.rel
    h, r, t = (_dev(x) for x in (k.h, k.r, k.t))
    lo_hi = CC.expected(c["model"], c["hidden"], False, CC.E, None)

    def run(verify):
        res = {}
        for name in ("kge_rank_eval", "kge_rank_eval_split"):
            ranks = torch.zeros(CC.E, dtype=torch.int32, device=DEV)
            head = (rk.model, 0, _lib.ptr(ent), CC.N_ENT) + ((_lib.ptr(ent), CC.N_ENT) if name.endswith("split") else ())
            mid = (_lib.ptr(rel), CC.N_REL) + ((None,) if name.endswith("split") else ())
            _lib.check(getattr(_lib.lib(), name)(*(head + mid + (_lib.ptr(h), _lib.ptr(r), _lib.ptr(t), CC.E, ent.shape[1], rel.shape[1], k.gamma,
                                                                   k.emb_init, None, CC.N_ENT, None, None, W.RANK_EB, _lib.ptr(ranks), None, 0, 0, 0,
                                                                   _lib.stream_ptr()))))
            if verify:
                _in_band(ranks.cpu().numpy(), lo_hi[0], lo_hi[1], lo_hi[2], name)
            res[name] = ranks
        return res
    _contract(run, ["kge_rank_eval", "kge_rank_eval_split"])


@pytest.mark.parametrize("c", W.CHUNKED_CASES, ids=lambda c: c["id"])
def test_rank_eval_chunked(c):
    """the workspace of ONE chunk: the entry walks its blocks over it (Ranker.chunked_ranks would ask for all chunks at once -
    the proxy hands over kge_rank_chunked_workspace_bytes(model, chunk, chunk, ...)).  Bounds: chunked_eval_cases.expected"""
    k, rk = _cc_ranker(c)
    cand = CC.candidates(c["chunk"], c["n_cand"])
    self_cand = c["kind"] == "self"

    def run(verify):
        res = {}
        for neg_head in (False, True):
            for filtered in ((False,) if self_cand else (False, True)):
                filt = CC.filter_lists(c["model"], c["hidden"], neg_head) if filtered else None
                got, pos = rk.chunked_ranks(k.h, k.r, k.t, neg_head, c["chunk"], cand=cand, filt=filt, self_cand=self_cand, want_pos_score=True)
                if verify:
                    lo, hi, free, p = CC.expected(c["model"], c["hidden"], neg_head, c["chunk"], cand, filtered=filtered, self_cand=self_cand)
                    _in_band(got.cpu().numpy(), lo, hi, free, (c["id"], neg_head, filtered))
                    assert np.abs(pos.cpu().numpy() - p).max() <= 1e-4
                res["ranks %d %d" % (neg_head, filtered)], res["pos %d %d" % (neg_head, filtered)] = got.clone(), pos.clone()
        return res
    _contract(run, ["kge_rank_eval_chunked"])


@pytest.mark.parametrize("c", W.REL_CASES, ids=lambda c: c["id"])
def test_rank_rel_eval(c):
    """Ranker.relation_ranks with Eb = 64 over 90 triples; inputs, bounds and tolerance: relation_rank_cases.py"""
    from dglke_amd import eval as kev
    k = RC.inputs(c["model"], c["hidden"], c["de"], c["n_rel"])
    rk = kev.Ranker(c["model"], _dev(np.array(k.ent)), _dev(np.array(k.rel)), k.gamma, k.emb_init, batch=W.REL_EB,
                    proj=_dev(np.array(k.proj)) if k.proj is not None else None)

    def run(verify):
        res = {}
        for filtered in (False, True):
            rng, ids = RC.relation_lists(c["n_rel"], filtered)
            got, pos = rk.relation_ranks(k.h, k.r, k.t, (_dev(np.array(rng)), _dev(np.array(ids))), want_pos_score=True)
            if verify:
                lo, hi, p = RC.expected(c["model"], c["hidden"], c["de"], c["n_rel"], filtered)
                g = got.cpu().numpy().astype(np.int64)
                assert np.all((lo <= g) & (g <= hi)) and np.array_equal(g[lo == hi], lo[lo == hi]), (c["id"], filtered)
                assert np.abs(pos.cpu().numpy() - p).max() <= RC.TOL
            res["ranks %d" % filtered], res["pos %d" % filtered] = got.clone(), pos.clone()
        return res
    _contract(run, ["kge_rank_rel_eval"])


# ---- QuatE, PairRE, TransH on their integer-grid tables (W.model_tie_inputs: 300 entities = relations = candidates, 90 test
# triples; float32 scores are exact there, so the baseline is EQUALITY with the float64 ranks and order, as in the models'
# test_ranking_entries_equal_float64_on_integer_grid_tables) ----
def _tie_ranker(c, batch):
    from dglke_amd import eval as kev
    Q = W.model_cases(c["model"])
    k = W.model_tie_inputs(c["model"], c["d_e"])
    gamma = 0.0 if c["model"] == "QuatE" else Q.TIE_GAMMA
    return Q, k, kev.Ranker(c["model"], _dev(np.array(k.ent)), _dev(np.array(k.rel)), gamma, 1.0, batch=batch), gamma


def _dev_lists(lists):
    return None if lists is None else (_dev(np.array(lists[0])), _dev(np.array(lists[1])))


@pytest.mark.parametrize("c", W.MODEL_RANK_CASES, ids=lambda c: c["id"])
def test_rank_eval_ex_of_quate_pairre_transh(c):
    """Ranker.ranks against every entity with Eb = 32 over 90 triples (32 + 32 + 26: the buffers are reused, the last batch is
    partial), both sides.  TransH keeps w^ . a and w^ in entries that kge_rank_workspace_bytes sizes for other models' use"""
    Q, k, rk, _ = _tie_ranker(c, W.RANK_EB)
    T = _model_test(c["model"])

    def run(verify):
        res = {}
        for neg_head in (False, True):
            lists = Q.filter_lists(k, neg_head) if c["filt"] else None
            got, pos = rk.ranks(k.h, k.r, k.t, neg_head, filt=_dev_lists(lists), want_pos_score=True)
            if verify:
                p, S = Q.tie_scores(k, k.h, k.r, k.t, neg_head)
                T._same(got.cpu().numpy(), Q.ranks_of(p, S, lists), "%s neg_head=%d" % (c["id"], neg_head))
                assert np.array_equal(pos.cpu().numpy(), Q.tie_scores(k, k.h, k.r, k.t, neg_head, np.float32)[0]), c["id"] + ": positive scores"
            res["ranks %d" % neg_head], res["pos %d" % neg_head] = got.clone(), pos.clone()
        return res
    _contract(run, ["kge_rank_eval_ex"], transh=_not_transh(c))


@pytest.mark.parametrize("c", W.MODEL_CHUNKED_CASES, ids=lambda c: c["id"])
def test_rank_eval_chunked_of_quate_pairre_transh(c):
    """every kind of W.CHUNKED_CASES on ONE chunk's workspace.  all: every entity, raw and filtered; lists / lists1: per-chunk lists
    with empty slots; self: the chunk's own corrupted-side entities prepended.  Expected ranks: ranks_of / chunked_ranks_of of
    pairre_cases.py (model-independent: they count in the model's float64 score matrix), the latter at this case's chunk"""
    import pairre_cases as PR
    Q, k, rk, _ = _tie_ranker(c, 1024)
    T = _model_test(c["model"])
    cand = W.chunk_candidates(c["kind"], c["chunk"], c["n_cand"])
    self_cand = c["kind"] == "self"

    def expected(p, S, neg_head, lists):
        if cand is None and not self_cand:
            return Q.ranks_of(p, S, lists)
        saved, PR.TIE_CHUNK = PR.TIE_CHUNK, c["chunk"]
        try:
            return PR.chunked_ranks_of(k, p, S, neg_head, cand, self_cand)
        finally:
            PR.TIE_CHUNK = saved

    def run(verify):
        res = {}
        for neg_head in (False, True):
            for filtered in ((False, True) if c["kind"] == "all" else (False,)):
                lists = Q.filter_lists(k, neg_head) if filtered else None
                got, pos = rk.chunked_ranks(k.h, k.r, k.t, neg_head, c["chunk"], cand=None if cand is None else _dev(cand),
                                            filt=_dev_lists(lists), self_cand=self_cand, want_pos_score=True)
                if verify:
                    p, S = Q.tie_scores(k, k.h, k.r, k.t, neg_head)
                    T._same(got.cpu().numpy(), expected(p, S, neg_head, lists), "%s neg_head=%d filtered=%d" % (c["id"], neg_head, filtered))
                    assert np.array_equal(pos.cpu().numpy(), Q.tie_scores(k, k.h, k.r, k.t, neg_head, np.float32)[0]), c["id"] + ": positive scores"
                res["ranks %d %d" % (neg_head, filtered)], res["pos %d %d" % (neg_head, filtered)] = got.clone(), pos.clone()
        return res
    _contract(run, ["kge_rank_eval_chunked"], transh=_not_transh(c))


@pytest.mark.parametrize("c", W.MODEL_REL_CASES, ids=lambda c: c["id"])
def test_rank_rel_eval_of_quate(c):
    """Ranker.relation_ranks with Eb = 32 over 90 triples against 300 relations, raw and filtered: RN, the relation table
    normalised per quaternion, stands behind the DistMult layout"""
    Q, k, rk, _ = _tie_ranker(c, W.RANK_EB)
    T = _model_test(c["model"])

    def run(verify):
        res = {}
        for filtered in (False, True):
            lists = Q.relation_lists(k, filtered)
            got, pos = rk.relation_ranks(k.h, k.r, k.t, _dev_lists(lists), want_pos_score=True)
            if verify:
                p, S = Q.rel_tie_scores(k, k.h, k.r, k.t)
                T._same(got.cpu().numpy(), Q.ranks_of(p, S, lists), "%s filtered=%d" % (c["id"], filtered))
                assert np.array_equal(pos.cpu().numpy(), p.astype(np.float32)), c["id"] + ": positive scores"
            res["ranks %d" % filtered], res["pos %d" % filtered] = got.clone(), pos.clone()
        return res
    _contract(run, ["kge_rank_rel_eval"], transh=_not_transh(c))


@pytest.mark.parametrize("filtered", [False, True], ids=["select", "filtered"])
@pytest.mark.parametrize("c", W.MODEL_TOPK_CASES, ids=lambda c: c["id"])
def test_topk_select_of_quate_pairre_transh(c, filtered):
    """kge_topk_select / _filtered called as in the models' integer-grid tests: 90 query rows against all 300 entities, both sides;
    equal scores come back in candidate order, listed entities never.  g9: groups of nine rows whose lists merge into one (the
    expected order: the group's rows concatenated, earlier rows first among equal scores)"""
    from dglke_amd import _lib
    Q, k, _, gamma = _tie_ranker(c, 1024)
    n, E, K, g, d_e = W.TIE_N, W.TIE_E, c["K"], c["group"], c["d_e"]
    ent, rel = _dev(np.array(k.ent)), _dev(np.array(k.rel))
    h, r, t, cd = _dev(np.array(k.h)), _dev(np.array(k.r)), _dev(np.array(k.t)), torch.arange(n, dtype=torch.int64, device=DEV)
    mid = _lib.model_id(c["model"])
    ws = torch.empty(_lib.topk_workspace_bytes(mid, E, n, d_e, K), dtype=torch.uint8, device=DEV)     # (the proxy hands over its own)

    def run(verify):
        res = {}
        for side in (0, 1):
            res_s = torch.zeros(E // g, K, dtype=torch.float32, device=DEV)
            res_o = torch.full((E // g, K), -1, dtype=torch.int64, device=DEV)         # (-1 = empty: the running result of the group)
            base = torch.arange(E, dtype=torch.int64, device=DEV) % g * n          # (position = row_base + column: unique inside a group)
            a = (mid, side, _lib.ptr(ent), n, _lib.ptr(rel), n, _lib.ptr(h), _lib.ptr(r), _lib.ptr(t), E, d_e, W.model_d_r(c["model"], d_e),
                 gamma, 1.0, _lib.ptr(cd), n, _lib.ptr(base), 1, g, K, _lib.ptr(res_s), _lib.ptr(res_o), _lib.ptr(ws), ws.numel())
            frng, fids = Q.filter_lists(k, bool(side))
            if filtered:
                fr, fi = _dev(np.array(frng).reshape(-1)), _dev(np.array(fids))
                _lib.check(_lib.lib().kge_topk_select_filtered(*a, _lib.ptr(fr), _lib.ptr(fi), _lib.stream_ptr()))
            else:
                _lib.check(_lib.lib().kge_topk_select(*a, _lib.stream_ptr()))
            torch.cuda.synchronize()
            if verify:
                _, S = Q.tie_scores(k, k.h, k.r, k.t, bool(side))
                S32 = Q.tie_scores(k, k.h, k.r, k.t, bool(side), np.float32)[1]
                go, gs = res_o.cpu().numpy(), res_s.cpu().numpy()
                for q in range(E // g):
                    keep = np.ones((g, n), bool)
                    if filtered:
                        for j in range(g):
                            keep[j, fids[frng[q * g + j, 0]:frng[q * g + j, 1]]] = False
                    pos_ = np.nonzero(keep.reshape(-1))[0]
                    order = pos_[np.argsort(-S[q * g:(q + 1) * g].reshape(-1)[pos_], kind="stable")][:K]
                    what = "%s %s side=%d group %d" % (c["id"], "filtered" if filtered else "select", side, q)
                    assert np.array_equal(go[q, :len(order)], order) and np.all(go[q, len(order):] == -1), what + ": order"
                    assert np.array_equal(gs[q, :len(order)], S32[q * g:(q + 1) * g].reshape(-1)[order]), what + ": scores"
            res["o %d" % side], res["s %d" % side] = res_o.clone(), res_s.clone()
        return res
    _contract(run, ["kge_topk_select_filtered" if filtered else "kge_topk_select"], transh=_not_transh(c))


def test_ranking_refuses_a_workspace_one_byte_short():
    from dglke_amd import _lib
    p = _probe()
    k, rk = _cc_ranker(W.RANK_CASES[0], batch=W.RANK_EB)
    rc = W.REL_CASES[0]
    kr = RC.inputs(rc["model"], rc["hidden"], rc["de"], rc["n_rel"])
    from dglke_amd import eval as kev
    rr = kev.Ranker(rc["model"], _dev(np.array(kr.ent)), _dev(np.array(kr.rel)), kr.gamma, kr.emb_init, batch=W.REL_EB)
    rng, ids = RC.relation_lists(rc["n_rel"], False)
    with _installed(p, 0xFF, short=True):
        with pytest.raises(_lib.KgeError, match="workspace too small"):
            rk.ranks(k.h, k.r, k.t, False)
        with pytest.raises(_lib.KgeError, match="workspace too small"):
            rk.chunked_ranks(k.h, k.r, k.t, False, 8)
        with pytest.raises(_lib.KgeError, match="workspace too small"):
            rr.relation_ranks(kr.h, kr.r, kr.t, (_dev(np.array(rng)), _dev(np.array(ids))))
        # the wrappers above allocate their outputs themselves; kge_rank_eval called directly with sentinel-filled ranks (the entry
        # sets them to 1 with a memset of its own once it has accepted its arguments): still the sentinel after the refusal
        ranks = torch.full((CC.E,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        h, r, t = (_dev(x) for x in (k.h, k.r, k.t))
        rc = _lib.lib().kge_rank_eval(rk.model, 0, _lib.ptr(rk.ent), CC.N_ENT, _lib.ptr(rk.rel), CC.N_REL, _lib.ptr(h), _lib.ptr(r), _lib.ptr(t),
                                      CC.E, rk.ent.shape[1], rk.rel.shape[1], k.gamma, k.emb_init, None, CC.N_ENT, None, None, W.RANK_EB,
                                      _lib.ptr(ranks), None, 0, 0, 0, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == W.ERR_WORKSPACE and bool((ranks == 0x5A5A5A5A).all()), "a refused kge_rank_eval wrote ranks"


# --------------------------------------------------------------------------------------------------------------------------
# top-K
# --------------------------------------------------------------------------------------------------------------------------
def _topk_inputs(c):
    from test_gpu_infer import _tables
    ent, rel = _tables(c["model"], c["n_cand"], c["R"], c["hidden"], 21)
    rng = np.random.RandomState(c["K"])
    head = rng.choice(c["n_cand"], c["H"], replace=False).astype(np.int64)
    return ent, rel, head, np.arange(c["R"], dtype=np.int64)


@pytest.mark.parametrize("filtered", [False, True], ids=["select", "filtered"])
@pytest.mark.parametrize("c", W.TOPK_CASES, ids=lambda c: c["id"])
def test_topk_select(c, filtered):
    """infer.predict_topk against every entity as tail; acceptance rule and float64 scores of test_gpu_infer.py.  filtered: with a
    known-triple index (kge_topk_select_filtered) whose triples must not come back"""
    from dglke_amd import _lib, infer
    from dglke_amd.known import KnownIndex
    from test_gpu_infer import _check_result, _exact_dict, _groups, exact_scores
    ent, rel, head, rels = _topk_inputs(c)
    emb_init = 10.0 / c["hidden"]
    ent_d, rel_d = _dev(ent), _dev(rel)
    known = None
    if filtered:
        rng = np.random.RandomState(8)
        kh, kr, kt = head[rng.randint(0, c["H"], 400)], rng.randint(0, c["R"], 400), rng.randint(0, c["n_cand"], 400)
        known = KnownIndex((kh, kr, kt), c["n_cand"], c["R"], DEV)
    tails = np.arange(c["n_cand"])

    def run(verify):
        res = infer.predict_topk(_lib.model_id(c["model"]), ent_d, rel_d, 0.0, emb_init, lambda s: s, head, rels, None, c["mode"], c["K"],
                                 known=known, exclude_mode="exclude" if filtered else None)
        if verify:
            S = exact_scores(c["model"], ent, rel, head, rels, tails, 0.0, emb_init)
            if filtered:
                hp = {int(x): i for i, x in enumerate(head)}
                for a, b_, t_ in zip(kh, kr, kt):
                    S[hp[int(a)], int(b_), int(t_)] = -float("inf")
            groups = _exact_dict(S, head, rels, tails, _groups(c["mode"], c["H"], c["R"], c["n_cand"]))
            if filtered:
                groups = [{key: v for key, v in g.items() if v[0] != -float("inf")} for g in groups]
            _check_result([g[:4] for g in res], groups, c["K"])
        out = {}
        for i, g in enumerate(res):
            for j, name in enumerate(("h", "r", "t", "s")):
                out["g%d %s" % (i, name)] = torch.from_numpy(np.ascontiguousarray(g[j]))
        return out
    _contract(run, ["kge_topk_select_filtered" if filtered else "kge_topk_select"])


@pytest.mark.parametrize("order", ["shuffled", "ascending"])
@pytest.mark.parametrize("K,n", W.TOPK_VECTOR, ids=lambda v: str(v))
def test_topk_vector(K, n, order):
    """infer.vector_topk on distinct scores: exactly the K largest, in order, with their positions.  ascending: the K best are
    the last K positions - the tail of the last list of the first ping-pong half and of every merge round's output, so an entry
    a kernel leaves unwritten there is part of the result"""
    from dglke_amd import infer
    score = (np.random.RandomState(n + K).permutation(n) if order == "shuffled" else np.arange(n)).astype(np.float32) * 0.25 - 7.0
    sd = _dev(score)

    def run(verify):
        s, o = infer.vector_topk(sd, K)
        if verify:
            order = np.argsort(-score.astype(np.float64), kind="stable")[:min(K, n)]
            assert np.array_equal(o.cpu().numpy(), order) and np.array_equal(s.cpu().numpy(), score[order])
        return dict(s=s.clone(), o=o.clone())
    _contract(run, ["kge_topk_vector"])


def test_topk_refuses_a_workspace_one_byte_short():
    from dglke_amd import _lib, infer
    c = W.TOPK_CASES[1]
    ent, rel, head, rels = _topk_inputs(c)
    p = _probe()
    with _installed(p, 0xFF, short=True):
        with pytest.raises(_lib.KgeError, match="workspace too small"):
            infer.predict_topk(_lib.model_id(c["model"]), _dev(ent), _dev(rel), 0.0, 1.0, lambda s: s, head, rels, None, c["mode"], c["K"])
        with pytest.raises(_lib.KgeError, match="workspace too small"):
            infer.vector_topk(_dev(np.arange(100, dtype=np.float32)), 10)
