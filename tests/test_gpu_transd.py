"""TransD (include/kge_hip.h, enum kge_model, KGE_TRANSD = 14) on the GPU against the float64 statement of tests/transd_cases.py
(inputs guarded on the CPU by tests/test_transd_inputs.py):
  1. the per-op entries (ops.score_pos / ops.score_neg and their backward) at half-widths 4, 8, 36 (a partial k-stage), 64, 260 and
     TransH's shapes - partial tiles on each edge, none, and one whose STACKED 2 * chunk rows cross a tile boundary that chunk alone
     does not; both corruption sides; gradients into both halves of x, r and the candidates;
  2. the fused step under every loss genre, -adv, -pw, Softmax, --neg_deg_sample, edge importance and the three regulariser norms,
     both corruption sides, each from the fixed tables; the step in four phases against the fused step, bit for bit; the known-pair
     variant; two runs of two consecutive steps, bit for bit; one Adam case against adam_cases.step; tables whose mapping halves
     are all zero under -rc 0 (those halves stay exactly zero, the rest is TransE_l2);
  3. exact ranks on integer-grid tables: every ranking entry and the top-K selection must EQUAL the float64 ranks / order, at 5,
     129 and 300 entities and k = 4 (the VALU top-K instance) and 36 (the MFMA one);
  4. the interface: TransDModel.link_predict, ScoreInfer.topK, dglke_train -> dglke_eval -> dglke_predict, and a run cut by
     --checkpoint_interval and continued with --resume against the uninterrupted run, bit for bit;
  5. the entries that refuse the model.
Tolerances are the suite's: scores 1e-4 abs + 1e-4 rel; gradients and updated rows 3e-4 of the compared array's largest component
+ 3e-4 relative (tests/modular_op_cases.py).  Nothing is excluded: the inputs keep every distance away from zero (transd_cases.py).

transd_errors.txt, written next to the suite's other reports, records per op / step and quantity the largest error next to its bound."""
import contextlib
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

import adam_cases as A
import transd_cases as Q
from test_gpu_loss_options import _f64, _report_dir
from test_gpu_parity import DEV, _close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ERRORS = {}          # (op, case) -> {quantity: (err / bound, err, bound)}
T0 = time.time()


def _record(op, case, **q):
    rec = ERRORS.setdefault((op, case), {})
    for k, v in q.items():
        if k not in rec or v[0] >= rec[k][0]:
            rec[k] = v
    try:
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "transd_errors.txt"), "w") as f:
            f.write("TransD per-op entries and fused step against float64: largest |error| / bound per op, case and quantity (<= 1 passes), "
                    "that error, its bound\n(wall time of this file up to the last record: %.0f s)\n" % (time.time() - T0))
            top = max(((v[0], o, c, k) for (o, c), r in ERRORS.items() for k, v in r.items()), default=None)
            if top:
                f.write("worst: %.4f of its bound (%s %s %s)\n" % top)
            for (o, c) in sorted(ERRORS):
                f.write("%-12s %s\n" % (o, c))
                for k in sorted(ERRORS[(o, c)]):
                    f.write("    %-10s err/bound %8.4f   err %.3e   bound %.3e\n" % ((k,) + tuple(ERRORS[(o, c)][k])))
    except OSError:
        pass


def _check(errs, tag):
    for k, (ratio, err, bound) in errs.items():
        print("%s %s: err/bound %.4f (error %.3e, bound %.3e)" % (tag, k, ratio, err, bound))
    for k, (ratio, err, bound) in errs.items():
        assert ratio <= 1.0, "%s %s: %.2f bounds off (error %.3e, bound %.3e)" % (tag, k, ratio, err, bound)


def _dev(a, grad=False):
    t = torch.from_numpy(np.array(a)).to(DEV)                 # (a copy: the case tables are read-only)
    return t.requires_grad_() if grad else t


# --------------------------------------------------------------------------------------------------------------------------
# 1. the per-op entries
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", Q.OP_SHAPES, ids=["C%d-c%d-N%d" % s for s in Q.OP_SHAPES])
@pytest.mark.parametrize("k", Q.OP_WIDTHS)
def test_per_op_entries_match_float64(k, shape):
    """kge_score_pos / _bwd and kge_score_neg_fwd / _bwd, both sides, a random signed upstream gradient"""
    from dglke_amd import ops
    C_, chunk, N = shape
    for neg_head in (False, True):
        inp = Q.op_inputs(k, C_, chunk, N, neg_head)
        ref = Q.op_reference(inp, C_, chunk, N, neg_head)
        tag = "k%d C%d c%d N%d neg_head=%d" % (k, C_, chunk, N, neg_head)
        x, y, r, nb = (_dev(inp[n_], True) for n_ in ("x", "y", "r", "nb"))
        h, t = (y, x) if neg_head else (x, y)
        pos = ops.score_pos(Q.MODEL, h, r, t, Q.GAMMA)
        (pos * _dev(inp["dp"])).sum().backward()
        got = dict(pos=pos.detach().cpu().numpy(), gh=h.grad.cpu().numpy(), grp=r.grad.cpu().numpy(), gt=t.grad.cpu().numpy())
        x.grad = y.grad = r.grad = None
        s = ops.score_neg(Q.MODEL, neg_head, x, r, nb, C_, chunk, N, Q.GAMMA, emb_init=1.0)
        (s * _dev(inp["W"])).sum().backward()
        got.update(score=s.detach().cpu().numpy(), gx=x.grad.cpu().numpy(), gr=r.grad.cpu().numpy(), gn=nb.grad.cpu().numpy())
        assert all(np.isfinite(v).all() for v in got.values()), tag + ": non-finite output"
        assert ref["share"] >= Q.DIST_SHARE and ref["cmax"] <= Q.C_MAX, tag
        for g in ("gx", "gn", "gh", "gt", "gr"):
            assert got[g].shape[1] == 2 * k and got[g][:, :k].any() and got[g][:, k:].any(), tag + ": both halves of %s" % g
        errs = {}
        for q in ("pos", "score"):
            errs[q] = Q.worst(got[q], ref[q], Q.score_bound(ref[q]))
        for q in Q.OP_GRADS:
            errs[q] = Q.worst(got[q], ref[q], Q.grad_bound(ref[q]))
        _record("per-op", tag, **errs)
        _check(errs, tag)


# --------------------------------------------------------------------------------------------------------------------------
# 2. the fused step
# --------------------------------------------------------------------------------------------------------------------------
def _engine(c, k, flags=0, zero_p=False):
    from dglke_amd.engine import StepEngine
    eng = StepEngine(Q.MODEL, c["n_ent"], c["n_rel"], k, Q.GAMMA, c["lr"], DEV, True, True, c["adv"], c["adv_temp"], c["reg_coef"],
                     c["reg_norm"], loss_genre=c["genre"], pairwise=c["pairwise"], margin=c["margin"],
                     flags=int(flags) | (Q.NEG_DEG if c["neg_deg"] else 0))
    ent, rel = Q.step_tables(k, zero_p)
    eng.load_tables(ent, rel)
    return eng


def _batch(c, bt):
    from dglke_amd import plan
    return plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV, bt["w"])


def _compare_step(c, eng, b, bt, want, out, before, tag, known=None):
    """the step's optional outputs, loss numbers, Adagrad states and tables against the float64 step `out` / tables `before`
    (ent64, es64, rel64, rs64 after the float64 step)"""
    ent64, es64, rel64, rs64 = before[:4]
    nd, chunk, N = c["neg_deg"], c["chunk"], c["N"]
    Np = chunk + N if nd else N
    gp, gn = want["pos_score"].cpu().numpy(), want["neg_score"].cpu().numpy()
    ref_n = out["neg_score"]
    sb = Q.score_bound(ref_n)
    if known is not None:
        from dglke_amd import _lib
        assert np.array_equal(gn.reshape(known.shape) == np.float32(_lib.KNOWN_SCORE), known), tag + ": the sentinel marks the known pairs"
    errs = dict(pos_score=Q.worst(gp, out["pos_score"], Q.score_bound(out["pos_score"])), neg_score=Q.worst(gn, ref_n, sb))
    l4 = eng.read_loss()
    if c["pairwise"] or c["genre"] == "Softmax":
        assert np.isnan(l4[0]) and np.isnan(l4[1]), tag
    else:
        _close(l4[0], out["log"][0], 1e-4, 1e-5, tag + " pos_loss")
        _close(l4[1], out["log"][1], 1e-4, 1e-5, tag + " neg_loss")
    _close(l4[2], out["log"][2], 1e-4, 1e-5, tag + " loss")
    _close(l4[3], out["log"][3], 1e-3, 1e-7, tag + " reg")
    sel = np.searchsorted(b.p["ue_id"], bt["nid"])
    g_pos = want["g_pos_ent"].cpu().numpy()[sel]
    g_neg = want["g_neg"].cpu().numpy()
    ref_gneg = out["g_neg"]
    if nd:          # sampled rows only; their regulariser is added by the update kernel in this mode
        g_neg = g_neg.reshape(-1, Np, g_neg.shape[1])[:, chunk:].reshape(-1, g_neg.shape[1])
        if c["reg_coef"] > 0:
            ref_gneg = ref_gneg - Q.O.reg_grad(before[4][bt["neg"]], c["reg_coef"], c["reg_norm"])
    errs.update(g_pos_ent=Q.worst(g_pos, out["g_pos_ent"], Q.grad_bound(out["g_pos_ent"])),
                g_neg=Q.worst(g_neg, ref_gneg, Q.grad_bound(out["g_neg"])),
                g_rel=Q.worst(want["g_rel"].cpu().numpy(), out["g_rel"], Q.grad_bound(out["g_rel"])),
                ent_rows=Q.worst(_f64(eng.ent), ent64, Q.grad_bound(ent64)), rel_rows=Q.worst(_f64(eng.rel), rel64, Q.grad_bound(rel64)),
                ent_state=Q.worst(_f64(eng.ent_state), es64, Q.grad_bound(es64)),
                rel_state=Q.worst(_f64(eng.rel_state), rs64, Q.grad_bound(rs64)))
    return errs


@pytest.mark.parametrize("c", Q.STEP_CASES, ids=[c["id"] for c in Q.STEP_CASES])
@pytest.mark.parametrize("k", Q.STEP_WIDTHS)
def test_fused_step_matches_float64_step(k, c):
    """kge_step_fused with every optional output of kge_step_out, one step per corruption side from the fixed tables; entities and
    relations repeat inside the batch and among the negatives"""
    for bt in Q.step_batches(c):
        eng = _engine(c, k)
        ent64, rel64, es64, rs64 = _f64(eng.ent), _f64(eng.rel), _f64(eng.ent_state), _f64(eng.rel_state)
        ent0 = ent64.copy()
        moved0 = eng.ent.clone()
        b = _batch(c, bt)
        want = eng.alloc_outputs(b)
        eng.step(b, want)
        torch.cuda.synchronize()
        out = Q.step(c, ent64, es64, rel64, rs64, bt)
        assert out["share"] >= Q.DIST_SHARE and Q.residual_rows(out) == 0 and out["cmax"] <= Q.C_MAX, \
            "a step input outside the conditions of transd_cases.py"
        tag = "k%d %s %s" % (k, c["id"], "head" if bt["neg_head"] else "tail")
        assert not torch.equal(moved0, eng.ent), tag + ": the step did not move the entity table"
        assert not torch.equal(moved0[:, k:], eng.ent[:, k:]), tag + ": the step did not move the mapping halves"
        errs = _compare_step(c, eng, b, bt, want, out, (ent64, es64, rel64, rs64, ent0), tag)
        _record("step", tag, **errs)
        _check(errs, tag)


@pytest.mark.parametrize("k", Q.STEP_WIDTHS)
def test_step_with_known_index_matches_float64_statement(k):
    """kge_step_fused_known: the planted known pairs take KGE_KNOWN_SCORE - no loss term, no gradient"""
    from dglke_amd.known import KnownIndex
    c = Q.STEP_CASES[1]
    for bt in Q.step_batches(c):
        eng = _engine(c, k)
        K, known = Q.planted_known(bt, c["chunk"], c["N"])
        eng.attach_known(KnownIndex(K, c["n_ent"], c["n_rel"], DEV))
        ent64, rel64, es64, rs64 = _f64(eng.ent), _f64(eng.rel), _f64(eng.ent_state), _f64(eng.rel_state)
        b = _batch(c, bt)
        want = eng.alloc_outputs(b)
        eng.step(b, want)
        torch.cuda.synchronize()
        out = Q.step(c, ent64, es64, rel64, rs64, bt, known)
        tag = "k%d known-pairs %s" % (k, "head" if bt["neg_head"] else "tail")
        errs = _compare_step(c, eng, b, bt, want, out, (ent64, es64, rel64, rs64, None), tag, known=known)
        _record("step", tag, **errs)
        _check(errs, tag)


def _run_two_steps(c, k, entry, with_known=False):
    from dglke_amd import _lib
    from dglke_amd.known import KnownIndex
    eng = _engine(c, k)
    for bt in Q.step_batches(c):
        b = _batch(c, bt)
        if with_known:
            eng.attach_known(KnownIndex(Q.planted_known(bt, c["chunk"], c["N"])[0], c["n_ent"], c["n_rel"], DEV))
            if entry == "fused":
                eng.step(b)
            else:
                eng.step_timed(b)
            torch.cuda.synchronize()
            continue
        ws = eng.workspace_for(b)
        out = _lib.KgeStepOut()
        out.loss_accum = _lib.ptr(eng.loss_accum)
        a = (C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(ws), eng._ws_bytes)
        if entry == "fused":
            _lib.check(_lib.lib().kge_step_fused(*a, _lib.stream_ptr()))
        else:
            for ph in (_lib.PHASE_GATHER, _lib.PHASE_FORWARD, _lib.PHASE_BACKWARD, _lib.PHASE_UPDATE):
                _lib.check(_lib.lib().kge_step_phase(*a, ph, _lib.stream_ptr()))
        torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)] + [np.array(eng.read_loss_sums(), np.float32)]


WHAT = ("entity table", "entity state", "relation table", "relation state", "loss sums")


@pytest.mark.parametrize("k", Q.STEP_WIDTHS)
def test_step_in_four_phases_equals_the_fused_step(k):
    """kge_step_phase, the four phase groups in order on one stream, is kge_step_fused - bit for bit; with a known index too
    (kge_step_phase_known through StepEngine.step_timed)"""
    c = Q.STEP_CASES[1]
    for with_known in (False, True):
        res = {entry: _run_two_steps(c, k, entry, with_known) for entry in ("fused", "phase")}
        assert np.abs(res["fused"][1]).max() > 0 and np.isfinite(res["fused"][4][2]) and res["fused"][4][2] > 0
        for x, y, what in zip(res["fused"], res["phase"], WHAT):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s (known index: %s)" % (what, with_known)


def test_two_consecutive_steps_are_deterministic():
    """the same two steps (tail, then head corruption on the moved tables) run twice give the same tables, bit for bit: no atomics,
    every sum in a fixed order - under the regulariser and with --neg_deg_sample too"""
    for c in (Q.STEP_CASES[1], Q.STEP_CASES[-1], [x for x in Q.STEP_CASES if x["neg_deg"]][0]):
        a, b = _run_two_steps(c, 36, "fused"), _run_two_steps(c, 36, "fused")
        assert np.abs(a[1]).max() > 0
        for x, y, what in zip(a, b, WHAT):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: %s" % (c["id"], what)


def test_adam_step_matches_the_statement():
    """--optimizer Adam works through kge_step_optim with no code of its own for the model: four steps against adam_cases.step on this
    file's gradients, step by step, with the ambiguity rule and cap of adam_cases"""
    from test_gpu_adam import _batch as a_batch, _compare_step as a_compare, _engine as a_engine, _f64 as a_f64, _state as a_state
    c = Q.ADAM_CASE
    ent, rel = A.tables(c)
    eng = a_engine(c)
    eng.load_tables(ent, rel)
    amb = dict(ent=np.zeros(ent.shape, bool), rel=np.zeros(rel.shape, bool))
    moved = 0.0
    for s_, bt in enumerate(A.batches(c), 1):
        before = a_state(eng)
        eng.step(a_batch(c, bt))
        after = a_state(eng)
        ref = a_f64(before)
        with Q.adam_gradients():
            info = A.step(c, ref, bt)
        assert info["out"]["share"] >= Q.DIST_SHARE
        for tab in ("ent", "rel"):
            amb[tab] |= A.ambiguous(info[tab][0], info[tab][1], amb[tab].shape[0])
            assert amb[tab].mean() <= A.AMBIGUITY_CAP, "step %d: %.4f of %s is ambiguous" % (s_, amb[tab].mean(), tab)
        errs = a_compare(c["id"], before, after, ref, info, amb, s_)
        _record("adam", "%s step %d" % (c["id"], s_), **errs)
        _check(errs, "%s step %d" % (c["id"], s_))
        moved = max(moved, float(np.abs(after["ent"] - before["ent"]).max()))
    assert moved > 0.5 * c["lr"], "the tables hardly moved (%.3e)" % moved


def test_zero_mapping_halves_stay_zero_and_train_as_transe_l2():
    """tables whose e_p and r_p halves are all zero, -rc 0: those halves - values and every gradient into them - stay exactly zero,
    and the first halves and r match the float64 statement, which there is TransE_l2"""
    c = dict(Q.STEP_CASES[1], reg_coef=0.0)
    k = 32
    for bt in Q.step_batches(c):
        eng = _engine(c, k, zero_p=True)
        assert not eng.ent[:, k:].any() and not eng.rel[:, k:].any() and eng.ent[:, :k].any()
        ent64, rel64, es64, rs64 = _f64(eng.ent), _f64(eng.rel), _f64(eng.ent_state), _f64(eng.rel_state)
        before = eng.ent.clone()
        b = _batch(c, bt)
        want = eng.alloc_outputs(b)
        eng.step(b, want)
        torch.cuda.synchronize()
        out = Q.step(c, ent64, es64, rel64, rs64, bt)
        tag = "k%d zero-halves %s" % (k, "head" if bt["neg_head"] else "tail")
        for name in ("g_pos_ent", "g_neg", "g_rel"):
            g = want[name].cpu().numpy()
            assert not g[:, k:].any() and g[:, :k].any(), "%s: %s into a zero half" % (tag, name)
            assert not out[name][:, k:].any()
        assert not eng.ent[:, k:].any() and not eng.rel[:, k:].any(), tag + ": a zero half moved"
        assert not torch.equal(before[:, :k], eng.ent[:, :k]), tag
        # the statement there is TransE_l2 on the first halves
        e1, r1 = Q.step_tables(k, True)
        hh, tt, rr = e1[bt["h"]].astype(np.float64)[:, :k], e1[bt["t"]].astype(np.float64)[:, :k], r1[bt["r"]].astype(np.float64)[:, :k]
        assert np.abs(out["pos_score"] - (Q.GAMMA - np.sqrt(((hh + rr - tt) ** 2).sum(-1)))).max() < 1e-12
        errs = _compare_step(c, eng, b, bt, want, out, (ent64, es64, rel64, rs64, None), tag)
        _record("step", tag, **errs)
        _check(errs, tag)


# --------------------------------------------------------------------------------------------------------------------------
# 3. exact ranks
# --------------------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: %d of %d ranks differ, first at triple %d (got %d, float64 %d)" % (
        what, len(bad), len(want), bad[0] if len(bad) else -1, got[bad[0]] if len(bad) else 0, want[bad[0]] if len(bad) else 0)


@pytest.mark.parametrize("n,k", Q.TIE_CASES, ids=["n%d-k%d" % c for c in Q.TIE_CASES])
def test_ranking_entries_equal_float64_on_integer_grid_tables(n, k):
    """Ranker.ranks raw and filtered on both sides, Ranker.chunked_ranks (all entities, lists with -1 pads, self_cand) and
    kge_topk_select / _filtered on tables whose float32 squared distances are exact: ranks and order EQUAL the float64 ones, the
    scores are the float32 statement's bit for bit"""
    from dglke_amd import _lib, eval as kev
    c = Q.tie_inputs(n, k)
    d_e = 2 * k
    ent, rel = _dev(c.ent), _dev(c.rel)
    E = len(c.h)
    cand = Q.tie_candidates(n, E, Q.TIE_CHUNK)
    for batch in (E, 16):
        rk = kev.Ranker(Q.MODEL, ent, rel, Q.TIE_GAMMA, 1.0, batch=batch)
        for neg_head in (False, True):
            p, S = Q.tie_scores(c, c.h, c.r, c.t, neg_head)
            p32 = Q.tie_scores(c, c.h, c.r, c.t, neg_head, np.float32)[0]         # (the scores are roots: float32 bits from the float32 statement)
            lists = Q.filter_lists(c, neg_head)
            for filt in (None, lists):
                what = "Ranker.ranks batch=%d neg_head=%d %s" % (batch, neg_head, "filtered" if filt else "raw")
                fl = None if filt is None else (_dev(filt[0]), _dev(filt[1]))
                got, pos = rk.ranks(c.h, c.r, c.t, neg_head, filt=fl, want_pos_score=True)
                _same(got.cpu().numpy(), Q.ranks_of(p, S, filt), what)
                assert np.array_equal(pos.cpu().numpy(), p32), what + ": positive scores"
                got = rk.chunked_ranks(c.h, c.r, c.t, neg_head, Q.TIE_CHUNK, filt=fl)
                _same(got.cpu().numpy(), Q.ranks_of(p, S, filt), what.replace("Ranker.ranks", "Ranker.chunked_ranks"))
            if batch == E:
                for self_cand in (False, True):
                    what = "Ranker.chunked_ranks lists neg_head=%d self_cand=%d" % (neg_head, self_cand)
                    got, pos = rk.chunked_ranks(c.h, c.r, c.t, neg_head, Q.TIE_CHUNK, cand=_dev(cand), self_cand=self_cand, want_pos_score=True)
                    _same(got.cpu().numpy(), Q.chunked_ranks_of(c, p, S, neg_head, cand, self_cand, Q.TIE_CHUNK), what)
                    assert np.array_equal(pos.cpu().numpy(), p32), what + ": positive scores"
                got = rk.chunked_ranks(c.h, c.r, c.t, neg_head, Q.TIE_CHUNK, self_cand=True)
                _same(got.cpu().numpy(), Q.chunked_ranks_of(c, p, S, neg_head, None, True, Q.TIE_CHUNK), "Ranker.chunked_ranks all entities self_cand")
    # top-K: every candidate (K = n) or the 128 best, equal scores in candidate order; filtered: the listed entities never enter
    L = _lib.lib()
    K = min(n, 128)
    h, r, t, cd = _dev(c.h), _dev(c.r), _dev(c.t), torch.arange(n, dtype=torch.int64, device=DEV)
    for side in (0, 1):
        _, S = Q.tie_scores(c, c.h, c.r, c.t, bool(side))
        S32 = Q.tie_scores(c, c.h, c.r, c.t, bool(side), np.float32)[1]
        frng, fids = Q.filter_lists(c, bool(side))
        for filtered in (False, True):
            res_s = torch.zeros(E, K, dtype=torch.float32, device=DEV)
            res_o = torch.full((E, K), -1, dtype=torch.int64, device=DEV)
            base = torch.zeros(E, dtype=torch.int64, device=DEV)
            ws = torch.empty(_lib.topk_workspace_bytes(Q.MODEL_ID, E, n, d_e, K), dtype=torch.uint8, device=DEV)
            a = (Q.MODEL_ID, side, _lib.ptr(ent), n, _lib.ptr(rel), n, _lib.ptr(h), _lib.ptr(r), _lib.ptr(t), E, d_e, d_e, Q.TIE_GAMMA,
                 1.0, _lib.ptr(cd), n, _lib.ptr(base), 1, 1, K, _lib.ptr(res_s), _lib.ptr(res_o), _lib.ptr(ws), ws.numel())
            if filtered:
                fr, fi = _dev(frng.reshape(-1)), _dev(fids)
                _lib.check(L.kge_topk_select_filtered(*a, _lib.ptr(fr), _lib.ptr(fi), _lib.stream_ptr()))
            else:
                _lib.check(L.kge_topk_select(*a, _lib.stream_ptr()))
            go, gs = res_o.cpu().numpy(), res_s.cpu().numpy()
            for i in range(E):
                keep = np.ones(n, bool)
                if filtered:
                    keep[fids[frng[i, 0]:frng[i, 1]]] = False
                ids = np.nonzero(keep)[0]
                order = ids[np.argsort(-S[i, ids], kind="stable")][:K]
                what = "kge_topk_select%s side=%d row %d" % ("_filtered" if filtered else "", side, i)
                assert np.array_equal(go[i, :len(order)], order) and np.all(go[i, len(order):] == -1), what + ": order"
                assert np.array_equal(gs[i, :len(order)], S32[i, order]), what + ": scores"


# --------------------------------------------------------------------------------------------------------------------------
# 4. the interface
# --------------------------------------------------------------------------------------------------------------------------
def _check_groups(res, S, triples_of, K, tag, excluded=None):
    """every group of `res` holds min(K, available) triples of its group, their scores are the float64 scores of those triples
    and, sorted, the float64 leaders of the group (1e-4 abs + 1e-4 rel: near-equal leaders may swap)"""
    for g, grp in enumerate(res):
        hh, rr, tt, ss = grp[:4]
        allowed = triples_of(g)
        if excluded is not None:
            allowed = [x for x in allowed if x not in excluded]
        assert len(ss) == min(K, len(allowed)), "%s group %d: %d results" % (tag, g, len(ss))
        got = list(zip(hh.tolist(), rr.tolist(), tt.tolist()))
        assert len(set(got)) == len(got) and set(got) <= set(allowed), "%s group %d: a result outside the group" % (tag, g)
        s64 = np.array([S[x] for x in got])
        _close(ss, s64, 1e-4, 1e-4, "%s group %d scores" % (tag, g))
        lead = np.sort(np.array([S[x] for x in allowed]))[::-1][:len(ss)]
        _close(np.sort(ss)[::-1], lead, 1e-4, 1e-4, "%s group %d leaders" % (tag, g))
        assert np.all(np.diff(ss) <= 0), "%s group %d: not in descending order" % (tag, g)


def test_link_predict_and_score_infer(tmp_path):
    from dglke_amd import infer, ke_model
    ent, rel = Q.interface_tables()
    S = Q.all_scores(ent, rel)
    K, nE, nR = Q.IF_K, Q.IF_ENT, Q.IF_REL
    path = str(tmp_path)
    np.save(os.path.join(path, "entity.npy"), ent)
    np.save(os.path.join(path, "relation.npy"), rel)
    m = ke_model.TransDModel(0, Q.IF_GAMMA)
    m.load(path)
    assert m.num_entity == nE and m.num_rel == nR and m.model_name == "TransD"
    heads, rels = [3, 17, 39], [0, 4]
    tails = [5, 21]
    # known triples: for every group some of its float64 leaders, so that 'exclude' changes the result
    known = []
    for hd in heads:
        sub = S[hd][rels]
        for o in np.argsort(-sub.reshape(-1))[:2]:
            known.append((hd, rels[o // nE], int(o % nE)))
    for tl in tails:
        sub = S[:, rels, tl]
        for o in np.argsort(-sub.reshape(-1))[:2]:
            known.append((int(o // len(rels)), rels[o % len(rels)], tl))
    kn = np.array(known, np.int64)
    m.attach_graph((kn[:, 0], kn[:, 1], kn[:, 2]))
    group = lambda g: [(heads[g], r_, t_) for r_ in rels for t_ in range(nE)]
    plain = m.link_predict(head=heads, rel=rels, exec_mode="batch_head", topk=K)
    _check_groups(plain, S, group, K, "link_predict")
    assert all(grp[4] is None for grp in plain)
    ex = m.link_predict(head=heads, rel=rels, exec_mode="batch_head", exclude_mode="exclude", topk=K)
    _check_groups(ex, S, group, K, "link_predict exclude", excluded=set(known))
    mk = m.link_predict(head=heads, rel=rels, exec_mode="batch_head", exclude_mode="mask", topk=K)
    _check_groups(mk, S, group, K, "link_predict mask")
    for grp in mk:
        want = [x in set(known) for x in zip(grp[0].tolist(), grp[1].tolist(), grp[2].tolist())]
        assert grp[4].tolist() == want and any(want)
    # the head side: candidates are heads
    tgroup = lambda g: [(h_, r_, tails[g]) for r_ in rels for h_ in range(nE)]
    _check_groups(m.link_predict(rel=rels, tail=tails, exec_mode="batch_tail", topk=K), S, tgroup, K, "link_predict batch_tail")
    _check_groups(m.link_predict(rel=rels, tail=tails, exec_mode="batch_tail", exclude_mode="exclude", topk=K), S, tgroup, K,
                  "link_predict batch_tail exclude", excluded=set(known))
    # embed_sim runs on the rows as they are, both halves
    sim = m.embed_sim(left=[5], embed_type="entity", sfunc="cosine", topk=3)
    e64 = ent.astype(np.float64)
    cos = (e64 @ e64[5]) / np.linalg.norm(e64, axis=1) / np.linalg.norm(e64[5])
    assert sim[0][1].tolist() == np.argsort(-cos)[:3].tolist() and sim[0][1][0] == 5
    _close(sim[0][2], np.sort(cos)[::-1][:3], 1e-4, 1e-4, "embed_sim")
    # ScoreInfer on the trainer's file names
    np.save(os.path.join(path, "toy_TransD_entity.npy"), ent)
    np.save(os.path.join(path, "toy_TransD_relation.npy"), rel)
    config = dict(model_name="TransD", dataset="toy", hidden_dim=Q.IF_K_HALF, gamma=Q.IF_GAMMA, double_ent=True, double_rel=True)
    si = infer.ScoreInfer(0, config, path, sfunc="logsigmoid")
    si.load_model()
    LS = -np.log1p(np.exp(-S))                                    # logsigmoid of the score with the trained gamma
    every = [(a, b_, c_) for a in range(nE) for b_ in range(nR) for c_ in range(nE)]
    _check_groups(si.topK(exec_mode="all", k=K), LS, lambda g: every, K, "ScoreInfer all")
    _check_groups(si.topK(head=heads, rel=rels, exec_mode="batch_head", k=K), LS, group, K, "ScoreInfer batch_head")
    th_, tr_, tt_ = [1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 0], [9, 8, 7, 6, 5, 4, 3]
    _check_groups(si.topK(head=th_, rel=tr_, tail=tt_, exec_mode="triplet_wise", k=K), LS, lambda g: list(zip(th_, tr_, tt_)), K,
                  "ScoreInfer triplet_wise")


def test_cli_round_trip(tmp_path, capsys):
    """dglke_train --model_name TransD -de -dr --test saves and its loss falls over 200 steps; dglke_eval on the saved files prints
    the same metrics; dglke_predict returns K rows"""
    from dglke_amd import eval_cli, predict_cli, train as T
    from test_gpu_cli import _planted
    data = str(tmp_path / "kg")
    _planted(data)
    files = ["--format", "udd_hrt", "--dataset", "toy", "--data_path", data, "--data_files", "e.dict", "r.dict", "train.txt", "valid.txt",
             "test.txt"]
    tr = T.main(["--model_name", "TransD", "-de", "-dr"] + files + ["--save_path", str(tmp_path / "ckpts"), "--gpu", "0", "--batch_size", "256",
                                                                   "--neg_sample_size", "64", "--hidden_dim", "32", "--gamma", "6.0",
                                                                   "--lr", "0.25", "-adv", "-rc", "1e-7", "--max_step", "200",
                                                                   "--log_interval", "20", "--test", "--graph_steps", "10"])
    out = capsys.readouterr().out
    assert "[proc 0][Train](200/200) average loss:" in out
    losses = [float(l.split("average loss:")[1].split()[0]) for l in out.split("\n") if "[Train](" in l and "average loss:" in l]
    assert len(losses) == 10 and np.isfinite(losses).all() and losses[-1] < 0.8 * losses[0], losses
    want = {l.split(" average ")[1].split(":")[0]: float(l.split(":")[1]) for l in out.split("\n") if l.startswith("[0]Test average")}
    assert {"MRR", "MR", "HITS@10"} <= set(want)
    save = tr.args.save_path
    assert os.path.basename(save) == "TransD_toy_0"
    ent, rel = np.load(os.path.join(save, "toy_TransD_entity.npy")), np.load(os.path.join(save, "toy_TransD_relation.npy"))
    assert ent.shape == (400, 64) and rel.shape == (6, 64) and np.isfinite(ent).all() and np.isfinite(rel).all()
    assert np.array_equal(ent, tr.model.entity_emb.emb.cpu().numpy())
    conf = json.load(open(os.path.join(save, "config.json")))
    assert conf["model_name"] == "TransD" and conf["hidden_dim"] == 32 and conf["double_ent"] is True and conf["double_rel"] is True
    ev = eval_cli.main(["--model_name", "TransD", "-de", "-dr"] + files + ["--model_path", save, "--gpu", "0", "--hidden_dim", "32",
                                                                          "--gamma", "6.0"])
    capsys.readouterr()
    assert set(ev) == set(want)
    for q in want:
        assert abs(ev[q] - want[q]) < 1e-9, (q, ev[q], want[q])
    hf, rf = str(tmp_path / "head.list"), str(tmp_path / "rel.list")
    open(hf, "w").write("1\n2\n3\n")
    open(rf, "w").write("0\n5\n")
    res = str(tmp_path / "result.tsv")
    predict_cli.main(["--model_path", save, "--format", "h_r_*", "--data_files", hf, rf, "--exec_mode", "batch_head", "--topK", "7",
                      "--output", res, "--gpu", "0", "--score_func", "none"])
    rows = open(res).read().strip().split("\n")
    assert rows[0] == "head\trel\ttail\tscore" and len(rows) == 1 + 3 * 7
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    for row in rows[1:]:
        a, b_, c_, s = row.split("\t")
        ref = Q.score(e64[int(a):int(a) + 1], r64[int(b_):int(b_) + 1], e64[int(c_):int(c_) + 1], 0.0)[0]      # score_func none: gamma 0
        assert int(a) in (1, 2, 3) and int(b_) in (0, 5) and abs(float(s) - ref) <= 1e-4 + 1e-4 * abs(ref)


def test_resumed_run_ends_with_the_uninterrupted_runs_tables(tmp_path):
    """run A: --max_step 230; B1: --max_step 45 --checkpoint_interval 45; B2: --resume B1 --max_step 230 (the protocol of
    tests/checkpoint_cases.py).  B2's tables and Adagrad states are A's, bit for bit"""
    import checkpoint_cases as CK
    import train_loop_cases as L
    from dglke_amd import train as T
    c = ("transd", "TransD", ["-de", "-dr"], False, [45], (20, 20))
    data = str(tmp_path / "kg")
    L.write_planted(data)

    def run(argv):
        with contextlib.redirect_stdout(io.StringIO()):
            tr = T.main(argv)
        torch.cuda.synchronize()
        return tr.args.save_path, {n_: t.detach().cpu().clone() for n_, t in tr.model.engine.named_tensors().items()}
    _, a = run(CK.argv_a(c, data, str(tmp_path / "a")))
    b1_dir, b1 = run(CK.argv_b(c, data, str(tmp_path / "b1"), 0))
    assert os.path.isdir(os.path.join(b1_dir, "checkpoint"))
    _, b2 = run(CK.argv_b(c, data, str(tmp_path / "b2"), 1, b1_dir))
    assert sorted(a) == sorted(b2) and len(a) == 4
    for name in sorted(a):
        assert not torch.equal(a[name], b1[name]), "%s: nothing was trained after step 45" % name
        assert torch.equal(a[name], b2[name]), "%s: the resumed run differs from the uninterrupted run" % name


# --------------------------------------------------------------------------------------------------------------------------
# 5. refusals on the device entries
# --------------------------------------------------------------------------------------------------------------------------
def test_device_entries_refuse_transd_before_any_launch():
    from dglke_amd import _lib, eval as kev
    from dglke_amd.engine import StepEngine
    c = Q.STEP_CASES[1]
    k = 32
    eng = _engine(c, k)
    bt = Q.step_batches(c)[0]
    b = _batch(c, bt)
    before = [x.clone() for x in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)]
    with pytest.raises(_lib.KgeError, match="kge_step_async.*TransD"):
        eng.step_async(b)
    UE, d = b.UE, 2 * k
    bufs = [torch.zeros(UE, d, device=DEV), torch.zeros(UE, device=DEV), torch.zeros(UE, d, device=DEV), torch.zeros(UE, device=DEV)]
    em = _lib.KgeEmit()
    em.g0, em.gs0, em.g1, em.gs1 = (x.data_ptr() for x in bufs)
    with pytest.raises(_lib.KgeError, match="kge_step_grads.*TransD"):
        eng.step(b, emit=em)
    sh = _lib.KgeShards()
    ws = eng.workspace_for(b)
    rc = _lib.lib().kge_step_sharded(C.byref(eng.hp), C.byref(sh), C.byref(b.c), None, _lib.ptr(ws), eng._ws_bytes, _lib.stream_ptr())
    assert rc == -1 and b"TransD" in _lib.lib().kge_last_error()
    # the sampler job
    out = _lib.KgeStepOut()
    out.loss_accum = _lib.ptr(eng.loss_accum)
    job = _lib.KgeSamplerJob()
    ids = torch.zeros(64, dtype=torch.int64, device=DEV)
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    job.heads = job.rels = job.tails = _lib.ptr(ids)
    job.state = job.slot = job.scratch = _lib.ptr(scratch)
    job.scratch_bytes = scratch.numel()
    job.n_train, job.n_ent, job.B, job.C, job.chunk, job.N = 64, c["n_ent"], c["B"], c["B"] // c["chunk"], c["chunk"], c["N"]
    rc = _lib.lib().kge_step_fused_sampling(C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(ws), eng._ws_bytes,
                                            C.byref(job), _lib.stream_ptr())
    assert rc == -1 and b"kge_step_fused_sampling" in _lib.lib().kge_last_error() and b"TransD" in _lib.lib().kge_last_error()
    ent, rel = eng.ent, eng.rel
    with pytest.raises(_lib.KgeError, match="kge_rank_eval_split.*TransD"):
        kev.SplitRanker(Q.MODEL, ent, rel, 0.0, 1.0).ranks(ent, bt["h"][:4], bt["r"][:4], bt["t"][:4], False)
    frng = torch.tensor([[0, 1]] * 4, dtype=torch.int64, device=DEV)
    fids = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.KgeError, match="kge_rank_rel_eval.*TransD"):
        kev.Ranker(Q.MODEL, ent, rel, 0.0, 1.0).relation_ranks(bt["h"][:4], bt["r"][:4], bt["t"][:4], (frng, fids))
    torch.cuda.synchronize()
    for x, y in zip(before, (eng.ent, eng.ent_state, eng.rel, eng.rel_state)):
        assert torch.equal(x, y), "a refused call moved a table"
    assert not any(x.any() for x in bufs)
    with pytest.raises(_lib.KgeError, match="TransD"):
        StepEngine(Q.MODEL, 10, 2, 32, 12.0, 0.1, DEV, False, True)              # entity rows without their mapping half
