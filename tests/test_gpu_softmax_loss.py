"""--loss_genre Softmax (softmax cross-entropy of the positive against the negatives of its own row; include/kge_hip.h
KGE_LOSS_SOFTMAX) on the GPU against the float64 statement of tests/softmax_loss_cases.py (inputs guarded on the CPU by
tests/test_softmax_loss_inputs.py):
  1. the loss op (ops.loss_fwd_bwd, LossGenerator.get_total_loss + backward) at one N per instance of the loss kernel;
  2. the fused step, by the method of tests/test_gpu_loss_options.py::run_case (two steps, the float64 oracle - hooked, the oracle
     itself has no such genre - restarted from the GPU's own tables), at that suite's tolerances;
  3. with --exclude_positive (known pairs at KGE_KNOWN_SCORE);
  4. the gradient-emitting step against the fused step's trace gradients, and the step in four phases against the fused step;
  5. dglke_train, one process and `--gpu 0 0`.
A Softmax step takes the pairwise launch sequence (edge rows, negative scores, the stand-alone loss kernel, backward, update):
the kernel-path flags that move the loss elsewhere are accepted and fall back, which 2. runs for the matrix-core models.

softmax_loss_errors.txt, beside loss_option_errors.txt, records the largest errors per case."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_option_cases as L
import softmax_loss_cases as S
from oracle import kge_oracle as O
from test_gpu_loss_options import _batch, _engine, _err, _f64, _report_dir, _union
from test_gpu_parity import DEV, _close, _l1_ambiguous, _masked, grad_tol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ERRORS = {}          # case -> dict(loss, score, grad, rows, note)


def _record(key, **kw):
    rec = ERRORS.setdefault(key, dict(loss=0.0, score=0.0, grad=0.0, rows=0.0, note=""))
    for k, v in kw.items():
        rec[k] = v if k == "note" else max(rec[k], float(v))
    try:
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "softmax_loss_errors.txt"), "w") as f:
            f.write("%-44s %11s %11s %14s %11s\n" % ("case", "|loss| rel", "max|score|", "max|grad|/gmax", "max|row|/lr"))
            for k in sorted(ERRORS):
                r = ERRORS[k]
                f.write("%-44s %11.3e %11.3e %14.3e %11.3e  %s\n" % (k, r["loss"], r["score"], r["grad"], r["rows"], r["note"]))
    except OSError:
        pass


# --------------------------------------------------------------------------------------------------------------------------
# 1. the loss op
# --------------------------------------------------------------------------------------------------------------------------
def _device_scores(neg, aligned):
    """[B, N] float32 on the device; aligned False: the array starts 4 bytes behind a 16-byte boundary (strided column layout)"""
    B, N = neg.shape
    buf = torch.zeros(B * N + 8, dtype=torch.float32, device=DEV)
    off = 0 if aligned else 1
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + B * N].view(B, N)
    v.copy_(torch.from_numpy(neg))
    assert (v.data_ptr() % 16 == 0) == aligned and v.is_contiguous()
    return v


@pytest.mark.parametrize("weights", [False, True], ids=["w1", "impts"])
@pytest.mark.parametrize("N,aligned,inst", S.OP_SHAPES, ids=["N%d-%s" % (s[0], s[2].replace(" ", "_")) for s in S.OP_SHAPES])
@pytest.mark.parametrize("B", S.OP_B)
def test_loss_op_matches_float64(B, N, aligned, inst, weights):
    from dglke_amd import ops
    from dglke_amd.loss import LossGenerator
    pos, neg, w = S.op_inputs(B, N, weights)
    (_, _, loss64), dpos64, dneg64 = S.softmax_fwd_bwd(pos.astype(np.float64), neg.astype(np.float64),
                                                       None if w is None else w.astype(np.float64))
    tw = None if w is None else torch.from_numpy(w).to(DEV)
    tag = "op B%d N%d %s" % (B, N, "impts" if weights else "w1")
    worst = dict(loss=0.0, grad=0.0)
    for route in ("ops", "LossGenerator"):
        tp = torch.from_numpy(pos).to(DEV).requires_grad_(True)
        tn = _device_scores(neg, aligned).requires_grad_(True)
        if route == "ops":
            loss, loss3 = ops.loss_fwd_bwd(tp, tn, tw, "Softmax", False, 1.0, False, 1.0)
            l3 = loss3.tolist()
            assert np.isnan(l3[0]) and np.isnan(l3[1]) and l3[2] == float(loss.detach()), tag + ": loss3 is {nan, nan, loss}"
        else:
            loss, log = LossGenerator(None, "Softmax").get_total_loss(tp, tn, None if tw is None else tw.view(-1, 1))
            assert set(log) == {"loss"} and log["loss"] == float(loss.detach())
        (3.0 * loss).backward()                   # (the op's backward scales the saved gradients)
        torch.cuda.synchronize()
        gp, gn = tp.grad.cpu().numpy() / 3.0, tn.grad.cpu().numpy() / 3.0
        t = "%s %s" % (tag, route)
        _close(float(loss), loss64, 1e-4, 1e-5, t + " loss")
        _close(gp, dpos64, 3e-4, grad_tol(dpos64), t + " dpos")
        _close(gn, dneg64, 3e-4, grad_tol(dneg64), t + " dneg")
        assert (gn >= 0).all() and (gp <= 0).all(), t + ": sign of the gradients"
        worst["loss"] = max(worst["loss"], abs(float(loss) - loss64) / max(abs(loss64), 1e-30))
        worst["grad"] = max(worst["grad"], _err(gn, dneg64) / max(float(np.abs(dneg64).max()), 1e-30),
                            _err(gp, dpos64) / max(float(np.abs(dpos64).max()), 1e-30))
    _record("op N%d %s %s" % (N, inst.replace(" ", "_"), "impts" if weights else "w1"), **worst)


def test_loss_op_hard_rows_keep_their_digits():
    """row by row, where the bound of the whole array says nothing: a dominating positive's dL/dp ~ -N exp(-60) / B is neither 0
    nor rounding residue of 1 - e_p / Z, a dominating negative takes the whole weight, equal scores share it"""
    from dglke_amd import ops
    B = 7
    for N, aligned, _ in S.OP_SHAPES:
        pos, neg, _w = S.op_inputs(B, N, False)
        (_, _, _), dpos64, dneg64 = S.softmax_fwd_bwd(pos.astype(np.float64), neg.astype(np.float64))
        tp = torch.from_numpy(pos).to(DEV).requires_grad_(True)
        tn = _device_scores(neg, aligned).requires_grad_(True)
        loss, _ = ops.loss_fwd_bwd(tp, tn, None, "Softmax", False, 1.0, False, 1.0)
        loss.backward()
        gp, gn = tp.grad.cpu().numpy().astype(np.float64), tn.grad.cpu().numpy().astype(np.float64)
        assert np.isfinite(gp).all() and np.isfinite(gn).all()
        for kind in S.HARD:
            k = S.HARD.index(kind)
            # per row: 3e-4 of the row's own largest gradient (the scores differ by up to 140: exp of a float32 difference)
            _close(gp[k], dpos64[k], 3e-4, 0.0, "N%d %s dpos" % (N, kind))
            _close(gn[k], dneg64[k], 3e-4, 3e-4 * np.abs(dneg64[k]).max(), "N%d %s dneg" % (N, kind))
        k = S.HARD.index("positive+60")
        assert -1e-20 < gp[k] < 0, "N%d: dL/dp of a dominating positive is %r" % (N, gp[k])


# --------------------------------------------------------------------------------------------------------------------------
# 2. the fused step
# --------------------------------------------------------------------------------------------------------------------------
def run_case(c, flags):
    """tests/test_gpu_loss_options.py::run_case for a genre whose loss has no positive / negative part: loss4 is
    {NaN, NaN, loss, regularization}.  The caller has installed the oracle hook."""
    eng = _engine(c, flags)
    key = "%s f%d" % (c["id"], flags)
    nd, transr = c["neg_deg"], c["model"] == "TransR"
    chunk, N, lr = c["chunk"], c["N"], c["lr"]
    Np = chunk + N if nd else N
    for step, bt in enumerate(L.batches(c), 1):
        ent64, rel64, es64, rs64 = _f64(eng.ent), _f64(eng.rel), _f64(eng.ent_state), _f64(eng.rel_state)
        pj64, ps64 = _f64(eng.proj), _f64(eng.proj_state)
        ent0, rel0 = ent64.copy(), rel64.copy()
        b = _batch(c, bt)
        want = eng.alloc_outputs(b)
        eng.step(b, want)
        torch.cuda.synchronize()
        out = L.oracle_step(c, ent64, es64, rel64, rs64, pj64, ps64, bt)
        tag = "%s step %d" % (key, step)
        gp, gn = want["pos_score"].cpu().numpy(), want["neg_score"].cpu().numpy()
        _close(gp, out["pos_score"], 1e-4, 1e-4, tag + " pos_score")
        _close(gn, out["neg_score"], 1e-4, 1e-4, tag + " neg_score")
        excl = dict(slots=[], edges=[], pos_local=[], ent=[], rel=[])
        if c["model"] == "TransE_l1":
            amb = _l1_ambiguous(bt, ent0, rel0, chunk, N, tau=1.1 * 2.0 ** -24 * float(max(np.abs(ent0).max(), 1e-30)) * 2)
            assert len(amb["ent"]) <= 30 and len(amb["rel"]) <= 15, "too many sign-ambiguous rows to call this a comparison: %r" % amb
            excl = _union(excl, amb)
        l4 = eng.read_loss()
        assert np.isnan(l4[0]) and np.isnan(l4[1]), tag + ": the Softmax loss has no positive / negative part"
        assert np.isnan(out["log"][0]) and np.isnan(out["log"][1])
        _close(l4[2], out["log"][2], 1e-4, 1e-5, tag + " loss")
        _close(l4[3], out["log"][3], 1e-3, 1e-7, tag + " reg")
        sel = np.searchsorted(b.p["ue_id"], bt["nid"])
        g_pos = want["g_pos_ent"].cpu().numpy()[sel]
        g_neg = want["g_neg"].cpu().numpy()
        ref_gneg = out["g_neg"]
        if nd:      # sampled rows only; their regulariser is added by the update kernel in this mode
            g_neg = g_neg.reshape(-1, Np, g_neg.shape[1])[:, chunk:].reshape(-1, g_neg.shape[1])
            if c["reg_coef"] > 0:
                ref_gneg = ref_gneg - O.reg_grad(ent0[bt["neg"]], c["reg_coef"], c["reg_norm"])
        g_rel = want["g_rel"].cpu().numpy()
        _close(_masked(g_pos, out["g_pos_ent"], excl["pos_local"]), out["g_pos_ent"], 3e-4, grad_tol(out["g_pos_ent"]), tag + " g_pos_ent")
        _close(_masked(g_neg, ref_gneg, excl["slots"]), ref_gneg, 3e-4, grad_tol(out["g_neg"]), tag + " g_neg")
        _close(_masked(g_rel, out["g_rel"], excl["edges"]), out["g_rel"], 3e-4, grad_tol(out["g_rel"]), tag + " g_rel")
        got_es, got_rs, got_e, got_r = _f64(eng.ent_state), _f64(eng.rel_state), _f64(eng.ent), _f64(eng.rel)
        _close(_masked(got_es, es64, excl["ent"]), es64, 2e-3, 1e-9, tag + " ent state")
        _close(_masked(got_rs, rs64, excl["rel"]), rs64, 2e-3, 1e-9, tag + " rel state")
        _close(_masked(got_e, ent64, excl["ent"]), ent64, 1e-4, c["rows"] * lr, tag + " entity rows")
        _close(_masked(got_r, rel64, excl["rel"]), rel64, 1e-4, c["rows"] * lr, tag + " relation rows")
        rows_err = max(_err(_masked(got_e, ent64, excl["ent"]), ent64), _err(_masked(got_r, rel64, excl["rel"]), rel64))
        if transr:
            got_p, got_ps = _f64(eng.proj), _f64(eng.proj_state)
            _close(_masked(got_ps, ps64, excl["rel"]), ps64, 2e-3, 1e-9, tag + " projection state")
            _close(_masked(got_p, pj64, excl["rel"]), pj64, 1e-4, c["rows"] * lr, tag + " projection rows")
            rows_err = max(rows_err, _err(_masked(got_p, pj64, excl["rel"]), pj64))
        gerr = max(_err(_masked(g, r, x), r) / max(float(np.abs(r).max()), 1e-30)
                   for g, r, x in ((g_pos, out["g_pos_ent"], excl["pos_local"]), (g_neg, ref_gneg, excl["slots"]),
                                   (g_rel, out["g_rel"], excl["edges"])))
        _record(key, loss=abs(l4[2] - out["log"][2]) / abs(out["log"][2]),
                score=max(_err(gp, out["pos_score"]), _err(gn, out["neg_score"])), grad=gerr, rows=rows_err / lr)
    return eng


_MATRIX = [pytest.param(c, f, id="%s-f%d" % (c["id"], f)) for c in S.STEP_CASES for f in c["flags"]]


@pytest.mark.parametrize("c,flags", _MATRIX)
def test_fused_step_with_softmax_matches_oracle(c, flags, monkeypatch):
    """every accepted kernel-path flag gives oracle-equal results: KGE_FLAG_FUSED_LOSS and KGE_FLAG_LOSS_IN_FWD fall back to the
    stand-alone loss kernel, as for -pw"""
    S.hook(monkeypatch)
    run_case(c, flags)


# --------------------------------------------------------------------------------------------------------------------------
# 3. --exclude_positive
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", S.KNOWN_IDS)
def test_step_with_known_index_and_softmax_matches_float64_statement(cid, monkeypatch):
    import known_negative_cases as KN
    from dglke_amd import _lib
    from dglke_amd.known import KnownIndex
    S.hook(monkeypatch)
    c = S.known_case(cid)
    bts, K, notes = KN.build(c)
    eng = _engine(c, 0)
    eng.attach_known(KnownIndex(K, c["n_ent"], c["n_rel"], DEV))
    lr, B, N = c["lr"], c["B"], c["N"]
    for step, (bt, note) in enumerate(zip(bts, notes), 1):
        ent64, rel64, es64, rs64 = _f64(eng.ent), _f64(eng.rel), _f64(eng.ent_state), _f64(eng.rel_state)
        before_e, before_s = eng.ent.cpu().numpy().copy(), eng.ent_state.cpu().numpy().copy()
        b = _batch(c, bt)
        want = eng.alloc_outputs(b)
        eng.step(b, want)
        torch.cuda.synchronize()
        known = KN.known_matrix(K, bt, c["chunk"], N)
        out = KN.masked_step(c, ent64, es64, rel64, rs64, None, None, bt, known)
        tag = "%s step %d" % (c["id"], step)
        gn = want["neg_score"].cpu().numpy()
        _close(want["pos_score"].cpu().numpy(), out["pos_score"], 1e-4, 1e-4, tag + " pos_score")
        _close(gn, out["neg_score"], 1e-4, 1e-4, tag + " neg_score")
        assert np.array_equal(gn.reshape(B, N) == np.float32(_lib.KNOWN_SCORE), known), tag + ": the sentinel marks the known pairs"
        l4 = eng.read_loss()
        assert np.isnan(l4[0]) and np.isnan(l4[1])
        _close(l4[2], out["log"][2], 1e-4, 1e-5, tag + " loss")
        _close(l4[3], out["log"][3], 1e-3, 1e-7, tag + " reg")
        sel = np.searchsorted(b.p["ue_id"], bt["nid"])
        g_neg = want["g_neg"].cpu().numpy()
        _close(want["g_pos_ent"].cpu().numpy()[sel], out["g_pos_ent"], 3e-4, grad_tol(out["g_pos_ent"]), tag + " g_pos_ent")
        _close(g_neg, out["g_neg"], 3e-4, grad_tol(out["g_neg"]), tag + " g_neg")
        _close(want["g_rel"].cpu().numpy(), out["g_rel"], 3e-4, grad_tol(out["g_rel"]), tag + " g_rel")
        _close(_f64(eng.ent_state), es64, 2e-3, 1e-9, tag + " ent state")
        _close(_f64(eng.rel_state), rs64, 2e-3, 1e-9, tag + " rel state")
        _close(_f64(eng.ent), ent64, 1e-4, c["rows"] * lr, tag + " entity rows")
        _close(_f64(eng.rel), rel64, 1e-4, c["rows"] * lr, tag + " relation rows")
        if not c["reg_coef"] > 0:
            # a slot whose every pair is known gets a gradient row of 0.0f; the entity that occurs only there keeps its row and state
            dead = np.nonzero(known.reshape(B // c["chunk"], c["chunk"], N).all(1).reshape(-1))[0]
            assert note["lone_slot"] in dead and (g_neg[dead] == 0.0).all()
            e = note["lone"]
            assert np.array_equal(eng.ent.cpu().numpy()[e].view(np.uint32), before_e[e].view(np.uint32))
            assert eng.ent_state.cpu().numpy()[e].tobytes() == before_s[e].tobytes()
        _record(c["id"], loss=abs(l4[2] - out["log"][2]) / abs(out["log"][2]), score=_err(gn, out["neg_score"]),
                grad=_err(g_neg, out["g_neg"]) / float(np.abs(out["g_neg"]).max()),
                rows=max(_err(_f64(eng.ent), ent64), _err(_f64(eng.rel), rel64)) / lr, note="--exclude_positive")


# --------------------------------------------------------------------------------------------------------------------------
# 4. the gradient-emitting step
# --------------------------------------------------------------------------------------------------------------------------
def test_step_grads_messages_equal_the_fused_steps_trace_gradients():
    """kge_step_grads with a dense emit by union entry (relation trace in place): g0 is the fused step's positive-trace gradient,
    g1 the sum of its negative-trace rows per entity in slot order, gs0 / gs1 their Adagrad increments; the relation table moves
    as in the fused step"""
    from dglke_amd import _lib
    c = S.case("grads-midT-softmax", "midT", rows=5e-3, n_ent=300)        # 300 entities: duplicates among the 96 negatives
    bt = L.batches(c, steps=1)[0]
    fe, ge = _engine(c, 0), _engine(c, 0)
    b = _batch(c, bt)
    want = fe.alloc_outputs(b)
    fe.step(b, want)
    UE, d = b.UE, c["hidden"]
    bufs = dict(g0=torch.zeros(UE, d, device=DEV), gs0=torch.zeros(UE, device=DEV), g1=torch.zeros(UE, d, device=DEV),
                gs1=torch.zeros(UE, device=DEV))
    em = _lib.KgeEmit()
    em.g0, em.gs0, em.g1, em.gs1 = (bufs[k].data_ptr() for k in ("g0", "gs0", "g1", "gs1"))
    ent_before = ge.ent.clone()
    ge.step(b, emit=em, per_step_loss=True)
    torch.cuda.synchronize()
    assert np.array_equal(np.array(ge.read_loss()[2:]), np.array(fe.read_loss()[2:])) and np.isnan(ge.read_loss()[0])
    assert torch.equal(ge.ent, ent_before), "the gradient-emitting step must not move the entity table"
    _close(ge.rel.cpu(), fe.rel.cpu(), 1e-6, 1e-7 * c["lr"], "relation table")
    _close(ge.rel_state.cpu(), fe.rel_state.cpu(), 1e-6, 1e-30, "relation state")
    ue = b.p["ue_id"]
    ue = ue.cpu().numpy() if torch.is_tensor(ue) else np.asarray(ue)
    g_pos, g_neg = want["g_pos_ent"].cpu().numpy(), want["g_neg"].cpu().numpy().astype(np.float64)
    sel = np.searchsorted(ue, bt["nid"])
    g0, g1 = bufs["g0"].cpu().numpy(), bufs["g1"].cpu().numpy()
    assert np.abs(g_pos[sel]).max() > 0
    _close(g0[sel], g_pos[sel], 1e-5, 1e-6 * np.abs(g_pos).max(), "g0")             # the same sums, possibly in another order
    _close(bufs["gs0"].cpu().numpy()[sel], (g_pos[sel].astype(np.float64) ** 2).mean(1), 1e-5, 1e-30, "gs0")
    s1, q1 = np.zeros((len(ue), d)), np.zeros(len(ue))
    slot_u = np.searchsorted(ue, bt["neg"])
    np.add.at(s1, slot_u, g_neg)
    np.add.at(q1, slot_u, (g_neg ** 2).mean(1))
    assert len(np.unique(slot_u)) < len(slot_u), "no entity occurs twice among the negatives"
    touched = np.unique(slot_u)
    _close(g1[touched], s1[touched], 1e-5, 1e-6 * np.abs(s1).max(), "g1")           # float32 sums of a few rows, in another order
    _close(bufs["gs1"].cpu().numpy()[touched], q1[touched], 1e-5, 1e-30, "gs1")


@pytest.mark.parametrize("shape", ["midT", "midR"])
def test_step_in_four_phases_equals_the_fused_step(shape):
    """kge_step_phase, the four phase groups in order on one stream, is kge_step_fused: same kernels, same workspace - bit for bit"""
    import ctypes as C
    from dglke_amd import _lib
    c = S.case("phase-%s-softmax" % shape, shape, rows=5e-3)
    bts = L.batches(c)
    res = {}
    for entry in ("fused", "phase"):
        eng = _engine(c, 0)
        for bt in bts:
            b = _batch(c, bt)
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
        res[entry] = [x.cpu().numpy().copy() for x in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)] + [
            np.array(eng.read_loss_sums(), np.float32)]
    sums = res["fused"][4]              # running sums: nothing is ever added to the positive / negative parts
    assert np.abs(res["fused"][1]).max() > 0 and np.isfinite(sums[2]) and sums[2] > 0 and sums[0] == 0 and sums[1] == 0
    for x, y, what in zip(res["fused"], res["phase"], ("entity table", "entity state", "relation table", "relation state", "loss sums")):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what


# --------------------------------------------------------------------------------------------------------------------------
# 5. dglke_train
# --------------------------------------------------------------------------------------------------------------------------
def _argv(data, save):
    return ["--model_name", "TransE_l2", "--format", "udd_hrt", "--dataset", "toy", "--data_path", data, "--data_files",
            "e.dict", "r.dict", "train.txt", "valid.txt", "test.txt", "--save_path", save, "--batch_size", "256",
            "--neg_sample_size", "64", "--hidden_dim", "32", "-g", "8", "--lr", "0.25", "-rc", "1e-7", "--loss_genre", "Softmax",
            "--max_step", "600", "--log_interval", "200", "--test", "--graph_steps", "100"]


def _losses(out, proc, steps=(200, 400, 600), total=600):
    """(two processes share one pipe: a line of one may end inside a line of the other)"""
    v = []
    for s in steps:
        m = re.findall(r"\[proc %d\]\[Train\]\(%d/%d\) average loss: ([0-9]+\.[0-9]+(?:e[+-]?[0-9]+)?)" % (proc, s, total), out)
        assert len(m) == 1, out[-2000:]
        v.append(float(m[0]))
    return v


def test_train_cli_with_softmax(tmp_path, capsys):
    from dglke_amd import train as T
    from test_gpu_cli import _planted
    data = str(tmp_path / "kg")
    _planted(data)
    tr = T.main(_argv(data, str(tmp_path / "ckpts")) + ["--gpu", "0"])
    out = capsys.readouterr().out
    v = _losses(out, 0)
    assert v[2] < v[1] < v[0], "the printed loss does not fall: %r" % (v,)
    assert "pos_loss" not in out and "neg_loss" not in out and "average regularization:" in out
    conf = json.load(open(os.path.join(tr.args.save_path, "config.json")))
    assert conf["loss_genre"] == "Softmax" and conf["neg_adversarial_sampling"] is False and conf["pairwise"] is False
    mrr = float([l for l in out.split("\n") if l.startswith("[0]Test average MRR:")][0].split(":")[1])
    assert mrr > 10 * 2.0 / 400, "training did not learn the planted graph (test MRR %.4f)" % mrr


def test_train_cli_with_softmax_two_processes(tmp_path):
    from test_gpu_cli import _planted
    data = str(tmp_path / "kg")
    _planted(data)
    cmd = [sys.executable, os.path.join(ROOT, "dgl-ke_amd", "dglke_train")] + _argv(data, str(tmp_path / "ckpts")) + ["--gpu", "0", "0"]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    for proc in (0, 1):
        v = _losses(out, proc)
        assert v[2] < v[1] < v[0], "proc %d: the printed loss does not fall: %r" % (proc, v)
    assert "pos_loss" not in out and "neg_loss" not in out
    saves = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp_path / "ckpts")) for f in fs if f == "config.json"]
    assert len(saves) == 1 and json.load(open(saves[0]))["loss_genre"] == "Softmax"
    mrr = float([l for l in out.split("\n") if l.startswith("[0]Test average MRR:")][0].split(":")[1])
    assert mrr > 10 * 2.0 / 400, out[-1500:]
