"""The fused step under every --loss_genre / -pw / -m / -a / -rn setting against the float64 oracle, at the shapes where the
kernels change instance (cases: tests/loss_option_cases.py; their inputs are guarded on the CPU by
tests/test_loss_option_inputs.py).

Method, as in test_fused_step_matches_oracle_at_config_shapes: two steps (tail then head corruption), the float64 oracle
restarted from the GPU's own float32 tables each step; scores, the four loss terms, the three trace gradients, both Adagrad
states and both tables (TransR: the projection table too) at the suite's tolerances.

The one exclusion - hinge flips.  Hinge's gradient is a step function of the score: a pair whose float32 score sits on the other
side of the kink than the float64 score moves its dL/dn by a whole unit.  The activity mask the kernel saw is recomputed from the
scores the step returned, in float32 (margin + n, margin - p, margin - (p - n)); the oracle's from its float64 scores; the flips
are the XOR.  Only the gradient and table rows a flipped pair feeds are excluded (whole rows: Adagrad scales the row), under
conditions that are asserted: every flip inside the score tolerance of the kink, flips <= 1e-4 of the pairs, excluded rows
<= 2 % of any compared array; the loss terms are never excluded.  Every other genre excludes nothing.  (TransE_l1 keeps the
sign-ambiguity exclusion of tests/test_gpu_parity.py::_l1_ambiguous, scaled to the magnitude of these tables.)

loss_option_errors.txt, written next to the suite's other reports (the directory of golden_row_errors.txt,
tests/test_gpu_parity.py::rows_close), records, per case and flag, the largest score, gradient and row error and the flips excluded.
"""
import os

import numpy as np
import pytest
import torch

import loss_option_cases as L
from oracle import kge_oracle as O
from test_gpu_parity import DEV, _close, _l1_ambiguous, _masked, grad_tol, rows_close

pytestmark = pytest.mark.gpu

ERRORS = {}          # "case flags" -> dict(score, grad, rows, flips, note)


def _report_dir():
    """the directory rows_close writes golden_row_errors.txt to, under the repository root: its name is taken from that function
    (its one string constant ending in `_out`) so that this report always lands beside the others"""
    names = [k for k in rows_close.__code__.co_consts if isinstance(k, str) and k.endswith("_out")]
    assert len(names) == 1, names
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), names[0])


def _record(key, **kw):
    rec = ERRORS.setdefault(key, dict(score=0.0, grad=0.0, rows=0.0, flips=0, note=""))
    for k, v in kw.items():
        rec[k] = v if k == "note" else (rec[k] + v if k == "flips" else max(rec[k], float(v)))
    try:
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "loss_option_errors.txt"), "w") as f:
            f.write("%-44s %11s %14s %11s %6s\n" % ("case flags", "max|score|", "max|grad|/gmax", "max|row|/lr", "flips"))
            for k in sorted(ERRORS):
                r = ERRORS[k]
                f.write("%-44s %11.3e %14.3e %11.3e %6d  %s\n" % (k, r["score"], r["grad"], r["rows"], r["flips"], r["note"]))
    except OSError:
        pass


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) if np.size(b) else 0.0


def _engine(c, flags):
    from dglke_amd.engine import StepEngine
    eng = StepEngine(c["model"], c["n_ent"], c["n_rel"], c["hidden"], c["gamma"], c["lr"], DEV, c["de"], c["dr"], c["adv"],
                     c["adv_temp"], c["reg_coef"], c["reg_norm"], loss_genre=c["genre"], pairwise=c["pairwise"], margin=c["margin"],
                     flags=int(flags) | (L.NEG_DEG if c["neg_deg"] else 0))
    ent, rel, proj = L.tables(c)
    eng.load_tables(ent, rel)
    if proj is not None:
        eng.proj.copy_(torch.from_numpy(proj))
        eng.proj_state.zero_()
    return eng


def _batch(c, bt):
    from dglke_amd import plan
    return plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV, bt["w"])


def _f64(t):
    return None if t is None else t.cpu().numpy().astype(np.float64)


def _union(a, b):
    return {k: sorted(set(a[k]) | set(b[k])) for k in ("slots", "edges", "pos_local", "ent", "rel")}


def run_case(c, flags):
    """two fused steps of case `c` under kernel-path flags `flags` against the float64 oracle"""
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
        # ---- scores first: they bound how far a legitimate hinge flip can sit from the kink
        gp, gn = want["pos_score"].cpu().numpy(), want["neg_score"].cpu().numpy()
        _close(gp, out["pos_score"], 1e-4, 1e-4, tag + " pos_score")
        _close(gn, out["neg_score"], 1e-4, 1e-4, tag + " neg_score")
        excl = dict(slots=[], edges=[], pos_local=[], ent=[], rel=[])
        fl = L.hinge_flips(c, bt, gp, gn, out["pos_score"], out["neg_score"])
        if fl is not None:
            L.check_flip_caps(c, bt, fl, tag)
            excl = _union(excl, fl)
        if c["model"] == "TransE_l1":
            amb = _l1_ambiguous(bt, ent0, rel0, chunk, N, tau=1.1 * 2.0 ** -24 * float(max(np.abs(ent0).max(), 1e-30)) * 2)
            assert len(amb["ent"]) <= 30 and len(amb["rel"]) <= 15, "too many sign-ambiguous rows to call this a comparison: %r" % amb
            excl = _union(excl, amb)
        # ---- loss terms: never excluded
        l4 = eng.read_loss()
        if c["pairwise"]:
            assert np.isnan(l4[0]) and np.isnan(l4[1]), tag + ": the pairwise loss has no positive / negative part"
            _close(l4[2], out["log"][2], 1e-4, 1e-5, tag + " loss")
        else:
            _close(l4[:3], out["log"][:3], 1e-4, 1e-5, tag + " loss")
        _close(l4[3], out["log"][3], 1e-3, 1e-7, tag + " reg")
        if c["reg_norm"] != 3 and c["shape"] != "fuzz":      # (the fuzz draws its coefficient blind)
            share = L.reg_share(c, out, ent0, rel0, bt)
            assert share >= 0.01, "%s: the regulariser is %.3g of the largest gradient component - the case does not test it" % (tag, share)
        # ---- the three trace gradients
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
        # ---- Adagrad states and rows
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
        _record(key, score=max(_err(gp, out["pos_score"]), _err(gn, out["neg_score"])), grad=gerr, rows=rows_err / lr,
                flips=0 if fl is None else fl["n_flips"])
    return eng


_MATRIX = [pytest.param(c, f, id="%s-f%d" % (c["id"], f)) for c in L.CASES for f in c["flags"]]


@pytest.mark.parametrize("c,flags", _MATRIX)
def test_fused_step_under_loss_options_matches_oracle(c, flags):
    """every accepted kernel-path flag must give oracle-equal results; nothing is asserted about which path ran (the library
    falls back by itself where a path does not carry an option, e.g. the fused loss for the pairwise forms)"""
    run_case(c, flags)


@pytest.mark.parametrize("seed", range(int(os.environ.get("KGE_LOSS_FUZZ_N", "48"))))      # KGE_LOSS_FUZZ_N=500 for a longer hunt
def test_fused_step_random_loss_options_match_oracle(seed):
    """fuzz over the option axes at small ragged shapes: genre, pairwise where legal, margin 0.5 / 1 / 2, adversarial temperature
    0.5 / 1 / 2, reg_norm 1 - 4, edge importance, --neg_deg_sample, kernel-path flags"""
    c = L.fuzz_case(seed)
    run_case(c, c["flags"][0])


# ------------------------------------------------------------------------------------------------------------------------
# the other step entry points
# ------------------------------------------------------------------------------------------------------------------------
def _small_hinge_case(cid, model, reg_coef, **over):
    """Hinge + -adv (temperature 0.5) with reg_norm 2 on tables scaled to straddle the kink; reg_coef: per model and batch size, so
    that the regulariser is ~5 % of the largest gradient component (asserted >= 1 %)"""
    shape = {"TransE_l2": "midT", "DistMult": "midD", "RotatE": "midR"}[model]
    return L.case(cid, shape, "Hinge", adv=True, adv_temp=0.5, reg_norm=2, reg_coef=reg_coef, rows=5e-3, **over)


@pytest.mark.parametrize("model,reg_coef", [("TransE_l2", 1e-4), ("DistMult", 1e-3), ("RotatE", 3e-3)])
def test_async_pipeline_under_hinge_adv_reg2_matches_the_stale_oracle(model, reg_coef):
    """kge_step_async (UPDATE(s-1) under SCORE(s)) with Hinge, -adv at temperature 0.5 and reg_norm 2 against
    oracle.train_steps_async, as tests/test_gpu_async.py does for the default options: 80 entities, so that every step
    re-touches rows and the staleness shows"""
    c = _small_hinge_case("async-" + model, model, reg_coef, n_ent=80, n_rel=5, B=32, chunk=16, N=16)
    cfg = L.config(c)
    ent, rel, _ = L.tables(c)
    bts = L.batches(c, steps=5)
    for bt in bts:
        bt.update(chunk=c["chunk"], N=c["N"])
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    es, rs = np.zeros(len(ent)), np.zeros(len(rel))
    outs = O.train_steps_async(cfg, e64, es, r64, rs, bts)
    assert any(L.activity_ok(c, o["pos_score"], o["neg_score"]) for o in outs), "the hinge is not exercised"
    assert L.reg_share(c, outs[0], ent, rel, bts[0]) >= 0.01, "the regulariser does not show in the gradients"
    s64, sr64, ses, srs = ent.astype(np.float64), rel.astype(np.float64), np.zeros(len(ent)), np.zeros(len(rel))
    for bt in bts:
        L.oracle_step(c, s64, ses, sr64, srs, None, None, bt)
    assert np.abs(s64 - e64).max() > 1e-3 * c["lr"], "strict and async oracles agree: the batches do not overlap"
    eng = _engine(c, 0)
    eng.steps_async([_batch(c, bt) for bt in bts])
    torch.cuda.synchronize()
    tag = "async " + model
    _close(eng.ent_state.cpu(), es, 2e-3, 1e-9, tag + " entity state")
    _close(eng.rel_state.cpu(), rs, 2e-3, 1e-9, tag + " relation state")
    _close(eng.ent.cpu(), e64, 1e-4, 1e-2 * c["lr"], tag + " entity table")
    _close(eng.rel.cpu(), r64, 1e-4, 1e-2 * c["lr"], tag + " relation table")
    assert np.abs(_f64(eng.ent) - s64).max() > 1e-3 * c["lr"]          # ... and NOT the strict result
    _record("async-%s f0" % model, rows=max(_err(eng.ent.cpu(), e64), _err(eng.rel.cpu(), r64)) / c["lr"], note="5 stale steps, final tables")


def test_sharded_engine_world1_under_hinge_adv_reg2_equals_fused_step():
    """DistEngine at world 1 (route -> pull -> kge_step_grads -> push -> merged apply: the gradient-emitting instance of the update
    kernel with a run-time norm) against the fused step, as test_sharded_engine_world1_equals_fused_step does for the defaults"""
    import torch.distributed as dist
    from dglke_amd import dist as kd
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29547")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        for model, reg_coef in (("TransE_l2", 2e-5), ("DistMult", 2e-4), ("RotatE", 6e-4)):
            c = _small_hinge_case("dist-" + model, model, reg_coef, B=128, chunk=32, N=32, n_rel=40)
            ent_np, rel_np, _ = L.tables(c)
            bts = L.batches(c, steps=3)
            p64, n64 = L.oracle_scores(c, ent_np.astype(np.float64), rel_np.astype(np.float64), None, bts[0])
            assert L.activity_ok(c, p64, n64), "the hinge is not exercised: %r" % (L.activity(c, p64, n64),)
            out0 = L.oracle_forward_backward(c, ent_np.astype(np.float64), rel_np.astype(np.float64), None, bts[0])
            assert L.reg_share(c, out0, ent_np, rel_np, bts[0]) >= 0.01, "the regulariser does not show in the gradients"
            a = _engine(c, 0)
            b = _engine(dict(c, n_ent=1), 0)
            b.rel.copy_(a.rel)
            ent = a.ent.clone()
            state = torch.zeros(c["n_ent"], device=DEV)
            deng = kd.DistEngine(b, kd.ShardSpec(c["n_ent"], 1, 0), ent, state)
            for bt in bts:
                a.step(_batch(c, bt))
                gb = _batch(c, bt)                                    # GLOBAL ids
                gb.UE = 2 * c["B"] + (c["B"] // c["chunk"]) * c["N"]    # the engine sizes its buffers once, for the bound
                deng.step(gb)
            assert deng.check_overflow() == 0
            torch.cuda.synchronize()
            assert float((a.ent_state > 0).sum()) > 100
            _close(ent.cpu(), a.ent.cpu(), 1e-5, 5e-6, model + " sharded entity table")
            _close(state.cpu(), a.ent_state.cpu(), 1e-5, 1e-8, model + " sharded entity state")
            _close(b.rel.cpu(), a.rel.cpu(), 1e-5, 5e-6, model + " relation table")
            _close(b.rel_state.cpu(), a.rel_state.cpu(), 1e-5, 1e-8, model + " relation state")
            _close(b.read_loss_sums(), a.read_loss_sums(), 1e-5, 1e-6, model + " loss sums")
            _record("dist-%s f0" % model, rows=_err(ent.cpu(), a.ent.cpu()) / c["lr"], note="world-1 DistEngine vs fused step")
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------------------
# Logistic against Logsigmoid: the same arithmetic (-logsigmoid(l s) == softplus(-l s)), but Logistic selects the generic
# (non-LEAN) instance of edge_fwd, of the merged forward launch, of the loss kernel and of neg_fwd_bcast_with_edge - also
# WITHOUT per-step outputs, which no other test runs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["cfgT", "cfgD", "rotate", "l1"])
def test_logistic_equals_logsigmoid_without_per_step_outputs(shape):
    res = {}
    base = L.case(shape + "-lean", shape, "Logsigmoid", adv=True, reg_coef=1e-9)
    bts = L.batches(base, steps=4)
    for genre in ("Logsigmoid", "Logistic"):
        c = dict(base, genre=genre)
        eng = _engine(c, 0)
        for bt in bts:
            eng.step(_batch(c, bt))
        torch.cuda.synchronize()
        res[genre] = [_f64(eng.ent), _f64(eng.rel), _f64(eng.ent_state), _f64(eng.rel_state), np.array(eng.read_loss_sums(), np.float64)]
    lr = base["lr"]
    ref, got = res["Logsigmoid"], res["Logistic"]
    assert np.isfinite(ref[4]).all() and np.abs(ref[4][:3]).min() > 0 and np.abs(ref[2]).max() > 0
    same = all(np.array_equal(x, y) for x, y in zip(ref, got))
    errs = [_err(x, y) for x, y in zip(got, ref)]
    _record("logistic-vs-logsigmoid %s" % shape, rows=max(errs[0], errs[1]) / lr,
            note="4 steps without outputs: %s" % ("bit-identical" if same else "NOT bit-identical, max differences %r" % (errs,)))
    for k, what in enumerate(("entity table", "relation table", "entity state", "relation state", "loss sums")):
        # the bound of test_loss_rows_inside_the_first_launch_equal_the_loss_launch for instance-to-instance rounding
        tol = 1e-4 * lr if k < 2 else 2e-5 * np.abs(ref[k]).max()
        assert errs[k] <= tol, "%s %s: Logistic differs from Logsigmoid by %.3e (bound %.3e)" % (shape, what, errs[k], tol)
