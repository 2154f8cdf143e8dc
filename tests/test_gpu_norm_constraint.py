"""GPU tests of the norm constraints (KGE_FLAG_ENT_NORM_* / KGE_FLAG_REL_NORM_*, csrc/kge_constrain.hip; dglke_train --ent_norm /
--rel_norm) against the float64 statement of tests/norm_constraint_cases.py: the value test of every case (widths on both sides of
every instance boundary and on both access paths, record counts below one workgroup and over several, host- and device-built plans,
every model with more than one slice, Adam, the known-triple entry, the sampler tail), the four phase calls against the fused
call, graph replay against eager steps, the invariant after 20 steps, and a cut and resumed run through the command line.
The largest |x - x64| / (|x64| (p + 8) 2^-24) of every case goes to norm_constraint_errors.txt in the suite's report directory."""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

import norm_constraint_cases as Q
from test_gpu_loss_options import _report_dir
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))      # planted_kg (train_loop_cases)
RATIOS = {}
T0 = time.time()


def _record(cid, stats):
    RATIOS[cid] = stats
    try:
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "norm_constraint_errors.txt"), "w") as f:
            f.write("norm constraints against float64: per case the compared slices of the batch's union (scaled / not scaled / ambiguous and "
                    "left out) and the\nlargest |x - x64| / (|x64| (p + 8) 2^-24) over the elements of the scaled slices (<= 1 passes)\n"
                    "(wall time of this file up to the last record: %.0f s)\n" % (time.time() - T0))
            f.write("worst: %.4f (%s)\n" % max((v[4], k) for k, v in RATIOS.items()))
            for k in sorted(RATIOS):
                f.write("%-24s slices %4d  scaled %4d  not scaled %4d  ambiguous %d  ratio %.4f\n" % ((k,) + tuple(RATIOS[k])))
    except OSError:
        pass


def _engine(c, constrained=True, fresh=False, **kw):
    from dglke_amd import _lib
    from dglke_amd.engine import StepEngine
    eng = StepEngine(c["model"], c["n_ent"], c["n_rel"], c["hidden"], c["gamma"], c["lr"], DEV, c["de"], c["dr"], c["adv"], c["adv_temp"],
                     c["reg_coef"], c["reg_norm"], c["genre"], c["pairwise"], c["margin"], optimizer=c["optimizer"],
                     ent_norm=c["ent_norm"] if constrained else None, rel_norm=c["rel_norm"] if constrained else None, **kw)
    want = (Q.FLAGS["ent"][c["ent_norm"]] | Q.FLAGS["rel"][c["rel_norm"]]) if constrained else 0
    assert eng.hp.flags == want and want == (eng.hp.flags & (_lib.FLAG_ENT_NORM_CLIP | _lib.FLAG_ENT_NORM_UNIT | _lib.FLAG_REL_NORM_CLIP |
                                                           _lib.FLAG_REL_NORM_UNIT))
    if not fresh:
        eng.load_tables(*Q.tables(c))           # (not projected: the union's rows are, by the step)
    return eng


def _host_batch(c, bt):
    from dglke_amd import plan
    return plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV)


def _sampler(c, seed=Q.SAMPLER_SEED):
    from dglke_amd.dataloader import DeviceSampler
    H, R, T = Q.sampler_triples(c)
    return DeviceSampler(H, R, T, c["n_ent"], c["B"], c["N"], DEV, n_slots=2, neg_chunk_size=c["chunk"], seed=seed, shuffle=False)


def _tensors(eng):
    torch.cuda.synchronize()
    return {k: t.detach().cpu().numpy().copy() for k, t in eng.named_tensors().items()}


def _one_step(c, constrained):
    """one step of case c from its tables -> (named tensors after it, the batch as ids, extra bytes to compare between the two runs)"""
    eng = _engine(c, constrained)
    bt = Q.batch(c)
    extra = None
    if c["plan"] == "device":
        smp = _sampler(c)
        b = smp.sample(1)[0]
        torch.cuda.synchronize()
        sl = smp.slot_arrays(0)
        for k, name in (("h", "h_gid"), ("t", "t_gid"), ("r", "rel_ids"), ("neg", "neg_ids")):
            assert np.array_equal(sl[name], bt[k]), "the device batch is not the statement's"
        ue, ur = int(sl["counts"][0]), int(sl["counts"][1])
        assert ue < b.UE and ur < b.UR, "the counts of the device-built plan do not stay below the bounds"
        assert np.array_equal(sl["ue_id"][:ue], Q.union(bt)[0]) and np.array_equal(np.sort(sl["ur_id"][:ur]), Q.union(bt)[1])
        if c["entry"] == "tail":       # this step's launches also build the first batch of another sampler's sequence
            other = _sampler(c, Q.SAMPLER_SEED + 1)
            jobs, _ = other.tail_jobs(1)
            eng.step(b, sample_job=jobs[0])
            torch.cuda.synchronize()
            extra = other.slots.cpu().numpy().copy()
        else:
            eng.step(b)
    else:
        if c["entry"] == "known":
            from dglke_amd.known import KnownIndex
            eng.attach_known(KnownIndex(Q.known_of(c, bt)[1], c["n_ent"], c["n_rel"], DEV))
        eng.step(_host_batch(c, bt))
    return _tensors(eng), bt, extra


@pytest.mark.parametrize("c", Q.CASES, ids=lambda c: c["id"])
def test_updated_rows_are_projected_and_nothing_else_moves(c):
    """the three checks of the value test (norm_constraint_cases.compare) on both tables, the mix of scaled and unscaled slices, and
    every other tensor of the engine - Adagrad state, Adam moments and counts - bit for bit the unconstrained engine's"""
    T, bt, extra_t = _one_step(c, False)
    X, _, extra_x = _one_step(c, True)
    ids_e, ids_r = Q.union(bt)
    start = dict(zip(("entity", "relation"), Q.tables(c)))
    assert not np.array_equal(T["entity"][ids_e], start["entity"][ids_e]), "the step did not move the union's rows"
    stats = [Q.compare(c, "ent", T["entity"], X["entity"], ids_e), Q.compare(c, "rel", T["relation"], X["relation"], ids_r)]
    tot, scaled, unscaled, exempt = Q.check_mix(c, stats)
    ratio = max(s["ratio"] for s in stats)
    print("%s: %d slices, %d scaled, %d not, %d ambiguous, largest error / bound %.4f" % (c["id"], tot, scaled, unscaled, exempt, ratio))
    _record(c["id"], (tot, scaled, unscaled, exempt, ratio))
    assert ratio <= 1.0, "%s: %.3f bounds off" % (c["id"], ratio)
    others = sorted(set(T) - {"entity", "relation"})
    assert len(others) == (4 if c["optimizer"] == "Adam" else 2)
    for k in others:
        assert np.array_equal(T[k].view(np.uint32), X[k].view(np.uint32)), "%s: %s differs from the unconstrained engine's" % (c["id"], k)
        assert np.abs(T[k]).max() > 0
    if c["entry"] == "tail":
        assert extra_t is not None and extra_t.any() and np.array_equal(extra_t, extra_x), "the batch the tail job built differs"
    if c["id"] == "transh-h8":      # d clipped, w of length 1 whatever the relation mode
        k = c["hidden"]
        rel = X["relation"][ids_r].astype(np.float64)
        nd, nw = np.sqrt((rel[:, :k] ** 2).sum(-1)), np.sqrt((rel[:, k:] ** 2).sum(-1))
        assert np.all(np.abs(nw - 1) <= Q.slack(k)) and np.all(nd <= 1 + Q.slack(k)) and (nd < 0.95).any()
        before = np.sqrt((T["relation"][ids_r].astype(np.float64)[:, k:] ** 2).sum(-1))
        assert (before < 0.95).any() and (before > 1.05).any()


def _steps(c, how, n_batches=3):
    eng = _engine(c)
    batches = [_host_batch(c, Q.batch(c, s)) for s in range(1, n_batches + 1)]
    if how == "fused":
        for b in batches:
            eng.step(b)
    elif how == "phases":
        for b in batches:
            eng.step_timed(b)
    elif how == "eager-twice":
        for b in batches + batches:
            eng.step(b)
    else:
        g = eng.capture(batches)
        g.replay()
        g.replay()
    return _tensors(eng)


@pytest.mark.parametrize("cid", ["transd-h8", "distmult-adam"])
def test_four_phase_calls_equal_the_fused_call(cid):
    """kge_step_phase (Adam: kge_step_optim with a phase mask), four groups in order: the constraint launch belongs to UPDATE"""
    c = Q.by_id(cid)
    a, b = _steps(c, "fused"), _steps(c, "phases")
    plain = _tensors(_engine(c))
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s: %s" % (cid, k)
        assert not np.array_equal(a[k], plain[k])
    e = a["entity"].astype(np.float64).reshape(c["n_ent"], len(Q.slice_modes(c, "ent")), -1)
    assert np.all(np.sqrt((e * e).sum(-1))[np.unique(np.concatenate([Q.union(Q.batch(c, s))[0] for s in (1, 2, 3)]))] <= 1 + Q.slack(e.shape[-1]))


def test_three_steps_replayed_twice_equal_six_eager_steps():
    c = Q.by_id("transd-h8")
    a, b = _steps(c, "eager-twice"), _steps(c, "graph")
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("mode", ["unit", "clip"])
def test_every_slice_satisfies_the_constraint_after_20_steps(mode):
    """from fresh tables, which the engine projects whole once (gamma 12: their rows start at norms around 2): under unit every slice
    of every row, touched or not, has a norm within (p + 8) 2^-24 of 1; under clip none is above 1 by more than that"""
    c = dict(Q.by_id("transd-h8"), ent_norm=mode, rel_norm=mode, gamma=12.0, lr=0.1)
    from dglke_amd.engine import StepEngine
    torch.manual_seed(7)
    raw = StepEngine(c["model"], c["n_ent"], c["n_rel"], c["hidden"], c["gamma"], c["lr"], DEV, c["de"], c["dr"])
    torch.manual_seed(7)
    eng = _engine(c, fresh=True)
    p = c["hidden"]

    def norms(t):
        x = t.detach().cpu().numpy().astype(np.float64)
        return np.sqrt((x.reshape(x.shape[0], 2, p) ** 2).sum(-1))
    n_raw = norms(raw.ent)
    assert (n_raw > 1.0).mean() > 0.9, "the fresh rows start outside the ball"
    # the projection of the fresh tables is the statement on the unprojected initialisation
    want = Q.project64(raw.ent.cpu().numpy(), [mode, mode])[0]
    assert np.allclose(eng.ent.cpu().numpy(), want, rtol=1e-6, atol=0)
    for s in range(1, 21):
        eng.step(_host_batch(c, Q.batch(c, s)))
    torch.cuda.synchronize()
    for t in (eng.ent, eng.rel):
        n = norms(t)
        assert np.isfinite(n).all()
        if mode == "unit":
            assert np.all(np.abs(n - 1) <= Q.slack(p)), float(np.abs(n - 1).max())
        else:
            assert np.all(n <= 1 + Q.slack(p)), float(n.max())
    assert not torch.equal(eng.ent, torch.from_numpy(want.astype(np.float32)).to(DEV)), "20 steps moved nothing"
    # reset_parameters projects too
    eng.reset_parameters()
    n = norms(eng.ent)
    assert np.all(n <= 1 + Q.slack(p)) and (mode == "clip" or np.all(np.abs(n - 1) <= Q.slack(p)))


def test_library_refuses_the_flags_where_there_is_no_launch_behind_the_update():
    """the engine hands the library's refusal on: the stale pipeline, with tables on the device"""
    from dglke_amd import _lib
    c = Q.by_id("l2-w256")
    eng = _engine(c)
    b = _host_batch(c, Q.batch(c))
    with pytest.raises(_lib.KgeError, match="kge_step_async.*KGE_FLAG_ENT_NORM_CLIP"):
        eng.step_async(b)
    with pytest.raises(_lib.KgeError, match="rel_norm is not available for RotatE"):
        from dglke_amd.engine import StepEngine
        StepEngine("RotatE", 10, 2, 8, 4.0, 0.1, DEV, True, False, rel_norm="clip")


def test_resumed_run_with_constraints_ends_with_the_uninterrupted_runs_tables(tmp_path, capsys):
    """run A: --max_step 230; B1: --max_step 45 --checkpoint_interval 45; B2: --resume B1 --max_step 230 (the protocol of
    tests/checkpoint_cases.py) with --ent_norm clip --rel_norm clip on TransD.  B2's tables and Adagrad states are A's, bit for bit;
    config.json records the two flags; the [Train] lines name them; every row ends inside the ball"""
    import checkpoint_cases as CK
    import train_loop_cases as L
    from dglke_amd import train as T
    c = ("norm", "TransD", ["-de", "-dr", "--ent_norm", "clip", "--rel_norm", "clip"], False, [45], (20, 20))
    data = str(tmp_path / "kg")
    L.write_planted(data)

    def run(argv, before_train=None):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            tr = T.main(argv, before_train=before_train)
        torch.cuda.synchronize()
        return tr, {n_: t.detach().cpu().clone() for n_, t in tr.model.engine.named_tensors().items()}, buf.getvalue()
    tr_a, a, out_a = run(CK.argv_a(c, data, str(tmp_path / "a")))
    tr_b1, b1, _ = run(CK.argv_b(c, data, str(tmp_path / "b1"), 0))
    b1_dir = tr_b1.args.save_path
    assert os.path.isdir(os.path.join(b1_dir, "checkpoint"))
    _, b2, out_b2 = run(CK.argv_b(c, data, str(tmp_path / "b2"), 1, b1_dir))
    assert sorted(a) == sorted(b2) and len(a) == 4
    for name in sorted(a):
        assert not torch.equal(a[name], b1[name]), "%s: nothing was trained after step 45" % name
        assert torch.equal(a[name], b2[name]), "%s: the resumed run differs from the uninterrupted run" % name
    conf = json.load(open(os.path.join(tr_a.args.save_path, "config.json")))
    assert conf["ent_norm"] == "clip" and conf["rel_norm"] == "clip"
    assert "[Train] --ent_norm clip, --rel_norm clip" in out_a and ", --ent_norm clip, --rel_norm clip" in out_a
    assert not [l for l in out_b2.split("\n") if l.startswith("--resume: --ent_norm") or l.startswith("--resume: --rel_norm")]
    p = tr_a.args.hidden_dim
    for name in ("entity", "relation"):
        x = a[name].numpy().astype(np.float64)
        n = np.sqrt((x.reshape(x.shape[0], 2, p) ** 2).sum(-1))
        assert np.all(n <= 1 + Q.slack(p)), (name, float(n.max()))
    assert tr_a.model.engine.hp.flags & 2048 and tr_a.model.engine.hp.flags & 8192
    # the flags may differ from the checkpointed run's: the command line wins, one line per changed flag, and the restored tables are
    # not projected (under `unit` the clipped rows of B1, most of them inside the ball, would all move)
    seen = {}

    def hook(trainer):
        torch.cuda.synchronize()
        seen.update({n_: t.detach().cpu().clone() for n_, t in trainer.model.engine.named_tensors().items()})
    tr_b3, b3, out_b3 = run(CK.argv_b(c, data, str(tmp_path / "b3"), 1, b1_dir, extra=["--ent_norm", "unit", "--rel_norm", "none"]), hook)
    assert "--resume: --ent_norm was 'clip' in the checkpointed run, is 'unit' now" in out_b3
    assert "--resume: --rel_norm was 'clip' in the checkpointed run, is 'none' now" in out_b3
    for name in sorted(b1):
        assert torch.equal(seen[name], b1[name]), "%s: the restored table is not the checkpoint's" % name
    n1 = np.sqrt((b1["entity"].numpy().astype(np.float64).reshape(-1, 2, p) ** 2).sum(-1))
    assert (n1 < 0.99).any(), "B1 holds slices inside the ball: a projection of the restored tables under unit would have moved them"
    assert tr_b3.model.engine.hp.flags & (2048 | 4096 | 8192 | 16384) == 4096
    conf = json.load(open(os.path.join(tr_b3.args.save_path, "config.json")))
    assert conf["ent_norm"] == "unit" and conf["rel_norm"] == "none"
    assert "[Train] --ent_norm unit, --rel_norm none" in out_b3
    n3 = np.sqrt((b3["entity"].numpy().astype(np.float64).reshape(-1, 2, p) ** 2).sum(-1))
    moved = (b3["entity"] != b1["entity"]).reshape(-1, 2, p).any(-1).numpy()
    assert moved.any() and np.all(np.abs(n3[moved] - 1) <= Q.slack(p)), "rows trained after the restart are on the sphere"
    assert not torch.equal(b3["entity"], b2["entity"])
