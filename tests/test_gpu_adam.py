"""--optimizer Adam on the device: kge_step_optim (include/kge_hip.h) and the Adam instances of the register-resident update
(csrc/kge_adam.hip) against the float64 statement of tests/adam_cases.py - parity over four consecutive steps on host-built and
device-built plans, preloaded state, the Adagrad kind and the phase groups bit for bit, the stream and workspace contracts of the
new entry, its refusals, and dglke_train --optimizer Adam on the planted toy graph.

The comparison is step by step (adam_cases.py, THE COMPARISON): before every step the device's tables, moments and counts are read
back and the statement takes its step from exactly that state.  Tolerances are the suite's (modular_op_cases.grad_tol): updated
rows and each moment array within 3e-4 of the compared array's largest component + 3e-4 relative; counts, and every row the step
does not touch, exact.  adam_errors.txt, written next to the suite's other reports, records per case and quantity the largest
error next to its bound and the share of elements the ambiguity rule took out."""
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import pytest
import torch

import adam_cases as A
from test_gpu_loss_options import _report_dir
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ERRORS = {}          # case -> {quantity: (err / bound, err, bound)}
AMBIG = {}           # case -> {table: share}
T0 = time.time()
KEYS = ("ent", "rel", "ent_mom", "rel_mom", "ent_state", "rel_state")


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """a lost GPU context fails every later call: end the session instead of running the rest of the file against it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU context is lost (%s): nothing more is run" % (e,), returncode=3)


def _record(case, amb=None, **q):
    rec = ERRORS.setdefault(case, {})
    for k, v in q.items():
        if k not in rec or v[0] >= rec[k][0]:
            rec[k] = v
    if amb:
        AMBIG[case] = amb
    try:
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "adam_errors.txt"), "w") as f:
            f.write("kge_step_optim, KGE_OPT_ADAM, against the float64 statement, step by step: largest |error| / bound per case and "
                    "quantity (<= 1 passes), that error, its bound; share of elements left out as ambiguous\n"
                    "(wall time of this file up to the last record: %.0f s)\n" % (time.time() - T0))
            top = max(((v[0], c, k) for c, r in ERRORS.items() for k, v in r.items()), default=None)
            if top:
                f.write("worst: %.4f of its bound (%s %s)\n" % top)
            for c in sorted(ERRORS):
                f.write("%s%s\n" % (c, "".join("   ambiguous %s %.4f" % kv for kv in sorted(AMBIG.get(c, {}).items()))))
                for k in sorted(ERRORS[c]):
                    f.write("    %-10s err/bound %8.4f   err %.3e   bound %.3e\n" % ((k,) + tuple(ERRORS[c][k])))
    except OSError:
        pass


# --------------------------------------------------------------------------------------------------------------------------
# engines, batches, state
# --------------------------------------------------------------------------------------------------------------------------
def _engine(c, optimizer="Adam", **kw):
    from dglke_amd import _lib
    from dglke_amd.engine import StepEngine
    return StepEngine(c["model"], c["n_ent"], c["n_rel"], c["hidden"], c["gamma"], c["lr"], DEV, c["de"], c["dr"], c["adv"],
                      c["adv_temp"], c["reg_coef"], c["reg_norm"], c["genre"], c["pairwise"], c["margin"],
                      flags=_lib.FLAG_NEG_DEG_SAMPLE if c["neg_deg"] else 0, optimizer=optimizer, **kw)


def _batch(c, bt):
    from dglke_amd import plan
    w = None if bt.get("w") is None else bt["w"].astype(np.float32)
    return plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV, edge_w=w)


def _state(eng):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).detach().cpu().numpy().copy() for k in KEYS if getattr(eng, k, None) is not None}


def _f64(st):
    return dict(ent=st["ent"].astype(np.float64), rel=st["rel"].astype(np.float64), ent_mom=st["ent_mom"].astype(np.float64),
                rel_mom=st["rel_mom"].astype(np.float64), ent_cnt=st["ent_state"].astype(np.float64),
                rel_cnt=st["rel_state"].astype(np.float64))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_state(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), "%s: %s differs (%d elements)" % (what, k, int((_bits(a[k]) != _bits(b[k])).sum()))


def _compare_step(cid, before, after, ref, info, amb, s):
    """one step: after (device) against ref (the statement from `before`); amb: the running ambiguity masks"""
    errs = {}
    for tab, cnt in (("ent", "ent_state"), ("rel", "rel_state")):
        ids = info[tab][0]
        un = np.setdiff1d(np.arange(before[tab].shape[0]), ids)
        for k in (tab, tab + "_mom", cnt):
            assert np.array_equal(_bits(before[k][un]), _bits(after[k][un])), "%s step %d: untouched rows of %s changed" % (cid, s, k)
        assert np.array_equal(after[cnt][ids].astype(np.float64), ref[tab + "_cnt"][ids]), "%s step %d: counts of %s" % (cid, s, tab)
        keep = ~amb[tab][ids]
        for name, got, want in ((tab, after[tab][ids], ref[tab][ids]), (tab + "_m", after[tab + "_mom"][ids, 0], ref[tab + "_mom"][ids, 0]),
                                (tab + "_v", after[tab + "_mom"][ids, 1], ref[tab + "_mom"][ids, 1])):
            err, bound = np.abs(got.astype(np.float64) - want), A.tol(want)
            assert np.isfinite(got).all(), (cid, s, name)
            ratio = np.where(keep, err / bound, 0.0)
            i = np.unravel_index(np.argmax(ratio), ratio.shape)
            errs[name] = (float(ratio[i]), float(err[i]), float(bound[i]))
    return errs


def _run_parity(c, steps=A.STEPS, preload=None, bts=None):
    """-> the final device state; asserts every step"""
    from dglke_amd.known import KnownIndex
    ent, rel = A.tables(c)
    eng = _engine(c)
    eng.load_tables(ent, rel, **{k: torch.from_numpy(v) for k, v in (preload or {}).items()})
    amb = dict(ent=np.zeros(ent.shape, bool), rel=np.zeros(rel.shape, bool))
    moved = 0.0
    for s, bt in enumerate(bts or A.batches(c, steps), 1):
        known = None
        if c["known"]:
            known, K = A.known_pairs(c, bt)
            eng.attach_known(KnownIndex(K, c["n_ent"], c["n_rel"], DEV))
        before = _state(eng)
        eng.step(_batch(c, bt))
        after = _state(eng)
        ref = _f64(before)
        info = A.step(c, ref, bt, known)
        for tab in ("ent", "rel"):
            amb[tab] |= A.ambiguous(info[tab][0], info[tab][1], amb[tab].shape[0])
            assert amb[tab].mean() <= A.AMBIGUITY_CAP, "%s step %d: %.4f of %s is ambiguous" % (c["id"], s, amb[tab].mean(), tab)
        errs = _compare_step(c["id"], before, after, ref, info, amb, s)
        for k, v in errs.items():
            print("%s step %d %-6s err/bound %.4f  err %.3e  bound %.3e" % ((c["id"], s, k) + v))
        _record(c["id"], amb={t: float(amb[t].mean()) for t in amb}, **errs)
        for k, (ratio, err, bound) in errs.items():
            assert ratio <= 1.0, "%s step %d %s: %.2f bounds off (error %.3e, bound %.3e)" % (c["id"], s, k, ratio, err, bound)
        moved = max(moved, float(np.abs(after["ent"] - before["ent"]).max()))
    assert moved > 0.5 * c["lr"], "the tables hardly moved (%.3e)" % moved
    return after


# --------------------------------------------------------------------------------------------------------------------------
# parity on host-built plans
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c["id"])
def test_four_steps_match_the_statement(c):
    _run_parity(c)


@pytest.mark.parametrize("cid", sorted(A.PRELOAD_CASES))
def test_preloaded_counts_and_moments(cid):
    """counts 0, 1, 1000, 2^24 - 1 and 2^24 (saturated: stays) over the rows, non-zero moments"""
    c = A.by_id(cid)
    after = _run_parity(c, steps=2, preload=A.preloaded(c, A.PRELOAD_CASES[cid]))
    assert after["ent_state"].max() == 2.0 ** 24 and after["rel_state"].max() <= 2.0 ** 24


def test_inactive_hinge_step_leaves_rows_and_moments_and_counts_the_touched_rows():
    """every margin inactive (-m very negative, -rc 0): all gradients are exactly 0 - rows bit-identical, moments stay 0, counts
    of the touched rows + 1"""
    c = A.case("l2-hinge-inactive", "TransE_l2", 16, genre="Hinge", margin=-1e4)
    d = A.case("distmult-hinge-inactive", "DistMult", 16, genre="Hinge", margin=-1e4)
    for c in (c, d):
        ent, rel = A.tables(c)
        eng = _engine(c)
        eng.load_tables(ent, rel)
        bt = A.batches(c, 1)[0]
        before = _state(eng)
        eng.step(_batch(c, bt))
        after = _state(eng)
        assert np.array_equal(_bits(before["ent"]), _bits(after["ent"])) and np.array_equal(_bits(before["rel"]), _bits(after["rel"]))
        assert not after["ent_mom"].any() and not after["rel_mom"].any()
        want_e, want_r = np.zeros(c["n_ent"], np.float32), np.zeros(c["n_rel"], np.float32)
        want_e[np.union1d(bt["nid"], bt["neg"])] = 1
        want_r[np.unique(bt["r"])] = 1
        assert np.array_equal(after["ent_state"], want_e) and np.array_equal(after["rel_state"], want_r)


# --------------------------------------------------------------------------------------------------------------------------
# device-built plans
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["TransE_l2", "DistMult"])
@pytest.mark.parametrize("long_list", [False, True], ids=["short-lists", "long-list"])
def test_device_built_plans_match_the_statement(model, long_list):
    """batches of a DeviceSampler, ids read back from the slots.  long-list: one relation carries most triples - the batch's longest
    relation list is beyond the shared-list threshold and the shared-list relation instance runs; short-lists: 40 relations over
    32 edges - the plain instance"""
    from dglke_amd.dataloader import DeviceSampler
    n_rel = 3 if long_list else 40
    c = A.case("dev-%s-%s" % (model, "long" if long_list else "short"), model, 16, n_ent=48, n_rel=n_rel, adv=True)
    rng = np.random.RandomState(11)
    n_train = 400
    h, t = rng.randint(0, c["n_ent"], n_train), rng.randint(0, c["n_ent"], n_train)
    r = np.where(rng.rand(n_train) < 0.9, 0, rng.randint(0, n_rel, n_train)) if long_list else np.arange(n_train) % n_rel
    smp = DeviceSampler(h, r, t, c["n_ent"], c["B"], c["N"], DEV, n_slots=4, neg_chunk_size=c["chunk"], seed=3)
    ent, rel = A.tables(c)
    eng = _engine(c)
    eng.load_tables(ent, rel)
    dbs = smp.sample(4)
    torch.cuda.synchronize()
    amb = dict(ent=np.zeros(ent.shape, bool), rel=np.zeros(rel.shape, bool))
    thr = A.rel_shared_threshold(*reversed(A.widths(c)))
    for s, db in enumerate(dbs, 1):
        sl = smp.slot_arrays(db.slot)
        bt = A._finish(dict(h=sl["h_gid"], t=sl["t_gid"], r=sl["rel_ids"], neg=sl["neg_ids"], neg_head=bool(sl["counts"][2]), w=None), c["B"])
        longest = int(np.bincount(bt["r"]).max())
        # (counts[3]: the longest relation list when it is longer than 8 edges, else 0 - csrc/kge_sampler_kernel.hpp)
        assert sl["counts"][3] == (longest if longest > 8 else 0) and (longest - 1 >= thr) == long_list, (longest, sl["counts"])
        before = _state(eng)
        eng.step(db)
        after = _state(eng)
        ref = _f64(before)
        info = A.step(c, ref, bt)
        for tab in ("ent", "rel"):
            amb[tab] |= A.ambiguous(info[tab][0], info[tab][1], amb[tab].shape[0])
            assert amb[tab].mean() <= A.AMBIGUITY_CAP, (c["id"], tab, amb[tab].mean())
        errs = _compare_step(c["id"], before, after, ref, info, amb, s)
        _record(c["id"], amb={k: float(amb[k].mean()) for k in amb}, **errs)
        for k, (ratio, err, bound) in errs.items():
            assert ratio <= 1.0, "%s step %d %s: %.2f bounds off (error %.3e, bound %.3e)" % (c["id"], s, k, ratio, err, bound)


# --------------------------------------------------------------------------------------------------------------------------
# the entry itself
# --------------------------------------------------------------------------------------------------------------------------
def _out(eng):
    from dglke_amd import _lib
    out = _lib.KgeStepOut()
    out.loss_accum, out.tickets = _lib.ptr(eng.loss_accum), _lib.ptr(eng.tickets)
    return out


def _optim_call(eng, opt, b, phases=15, hp=None, ws=None, ws_bytes=None, known=None, mask=None, mask_bytes=0):
    from dglke_amd import _lib
    if ws is None:
        ws, ws_bytes = _lib.ptr(eng.workspace_for(b)), eng._ws_bytes
    return _lib.lib().kge_step_optim(C.byref(hp or eng.hp), C.byref(opt), C.byref(eng.tb), C.byref(b.c), C.byref(_out(eng)), ws, ws_bytes,
                                     phases, known, mask, mask_bytes, _lib.stream_ptr())


@pytest.mark.parametrize("cid", ["TransE_l2-w16", "TransE_l1-w16", "DistMult-w260", "l2-known"])
def test_adagrad_kind_is_the_existing_step_bit_for_bit(cid):
    """kind = KGE_OPT_ADAGRAD through the new entry: the tables and state of kge_step_fused (l2-known: of kge_step_fused_known)"""
    from dglke_amd import _lib
    from dglke_amd.known import KnownIndex
    c = A.by_id(cid)
    ent, rel = A.tables(c)
    bts = A.batches(c, 2)
    res = []
    for through_optim in (False, True):
        eng = _engine(c, "Adagrad")
        eng.load_tables(ent, rel)
        opt = _lib.KgeOptim()
        opt.kind = _lib.OPT_ADAGRAD
        for bt in bts:
            b = _batch(c, bt)
            if c["known"]:
                eng.attach_known(KnownIndex(A.known_pairs(c, bt)[1], c["n_ent"], c["n_rel"], DEV))
            if not through_optim:
                eng.step(b)
            elif c["known"]:
                km = eng.known_mask_for(b)
                assert _optim_call(eng, opt, b, known=C.byref(eng._known[0]), mask=_lib.ptr(km), mask_bytes=eng._kmask_bytes) == 0
            else:
                assert _optim_call(eng, opt, b) == 0
        res.append(dict(_state(eng), loss=eng.loss_accum.cpu().numpy()))
    _same_state(res[0], res[1], cid)
    assert not np.array_equal(res[0]["ent"], ent)


@pytest.mark.parametrize("cid", ["TransE_l2-w16", "TransE_l1-w16", "DistMult-w260", "RotatE-w16", "l2-known"])
def test_four_phase_groups_are_the_whole_step_bit_for_bit(cid):
    from dglke_amd.known import KnownIndex
    c = A.by_id(cid)
    ent, rel = A.tables(c)
    res = []
    for timed in (False, True):
        eng = _engine(c)
        eng.load_tables(ent, rel)
        for bt in A.batches(c, 2):
            if c["known"]:
                eng.attach_known(KnownIndex(A.known_pairs(c, bt)[1], c["n_ent"], c["n_rel"], DEV))
            b = _batch(c, bt)
            eng.step_timed(b) if timed else eng.step(b)
        res.append(dict(_state(eng), loss=eng.loss_accum.cpu().numpy()))
    _same_state(res[0], res[1], cid)


@pytest.mark.parametrize("cid", ["TransE_l2-w16", "DistMult-w516"])
def test_stream_contract(cid):
    """default stream, a side stream, and every call captured alone into a graph and replayed on the side stream: bit for bit"""
    from dglke_amd import _lib
    c = A.by_id(cid)
    ent, rel = A.tables(c)
    bts = A.batches(c, 2)
    side = torch.cuda.Stream()
    res = {}
    for mode in ("default", "side", "capture"):
        eng = _engine(c)
        eng.load_tables(ent, rel)
        bs = [_batch(c, bt) for bt in bts]
        for b in bs:
            eng.workspace_for(b)
        torch.cuda.synchronize()
        graphs = []
        if mode == "default":
            for b in bs:
                eng.step(b)
        else:
            with torch.cuda.stream(side):
                for b in bs:
                    assert _lib.stream_ptr() == side.cuda_stream
                    if mode == "side":
                        eng.step(b)
                    else:
                        g = torch.cuda.CUDAGraph()
                        with _lib.graph_capture(g, stream=side):
                            eng.step(b)
                        g.replay()
                        graphs.append(g)
        res[mode] = dict(_state(eng), loss=eng.loss_accum.cpu().numpy())
        del graphs
    _same_state(res["default"], res["side"], cid + ": side stream")
    _same_state(res["default"], res["capture"], cid + ": captured and replayed")
    assert not np.array_equal(res["default"]["ent"], ent)


@pytest.mark.parametrize("cid", ["TransE_l2-w16", "TransE_l1-w16", "DistMult-w260"])
def test_workspace_contract(cid):
    """the workspace of kge_step_workspace_bytes, to the byte, between two guards; its contents on entry are arbitrary"""
    from dglke_amd import _lib
    c = A.by_id(cid)
    ent, rel = A.tables(c)
    bts = A.batches(c, 2)
    GUARD = 4096
    res = []
    for fill in (0x00, 0xFF, 0x5A):
        eng = _engine(c)
        eng.load_tables(ent, rel)
        for bt in bts:
            b = _batch(c, bt)
            need = int(_lib.lib().kge_step_workspace_bytes(C.byref(eng.hp), b.B, b.C, b.chunk, b.N, b.UE, b.UR))
            buf = torch.full((need + 2 * GUARD,), 0xC3, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 256 == 0
            buf[GUARD:GUARD + need] = fill
            assert _optim_call(eng, eng.opt, b, ws=buf.data_ptr() + GUARD, ws_bytes=need) == 0
            torch.cuda.synchronize()
            assert bool((buf[:GUARD] == 0xC3).all()) and bool((buf[GUARD + need:] == 0xC3).all()), "a guard was written"
            assert _optim_call(eng, eng.opt, b, ws=buf.data_ptr() + GUARD, ws_bytes=need - 1) == -2       # KGE_ERR_WORKSPACE
        res.append(dict(_state(eng), loss=eng.loss_accum.cpu().numpy()))
    _same_state(res[0], res[1], cid + ": workspace of 0xFF bytes")
    _same_state(res[0], res[2], cid + ": workspace of 0x5A bytes")


def test_refusals_arrive_before_any_launch():
    from dglke_amd import _lib
    c = A.by_id("TransE_l2-w16")
    ent, rel = A.tables(c)
    eng = _engine(c)
    eng.load_tables(ent, rel)
    b = _batch(c, A.batches(c, 1)[0])
    before = _state(eng)

    def opt(**kw):
        o = _lib.KgeOptim()
        for k in ("kind", "beta1", "beta2", "eps", "ent_mom", "rel_mom"):
            setattr(o, k, kw.get(k, getattr(eng.opt, k)))
        return o

    def hp(**kw):
        h = _lib.KgeHParams()
        C.memmove(C.byref(h), C.byref(eng.hp), C.sizeof(h))
        for k, v in kw.items():
            setattr(h, k, v)
        return h
    bad = [("RESCAL", dict(hp=hp(model=_lib.MODEL_IDS["RESCAL"])), "RESCAL"), ("TransR", dict(hp=hp(model=_lib.MODEL_IDS["TransR"])), "TransR"),
           ("ent_mom", dict(opt=opt(ent_mom=None)), "moment"), ("rel_mom", dict(opt=opt(rel_mom=None)), "moment"),
           ("beta1", dict(opt=opt(beta1=1.0)), "beta"), ("beta2", dict(opt=opt(beta2=-0.5)), "beta"), ("eps", dict(opt=opt(eps=0.0)), "eps"),
           ("d_e", dict(hp=hp(d_e=18)), "multiples of 4"), ("d_r", dict(hp=hp(d_r=1028)), "1024"), ("kind", dict(opt=opt(kind=7)), "kind"),
           ("phases", dict(phases=16), "phase")]
    for name, kw, word in bad:
        rc = _optim_call(eng, kw.get("opt", eng.opt), b, phases=kw.get("phases", 15), hp=kw.get("hp"))
        msg = _lib.lib().kge_last_error().decode()
        assert rc == -1 and "kge_step_optim" in msg and word in msg, (name, rc, msg)
        _same_state(before, _state(eng), "refusal %s" % name)
    # the Python side
    from dglke_amd._lib import KgeError
    with pytest.raises(KgeError, match="async"):
        eng.step_async(b)
    with pytest.raises(KgeError, match="sample_job"):
        eng.step(b, sample_job=_lib.KgeSamplerJob())
    for model, kw in (("RESCAL", {}), ("TransR", {})):
        with pytest.raises(KgeError, match="RESCAL / TransR"):
            _engine(dict(c, model=model, hidden=4))
    with pytest.raises(KgeError, match="multiples of 4"):
        _engine(dict(c, hidden=18))
    _same_state(before, _state(eng), "python refusals")
    assert _optim_call(eng, eng.opt, b) == 0


def test_engine_owns_zeroed_moments_and_takes_them_from_the_caller():
    c = A.by_id("TransE_l2-w16")
    d_e, d_r = A.widths(c)
    eng = _engine(c)
    assert tuple(eng.ent_mom.shape) == (c["n_ent"], 2, d_e) and tuple(eng.rel_mom.shape) == (c["n_rel"], 2, d_r)
    assert not eng.ent_mom.any() and not eng.rel_mom.any() and not eng.ent_state.any()
    ent, rel = A.tables(c)
    pre = A.preloaded(c, 1)
    eng.load_tables(ent, rel, **{k: torch.from_numpy(v) for k, v in pre.items()})
    st = _state(eng)
    assert np.array_equal(st["ent_mom"], pre["ent_mom"]) and np.array_equal(st["rel_state"], pre["rel_state"])
    eng.reset_parameters()
    assert not eng.ent_mom.any() and not eng.rel_mom.any() and not eng.ent_state.any() and not eng.rel_state.any()
    # a second engine on the same tables and moments (the lanes of --num_proc)
    lane = _engine(c, tables=(eng.ent, eng.ent_state, eng.rel, eng.rel_state), moments=(eng.ent_mom, eng.rel_mom))
    lane.step(_batch(c, A.batches(c, 1)[0]))
    torch.cuda.synchronize()
    assert bool(eng.ent_mom.any()) and bool(eng.ent_state.any())


# --------------------------------------------------------------------------------------------------------------------------
# the CLI, on the planted toy graph of tests/test_gpu_cli.py
# --------------------------------------------------------------------------------------------------------------------------
def _argv(tmp_path, extra, max_step=300, model="TransE_l2"):
    return ["--model_name", model, "--format", "udd_hrt", "--dataset", "toy", "--data_path", str(tmp_path / "kg"), "--data_files",
            "e.dict", "r.dict", "train.txt", "valid.txt", "test.txt", "--save_path", str(tmp_path / "ckpts"), "--gpu", "0",
            "--batch_size", "256", "--neg_sample_size", "64", "--hidden_dim", "32", "-g", "8", "--lr", "0.01", "-adv",
            "--max_step", str(max_step), "--log_interval", "50", "--graph_steps", "100", "--optimizer", "Adam"] + extra


def test_train_cli_graph_replay_equals_the_eager_loop_and_learns(tmp_path, capsys):
    """dglke_train --optimizer Adam --graph_steps 100 trains the same tables, moments and counts, bit for bit, as the eager loop
    `for s: engine.step(sampler.sample(1)[0])` (the method of test_gpu_train_trajectory.py); config.json holds the four fields,
    --test prints its metrics, and the mean loss of the last 50 of 300 steps is below that of the first 50"""
    from dglke_amd import train as T
    from test_gpu_cli import _planted
    _planted(str(tmp_path / "kg"))
    ref = {}

    def before_train(tr):
        clones = tuple(t.clone() for t in tr.model.tables())
        mom = (torch.zeros_like(tr.model.engine.ent_mom), torch.zeros_like(tr.model.engine.rel_mom))
        eng = tr.make_engine(tables=clones, moments=mom)
        smp = tr.make_sampler(0, slice(None))
        for _ in range(300):
            eng.step(smp.sample(1)[0])
        torch.cuda.synchronize()
        ref.update(ent=clones[0].cpu(), ent_state=clones[1].cpu(), rel=clones[2].cpu(), rel_state=clones[3].cpu(), ent_mom=mom[0].cpu(),
                   rel_mom=mom[1].cpu())
    tr = T.main(_argv(tmp_path, ["--test"]), before_train=before_train)
    out = capsys.readouterr().out
    eng = tr.model.engine
    assert eng.optimizer == "Adam" and eng.opt is not None and tr.device_sampler
    for k in KEYS:
        assert torch.equal(getattr(eng, k).cpu(), ref[k]), "%s: graph replay against the eager loop" % k
    assert float(eng.ent_state.max()) > 1 and bool(eng.ent_mom.any())
    conf = json.load(open(os.path.join(tr.args.save_path, "config.json")))
    assert (conf["optimizer"], conf["adam_beta1"], conf["adam_beta2"], conf["adam_eps"]) == ("Adam", 0.9, 0.999, 1e-8)
    assert "fused HIP step, Adam" in out
    assert "Test average MRR" in out and "Test average HITS@10" in out
    losses = [float(l.split(":")[1]) for l in out.split("\n") if ") average loss:" in l]
    assert len(losses) == 6 and all(math.isfinite(x) for x in losses)
    assert losses[-1] < losses[0], losses


def test_train_cli_two_lanes_share_the_moments(tmp_path, capsys):
    from dglke_amd import train as T
    from test_gpu_cli import _planted
    _planted(str(tmp_path / "kg"))
    tr = T.main(_argv(tmp_path, ["--num_proc", "2"], max_step=100))
    out = capsys.readouterr().out
    assert len(tr.lanes) == 2
    a, b = tr.lanes[0].engine, tr.lanes[1].engine
    assert a.ent_mom.data_ptr() == b.ent_mom.data_ptr() and a.rel_mom.data_ptr() == b.rel_mom.data_ptr()
    last = [l for l in out.split("\n") if "(100/100) average loss:" in l]
    assert len(last) == 2 and all(math.isfinite(float(l.split(":")[1])) for l in last)
    assert np.isfinite(tr.model.entity_emb.emb.cpu().numpy()).all()


def test_train_cli_host_built_plans(tmp_path, capsys):
    """--has_edge_importance: batches of the host sampler - nothing in the Adam step reads a device-side step number"""
    from dglke_amd import train as T
    import train_loop_cases as L
    L.write_planted(str(tmp_path / "kg"), weights=True)
    tr = T.main(_argv(tmp_path, ["--has_edge_importance", "--batch_size", "64", "--neg_sample_size", "16"], max_step=100))
    out = capsys.readouterr().out
    assert not tr.device_sampler
    last = [l for l in out.split("\n") if "(100/100) average loss:" in l]
    assert len(last) == 1 and math.isfinite(float(last[0].split(":")[1]))
    assert float(tr.model.engine.ent_state.max()) >= 1
