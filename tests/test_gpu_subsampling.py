"""Per-edge weights from the DEVICE sampler (dglke_train --subsampling_weight, --has_edge_importance --edge_importance_on_device):
  1. the weighted sampler launch (kge_sample_batches_weighted): every slot's edge_w is W of its triples, bit for bit, and every
     other array and the device state are the unweighted launch's, in all four instances and across four epochs;
  2. kge_subsampling_weights / dataloader.subsampling_weights against the float64 statement of tests/subsampling_cases.py;
  3. one fused step per corruption side on a weighted device batch against the float64 oracles, with the bounds of the
     edge-importance cases of test_gpu_loss_options.py / test_gpu_pairre.py / test_gpu_quate.py (their own check code runs);
  4. doubling every weight doubles the positive and negative loss terms exactly and leaves the regulariser alone;
  5. dglke_train with the two flags trains the straight-line sequence of steps over a fresh weighted sampler, bit for bit;
  6. the refused combinations, before anything is loaded; tail_jobs() and the C entry's argument checks;
  7. the two new stream-taking entries on the default stream, on a side stream and captured alone, same bits.
Case table: tests/subsampling_cases.py (guarded on the CPU by tests/test_subsampling_inputs.py)."""
import contextlib
import ctypes as C
import gc
import io
import os

import numpy as np
import pytest
import torch

import loss_option_cases as L
import pairre_cases as PQ
import quate_cases as QQ
import subsampling_cases as SC
import test_gpu_loss_options as TL
import test_gpu_pairre as TP
import test_gpu_quate as TQ
import test_gpu_stream_contract as SG
import train_loop_cases as TC
from test_gpu_parity import DEV
from test_gpu_train_trajectory import Loop, _assert_counters, _assert_trajectory

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # the largest relative error of one correctly rounded fp32 operation
ERRORS = {}             # what -> largest error as a fraction of its bound


def _note(what, frac):
    ERRORS[what] = max(ERRORS.get(what, 0.0), float(frac))
    try:
        out = TL._report_dir()
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "subsampling_errors.txt"), "w") as f:
            f.write("largest error as a fraction of its bound (<= 1 passes)\n")
            for k in sorted(ERRORS):
                f.write("%-60s %.4f\n" % (k, ERRORS[k]))
    except OSError:
        pass


# --------------------------------------------------------------------------------------------------------------------------
# 1. the weighted sampler launch
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", SC.GEOMETRIES, ids=[g[0] for g in SC.GEOMETRIES])
def test_weighted_sampler_carries_the_weights_and_changes_nothing_else(g):
    from dglke_amd.dataloader import DeviceSampler
    _, B, N, n_train, n_ent, slots, _ = g
    h, r, t, w = SC.unique_triples(n_train, n_ent)
    weight_of = dict(zip(zip(h.tolist(), r.tolist(), t.tolist()), w.tolist()))
    plain = DeviceSampler(h, r, t, n_ent, B, N, DEV, n_slots=slots, seed=3)
    wtd = DeviceSampler(h, r, t, n_ent, B, N, DEV, n_slots=slots, seed=3, edge_importance=w)
    assert wtd.slot_bytes == plain.slot_bytes + SC.al32(4 * B)
    seen = set()
    for launch in range(SC.N_LAUNCHES):
        bp, bw = plain.sample(), wtd.sample()
        torch.cuda.synchronize()
        assert torch.equal(plain.state, wtd.state), "device state after launch %d" % launch
        for k in range(slots):
            a, b = plain.slot_arrays(k), wtd.slot_arrays(k)
            assert sorted(b) == sorted(list(a) + ["edge_w"])
            for name in a:
                assert np.array_equal(a[name], b[name]), "launch %d slot %d: %s differs from the unweighted sampler's" % (launch, k, name)
            want = np.array([weight_of[x] for x in zip(b["h_gid"].tolist(), b["rel_ids"].tolist(), b["t_gid"].tolist())], np.float32)
            assert np.array_equal(b["edge_w"].view(np.int32), want.view(np.int32)), "launch %d slot %d: edge_w" % (launch, k)
            assert bp[k].neg_head == bw[k].neg_head and bw[k].c.edge_w and not bp[k].c.edge_w and bw[k].c.edge_w_mean == 0.0
            assert bw[k].c.edge_w == wtd.slots.data_ptr() + k * wtd.slot_bytes + plain.slot_bytes
            seen.update(b["edge_w"].tolist())
    assert len(seen) > B, "the launches repeated one batch"


# --------------------------------------------------------------------------------------------------------------------------
# 2. the weights against float64
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.weight_graphs()))
def test_weights_match_the_float64_statement(name):
    """Bound: relative error <= 4 * 2^-24.  The conversion of n_hr + n_tr + 6 to fp32 is exact (the sum is far below 2^24); then
    three correctly rounded fp32 operations - sqrtf, the division, the product with scale - each within 2^-24 relative, plus the
    rounding of scale = float32(1 / mean) itself: four roundings."""
    from dglke_amd.dataloader import subsampling_weights
    h, r, t, n_ent, n_rel = SC.weight_graphs()[name]
    w = subsampling_weights(h, r, t, n_ent, n_rel, DEV)
    assert w.dtype == torch.float32 and w.shape == (len(h),) and w.device.type == "cuda"
    got = w.cpu().numpy().astype(np.float64)
    ref = SC.weights64(h, r, t, n_rel)
    rel = np.abs(got - ref) / ref
    mean_err = abs(got.mean() - 1.0)
    print("%s: largest relative error %.3e = %.3f of 4 * 2^-24; |mean - 1| = %.3e (bound %.3e)" % (
        name, rel.max(), rel.max() / (4 * U), mean_err, len(h) * U))
    _note("weights %s relative error" % name, rel.max() / (4 * U))
    assert rel.max() <= 4 * U
    assert mean_err <= len(h) * U
    if name == "table":
        # the triple present three times carries the weight of count 3 on both sides - and its copies the same
        raw = SC.raw_weights64(h, r, t, n_rel)
        assert raw[SC.TRIPLED] == 1.0 / np.sqrt(3 + 3 + 6.0)
        scale = 1.0 / raw.mean()
        assert abs(got[SC.TRIPLED] - scale / np.sqrt(12.0)) <= 4 * U * got[SC.TRIPLED]
        assert abs(got[SC.TRIPLED] - scale / np.sqrt(8.0)) > 0.1 * got[SC.TRIPLED], "counted without multiplicity"
        assert got[-1] == got[-2] == got[SC.TRIPLED]
        assert got.max() > 3 * got.min()


def test_weights_entry_refuses_keys_beyond_62_bits():
    from dglke_amd import _lib
    from dglke_amd.dataloader import subsampling_weights
    z = np.zeros(4, np.int64)
    with pytest.raises(_lib.KgeError, match="2\\^62"):
        subsampling_weights(z, z, z, 1 << 40, 1 << 22, DEV)
    k = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.full((4,), -1.0, device=DEV)
    rc = _lib.lib().kge_subsampling_weights(_lib.ptr(k), 4, _lib.ptr(k), 4, _lib.ptr(k), _lib.ptr(k), _lib.ptr(k), 4, 1 << 40, 1 << 22, 1.0,
                                            _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b"2^62" in _lib.lib().kge_last_error() and bool((out == -1.0).all())


# --------------------------------------------------------------------------------------------------------------------------
# 3. the step on a weighted device batch
# --------------------------------------------------------------------------------------------------------------------------
STEP_B, STEP_CHUNK, STEP_N, STEP_HIDDEN = 64, 16, 16, 32


def _device_batches(n_ent, seed=5):
    """two weighted device batches (step 1 corrupts tails, step 2 heads) over the case table's graph folded onto n_ent entities,
    its subsampling weights (float64 statement, rounded to fp32) as edge importance: [(bt, DeviceBatch)], bt as the oracles take
    it - ids and weights READ BACK from the slot"""
    from dglke_amd.dataloader import DeviceSampler
    h, r, t = SC.graph()
    h, t = h % n_ent, t % n_ent
    same = h == t
    t[same] = (t[same] + 1) % n_ent
    w = SC.weights64(h, r, t, SC.N_REL).astype(np.float32)
    smp = DeviceSampler(h, r, t, n_ent, STEP_B, STEP_N, DEV, n_slots=2, neg_chunk_size=STEP_CHUNK, seed=seed, edge_importance=w)
    dbs = smp.sample(2)
    torch.cuda.synchronize()
    out = []
    for k, db in enumerate(dbs):
        a = smp.slot_arrays(k)
        assert db.neg_head == (k == 1) and a["counts"][2] == int(db.neg_head)
        nid, inv = np.unique(np.concatenate([a["h_gid"], a["t_gid"]]), return_inverse=True)
        bt = dict(h=a["h_gid"], t=a["t_gid"], r=a["rel_ids"], neg=a["neg_ids"], neg_head=bool(db.neg_head), C=STEP_B // STEP_CHUNK,
                  nid=nid.astype(np.int64), h_local=inv[:STEP_B].astype(np.int64), t_local=inv[STEP_B:].astype(np.int64),
                  w=a["edge_w"].copy())
        assert bt["w"].max() > 1.5 * bt["w"].min(), "the batch's weights hardly differ: the step would not tell them from none"
        db.p = dict(ue_id=a["ue_id"][:int(a["counts"][0])])      # (what the check code reads of a host plan)
        db.sampler_ref = smp
        out.append((bt, db))
    return out


_SHAPE_OF = {"TransE_l2": "midT", "DistMult": "midD", "RotatE": "midR", "TransR": "transr", "RESCAL": "rescal"}


def _generic_case(cid, model, **kw):
    return L.case("subsampling-" + cid, _SHAPE_OF[model], impts=True, rows=5e-3, n_ent=SC.N_ENT, n_rel=SC.N_REL, hidden=STEP_HIDDEN,
                  B=STEP_B, N=STEP_N, chunk=STEP_CHUNK, **kw)


GENERIC = [_generic_case(m, m) for m in ("TransE_l2", "DistMult", "RotatE", "TransR", "RESCAL")] + [
    _generic_case("TransE_l2-neg_deg_sample", "TransE_l2", neg_deg=True),
    _generic_case("DistMult-pw", "DistMult", genre="Logistic", pairwise=True),
]


@pytest.mark.parametrize("c", GENERIC, ids=[c["id"] for c in GENERIC])
def test_step_on_weighted_device_batch_matches_oracle(c, monkeypatch):
    """test_gpu_loss_options.run_case itself - its comparisons and bounds - fed with the weighted device batches instead of host
    plans: the oracle gets the ids and weights read back from the slots"""
    pairs = _device_batches(c["n_ent"])
    by_id = {id(bt): db for bt, db in pairs}
    monkeypatch.setattr(L, "batches", lambda c_, steps=2: [bt for bt, _ in pairs])
    monkeypatch.setattr(TL, "_batch", lambda c_, bt: by_id[id(bt)])
    close = TL._close

    def recording_close(a, b, rtol, atol, what):
        """run_case's own comparison, after noting the largest error as a fraction of the bound it applies"""
        a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
        if a64.shape == b64.shape and a64.size and np.isfinite(a64).all():
            _note("step " + what.replace(" step 1", "").replace(" step 2", ""), (np.abs(a64 - b64) / (atol + rtol * np.abs(b64))).max())
        close(a, b, rtol, atol, what)
    monkeypatch.setattr(TL, "_close", recording_close)
    TL.run_case(c, 0)


def _own_oracle_step(T, Q, c, d_e, known_index=False):
    """the body of test_gpu_pairre / test_gpu_quate.test_fused_step_matches_float64_step (their engines, oracles, comparison and
    bounds) on the weighted device batches; known_index: with a known-triple index attached (--exclude_positive)"""
    from dglke_amd.known import KnownIndex
    for bt, db in _device_batches(c["n_ent"]):
        eng = T._engine(c, d_e)
        known = None
        if known_index:
            K, known = Q.planted_known(bt, c["chunk"], c["N"])
            assert known.any()
            eng.attach_known(KnownIndex(K, c["n_ent"], c["n_rel"], DEV))
        ent64, rel64, es64, rs64 = (TL._f64(x) for x in (eng.ent, eng.rel, eng.ent_state, eng.rel_state))
        ent0 = ent64.copy()
        want = eng.alloc_outputs(db)
        eng.step(db, want)
        torch.cuda.synchronize()
        out = Q.step(c, ent64, es64, rel64, rs64, bt, known) if known_index else Q.step(c, ent64, es64, rel64, rs64, bt)
        tag = "%s D%d %s %s" % (Q.MODEL, d_e, c["id"], "head" if bt["neg_head"] else "tail")
        errs = T._compare_step(c, eng, db, bt, want, out, (ent64, es64, rel64, rs64, ent0), tag, known=known)
        for k, v in errs.items():
            _note("step %s %s" % (tag, k), v[0])
        T._check(errs, tag)


def _own_case(Q, cid, **kw):
    return dict(Q.step_case(cid, impts=True, **kw), B=STEP_B, chunk=STEP_CHUNK, N=STEP_N)


@pytest.mark.parametrize("d_e", PQ.STEP_WIDTHS)
@pytest.mark.parametrize("cid,kw,known", [("impts-adv", dict(adv=True), False), ("impts-softmax", dict(genre="Softmax"), False),
                                           ("impts-exclude_positive", dict(adv=True), True)])
def test_pairre_step_on_weighted_device_batch_matches_float64(cid, kw, known, d_e):
    _own_oracle_step(TP, PQ, _own_case(PQ, cid, **kw), d_e, known_index=known)


@pytest.mark.parametrize("d_e", QQ.STEP_WIDTHS)
def test_quate_step_on_weighted_device_batch_matches_float64(d_e):
    _own_oracle_step(TQ, QQ, _own_case(QQ, "impts-adv", adv=True), d_e)


# --------------------------------------------------------------------------------------------------------------------------
# 4. doubling the weights
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adv", [True, False], ids=["adv", "no-adv"])
def test_doubled_weights_double_the_loss_terms_exactly(adv):
    """a factor 2 on every fp32 weight is exact through every product and sum: the positive and the negative loss term double, bit
    for bit, the regulariser does not move; without -adv and without regulariser the gradient messages double too"""
    from dglke_amd.dataloader import DeviceSampler
    from dglke_amd.engine import StepEngine
    h, r, t = SC.graph()
    w = SC.weights64(h, r, t, SC.N_REL).astype(np.float32)
    rc = 1e-4 if adv else 0.0
    res = []
    torch.manual_seed(3)
    base = StepEngine("TransE_l2", SC.N_ENT, SC.N_REL, STEP_HIDDEN, 8.0, 0.25, DEV, False, False, adv, 1.0, rc, 3)
    for f in (1.0, 2.0):
        eng = StepEngine("TransE_l2", SC.N_ENT, SC.N_REL, STEP_HIDDEN, 8.0, 0.25, DEV, False, False, adv, 1.0, rc, 3)
        eng.load_tables(base.ent.clone(), base.rel.clone())
        smp = DeviceSampler(h, r, t, SC.N_ENT, STEP_B, STEP_N, DEV, n_slots=2, neg_chunk_size=STEP_CHUNK, seed=11,
                            edge_importance=w * np.float32(f))
        steps = []
        for db in smp.sample(2):
            eng.load_tables(base.ent.clone(), base.rel.clone())      # every step from the same tables: the update depends on the weights
            want = eng.alloc_outputs(db)
            for v in want.values():
                v.zero_()
            eng.step(db, want)
            torch.cuda.synchronize()
            steps.append((np.array(eng.read_loss(), np.float32), {k: v.cpu().numpy() for k, v in want.items()}))
        res.append(steps)
    for (l1, o1), (l2, o2) in zip(*res):
        assert l1[0] > 0 and l1[1] > 0
        assert l2[0] == np.float32(2) * l1[0] and l2[1] == np.float32(2) * l1[1], (l1, l2)
        assert l2[3] == l1[3] and (l1[3] > 0) == adv
        assert np.array_equal(o1["pos_score"], o2["pos_score"]) and np.array_equal(o1["neg_score"], o2["neg_score"])
        if not adv:
            for k in ("g_pos_ent", "g_neg", "g_rel"):
                assert np.abs(o1[k]).max() > 0 and np.array_equal(o2[k], np.float32(2) * o1[k]), k


# --------------------------------------------------------------------------------------------------------------------------
# 5. the training loop
# --------------------------------------------------------------------------------------------------------------------------
LOOP_MODES = [
    ("subsampling_weight", "TransE_l2", ["--subsampling_weight"], False),
    ("edge_importance_on_device", "TransE_l2", ["--has_edge_importance", "--edge_importance_on_device"], True),
]
LOOP_ROWS = [r for r in TC.ROWS if r[0] in ("eager", "replays", "parity_flips")]


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    return Loop(str(tmp_path_factory.mktemp("subsampling_loop")))


@pytest.mark.parametrize("row", LOOP_ROWS, ids=[r[0] for r in LOOP_ROWS])
@pytest.mark.parametrize("mode", LOOP_MODES, ids=[m[0] for m in LOOP_MODES])
def test_flags_train_the_straight_line_sequence_over_a_weighted_device_sampler(loop, mode, row):
    """all four tables after MAX_STEP steps equal those of `for s: engine.step(sampler.sample(1)[0])` over a fresh weighted
    DeviceSampler (test_gpu_train_trajectory.straight_line through tr.make_sampler), bit for bit"""
    rec = loop.run(mode, row)
    assert rec["device_sampler"] is True
    assert ("subsampling weights" if mode[0] == "subsampling_weight" else "edge importance on the device") in rec["out"]
    _assert_trajectory(loop, mode, row)
    _assert_counters(rec)


def test_straight_line_reference_is_weighted(loop):
    """the reference of the loop test is itself trained on weights: its losses differ from the unweighted run's"""
    ref_w = loop.reference(LOOP_MODES[0])[2]
    ref_p = loop.reference(("plain", "TransE_l2", [], False))[2]
    assert ref_w.shape == ref_p.shape and np.abs(ref_w[:, 1] - ref_p[:, 1]).max() > 1e-3


@pytest.mark.parametrize("mode", LOOP_MODES, ids=[m[0] for m in LOOP_MODES])
def test_two_lanes_get_the_rows_of_their_parts(loop, mode):
    """--num_proc 2: lock-free lanes on shared tables (nobody's reference); each lane has built and run MAX_STEP batches, and its
    sampler carries the weights of ITS rows of the split - counts from the whole split"""
    from dglke_amd import train as T
    seen = {}

    def before_train(tr):
        parts = tr.split(2)
        seen["w"] = [lane.sampler.W.cpu().numpy() for lane in tr.lanes]
        seen["want"] = [tr.edge_weights.cpu().numpy()[np.asarray(p)] for p in parts]
        seen["all"] = tr.edge_weights.cpu().numpy()
        seen["train"] = tr.dataset.train
    with contextlib.redirect_stdout(io.StringIO()) as out:
        tr = T.main(loop.argv(mode, TC.ROWS[2], ("--num_proc", "2")), before_train=before_train)
    torch.cuda.synchronize()
    assert len(tr.lanes) == 2 and tr.device_sampler
    for got, want in zip(seen["w"], seen["want"]):
        assert np.array_equal(got, want)
    if mode[0] == "subsampling_weight":
        h, r, t = (np.asarray(x) for x in seen["train"][:3])
        ref = SC.weights64(h, r, t, TC.N_REL)
        assert np.abs(seen["all"] - ref).max() <= 4 * U * ref.max()
    for lane in tr.lanes:
        assert lane.sampler.host_step == TC.MAX_STEP + 1 and int(lane.sampler.state[1]) == TC.MAX_STEP + 1
    assert "[proc 1][Train](200/230) average loss:" in out.getvalue()


def test_config_json_records_the_flag(loop):
    import json
    rec_argv = loop.argv(LOOP_MODES[0], ("", 0, 10, []), max_step=10)
    from dglke_amd import train as T
    with contextlib.redirect_stdout(io.StringIO()):
        tr = T.main(rec_argv)
    conf = json.load(open(os.path.join(tr.args.save_path, "config.json")))
    assert conf["subsampling_weight"] is True and conf["edge_importance_on_device"] is False


# --------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,message", [
    (["--subsampling_weight", "--has_edge_importance"], "two weightings"),
    (["--subsampling_weight", "--gpu", "0", "0"], "more than one GPU"),
    (["--subsampling_weight", "--async_update", "--async_update_pipeline"], "one-step-stale pipeline"),
    (["--subsampling_weight", "--async_update", "--async_update_rel"], "one-step-stale pipeline"),
    (["--subsampling_weight", "--batch_size", "4096", "--neg_sample_size", "256"], "no host sampler for this flag"),
    (["--has_edge_importance", "--edge_importance_on_device", "--gpu", "0", "0"], "more than one GPU"),
    (["--has_edge_importance", "--edge_importance_on_device", "--async_update", "--async_update_rel"], "one-step-stale pipeline"),
    (["--has_edge_importance", "--edge_importance_on_device", "--batch_size", "4096", "--neg_sample_size", "256"], "no host sampler"),
    (["--edge_importance_on_device"], "needs --has_edge_importance"),
], ids=lambda x: "+".join(f.lstrip("-") for f in x if f.startswith("--")) if isinstance(x, list) else None)
def test_refused_combinations_exit_before_anything_is_loaded(tmp_path, flags, message):
    """the data path does not exist and the save path is never made: the refusal comes before the dataset and before any table"""
    from dglke_amd import _lib
    from dglke_amd import train as T
    save = str(tmp_path / "ckpts")
    argv = TC.argv(str(tmp_path / "no_such_data"), save, "TransE_l2", 20, 50, flags)
    gc.collect()                                   # (what earlier tests left behind is freed now, not during the call)
    before = torch.cuda.memory_allocated()
    with pytest.raises(_lib.KgeError, match=message):
        T.main(argv)
    assert not os.path.exists(save) and torch.cuda.memory_allocated() <= before


def test_weighted_sampler_refusals():
    from dglke_amd import _lib
    from dglke_amd.dataloader import DeviceSampler
    h, r, t, w = SC.unique_triples(200, 50)
    with pytest.raises(ValueError, match="Edge importance score should > 0"):
        DeviceSampler(h, r, t, 50, 16, 4, DEV, n_slots=2, edge_importance=np.where(np.arange(200) == 7, 0.0, w))
    with pytest.raises(ValueError, match="one weight per training triple"):
        DeviceSampler(h, r, t, 50, 16, 4, DEV, n_slots=2, edge_importance=w[:-1])
    s = DeviceSampler(h, r, t, 50, 16, 4, DEV, n_slots=2, seed=1, edge_importance=w)
    with pytest.raises(_lib.KgeError, match="tail_jobs"):
        s.tail_jobs(2)
    # the C entry: null weights, then a slot of the unweighted size - the documented codes, nothing launched
    state0, lib = s.state.clone(), _lib.lib()
    args = lambda weights, slot_bytes: (_lib.ptr(s.H), _lib.ptr(s.R), _lib.ptr(s.T), _lib.ptr(s.perm), weights, s.n_train, 50, 16, 4, 4, 4,
                                        1, _lib.ptr(s.state), _lib.ptr(s.slots), slot_bytes, 2, _lib.stream_ptr())
    assert lib.kge_sample_batches_weighted(*args(None, s.slot_bytes)) == -1            # KGE_ERR_ARG
    assert b"kge_sample_batches_weighted" in lib.kge_last_error() and b"weights" in lib.kge_last_error()
    short = int(lib.kge_sampler_slot_bytes(16, 4, 4))
    assert short < s.slot_bytes
    assert lib.kge_sample_batches_weighted(*args(_lib.ptr(s.W), short)) == -2          # KGE_ERR_WORKSPACE
    kb = _lib.KgeBatch()
    assert lib.kge_batch_from_slot_weighted(_lib.ptr(s.slots), short, 0, 16, 4, 4, 4, 0, C.byref(kb)) == -2
    torch.cuda.synchronize()
    assert torch.equal(s.state, state0) and not bool(s.slots.any()), "a refused call launched"
    assert lib.kge_sample_batches_weighted(*args(_lib.ptr(s.W), s.slot_bytes)) == 0
    torch.cuda.synchronize()
    assert int(s.state[1]) == 3 and bool(s.slots.any())


# --------------------------------------------------------------------------------------------------------------------------
# 7. the stream contract of the two new launches
# --------------------------------------------------------------------------------------------------------------------------
STREAM_ENTRIES = ("kge_sample_batches_weighted", "kge_subsampling_weights")


class _Probe(SG.StreamProbe):
    """test_gpu_stream_contract.StreamProbe for the entries of this file: every call of one of them is held to the stream of the
    mode and, in capture mode, captured alone into a fresh graph, closed and replayed"""

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in STREAM_ENTRIES:
            return fn

        def call(*a):
            from dglke_amd import _lib
            self.calls.append((self.mode, name))
            want = torch.cuda.default_stream() if self.mode == "default" else self.side
            assert torch.cuda.current_stream() == want, "%s: the run left the %s stream" % (name, self.mode)
            assert int(a[-1] or 0) == int(want.cuda_stream), "%s was given stream %r, the current stream is %r" % (name, a[-1], want.cuda_stream)
            if self.mode != "capture":
                return fn(*a)
            g = torch.cuda.CUDAGraph()
            with _lib.graph_capture(g, stream=self.side):
                rc = fn(*a)
            if rc == 0:
                g.replay()
                self.graphs.append(g)
            return rc
        return call


def test_new_entries_keep_the_stream_contract():
    """default stream, side stream, and every call captured alone then replayed: the weights of the table's graph and the slots
    and state of two weighted sampler launches are the same bits in all three"""
    from dglke_amd import _lib
    from dglke_amd.dataloader import DeviceSampler, subsampling_weights
    h, r, t = SC.graph()
    ref = SC.weights64(h, r, t, SC.N_REL)

    def run(verify):
        w = subsampling_weights(h, r, t, SC.N_ENT, SC.N_REL, DEV)
        smp = DeviceSampler(h, r, t, SC.N_ENT, STEP_B, STEP_N, DEV, n_slots=3, seed=2, edge_importance=w)
        smp.sample(3)
        first = smp.slots.clone()
        smp.sample(2)
        torch.cuda.current_stream().synchronize()
        if verify:
            got = w.cpu().numpy().astype(np.float64)
            assert (np.abs(got - ref) / ref).max() <= 4 * U
            a = smp.slot_arrays(0)
            where = dict(zip(zip(h.tolist(), r.tolist(), t.tolist()), got.tolist()))
            assert [where[x] for x in zip(a["h_gid"].tolist(), a["rel_ids"].tolist(), a["t_gid"].tolist())] == a["edge_w"].astype(np.float64).tolist()
        return dict(weights=w, first=first, slots=smp.slots.clone(), state=smp.state.clone())
    p = _Probe(_lib.lib(), torch.cuda.Stream())
    got = {}
    for mode in SG.MODES:
        n0 = len(p.calls)
        with SG._installed(p, mode):
            got[mode] = SG._tensors(run(mode == "default"))
        names = [n for m, n in p.calls[n0:] if m == mode]
        assert names.count("kge_subsampling_weights") == 2 and names.count("kge_sample_batches_weighted") == 2, (mode, names)
    SG._same(got["default"], got["side"], "on the side stream against the default stream")
    SG._same(got["default"], got["capture"], "every call captured and replayed against the default stream")
