"""CPU side of `--checkpoint_interval` / `--resume`: the file layer of dglke_amd/checkpoint.py, `find_latest`, the compatibility
check, the refusals `dglke_train` raises before it touches anything, the host sampler's state and the loop's marks.  The restarts
themselves run in tests/test_gpu_checkpoint.py."""
import json
import os

import numpy as np
import pytest
import torch

import checkpoint_cases as CK
import train_loop_cases as L
from dglke_amd import checkpoint as C
from dglke_amd import train as T
from dglke_amd._lib import KgeError
from dglke_amd.dataloader import UniformChunkedSampler


# ---- file layer --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,dtype", [((1001, 12), np.float32), ((1001,), np.float32), ((37, 2, 8), np.float32),
                                         ((0, 4), np.float32), ((4000,), np.int64)])
@pytest.mark.parametrize("tensor", [False, True], ids=["array", "tensor"])
def test_blockwise_file_is_np_saves_file(tmp_path, shape, dtype, tensor):
    """a block of 1000 bytes divides neither 1001 rows of 48 bytes nor 1001 floats: the last block is a short one"""
    a = (np.random.RandomState(1).standard_normal(shape) * 100).astype(dtype)
    np.save(str(tmp_path / "want.npy"), a)
    n = C.write_npy_blocks(str(tmp_path / "got.npy"), torch.from_numpy(a) if tensor else a, block_bytes=1000)
    want, got = (tmp_path / "want.npy").read_bytes(), (tmp_path / "got.npy").read_bytes()
    assert n == len(got) and got == want
    back = np.load(str(tmp_path / "got.npy"))
    assert back.dtype == a.dtype and back.shape == a.shape and np.array_equal(back, a)
    assert C.file_entry(str(tmp_path / "got.npy")) == dict(shape=list(shape), dtype=np.dtype(dtype).str, bytes=len(want))


def test_blockwise_read_fills_the_tensor_in_place(tmp_path):
    a = np.random.RandomState(2).standard_normal((1001, 12)).astype(np.float32)
    np.save(str(tmp_path / "a.npy"), a)
    dst = torch.zeros(1001, 12)
    p = dst.data_ptr()
    C.read_npy_blocks(str(tmp_path / "a.npy"), dst, block_bytes=1000)
    assert dst.data_ptr() == p and np.array_equal(dst.numpy(), a)
    with pytest.raises(KgeError, match="a.npy"):
        C.read_npy_blocks(str(tmp_path / "a.npy"), torch.zeros(1001, 13))
    with pytest.raises(KgeError, match="a.npy"):
        C.read_npy_blocks(str(tmp_path / "a.npy"), torch.zeros(1001, 12, dtype=torch.float64))


def _tensors(seed):
    r = np.random.RandomState(seed)
    return {"toy_TransE_l2_entity.npy": torch.from_numpy(r.standard_normal((50, 8)).astype(np.float32)),
            "toy_TransE_l2_relation.npy": r.standard_normal((5, 8)).astype(np.float32),
            "toy_TransE_l2_entity_state.npy": r.uniform(size=50).astype(np.float32)}


def _args(**over):
    a = vars(T.ArgParser().parse_args(L.argv("data", "ckpts", "TransE_l2", 20, 50, [])))
    a.update(over)
    return a


def _write(run, step, seed=0, **over):
    meta = dict(step=step, since_log=step % 50, args=_args(**over), n_entities=50, n_relations=5, n_train=4000, lanes=[])
    return C.write_checkpoint(str(run), _tensors(seed), meta)


def test_round_trip_and_only_the_newest_is_kept(tmp_path):
    run = tmp_path / "TransE_l2_toy_0"
    run.mkdir()
    n = _write(run, 100, seed=1)
    assert n == sum(f.stat().st_size for f in (run / "checkpoint").iterdir())
    _write(run, 200, seed=2)
    assert sorted(os.listdir(str(run))) == ["checkpoint"]
    d, meta = C.locate(str(run))
    assert d == str(run / "checkpoint") and meta["step"] == 200 and meta["format_version"] == C.FORMAT_VERSION
    C.verify_files(d, meta)
    for name, t in _tensors(2).items():
        got = np.load(os.path.join(d, name))
        assert got.dtype == np.float32 and np.array_equal(got, np.asarray(t))
        assert meta["files"][name] == dict(shape=list(got.shape), dtype="<f4", bytes=os.path.getsize(os.path.join(d, name)))
    # the checkpoint directory itself is a PATH too
    assert C.locate(d)[1]["step"] == 200


def test_interrupted_write_leaves_the_previous_checkpoint(tmp_path, monkeypatch):
    run = tmp_path / "TransE_l2_toy_0"
    run.mkdir()
    _write(run, 100, seed=1)
    real, calls = C.write_npy_blocks, []

    def failing(path, src, block_bytes=C.BLOCK_BYTES):
        calls.append(path)
        if len(calls) == 2:
            raise OSError("disk full")
        return real(path, src, block_bytes)
    monkeypatch.setattr(C, "write_npy_blocks", failing)
    with pytest.raises(OSError):
        _write(run, 200, seed=2)
    monkeypatch.setattr(C, "write_npy_blocks", real)
    assert len(calls) == 2 and os.path.isdir(str(run / "checkpoint.tmp"))
    d, meta = C.locate(str(run))
    assert d == str(run / "checkpoint") and meta["step"] == 100
    C.verify_files(d, meta)
    assert np.array_equal(np.load(os.path.join(d, "toy_TransE_l2_relation.npy")), _tensors(1)["toy_TransE_l2_relation.npy"])
    # the next write clears the partial directory away
    _write(run, 300, seed=3)
    assert sorted(os.listdir(str(run))) == ["checkpoint"] and C.locate(str(run))[1]["step"] == 300


def test_checkpoint_old_is_the_fallback_and_is_announced(tmp_path):
    run = tmp_path / "TransE_l2_toy_0"
    run.mkdir()
    _write(run, 100)
    # a write interrupted between its two renames: checkpoint/ is gone, checkpoint.old/ stands
    os.rename(str(run / "checkpoint"), str(run / "checkpoint.old"))
    said = []
    d, meta = C.locate(str(run), log=said.append)
    assert d == str(run / "checkpoint.old") and meta["step"] == 100
    assert len(said) == 1 and "checkpoint.old" in said[0]
    # ... or checkpoint/ is there without a readable checkpoint.json
    (run / "checkpoint").mkdir()
    (run / "checkpoint" / "checkpoint.json").write_text("{ not json")
    assert C.locate(str(run), log=said.append)[0] == str(run / "checkpoint.old")
    # neither: refused
    os.rename(str(run / "checkpoint.old"), str(run / "gone"))
    with pytest.raises(KgeError, match="no readable checkpoint"):
        C.locate(str(run), log=said.append)
    # the next write of a run whose checkpoint.old was left behind ends with checkpoint/ alone
    os.rename(str(run / "gone"), str(run / "checkpoint.old"))
    os.remove(str(run / "checkpoint" / "checkpoint.json"))
    os.rmdir(str(run / "checkpoint"))
    _write(run, 200)
    assert sorted(os.listdir(str(run))) == ["checkpoint"] and C.locate(str(run))[1]["step"] == 200


def test_truncated_file_is_refused_by_name(tmp_path):
    run = tmp_path / "TransE_l2_toy_0"
    run.mkdir()
    _write(run, 100)
    d, meta = C.locate(str(run))
    f = os.path.join(d, "toy_TransE_l2_entity.npy")
    raw = open(f, "rb").read()
    with open(f, "wb") as fh:
        fh.write(raw[:-4])
    with pytest.raises(KgeError, match="toy_TransE_l2_entity.npy"):
        C.verify_files(d, meta)
    # the right size with another header
    np.save(f, np.zeros((8, 50), np.float32))
    assert os.path.getsize(f) == len(raw)
    with pytest.raises(KgeError, match=r"toy_TransE_l2_entity.npy holds .*\[8, 50\]"):
        C.verify_files(d, meta)
    os.remove(f)
    with pytest.raises(KgeError, match="toy_TransE_l2_entity.npy is missing"):
        C.verify_files(d, meta)


def test_future_format_is_refused(tmp_path):
    run = tmp_path / "TransE_l2_toy_0"
    run.mkdir()
    _write(run, 100)
    f = run / "checkpoint" / "checkpoint.json"
    meta = json.loads(f.read_text())
    meta["format_version"] = C.FORMAT_VERSION + 1
    f.write_text(json.dumps(meta))
    with pytest.raises(KgeError, match="format %d" % (C.FORMAT_VERSION + 1)):
        C.locate(str(run))
    # (not skipped in favour of an older one either)
    os.makedirs(str(run / "checkpoint.old"))
    (run / "checkpoint.old" / "checkpoint.json").write_text(json.dumps(dict(meta, format_version=C.FORMAT_VERSION)))
    with pytest.raises(KgeError, match="format %d" % (C.FORMAT_VERSION + 1)):
        C.locate(str(run))


# ---- find_latest ---------------------------------------------------------------------------------------------------------------

def test_find_latest(tmp_path):
    save = tmp_path / "ckpts"
    assert C.find_latest(str(save), "TransE_l2", "toy") is None           # no save path at all
    save.mkdir()
    assert C.find_latest(str(save), "TransE_l2", "toy") is None           # an empty one
    for n in (0, 1, 2, 10, 11):
        (save / ("TransE_l2_toy_%d" % n)).mkdir()
    (save / "TransE_l2_toy_x").mkdir()
    (save / "TransE_l2_toyota_50").mkdir()
    (save / "RotatE_toy_40").mkdir()
    assert C.find_latest(str(save), "TransE_l2", "toy") is None           # runs, none with a checkpoint
    _write(save / "TransE_l2_toy_1", 100)
    _write(save / "TransE_l2_toy_2", 40)
    _write(save / "RotatE_toy_40", 70)
    _write(save / "TransE_l2_toyota_50", 70)
    assert C.find_latest(str(save), "TransE_l2", "toy") == str(save / "TransE_l2_toy_2")
    _write(save / "TransE_l2_toy_10", 60)                                 # numbered, not sorted as text: 10 > 2
    assert C.find_latest(str(save), "TransE_l2", "toy") == str(save / "TransE_l2_toy_10")
    # run 11 stands without a checkpoint and is skipped; one whose write never finished is skipped too
    (save / "TransE_l2_toy_11" / "checkpoint.tmp").mkdir()
    assert C.find_latest(str(save), "TransE_l2", "toy") == str(save / "TransE_l2_toy_10")
    os.rename(str(save / "TransE_l2_toy_10" / "checkpoint"), str(save / "TransE_l2_toy_10" / "checkpoint.old"))
    assert C.find_latest(str(save), "TransE_l2", "toy") == str(save / "TransE_l2_toy_10")
    assert C.find_latest(str(save), "RotatE", "toy") == str(save / "RotatE_toy_40")


# ---- compatibility -------------------------------------------------------------------------------------------------------------

OTHER = dict(model_name="RotatE", hidden_dim=64, double_ent=True, double_rel=True, optimizer="Adam", num_proc=3, batch_size=128,
             neg_sample_size=32, seed=7, has_edge_importance=True, subsampling_weight=True, edge_importance_on_device=True,
             dataset="FB15k")


def test_the_must_equal_keys_are_the_issues():
    assert sorted(OTHER) == sorted(C.MUST_EQUAL) and len(C.MUST_EQUAL) == 13


@pytest.mark.parametrize("key", sorted(OTHER))
def test_every_must_equal_key_is_refused_with_both_values(key):
    saved, given = _args(), _args(**{key: OTHER[key]})
    assert C.check_compatible(saved, saved) == []
    with pytest.raises(KgeError) as e:
        C.check_compatible(saved, given)
    assert "--%s " % key in str(e.value) and repr(saved[key]) in str(e.value) and repr(given[key]) in str(e.value)


def test_batch_size_is_compared_after_rounding_to_the_negative_sample_size():
    saved = _args(batch_size=64, neg_sample_size=16)
    assert C.check_compatible(saved, _args(batch_size=60, neg_sample_size=16)) == []      # 60 trains as 64
    with pytest.raises(KgeError, match="--batch_size"):
        C.check_compatible(saved, _args(batch_size=48, neg_sample_size=16))
    assert T.get_compatible_batch_size(60, 16, quiet=True) == 64


FREE = dict(lr=0.01, adam_beta1=0.8, adam_beta2=0.99, adam_eps=1e-6, regularization_coef=0.0, regularization_norm=2,
            loss_genre="Hinge", neg_adversarial_sampling=False, adversarial_temperature=0.5, graph_steps=0, log_interval=7,
            eval_interval=9, checkpoint_interval=11, max_step=1000, valid=True, test=True, gamma=3.0, margin=2.0, pairwise=True,
            neg_deg_sample=True, exclude_positive=True, async_update=True, force_sync_interval=10, batch_size_eval=4,
            neg_sample_size_eval=12, no_save_emb=True, gpu=[1], data_path="elsewhere", eval_percent=0.5)


@pytest.mark.parametrize("key", sorted(FREE))
def test_every_free_key_is_accepted_and_reported(key):
    saved = _args()
    assert key in saved and key not in C.MUST_EQUAL and saved[key] != FREE[key]
    assert C.check_compatible(saved, _args(**{key: FREE[key]})) == [(key, saved[key], FREE[key])]


def test_where_a_run_writes_is_no_difference_and_later_derived_values_are_not_either():
    saved = _args(save_path="ckpts/TransE_l2_toy_0", neg_sample_size_eval=700, eval_filter=True)
    parsed = _args()
    given = _args(save_path="ckpts", resume="ckpts/TransE_l2_toy_0", lr=0.1)
    assert C.check_compatible(saved, given, parsed) == [("lr", 0.25, 0.1)]


# ---- refusals of dglke_train: before the GPU, the dataset or --save_path ----------------------------------------------------------

@pytest.mark.parametrize("flag", [["--checkpoint_interval", "10"], ["--resume", "nowhere"]], ids=["checkpoint_interval", "resume"])
@pytest.mark.parametrize("extra,word", [(["--gpu", "0", "1"], "more than one GPU"),
                                        (["--async_update", "--async_update_pipeline"], "--async_update_pipeline"),
                                        (["--async_update", "--async_update_rel"], "--async_update_rel")],
                         ids=["two_gpus", "pipeline", "async_rel"])
def test_flag_refusals_arrive_before_anything_is_touched(tmp_path, flag, extra, word):
    a = L.argv(str(tmp_path / "no_data"), str(tmp_path / "ckpts"), "TransE_l2", 20, 50, flag + extra)
    with pytest.raises(KgeError) as e:
        T.main(a)
    assert word in str(e.value) and flag[0] in str(e.value)
    assert not os.path.exists(str(tmp_path / "ckpts")) and not os.path.exists(str(tmp_path / "no_data"))


def test_plain_async_update_is_not_refused():
    C.check_flags(T.ArgParser().parse_args(["--checkpoint_interval", "10", "--async_update", "--gpu", "0"]))
    C.check_flags(T.ArgParser().parse_args(["--gpu", "0", "1", "--async_update", "--async_update_rel"]))      # neither flag


@pytest.mark.parametrize("max_step", [100, 60])
def test_max_step_at_or_below_the_checkpoint_is_refused_with_both_numbers(tmp_path, max_step):
    run = tmp_path / "old" / "TransE_l2_toy_0"
    run.mkdir(parents=True)
    _write(run, 100)
    a = L.argv(str(tmp_path / "no_data"), str(tmp_path / "ckpts"), "TransE_l2", 20, 50, ["--resume", str(run)], max_step)
    with pytest.raises(KgeError) as e:
        T.main(a)
    assert "step 100" in str(e.value) and "--max_step is %d" % max_step in str(e.value)
    assert not os.path.exists(str(tmp_path / "ckpts"))
    assert sorted(os.listdir(str(run))) == ["checkpoint"]                 # --resume only reads


def test_incompatible_resume_is_refused_before_the_dataset(tmp_path):
    run = tmp_path / "old" / "TransE_l2_toy_0"
    run.mkdir(parents=True)
    _write(run, 100)
    a = L.argv(str(tmp_path / "no_data"), str(tmp_path / "ckpts"), "TransE_l2", 20, 50, ["--resume", str(run), "--seed", "3"])
    with pytest.raises(KgeError, match="--seed is 0 in the checkpoint and 3 on this command line"):
        T.main(a)
    assert not os.path.exists(str(tmp_path / "ckpts"))


def test_resume_latest_without_a_checkpoint_says_so(tmp_path):
    args = T.ArgParser().parse_args(L.argv("data", str(tmp_path / "ckpts"), "TransE_l2", 20, 50, ["--resume", "latest"]))
    said = []
    assert C.open_resume(args, log=said.append) is None
    assert len(said) == 1 and "fresh run" in said[0]
    run = tmp_path / "ckpts" / "TransE_l2_toy_0"
    run.mkdir(parents=True)
    _write(run, 100, save_path=str(run))
    r = C.open_resume(args, log=said.append)
    assert (r.path, r.step, r.since_log) == (str(run / "checkpoint"), 100, 0)


# ---- the host sampler ------------------------------------------------------------------------------------------------------------

def test_host_sampler_continues_across_its_epoch_boundary():
    """70 plans of 64 out of 4000 triples: the second permutation is drawn for plan 63; the state is taken after 40"""
    r = np.random.RandomState(5)
    h, rel, t = r.randint(0, L.N_ENT, L.N_TRAIN), r.randint(0, L.N_REL, L.N_TRAIN), r.randint(0, L.N_ENT, L.N_TRAIN)
    w = r.uniform(0.5, 1.5, L.N_TRAIN).astype(np.float32)

    def sampler():
        return UniformChunkedSampler(h, rel, t, L.N_ENT, L.BATCH, L.NEG, "cpu", neg_chunk_size=L.NEG, seed=11, edge_importance=w)
    a = sampler()
    plans = a.next_plans(40)
    st = a.get_state()
    assert (st["kind"], st["step"], st["pos"]) == ("host", 40, 40 * L.BATCH)
    st = json.loads(json.dumps(dict(st, perm=st["perm"].tolist())))        # through text, as a checkpoint stores it
    plans += a.next_plans(30)
    assert a._pos == 8 * L.BATCH                                            # 62 + 8: the boundary is behind
    b = sampler()
    b.set_state(st)
    again = b.next_plans(30)
    assert b.step == a.step == 70
    for k, (p, q) in enumerate(zip(plans[40:], again)):
        assert sorted(p) == sorted(q)
        for key in p:
            x, y = p[key], q[key]
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and np.array_equal(x, y), (41 + k, key)
            else:
                assert x == y, (41 + k, key)
        assert bool(p["neg_head"]) == ((41 + k) % 2 == 0)
    # a fresh sampler's state (no permutation yet) goes through too
    c = sampler()
    c.set_state(sampler().get_state())
    assert np.array_equal(c.next_plans(1)[0]["neg_ids"], plans[0]["neg_ids"])


# ---- step_marks ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", L.ROWS, ids=L.ROW_IDS)
def test_step_marks_defaults_change_nothing(row):
    _, G, log, flags = row
    ev, valid = L.eval_interval(flags), "--valid" in flags
    want = sorted({L.MAX_STEP} | set(range(log, L.MAX_STEP + 1, log)) | (set(range(ev, L.MAX_STEP + 1, ev)) if valid else set()))
    assert T.step_marks(L.MAX_STEP, log, ev, valid) == want
    assert T.step_marks(L.MAX_STEP, log, ev, valid, -1, False) == want
    assert T.step_marks(L.MAX_STEP, log, ev, valid, -1, False, checkpoint_interval=0, start_step=0) == want


def test_step_marks_with_an_interval_and_a_start():
    assert T.step_marks(230, 50, 10000, False, checkpoint_interval=45) == [45, 50, 90, 100, 135, 150, 180, 200, 225, 230]
    assert T.step_marks(230, 50, 10000, False, checkpoint_interval=45, start_step=45) == [50, 90, 100, 135, 150, 180, 200, 225, 230]
    assert T.step_marks(230, 50, 10000, False, start_step=100) == [150, 200, 230]
    assert T.step_marks(230, 50, 10000, False, start_step=124) == [150, 200, 230]
    assert T.step_marks(124, 50, 10000, False, checkpoint_interval=124, start_step=45) == [50, 100, 124]
    assert T.step_marks(230, 1000, 10000, False, checkpoint_interval=1000, start_step=229) == [230]


# ---- the case table ----------------------------------------------------------------------------------------------------------------

def test_cases_are_what_their_comments_say():
    assert CK.EPOCH == 62 and CK.MAX_STEP == 230
    assert CK.case("odd_step")[4] == [45] and 45 % 2 == 1 and 45 % 20 and 45 % 50
    assert CK.case("epoch_opens")[4] == [124] and 124 % CK.EPOCH == 0            # step 125 is an epoch's first batch
    assert CK.case("host_sampler")[4] == [100] and 100 - CK.EPOCH == 38
    assert CK.case("graphs_to_eager")[5] == (20, 0)
    assert CK.case("chained")[4] == [45, 124]
    for c in CK.CASES:
        assert all(0 < k < CK.MAX_STEP for k in c[4]) and CK.n_tables(c) in (4, 6)
    assert CK.n_tables(CK.case("transr")) == 6 and CK.n_tables(CK.case("adam")) == 6


def test_case_command_lines():
    c = CK.case("chained")
    a = T.ArgParser().parse_args(CK.argv_a(c, "d", "s"))
    assert (a.max_step, a.checkpoint_interval, a.resume) == (230, 0, None)
    b0, b1, b2 = (T.ArgParser().parse_args(CK.argv_b(c, "d", "s", i, resume="run")) for i in range(3))
    assert (b0.max_step, b0.checkpoint_interval, b0.resume) == (45, 45, None)
    assert (b1.max_step, b1.checkpoint_interval, b1.resume) == (124, 124, "run")
    assert (b2.max_step, b2.checkpoint_interval, b2.resume) == (230, 0, "run")
    g = CK.case("graphs_to_eager")
    assert T.ArgParser().parse_args(CK.argv_b(g, "d", "s", 0)).graph_steps == 20
    assert T.ArgParser().parse_args(CK.argv_b(g, "d", "s", 1, resume="run")).graph_steps == 0
