"""`--checkpoint_interval` / `--resume`: a run cut at step K and continued from its checkpoint ends with the tables, optimizer
state and moment tables of the uninterrupted run, bit for bit - no tolerance anywhere but on the printed averages, which are fp32
sums.  What makes that checkable: one lane on the strict step trains the straight-line sequence of steps whatever the marks and
groups are (test_gpu_train_trajectory), batch k depends on (seed, k) alone (test_gpu_sampler_statement), validation only reads.

Protocol (tests/checkpoint_cases.py): run A = `--max_step 230`; B1 = `--max_step K --checkpoint_interval K`; B2 = `--resume <B1's
run directory> --max_step 230`.  Every run is cached per module and only read afterwards."""
import contextlib
import io
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import checkpoint_cases as CK
import train_loop_cases as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _cpu(named):
    torch.cuda.synchronize()
    return {k: t.detach().cpu().clone() for k, t in named.items()}


def last_group(start, max_step, log, G, timers, ckpt_iv=0):
    """(steps in it, its first step) of the last group of steps a one-lane device-sampler run from step `start` enqueues: the
    loop of train_loop_cases.chain from a start step (the slot of step max_step is the group's last)"""
    from dglke_amd import train as T
    n_slots = max(2, G or 2)
    hs, have, rem, step, last = start + 1, False, set(), start, None
    for nxt in T.step_marks(max_step, log, 10000, False, -1, False, ckpt_iv, start):
        n = nxt - step
        want = timers and nxt % log == 0
        acts, after = T.plan_enqueue(n - 1 if want else n, G, hs, have, n_slots, frozenset(rem))
        s = hs
        for kind, k, par in acts:
            have = have or kind == "capture_group"
            if kind == "capture_rem":
                rem.add((k, par))
            if kind in L.RUNNING:
                last, s = (k, s), s + k
        assert s == after
        hs = after
        if want:
            last, hs = (1, hs), hs + 1
        step = nxt
    assert hs == max_step + 1
    return last


class Runs(object):
    """the runs of this module, each trained once"""

    def __init__(self, root):
        self.root, self.n, self.data, self.done = root, 0, {}, {}

    def data_dir(self, weights):
        if weights not in self.data:
            self.data[weights] = os.path.join(self.root, "kg_w" if weights else "kg")
            L.write_planted(self.data[weights], weights=weights)
        return self.data[weights]

    def save_dir(self):
        self.n += 1
        return os.path.join(self.root, "ckpts%d" % self.n)

    def train(self, key, argv, keep=False):
        if key in self.done:
            return self.done[key]
        from dglke_amd import train as T
        rec = {}

        def before_train(tr):
            rec["hook"] = _cpu(tr.model.engine.named_tensors())
            rec["hook_accum"] = [lane.engine.loss_accum.detach().cpu().clone() for lane in tr.lanes]
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            tr = T.main(argv, before_train=before_train)
        a = tr.args
        rec.update(out=out.getvalue(), final=_cpu(tr.model.engine.named_tensors()), run_dir=a.save_path, args=a,
                   accum=[lane.engine.loss_accum.detach().cpu().clone() for lane in tr.lanes],
                   device_sampler=tr.device_sampler, n_lanes=tr.n_lanes)
        rec["saved"] = {n: np.load(os.path.join(a.save_path, "toy_%s%s.npy" % (a.model_name, s)))
                        for n, s in (("entity", "_entity"), ("relation", "_relation"), ("projection", "projection"))
                        if n in rec["final"]}
        start = int(re.search(r"at step (\d+) of the run", rec["out"]).group(1)) if a.resume else 0
        rec["lanes"] = []
        for lane in tr.lanes:
            smp = lane.sampler
            if not tr.device_sampler:
                rec["lanes"].append(dict(host_step=smp.step + 1))
                continue
            k, first = last_group(start, a.max_step, a.log_interval, a.graph_steps, tr.n_lanes == 1, a.checkpoint_interval)
            rec["lanes"].append(dict(host_step=smp.host_step, device_step=int(smp.state[1]), last_first=first, last_slot=k - 1,
                                     slot_neg_head=int(smp.slot_arrays(k - 1)["counts"][2])))
        ck = os.path.join(a.save_path, "checkpoint")
        if os.path.isdir(ck):
            with open(os.path.join(ck, "checkpoint.json")) as f:
                rec["meta"] = json.load(f)
            rec["files"] = {n: np.load(os.path.join(ck, n)) for n in rec["meta"]["files"]}
            rec["run_listing"] = sorted(os.listdir(a.save_path))
        if keep:
            rec["trainer"] = tr
        self.done[key] = rec
        return rec

    def run_a(self, c, extra=()):
        return self.train(("A", c[1], tuple(c[2]), c[5][0], tuple(extra)),
                          CK.argv_a(c, self.data_dir(c[3]), self.save_dir()) + list(extra), keep=bool(extra))

    def run_b(self, c, i, extra=(), all_extra=()):
        """run i of the case's chain (0: B1 ... len(K): the last), its predecessors trained first"""
        prev = self.run_b(c, i - 1, all_extra=all_extra)["run_dir"] if i > 0 else None
        g = c[5][0] if i == 0 else c[5][1]
        key = ("B", c[1], tuple(c[2]), tuple(c[4][:i + 1]), i == len(c[4]), g, tuple(extra), tuple(all_extra))
        return self.train(key, CK.argv_b(c, self.data_dir(c[3]), self.save_dir(), i, prev, list(extra) + list(all_extra)))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(str(tmp_path_factory.mktemp("checkpoint")))


FILE_OF = {"entity": "_entity", "relation": "_relation", "projection": "projection", "entity_state": "_entity_state",
           "relation_state": "_relation_state", "projection_state": "projection_state", "entity_mom": "_entity_mom",
           "relation_mom": "_relation_mom"}


def _file(rec, name):
    return rec["files"]["toy_%s%s.npy" % (rec["args"].model_name, FILE_OF[name])]


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    for name in sorted(a):
        x, y = a[name], b[name]
        assert x.shape == y.shape and x.dtype == y.dtype, name
        bad = (x != y).reshape(x.shape[0], -1).any(1).nonzero().flatten()
        assert torch.equal(x, y), "%s: %s differs in %d rows (first: %s)" % (what, name, len(bad), bad[:8].tolist())


def _assert_counters(rec, max_step=CK.MAX_STEP):
    assert rec["lanes"]
    for k, lane in enumerate(rec["lanes"]):
        assert lane["host_step"] == max_step + 1, (k, lane)
        if rec["device_sampler"]:
            assert lane["device_step"] == max_step + 1, (k, lane)
            assert lane["last_first"] + lane["last_slot"] == max_step, (k, lane)
            assert lane["slot_neg_head"] == int(max_step % 2 == 0), (k, lane)


def _assert_hook_is_the_checkpoint(b_prev, b):
    """in the resumed run's before_train hook the tables are the predecessor's final tables and its checkpoint's files"""
    _assert_same(b["hook"], b_prev["final"], "restored state against the checkpointed run's final tables")
    for name, t in b["hook"].items():
        f = _file(b_prev, name)
        assert f.dtype == np.float32 and np.array_equal(f, t.numpy()), "%s: the restored table is not the checkpoint's file" % name
    for k, acc in enumerate(b["hook_accum"]):
        assert torch.equal(acc, b_prev["accum"][k]), "lane %d: loss sums" % k
        assert np.array_equal(b_prev["files"]["lane%d_loss_accum.npy" % k], acc.numpy())


@pytest.mark.parametrize("cid", CK.CASE_IDS)
def test_restart_is_bit_exact(runs, cid):
    """1: after the last run of the chain every table, state and moment table is run A's; the saved model files are the tables;
    run A trained every one of them"""
    c = CK.case(cid)
    a, b = runs.run_a(c), runs.run_b(c, len(c[4]))
    assert len(a["final"]) == len(b["final"]) == CK.n_tables(c)
    assert a["device_sampler"] == b["device_sampler"] == (cid != "host_sampler")
    for name in a["final"]:
        assert not torch.equal(a["final"][name], a["hook"][name]), "%s: run A did not train it" % name
    _assert_same(b["final"], a["final"], "resumed run against the uninterrupted run")
    for name, arr in b["saved"].items():
        assert np.array_equal(arr, b["final"][name].numpy()), "%s: the saved file is not the table" % name
    assert "checkpoint at step" not in a["out"] and not os.path.exists(os.path.join(a["run_dir"], "checkpoint"))


@pytest.mark.parametrize("cid", CK.CASE_IDS)
def test_restored_state_and_counters(runs, cid):
    """2: the hook of every resumed run sees its predecessor's final state, which is the checkpoint's files; after the last run
    host step = device step = 231 on the lane and the last slot holds step 230's side"""
    c = CK.case(cid)
    for i in range(1, len(c[4]) + 1):
        prev, b = runs.run_b(c, i - 1), runs.run_b(c, i)
        k = c[4][i - 1]
        assert prev["meta"]["step"] == k and prev["meta"]["since_log"] == k % CK.LOOP[1]
        assert prev["run_listing"].count("checkpoint") == 1 and "checkpoint.tmp" not in prev["run_listing"]
        assert "checkpoint.old" not in prev["run_listing"]
        assert "[proc 0]checkpoint at step %d: " % k in prev["out"]
        _assert_counters(prev, k)
        _assert_hook_is_the_checkpoint(prev, b)
        assert b["run_dir"] != prev["run_dir"]                    # a run directory of its own
    _assert_counters(b)


def test_log_across_a_restart(runs):
    """3: K = 45, --log_interval 50: the resumed run's averages at mark 50 cover steps 1 .. 50 - those of run A at rtol 1e-3 (fp32
    sums of <= 64 non-negative terms per step over <= 230 steps: 64 * 230 * 2^-24 ~ 9e-4, the bound of
    test_gpu_train_trajectory.test_printed_averages_are_the_means_of_the_straight_line_losses).  A lost step count or lost sums
    move the value by a factor 5 / 50 or 50 / 5"""
    c = CK.case("odd_step")
    a, b = runs.run_a(c), runs.run_b(c, 1)

    def lines(rec):
        return {(int(m.group(1)), m.group(2)): float(m.group(3)) for m in
                re.finditer(r"^\[proc 0\]\[Train\]\((\d+)/%d\) average (\w+): (\S+)$" % CK.MAX_STEP, rec["out"], re.M)}
    la, lb = lines(a), lines(b)
    marks = [50, 100, 150, 200]
    assert sorted({k for k, _ in la}) == sorted({k for k, _ in lb}) == marks
    assert min(k for k, _ in lb) > 45
    for term in ("pos_loss", "neg_loss", "loss", "regularization"):
        for k in marks:
            x, y = lb[(k, term)], la[(k, term)]
            print("%s at %d: resumed %.9g, uninterrupted %.9g, rel %.2e" % (term, k, x, y, abs(x - y) / y))
            assert y > 0 and abs(x - y) <= 1e-3 * y, (term, k, x, y)
    assert "[proc 0][Train] 50 steps take" in b["out"]


def test_checkpointing_is_read_only(runs):
    """4: run A with checkpoints at 100, 200 and 230 ends with run A's tables; checkpoint/ holds step 230 and its files are the
    final tables, states and loss sums"""
    c = CK.case("odd_step")
    a, w = runs.run_a(c), runs.run_a(c, ("--checkpoint_interval", "100", "--test"))
    _assert_same(w["final"], a["final"], "run with checkpoints against run without")
    assert [int(k) for k in re.findall(r"^\[proc 0\]checkpoint at step (\d+): \d+ bytes in [\d.]+ s$", w["out"], re.M)] == [100, 200, 230]
    meta = w["meta"]
    assert (meta["step"], meta["since_log"]) == (230, 30)
    assert (meta["n_entities"], meta["n_relations"], meta["n_train"]) == (L.N_ENT, L.N_REL, L.N_TRAIN)
    assert meta["abi_version"] == 8 and meta["torch_version"] == torch.__version__ and meta["args"]["max_step"] == 230
    assert w["run_listing"].count("checkpoint") == 1
    assert not [n for n in w["run_listing"] if n in ("checkpoint.tmp", "checkpoint.old")]
    for name, t in w["final"].items():
        assert np.array_equal(_file(w, name), t.numpy()), name
    assert np.array_equal(w["files"]["lane0_loss_accum.npy"], w["accum"][0].numpy()) and w["accum"][0].abs().sum() > 0
    st = meta["lanes"][0]["sampler"]
    assert st["kind"] == "device" and len(st["state"]) == 8 and st["state"][1] == 231 and st["host_step"] == 231
    with open(os.path.join(w["run_dir"], "checkpoint", "config.json")) as f, open(os.path.join(w["run_dir"], "config.json")) as g:
        assert json.load(f) == json.load(g)
    for n, e in meta["files"].items():
        assert e["bytes"] == os.path.getsize(os.path.join(w["run_dir"], "checkpoint", n)) and list(w["files"][n].shape) == e["shape"]


def test_a_checkpoint_is_a_model_directory(runs):
    """5: dglke_eval on RUN/checkpoint prints the metrics the trainer's own test gives on the same tables"""
    from dglke_amd import eval_cli
    c = CK.case("odd_step")
    w = runs.run_a(c, ("--checkpoint_interval", "100", "--test"))
    want = re.findall(r"^\[0\]Test average (\S+): (\S+)$", w["out"], re.M)
    assert {"MRR", "MR", "HITS@1", "HITS@3", "HITS@10"} <= {k for k, _ in want}, w["out"][-1500:]
    data = runs.data_dir(False)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        eval_cli.main(["--model_name", c[1], "--format", "udd_hrt", "--dataset", "toy", "--data_path", data, "--data_files", "e.dict",
                       "r.dict", "train.txt", "valid.txt", "test.txt", "--model_path", os.path.join(w["run_dir"], "checkpoint"),
                       "--gpu", "0", "--hidden_dim", str(L.HIDDEN), "-g", "8"])
    got = re.findall(r"^\[0\]Test average (\S+): (\S+)$", out.getvalue(), re.M)
    assert got == want and float(dict(got)["MRR"]) > 0


def test_lanes(runs):
    """6: --num_proc 3, K = 100.  The lanes are lock-free on shared tables, so the tables are nobody's reference; the restored
    state is the checkpoint, every lane ends at step 231 with its sides in step and prints its average at 150"""
    c = ("lanes", "TransE_l2", [], False, [100], (20, 20))
    flags = ("--num_proc", "3")
    b1, b2 = runs.run_b(c, 0, all_extra=flags), runs.run_b(c, 1, all_extra=flags)
    assert b1["n_lanes"] == b2["n_lanes"] == 3 and len(b1["meta"]["lanes"]) == 3
    _assert_hook_is_the_checkpoint(b1, b2)
    _assert_counters(b1, 100)
    _assert_counters(b2)
    for k in range(3):
        assert "[proc %d][Train](150/230) average loss:" % k in b2["out"]
        assert "[proc %d][Train](100/230)" % k not in b2["out"]
        assert b1["meta"]["lanes"][k]["sampler"]["host_step"] == 101


def test_changed_flags(runs):
    """7: everything but the must-equal flags may change: a restart at another --lr says so, runs to the end and trains other
    tables"""
    c = CK.case("odd_step")
    a, b = runs.run_a(c), runs.run_b(c, 1, extra=("--lr", "0.1"))
    assert "--resume: --lr was 0.25 in the checkpointed run, is 0.1 now" in b["out"]
    assert "--resume: --max_step was 45 in the checkpointed run, is 230 now" in b["out"]
    assert "[proc 0][Train](200/230) average loss:" in b["out"]
    _assert_counters(b)
    for name in ("entity", "relation", "entity_state", "relation_state"):
        assert not torch.equal(a["final"][name], b["final"][name]), name
