"""What `_Trainer.train` and `_Lane.enqueue` enqueue, pinned against the plainest loop: for one lane on the strict step the tables
after max_step steps are those of

    for s in range(max_step): engine.step(sampler.sample(1)[0])

bit for bit, whatever the log / validation marks and the group size made of them (eager groups, the group graph, remainder graphs
of either parity, the phase-timed step of a log mark, validations in between).  The pieces below the loop carry that: batch k
depends on (seed, k) alone (test_gpu_sampler), graph replay equals eager launch and the four phase calls equal the fused step
(test_gpu_end_to_end, test_gpu_reference_style).  The straight-line run of a mode is computed once per module, on clones of the
trainer's initial tables, and only read afterwards.  Case table: tests/train_loop_cases.py (held to the branches it names by
tests/test_train_loop_inputs.py)."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

import train_loop_cases as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TABLE_NAMES = ("entity", "entity state", "relation", "relation state", "projection", "projection state")
BASE = ("TransE_l2", "TransE_l2", [], False)


def _cpu(tables):
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().clone() for t in tables)


def straight_line(tr, max_step):
    """the reference: a second engine over clones of the trainer's tables, a fresh sampler, one eager step after the other - no
    graphs, no groups, no marks, no timed step.  Returns (final tables, [max_step, 4] per-step loss terms), on the host"""
    clones = tuple(t.clone() for t in tr.model.tables())
    eng = tr.make_engine(tables=clones)
    if tr.known is not None:
        eng.attach_known(tr.known)
    smp = tr.make_sampler(0, slice(None))
    losses = []
    for _ in range(max_step):
        b = smp.sample(1)[0] if tr.device_sampler else smp.next_batches(1)[0]
        eng.step(b, per_step_loss=True)
        losses.append(eng.read_loss())
    return _cpu(clones), np.asarray(losses, np.float64)


def _lane_record(lane, device_sampler, last):
    smp = lane.sampler
    if not device_sampler:
        return dict(host_step=smp.step + 1)
    kind, k, first = last
    par = int(smp.slot_arrays(k - 1)["counts"][2])
    return dict(host_step=smp.host_step, device_step=int(smp.state[1]), last_slot=k - 1, last_first=first, slot_neg_head=par,
                host_objects=sorted(key for key in smp._batches if key[0] == k - 1))


class Loop(object):
    """the runs of this module: every (mode, row, extra flags) trains once, every mode's straight-line reference is computed once"""

    def __init__(self, root):
        self.root, self.n = root, 0
        self.data = {}
        self.ref, self.done = {}, {}

    def data_dir(self, weights):
        if weights not in self.data:
            self.data[weights] = os.path.join(self.root, "kg_w" if weights else "kg")
            L.write_planted(self.data[weights], weights=weights)
        return self.data[weights]

    def argv(self, mode, row, extra=(), max_step=L.MAX_STEP):
        _, model, flags, weights = mode
        _, G, log, row_flags = row
        self.n += 1
        return L.argv(self.data_dir(weights), os.path.join(self.root, "ckpts%d" % self.n), model, G, log,
                      list(flags) + list(row_flags) + list(extra), max_step)

    def run(self, mode, row, extra=()):
        key = (mode[0], row[0], tuple(extra))
        if key in self.done:
            return self.done[key]
        from dglke_amd import train as T
        rec = {}

        def before_train(tr):
            rec["init"] = _cpu(tr.model.tables())
            if mode[0] not in self.ref and tr.n_lanes == 1:
                self.ref[mode[0]] = (rec["init"],) + straight_line(tr, L.MAX_STEP)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            tr = T.main(self.argv(mode, row, extra), before_train=before_train)
        rec["out"] = out.getvalue()
        rec["final"] = _cpu(tr.model.tables())
        save, model = tr.args.save_path, mode[1]
        rec["saved"] = [np.load(os.path.join(save, "toy_%s_%s.npy" % (model, n))) for n in ("entity", "relation")]
        if model == "TransR":
            rec["saved"].append(np.load(os.path.join(save, "toy_TransRprojection.npy")))
        timers = tr.n_lanes == 1
        fsi = tr.args.force_sync_interval
        events = L.chain(L.MAX_STEP, row[2], L.eval_interval(row[3]), "--valid" in row[3], row[1], timers, None, fsi,
                         fsi > 0 and tr.n_lanes > 1)
        rec["lanes"] = [_lane_record(lane, tr.device_sampler, L.runs(events)[-1]) for lane in tr.lanes]
        rec["device_sampler"] = tr.device_sampler
        self.done[key] = rec
        return rec

    def reference(self, mode):
        """(initial tables, final tables, per-step losses) of the mode's straight-line run"""
        if mode[0] not in self.ref:
            self.run(mode, L.ROWS[0])
        return self.ref[mode[0]]


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    return Loop(str(tmp_path_factory.mktemp("train_loop")))


def _assert_trajectory(loop, mode, row):
    rec = loop.run(mode, row)
    init, final, _ = loop.reference(mode)
    assert len(rec["final"]) == len(final) == (6 if mode[1] == "TransR" else 4)
    for name, a, b in zip(TABLE_NAMES, rec["init"], init):
        assert torch.equal(a, b), "%s: the run does not start from the tables of the straight-line run" % name
    for name, a, b, c in zip(TABLE_NAMES, rec["final"], final, init):
        assert not torch.equal(b, c), "%s: the straight-line run did not train it" % name
        bad = (a != b).reshape(a.shape[0], -1).any(1).nonzero().flatten()
        assert torch.equal(a, b), "%s table after %d steps differs from the straight-line loop's in %d rows (first: %s)" % (
            name, L.MAX_STEP, len(bad), bad[:8].tolist())
    for saved, k in zip(rec["saved"], (0, 2, 4)):
        assert np.array_equal(saved, rec["final"][k].numpy()), "%s: the saved file is not the table" % TABLE_NAMES[k]


def _assert_counters(rec):
    assert rec["lanes"]
    for k, lane in enumerate(rec["lanes"]):
        assert lane["host_step"] == L.MAX_STEP + 1, (k, lane)
        if rec["device_sampler"]:
            assert lane["device_step"] == L.MAX_STEP + 1, (k, lane)
            # the last group ran steps first .. max_step through slots 0 .. last_slot: the slot holds step max_step's batch, with
            # the side the device gave it, and the host's batch object of that slot and side is the one the step was run with
            assert lane["last_first"] + lane["last_slot"] == L.MAX_STEP
            assert lane["slot_neg_head"] == int(L.MAX_STEP % 2 == 0), (k, lane)
            assert (lane["last_slot"], L.MAX_STEP % 2 == 0) in lane["host_objects"], (k, lane)


@pytest.mark.parametrize("row", L.ROWS, ids=L.ROW_IDS)
def test_tables_do_not_depend_on_marks_and_group_size(loop, row):
    """2a: TransE_l2, one lane, strict step, device sampler - both tables and both Adagrad states equal the straight-line loop's
    under every row of the table (and so each other's); the saved files are the tables"""
    _assert_trajectory(loop, BASE, row)


@pytest.mark.parametrize("r", L.MODE_ROWS, ids=[L.ROW_IDS[r] for r in L.MODE_ROWS])
@pytest.mark.parametrize("mode", L.MODES, ids=[m[0] for m in L.MODES])
def test_every_mode_trains_its_own_straight_line_sequence(loop, mode, r):
    """2b: eager, group replays with a timed step at every mark, and flipped parity, for every mode with its own path through the
    loop (TransR: the projection table and its state too; --exclude_positive: the timed step through kge_step_phase_known;
    --has_edge_importance: host batches, no graphs)"""
    rec = loop.run(mode, L.ROWS[r])
    assert rec["device_sampler"] == (not mode[3])
    if mode[0] == "exclude_positive":
        assert "known training triples excluded" in rec["out"]
    _assert_trajectory(loop, mode, L.ROWS[r])


@pytest.mark.parametrize("r", [2, 7], ids=[L.ROW_IDS[2], L.ROW_IDS[7]])
def test_printed_averages_are_the_means_of_the_straight_line_losses(loop, r):
    """2c: every '[proc 0][Train](k/230) average <term>' line is the mean of the straight-line per-step values over (previous log
    mark, k] - a timed step missing from the sums, or a wrong step count, moves it by >= 1 / 64.  The per-step values are the same
    bits (2a); the printed value is an fp32 sum of <= 64 non-negative terms per step over <= 230 steps: relative error
    <= 64 * 230 * 2^-24 ~ 9e-4, asserted at rtol 1e-3"""
    row = L.ROWS[r]
    rec = loop.run(BASE, row)
    losses = loop.reference(BASE)[2]
    assert losses.shape == (L.MAX_STEP, 4) and (losses >= 0).all()
    got = {}
    for m in re.finditer(r"^\[proc 0\]\[Train\]\((\d+)/%d\) average (\w+): (\S+)$" % L.MAX_STEP, rec["out"], re.M):
        got[(int(m.group(1)), m.group(2))] = float(m.group(3))
    marks = list(range(row[2], L.MAX_STEP + 1, row[2]))
    assert sorted({k for k, _ in got}) == marks, rec["out"][-2000:]
    for i, term in enumerate(("pos_loss", "neg_loss", "loss", "regularization")):
        for prev, k in zip([0] + marks, marks):
            want = losses[prev:k, i].mean()
            print("%s (%d, %d]: printed %.9g, straight-line mean %.9g, rel %.2e" % (term, prev, k, got[(k, term)], want,
                                                                                   abs(got[(k, term)] - want) / want))
            assert abs(got[(k, term)] - want) <= 1e-3 * want, (term, prev, k, got[(k, term)], want)


@pytest.mark.parametrize("row", L.ROWS, ids=L.ROW_IDS)
def test_counters_after_training(loop, row):
    """2d, the rows of 2a: the host's step counter, the device's, and the side of the last batch built agree"""
    _assert_counters(loop.run(BASE, row))


@pytest.mark.parametrize("r", L.MODE_ROWS, ids=[L.ROW_IDS[r] for r in L.MODE_ROWS])
@pytest.mark.parametrize("mode", L.MODES, ids=[m[0] for m in L.MODES])
def test_counters_after_training_in_every_mode(loop, mode, r):
    _assert_counters(loop.run(mode, L.ROWS[r]))


def test_counters_of_three_lanes(loop):
    """2d, `--num_proc 3 --force_sync_interval 100`: the lanes are lock-free on shared tables, so their tables are nobody's
    reference - their batch streams are: every lane has built and run exactly max_step batches, sides in step"""
    rec = loop.run(BASE, L.ROWS[2], ("--num_proc", "3", "--force_sync_interval", "100"))
    assert len(rec["lanes"]) == 3
    _assert_counters(rec)
    for k in range(3):
        assert "[proc %d][Train](200/230) average loss:" % k in rec["out"]


@pytest.mark.parametrize("mode,flags", [(BASE, []), (L.MODES[1], ["--neg_sample_size_eval", "24", "--batch_size_eval", "8"])],
                         ids=["TransE_l2_all_entities", "TransR_sampled_candidates"])
def test_validation_is_read_only(loop, mode, flags):
    """2e: `evaluate('valid')` leaves every table and state as it was, and the step after it gives the tables of that step on a
    fresh engine and sampler without a validation in between (a workspace or sampler slot it had disturbed would show there)"""
    from dglke_amd import train as T
    steps = 40
    with contextlib.redirect_stdout(io.StringIO()):
        tr = T.main(loop.argv(mode, ("", 16, steps, flags), max_step=steps))
        before = tuple(t.clone() for t in tr.model.tables())
        m = tr.evaluate("valid", "Valid")
    torch.cuda.synchronize()
    assert 0.0 < m["MRR"] <= 1.0
    for name, a, b in zip(TABLE_NAMES, tr.model.tables(), before):
        assert torch.equal(a, b), "%s changed during the validation" % name
    tr.lanes[0].enqueue(1)
    alone = tuple(t.clone() for t in before)
    eng = tr.make_engine(tables=alone)
    smp = tr.make_sampler(0, slice(None))
    for _ in range(steps):                      # (batch k depends on (seed, k) alone: the sampler is walked to step 41)
        smp.sample(1)
    eng.step(smp.sample(1)[0])
    torch.cuda.synchronize()
    assert tr.lanes[0].sampler.host_step == smp.host_step == steps + 2
    for name, a, b, c in zip(TABLE_NAMES, tr.model.tables(), alone, before):
        assert not torch.equal(b, c), "%s: the step alone did not train it" % name
        assert torch.equal(a, b), "%s after validation + step differs from the step alone" % name


def test_all_to_all_trainers_do_not_depend_on_marks_and_group_size(loop):
    """2f: `--gpu 0 0`, synchronous schedule - the owner applies the trainers' gradients in rank order, so the mode is
    deterministic: two runs with different group sizes and marks save the same entity and relation files, bit for bit"""
    from test_gpu_sharded_eval import _run
    saved = []
    for G, log in ((20, 30), (0, 45)):
        a = loop.argv(BASE, ("", G, log, ["--gpu", "0", "0"]), max_step=90)
        _run([sys.executable, os.path.join(ROOT, "dgl-ke_amd", "dglke_train")] + a)
        save = os.path.join(a[a.index("--save_path") + 1], "TransE_l2_toy_0")
        saved.append([np.load(os.path.join(save, "toy_TransE_l2_%s.npy" % n)) for n in ("entity", "relation")])
    init = (8.0 + 2.0) / L.HIDDEN
    for name, a, b in zip(("entity", "relation"), *saved):
        assert a.shape == b.shape and np.abs(a).max() > init, "%s: not trained" % name
        bad = np.nonzero((a != b).any(1))[0]
        assert np.array_equal(a, b), "%s files differ in %d rows (first: %s)" % (name, len(bad), bad[:8].tolist())
