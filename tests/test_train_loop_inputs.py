"""CPU guard of tests/test_gpu_train_trajectory.py: the decisions of `_Lane.enqueue` as the pure `train.plan_enqueue`, chained
with `train.step_marks` the way `_Trainer.train` chains them (tests/train_loop_cases.chain); the case table reaches the branches
it names; the host sampler's batches do not depend on how they are grouped."""
import numpy as np
import pytest

import train_loop_cases as L


def _check_chain(events, max_step, G):
    """the invariants of one run: returns the set of things it reached (for the guard on the case table)"""
    n_slots = max(2, G or 2)
    hs, group_par, rem, reached = 1, None, set(), set()
    for e in events:
        if e[0] not in ("enqueue", "timed"):
            reached.add(e[0])
            continue
        _, before, acts, after = e
        assert before == hs
        for kind, k, par in acts:
            assert 1 <= k <= n_slots, (kind, k, n_slots)
            assert par == hs % 2, "%s of %d steps labelled parity %d at host step %d" % (kind, k, par, hs)
            if kind == "capture_group":
                assert group_par is None and k == G
                group_par = par
            elif kind == "capture_rem":
                assert (k, par) not in rem and len(rem) < 8 and group_par is not None
                rem.add((k, par))
            elif kind == "replay_group":
                assert k == G and group_par == hs % 2 == 1, "group graph recorded at parity %r replayed at host step %d" % (group_par, hs)
            elif kind == "replay_rem":
                assert (k, hs % 2) in rem, "no remainder graph of %d steps was recorded at the parity of host step %d" % (k, hs)
            else:
                assert kind in ("eager", "timed"), kind
            if kind in L.RUNNING:                   # captures are net zero
                hs += k
            reached.add(kind)
            if kind == "replay_rem":
                reached.add(("rem", par))
        assert after == hs, "the plan says host step %d, its steps add up to %d" % (after, hs)
    assert hs == max_step + 1
    assert sum(k for _, k, _ in L.runs(events)) == max_step
    return reached


def test_marks_and_plans_run_every_step_once_at_its_own_parity():
    """a few hundred seeded (max_step, log_interval, eval_interval, valid, G): the sizes sum to max_step, the host step advances by
    exactly the steps run (captures net zero), a graph is replayed only at the parity it was recorded at, no group exceeds the
    sampler's slots, the log lines cover every step once"""
    rng = np.random.RandomState(11)
    seen = set()
    for _ in range(400):
        max_step = int(rng.randint(1, 700))
        log = int(rng.randint(1, 300))
        ev = int(rng.randint(1, 300))
        valid = bool(rng.randint(2))
        G = int(rng.choice([0, 1, 2, 3, 4, 7, 10, 16, 20, 50, 100, 101, 300]))
        for timers in (True, False):
            events = L.chain(max_step, log, ev, valid, G, timers)
            seen |= _check_chain(events, max_step, G)
            logs = [e for e in events if e[0] == "log"]
            assert sum(e[2] for e in logs) == (max_step // log) * log and [e[1] for e in logs] == list(range(log, max_step + 1, log))
            assert [e[1] for e in events if e[0] == "valid"] == ([s for s in range(ev, max_step + 1, ev) if s > 1] if valid else [])
            assert sum(1 for e in events if e[0] == "timed") == (len(logs) if timers else 0)
    assert {"eager", "capture_group", "replay_group", "capture_rem", "replay_rem", "timed", ("rem", 0), ("rem", 1)} <= seen


def test_the_checks_above_see_a_remainder_graph_keyed_by_its_size_alone():
    """the planner with its remainder graphs keyed by k alone (what the parity in the key is there for): the chain check refuses it
    on the `parity_flips` row - a graph recorded at an odd host step replayed at an even one"""
    from dglke_amd import train as T

    def by_size_alone(n, G, hs, have, n_slots, rem_keys):
        acts, after = T.plan_enqueue(n, G, hs, have, n_slots, {(k, hs_par) for k, _ in rem_keys for hs_par in (0, 1)})
        return acts, after
    row = L.ROWS[L.ROW_IDS.index("parity_flips")]
    events = L.chain(L.MAX_STEP, row[2], 10000, False, row[1], True, plan=by_size_alone)
    with pytest.raises(AssertionError, match="no remainder graph of 4 steps was recorded at the parity"):
        _check_chain(events, L.MAX_STEP, row[1])


def test_plans_against_hand_written_lists():
    from dglke_amd.train import plan_enqueue as P
    # first call of a run: eager warm-up, capture, replays, remainder recorded and replayed
    assert P(49, 20, 1, False, 20, ()) == ([("eager", 20, 1), ("capture_group", 20, 1), ("replay_group", 20, 1), ("capture_rem", 9, 1),
                                            ("replay_rem", 9, 1)], 50)
    # the graphs exist: replays only
    assert P(49, 20, 51, True, 20, {(9, 1)}) == ([("replay_group", 20, 1), ("replay_group", 20, 1), ("replay_rem", 9, 1)], 100)
    # even host step: full groups as remainder graphs of the other parity
    assert P(44, 20, 46, True, 20, {(4, 1)}) == ([("capture_rem", 20, 0), ("replay_rem", 20, 0), ("replay_rem", 20, 0),
                                                  ("capture_rem", 4, 0), ("replay_rem", 4, 0)], 90)
    # warm-up only: too short for a capture, and no remainder graph without the group graph
    assert P(30, 20, 1, False, 20, ()) == ([("eager", 20, 1), ("eager", 10, 1)], 31)
    # odd G, G = 0 (two slots), G > n: eager
    assert P(15, 7, 1, False, 7, ()) == ([("eager", 7, 1), ("eager", 7, 0), ("eager", 1, 1)], 16)
    assert P(5, 0, 2, False, 2, ()) == ([("eager", 2, 0), ("eager", 2, 0), ("eager", 1, 0)], 7)
    assert P(114, 300, 1, False, 300, ()) == ([("eager", 114, 1)], 115)
    # eight remainder graphs are recorded, a ninth key runs eagerly
    full = {(k, 1) for k in range(1, 9)}
    assert P(9, 20, 1, True, 20, full) == ([("eager", 9, 1)], 10)
    assert P(0, 20, 1, True, 20, ()) == ([], 1)


def test_rows_reach_the_branches_they_name():
    """the eight rows of the trajectory test, by the planner: group-graph replay, a remainder graph of each parity, the eager
    fallback next to recorded graphs, odd G, timed steps, a validation-only mark, an epoch boundary inside a replayed group"""
    reached = {}
    for row in L.ROWS:
        events = L.row_chain(row)
        reached[row[0]] = _check_chain(events, L.MAX_STEP, row[1])
    kinds = lambda i: {k for k in reached[i] if isinstance(k, str)}
    assert kinds("eager") == {"eager", "timed", "log"}
    assert kinds("one_mark") == {"eager", "capture_group", "replay_group", "capture_rem", "replay_rem"}      # no log line, no timed step
    assert {"replay_group", "timed", ("rem", 1)} <= reached["replays"] and ("rem", 0) not in reached["replays"]
    assert ("replay_rem", 9, 41) in L.runs(L.row_chain(L.ROWS[2]))
    flips = L.runs(L.row_chain(L.ROWS[3]))
    assert {("rem", 0), ("rem", 1), "replay_group"} <= reached["parity_flips"]
    assert ("replay_rem", 20, 46) in flips and ("replay_group", 20, 91) in flips          # full groups through both kinds of graph
    assert kinds("odd_group") == {"eager", "timed", "log"} and L.ROWS[4][1] % 2 == 1
    assert ("replay_rem", 2, 24) in L.runs(L.row_chain(L.ROWS[5])) and sum(1 for e in L.row_chain(L.ROWS[5]) if e[0] == "log") == 10
    assert kinds("group_above_max_step") == {"eager", "timed", "log"}
    assert [e[1] for e in L.row_chain(L.ROWS[6]) if e[0] == "log"] == [115, 230]
    # validation marks inside and between the log marks; at 32 nothing else happens
    v = L.row_chain(L.ROWS[7])
    assert [e[1] for e in v if e[0] == "valid"] == [32, 64, 96, 128, 160, 192, 224] and [e[1] for e in v if e[0] == "log"] == [64, 128, 192]
    # (the eager fallback: whole runs in three rows above and the warm-up group everywhere else; an eager group NEXT to recorded
    #  graphs needs a ninth remainder key - test_plans_against_hand_written_lists)
    # an epoch boundary (steps 62 | 63, 124 | 125, 186 | 187) inside a replayed group graph, a remainder graph and an eager group
    def straddles(row, kind):
        return any(k == kind and s <= b < s + n - 1 for k, n, s in L.runs(L.row_chain(row)) for b in (L.EPOCH, 2 * L.EPOCH, 3 * L.EPOCH))
    assert straddles(L.ROWS[2], "replay_group") and straddles(L.ROWS[3], "replay_rem")
    assert straddles(L.ROWS[4], "eager") and straddles(L.ROWS[7], "replay_rem")
    assert L.EPOCH == 62 and L.N_TRAIN % L.BATCH != 0 and 3 * L.EPOCH < L.MAX_STEP < 4 * L.EPOCH


def test_case_table_graph_has_the_sizes_the_table_assumes(tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    train, valid, test = L.write_planted(str(tmp_path / "kg"), weights=True)
    assert len(train) == L.N_TRAIN and len(valid) >= 100 and train.max() < L.N_ENT
    rows = open(str(tmp_path / "kg" / "train.txt")).read().split("\n")
    assert len(rows[0].split("\t")) == 4 and 0.5 <= float(rows[0].split("\t")[3]) <= 1.5


def test_host_sampler_batches_do_not_depend_on_the_grouping():
    """UniformChunkedSampler.next_plans(5) == next_plans(2) + next_plans(3) from the same seed: ids, negatives, corruption sides and
    weights - across an epoch boundary (the third batch opens a new permutation)"""
    from dglke_amd.dataloader import UniformChunkedSampler
    rng = np.random.RandomState(5)
    n = 2 * 64 + 10
    h, r, t = rng.randint(0, 300, n), rng.randint(0, 7, n), rng.randint(0, 300, n)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    mk = lambda: UniformChunkedSampler(h, r, t, 300, 64, 16, "cpu", neg_chunk_size=16, seed=9, edge_importance=w)
    a, b = mk(), mk()
    one = a.next_plans(5)
    two = b.next_plans(2) + b.next_plans(3)
    assert a.step == b.step == 5
    assert [p["neg_head"] for p in one] == [0, 1, 0, 1, 0]
    for p, q in zip(one, two):
        assert p.keys() == q.keys()
        for k in p:
            if isinstance(p[k], np.ndarray):
                assert p[k].dtype == q[k].dtype and np.array_equal(p[k], q[k]), k
            else:
                assert p[k] == q[k], k
    assert not np.array_equal(one[0]["h_gid"], one[2]["h_gid"])
