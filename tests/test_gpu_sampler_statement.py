"""The device sampler's ids against an independent statement in Python integers (tests/sampler_statement.py; its own checks and the
quality of the RNG it states: tests/test_sampler_statement_inputs.py).

tests/test_gpu_sampler.py rebuilds the plan from the ids the kernel sampled and compares the tail jobs with the sampler launch, which
share sample_negative, epoch_affine and epoch_index*: a wrong hash constant, a truncated step counter or a stale cached epoch passes
all of it.  Here every slot of every launch - and of every group of tail jobs - is compared bit for bit with the statement:
h_gid, t_gid, rel_ids, neg_ids and the edge weights with batch_ids; every plan array with plan.build_plan of the RESTATED ids;
counts[0..3]; state[0..2]; the tail jobs' cached epoch constants state[4..7]; DeviceBatch.neg_head.  The geometries (S.CASES) cross
epoch boundaries inside and between launches, make every step an epoch, use a seed with bit 63 set, entity ids beyond 2^32, the wide
instance, a sampler that does not shuffle and steps beyond 10^12.

Last: kge_debug_epoch_order (test support, csrc/kge_debug.hip) evaluates the sampler's own epoch functions for graphs no test could
hold - up to 2^62 triples: the shift-and-add product, the `m % n` multiplier, the reciprocal remainder next to 2^32.
"""
import numpy as np
import pytest
import torch

import sampler_statement as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """a lost GPU context fails every later call: end the session instead of running the rest of the file against it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU context is lost (%s): nothing more is run" % (e,), returncode=3)


def _sampler(c, n_slots):
    from dglke_amd.dataloader import DeviceSampler
    H, R, T, W = S.triples(c)
    seed = c["seed"]
    s = DeviceSampler(H, R, T, c["n_ent"], c["B"], c["N"], DEV, n_slots=n_slots, neg_chunk_size=c["chunk"],
                      seed=seed if seed < 1 << 63 else 5, shuffle=c["shuffle"], edge_importance=W)
    s.seed = seed                                            # (the base permutation is read back: whatever seed made it)
    if c["step0"] != 1:
        s.state[1] = c["step0"]
        s.host_step = c["step0"]
    assert (s.perm is not None) == c["shuffle"]
    perm = s.perm.cpu().numpy() if c["shuffle"] else None
    assert perm is None or np.array_equal(np.sort(perm), np.arange(c["n_train"]))
    return s, (H, R, T, W, perm)


def _check_slot(c, s, data, slot, step, batch, what):
    from dglke_amd import plan
    H, R, T, W, perm = data
    B, N, chunk = c["B"], c["N"], c["chunk"]
    want = S.batch_ids(H, R, T, perm, W, c["n_ent"], B, N, chunk, c["seed"], step)
    a = s.slot_arrays(slot)
    for name in ("h_gid", "t_gid", "rel_ids", "neg_ids"):
        assert np.array_equal(a[name], want[name]), "%s: %s differs from the statement" % (what, name)
    if W is not None:
        assert np.array_equal(a["edge_w"].view(np.uint32), want["edge_w"].view(np.uint32)), "%s: edge_w" % what
    assert batch.neg_head == want["neg_head"] and batch.slot == slot, what
    p = plan.build_plan(want["h_gid"], want["t_gid"], want["rel_ids"], want["neg_ids"], chunk, N, want["neg_head"])
    UE, UR = p["UE"], p["UR"]
    longest = int(np.bincount(want["rel_ids"]).max())
    assert a["counts"].tolist() == [UE, UR, int(want["neg_head"]), longest if longest > 8 else 0], (what, a["counts"], UE, UR, longest)
    for name, n in (("ue_id", UE), ("ue_pos_ptr", UE + 1), ("ue_pos_adj", 2 * B), ("ue_neg_ptr", UE + 1), ("ue_neg_slot", (B // chunk) * N),
                    ("ur_id", UR), ("ur_ptr", UR + 1), ("ur_edge", B), ("ue_rec", 8 * UE), ("ur_rec", 8 * UR)):
        assert p[name].shape[0] == n and np.array_equal(a[name][:n], p[name]), "%s: %s differs from the plan of the restated ids" % (what, name)
    return want


@pytest.mark.parametrize("c", S.CASES, ids=lambda c: c["id"])
def test_sampler_launch_equals_the_statement(c):
    n_slots = max(n + slot0 for n, slot0 in c["launches"])
    s, data = _sampler(c, n_slots)
    pos, hi_words = 0, 0
    for step0, n, slot0 in S.steps_of(c):
        batches = s.sample(n, slot0=slot0)
        torch.cuda.synchronize()
        for k in range(n):
            w = _check_slot(c, s, data, slot0 + k, step0 + k, batches[k], "%s step %d (slot %d)" % (c["id"], step0 + k, slot0 + k))
            hi_words += int((np.concatenate([w["h_gid"], w["t_gid"], w["neg_ids"]]) >> 32 > 0).sum())
        pos, nxt, ticket = S.state_after(pos, step0, n, c["B"], c["n_train"])
        assert s.state[:3].tolist() == [pos, nxt, ticket] and s.host_step == nxt, (c["id"], s.state.tolist())
    assert s.state[4:].tolist() == [-1, 0, 0, 0]             # (the launch does not touch the tail jobs' cache)
    assert (hi_words > 0) == (c["n_ent"] > 1 << 32)


@pytest.mark.parametrize("c", S.TAIL_CASES, ids=lambda c: c["id"])
def test_sampler_tail_jobs_equal_the_statement(c):
    """the same comparison for batches built by tail workgroups of training steps (kge_step_fused_sampling), three groups of three
    jobs; the carrying steps train a small stand-in table on batches of another sampler of the same geometry.  After every group
    the cached epoch constants are those of the NEXT job's epoch: with one or two batches per epoch every job's differ from its
    neighbour's"""
    from dglke_amd.dataloader import DeviceSampler
    from dglke_amd.engine import StepEngine
    G = S.TAIL_GROUP_JOBS
    B, N, n_train = c["B"], c["N"], c["n_train"]
    s, data = _sampler(c, G)
    small = min(c["n_ent"], 5000)
    rng = np.random.RandomState(1)
    eng = StepEngine("DistMult", small, c["n_rel"], 32, 12.0, 0.1, DEV, False, False, True, 1.0, 1e-6, 3)
    carrier = DeviceSampler(rng.randint(0, small, 3 * B), rng.randint(0, c["n_rel"], 3 * B), rng.randint(0, small, 3 * B), small, B, N, DEV,
                            n_slots=G, neg_chunk_size=c["chunk"], seed=1)
    pos, epochs = 0, set()
    for grp, (step0, n, slot0) in enumerate(S.steps_of(c, tail=True)):
        cur = carrier.sample(n)
        jobs, batches = s.tail_jobs(n, slot0=slot0)
        for k in range(n):
            eng.step(cur[k], sample_job=jobs[k])
        torch.cuda.synchronize()
        for k in range(n):
            _check_slot(c, s, data, slot0 + k, step0 + k, batches[k], "%s group %d job %d (step %d)" % (c["id"], grp, k, step0 + k))
            epochs.add(S.step_position(step0 + k, B, n_train)[1])
        pos, nxt, _ = S.state_after(pos, step0, n, B, n_train)
        st = s.state.tolist()
        assert st[:2] == [pos, nxt] and s.host_step == nxt, (c["id"], grp, st)
        # the last job cached the constants of the epoch of the next group's first batch (batch index = that job's step number)
        assert st[4] == (nxt - 1) // (n_train // B), (c["id"], grp, st)
        if st[4] != -1:
            assert tuple(v & S.M64 for v in st[5:8]) == S.epoch_consts(c["seed"], st[4], n_train, c["shuffle"]), (c["id"], grp, st)
    assert len(epochs) > 1


# ---- the epoch order beyond what an array can hold ------------------------------------------------------------------------------
ORDER_N = (1, 2, 3, 4096, 30030, 483142, 338586276, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 15, 3 << 33, (1 << 62) + 57)
ORDER_EPOCHS = (0, 1, 2, 7, 8, 9, 10 ** 6, 1 << 40)
ORDER_SEEDS = (3, (1 << 63) + 5)


def epoch_order(n_train, seed, shuffled, epochs, pos):
    """kge_debug_epoch_order on the current stream -> uint64 [n, 5]: index, index_fast, mul, add, rinv"""
    from dglke_amd import _lib
    e = torch.tensor(list(epochs), dtype=torch.int64, device=DEV)
    p = torch.tensor(list(pos), dtype=torch.int64, device=DEV)
    out = torch.full((e.numel(), 5), -7, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().kge_debug_epoch_order(n_train, seed, int(shuffled), _lib.ptr(e), _lib.ptr(p), e.numel(), _lib.ptr(out), _lib.stream_ptr()))
    return out


def order_statement(n_train, seed, shuffled, epochs, pos):
    rows, consts = [], {}
    for ep, p in zip(epochs, pos):
        if ep not in consts:
            consts[ep] = S.epoch_consts(seed, ep, n_train, shuffled)
        mul, add, rinv = consts[ep]
        i = S.epoch_index(p, mul, add, n_train)
        rows.append((i, i, mul, add, rinv))
    return np.array(rows, np.uint64)


@pytest.mark.parametrize("n", ORDER_N)
def test_epoch_order_of_any_graph_size_equals_the_statement(n):
    rng = np.random.RandomState(n % 1000)
    if n <= 30030:
        positions = list(range(n))
    else:
        positions = [0, 1, n - 2, n - 1] + [int(x) % n for x in rng.randint(0, 1 << 62, 1000, dtype=np.int64)]
    epochs = [ep for ep in ORDER_EPOCHS for _ in positions]
    pos = positions * len(ORDER_EPOCHS)
    for seed, shuffled in [(sd, True) for sd in ORDER_SEEDS] + [(ORDER_SEEDS[0], False)]:
        got = epoch_order(n, seed, shuffled, epochs, pos).cpu().numpy().view(np.uint64)
        want = order_statement(n, seed, shuffled, epochs, pos)
        for col, name in enumerate(("index", "index_fast", "mul", "add", "rinv")):
            bad = np.flatnonzero(got[:, col] != want[:, col])
            assert bad.size == 0, "n %d seed %d: %s of (epoch %d, pos %d) is %d, the statement says %d" % (
                n, seed, name, epochs[bad[0]], pos[bad[0]], got[bad[0], col], want[bad[0], col])
        assert np.array_equal(got[:, 0], got[:, 1])
        if n <= 30030:                                       # every epoch's order is a bijection of [0, n)
            per = got[:, 0].reshape(len(ORDER_EPOCHS), n)
            assert all(np.array_equal(np.sort(row), np.arange(n, dtype=np.uint64)) for row in per)
        if not shuffled:
            assert np.array_equal(got[:, 0], np.array(pos, np.uint64))


def test_epoch_order_refuses_bad_arguments():
    from dglke_amd import _lib
    h = _lib.lib()
    x = torch.zeros(5, dtype=torch.int64, device=DEV)
    p, st = _lib.ptr(x), _lib.stream_ptr()
    for args in ((0, 3, 1, p, p, 1, p), (-5, 3, 1, p, p, 1, p), (10, 3, 1, p, p, -1, p), (10, 3, 1, None, p, 1, p), (10, 3, 1, p, None, 1, p),
                 (10, 3, 1, p, p, 1, None)):
        assert h.kge_debug_epoch_order(*(args + (st,))) == -1, args
        assert b"kge_debug_epoch_order" in h.kge_last_error()
    assert h.kge_debug_epoch_order(10, 3, 1, p, p, 0, p, st) == 0
    torch.cuda.synchronize()
    assert not bool(x.any())
