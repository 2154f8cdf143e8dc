"""Host side of the sharded evaluation (no GPU): the per-rank filter lists and sampled-candidate columns are the full lists
split by owner, and the sharded .npy writer produces np.save's bytes."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bounds(n, world):
    per = (n + world - 1) // world
    return [(min(k * per, n), min((k + 1) * per, n)) for k in range(world)]


def _graph(n_ent, n_rel, n_known, n_test, seed):
    rng = np.random.RandomState(seed)
    known = np.stack([rng.randint(0, n_ent, n_known), rng.randint(0, n_rel, n_known), rng.randint(0, n_ent, n_known)], 1)
    test = known[rng.choice(n_known, n_test, replace=False)]
    return (known[:, 0], known[:, 1], known[:, 2]), (test[:, 0], test[:, 1], test[:, 2])


def _lists(filt, i):
    return filt[1][filt[0][i, 0]:filt[0][i, 1]]


@pytest.mark.parametrize("n_ent,world", [(50, 1), (50, 2), (50, 3), (37, 4), (5, 4)])
def test_shard_filter_lists_are_the_full_lists_split_by_owner(n_ent, world):
    from dglke_amd import eval as E
    known, test = _graph(n_ent, 4, 400, 60, seed=n_ent + world)
    for neg_head in (False, True):
        full = E.build_filter(*known, *test, neg_head, 4)
        parts = []
        for lo, hi in _bounds(n_ent, world):
            kn = E.shard_known(known, neg_head, lo, hi)
            f = E.build_filter(*kn, *test, neg_head, 4)
            for i in range(len(test[0])):
                assert np.all((_lists(f, i) >= 0) & (_lists(f, i) < hi - lo))
            parts.append((lo, f))
        for i in range(len(test[0])):
            want = _lists(full, i)
            got = np.concatenate([_lists(f, i) + lo for lo, f in parts])
            assert np.array_equal(got, want), (neg_head, i)          # owners ascending: the same ids in the same order
            for lo, f in parts:
                hi = lo + (n_ent + world - 1) // world
                assert np.array_equal(_lists(f, i) + lo, want[(want >= lo) & (want < hi)])


@pytest.mark.parametrize("n_ent,world", [(50, 2), (50, 3), (37, 4), (5, 4)])
def test_sampled_owned_columns_are_the_full_columns_split_by_owner(n_ent, world):
    from dglke_amd import eval as E
    known, test = _graph(n_ent, 4, 400, 60, seed=7 * n_ent + world)
    rng = np.random.RandomState(3)
    for neg_head in (False, True):
        full = E.build_filter(*known, *test, neg_head, 4)
        for e0, e1 in ((0, 60), (10, 25)):
            cand = rng.randint(0, n_ent, size=n_ent // 2 + 1)           # duplicates: separate columns
            fc = E.filter_columns(cand, full, e0, e1)
            seen = np.zeros(len(cand), bool)
            per_rank = []
            for lo, hi in _bounds(n_ent, world):
                pos, local = E.owned_candidates(cand, lo, hi)
                assert np.array_equal(cand[pos], local + lo) and not seen[pos].any()
                seen[pos] = True
                f = E.filter_columns(local, E.build_filter(*E.shard_known(known, neg_head, lo, hi), *test, neg_head, 4), e0, e1)
                per_rank.append((pos, f))
            assert seen.all()                                         # every column is owned by exactly one rank
            for i in range(e1 - e0):
                want = np.sort(_lists(fc, i))
                got = np.sort(np.concatenate([pos[_lists(f, i)] for pos, f in per_rank]))
                assert np.array_equal(got, want), (neg_head, e0, i)


def _writer(rank, world, port, path, n_rows, d, max_copy, ret):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dglke_amd import dist as kd
        full = torch.from_numpy(np.random.RandomState(0).randn(n_rows, d).astype(np.float32))
        full[0, 0] = -0.0
        spec = kd.ShardSpec(n_rows, world, rank)
        ret[rank] = kd.write_npy_sharded(path, full[spec.lo:spec.hi].clone(), spec.lo, n_rows, max_copy_bytes=max_copy)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("world,n_rows,d,max_copy", [(1, 10, 3, 1 << 20), (2, 11, 5, 64), (3, 7, 4, 16), (4, 5, 6, 100),
                                                     (4, 1, 2, 8)])
def test_sharded_writer_gives_np_save_bytes(tmp_path, world, n_rows, d, max_copy):
    """uneven shards, empty shards (5 rows over 4 ranks: 2, 2, 1, 0; 1 row: 1, 0, 0, 0) and copies of a few rows at a time"""
    path = str(tmp_path / "ent.npy")
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_writer, args=(world, _free_port(), path, n_rows, d, max_copy, ret), nprocs=world, join=True)
    full = np.random.RandomState(0).randn(n_rows, d).astype(np.float32)
    full[0, 0] = -0.0
    ref = str(tmp_path / "ref.npy")
    np.save(ref, full)
    with open(path, "rb") as a, open(ref, "rb") as b:
        assert a.read() == b.read()
    for r in range(world):                                         # one staging buffer per rank, never above the copy bound
        assert ret[r] <= max(max_copy, 4 * d)
