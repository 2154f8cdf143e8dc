"""Ranking evaluation on a range-sharded entity table (kge_rank_eval_split through dglke_amd.eval): the shards' counts add
up to kge_rank_eval_ex's ranks on the whole table, and the CLIs evaluate sharded models without assembling them."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (model, d_e, d_r): every model; TransE_l2 at 30 takes the score-block path instead of the tiled GEMM; TransR at 2000 entities
# ranks the whole table with one forward kernel and a shard of <= 1296 rows with the other (kge_transr.hip transr_use_wide)
MODELS = [("TransE_l1", 32, 32), ("TransE_l2", 32, 32), ("TransE_l2", 30, 30), ("DistMult", 40, 40), ("ComplEx", 48, 48),
          ("RotatE", 48, 24), ("SimplE", 40, 40), ("RESCAL", 16, 256), ("TransR", 32, 16)]


def _bounds(n, world):
    per = (n + world - 1) // world
    return [(min(k * per, n), min((k + 1) * per, n)) for k in range(world)]


def _tables(model, d_e, d_r, n_ent, n_rel, seed):
    rng = np.random.RandomState(seed)
    emb_init = 0.3
    ent = ((rng.rand(n_ent, d_e) - 0.5) * 2 * emb_init).astype(np.float32)
    rel = ((rng.rand(n_rel, d_r) - 0.5) * 2 * emb_init).astype(np.float32)
    proj = ((rng.rand(n_rel, d_e * d_r) - 0.5) * 0.4).astype(np.float32) if model == "TransR" else None
    return ent, rel, proj, emb_init


def _split_ranks(E, model, ent, rel, proj, emb_init, h, r, t, neg_head, known, world, cand=None, batch=40):
    """1 + sum over the shards of (kge_rank_eval_split - 1); known = None: raw"""
    n_ent = ent.shape[0]
    ids, inv = np.unique(np.concatenate([h, t]), return_inverse=True)
    te = torch.from_numpy(ent).to(DEV)
    qent = te[torch.from_numpy(ids).to(DEV)].contiguous()
    qh, qt = inv[:len(h)], inv[len(h):]
    total = np.zeros(len(h), np.int64)
    for lo, hi in _bounds(n_ent, world):
        rk = E.SplitRanker(model, te[lo:hi].contiguous(), torch.from_numpy(rel).to(DEV), 12.0, emb_init, batch=batch,
                           proj=None if proj is None else torch.from_numpy(proj).to(DEV))
        filt = None
        if known is not None:
            filt = E.build_filter(*E.shard_known(known, neg_head, lo, hi), h, r, t, neg_head, rel.shape[0])
        local = None
        if cand is not None:
            _, local = E.owned_candidates(cand, lo, hi)
            if filt is not None:
                filt = E.filter_columns(local, filt, 0, len(h))
        got = rk.ranks(qent, qh, r, qt, neg_head, filt, cand=local).cpu().numpy()
        total += got.astype(np.int64) - 1
    return total + 1


@pytest.mark.parametrize("model,d_e,d_r", MODELS, ids=["%s_%d" % (m, d) for m, d, _ in MODELS])
def test_split_entry_point_sums_to_the_whole_table_ranks(model, d_e, d_r):
    from dglke_amd import eval as E
    n_rel, Et = 5, 150
    for n_ent, worlds in ((2000 if model == "TransR" else 700, (1, 2, 3)), (5, (4,))):
        ent, rel, proj, emb_init = _tables(model, d_e, d_r, n_ent, n_rel, seed=n_ent)
        rng = np.random.RandomState(1)
        known = np.stack([rng.randint(0, n_ent, 3000), rng.randint(0, n_rel, 3000), rng.randint(0, n_ent, 3000)], 1)
        k3 = (known[:, 0], known[:, 1], known[:, 2])
        h, r, t = known[:Et, 0].copy(), known[:Et, 1].copy(), known[:Et, 2].copy()
        tp = None if proj is None else torch.from_numpy(proj).to(DEV)
        whole = E.Ranker(model, torch.from_numpy(ent).to(DEV), torch.from_numpy(rel).to(DEV), 12.0, emb_init, batch=40, proj=tp)
        cand = rng.randint(0, n_ent, size=max(3, n_ent // 3))         # a sampled list, duplicates included
        for neg_head in (False, True):
            full_filt = E.build_filter(*k3, h, r, t, neg_head, n_rel)
            for filtered in (True, False):
                want = whole.ranks(h, r, t, neg_head, full_filt if filtered else None).cpu().numpy()
                fc = E.filter_columns(cand, full_filt, 0, Et) if filtered else None
                want_s = whole.ranks(h, r, t, neg_head, fc, cand=cand).cpu().numpy()
                for world in worlds:
                    got = _split_ranks(E, model, ent, rel, proj, emb_init, h, r, t, neg_head, k3 if filtered else None, world)
                    assert np.array_equal(got, want), (n_ent, world, neg_head, filtered, np.nonzero(got != want)[0][:8])
                    got_s = _split_ranks(E, model, ent, rel, proj, emb_init, h, r, t, neg_head, k3 if filtered else None, world,
                                         cand=cand)
                    assert np.array_equal(got_s, want_s), (n_ent, world, neg_head, filtered, np.nonzero(got_s != want_s)[0][:8])


def test_split_entry_point_with_no_candidates_sets_rank_one():
    from dglke_amd import _lib
    from dglke_amd import eval as E
    q = torch.rand(4, 8, device=DEV)
    rel = torch.rand(2, 8, device=DEV)
    rk = E.SplitRanker("DistMult", torch.empty(0, 8, device=DEV), rel, 12.0, 0.3, batch=4)
    ids = np.array([0, 1, 2, 3])
    assert rk.ranks(q, ids, ids % 2, ids[::-1].copy(), False).cpu().tolist() == [1, 1, 1, 1]
    assert rk.ranks(q, ids, ids % 2, ids, True, cand=np.zeros(0, np.int64)).cpu().tolist() == [1, 1, 1, 1]
    with pytest.raises(_lib.KgeError):          # TransR without its projection table
        E.SplitRanker("TransR", q, rel, 12.0, 0.3)


def _planted(path, n_ent=400, n_rel=6, n=9000, seed=3):
    from planted_kg import make_planted
    train, test = make_planted(n_ent, n_rel, n, dim=8, seed=seed)
    valid, test = test[:len(test) // 2], test[len(test) // 2:]
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "e.dict"), "w") as f:
        f.writelines("%d\te%d\n" % (i, i) for i in range(n_ent))
    with open(os.path.join(path, "r.dict"), "w") as f:
        f.writelines("%d\tr%d\n" % (i, i) for i in range(n_rel))
    for name, t in (("train.txt", train), ("valid.txt", valid), ("test.txt", test)):
        np.savetxt(os.path.join(path, name), t, fmt="%d", delimiter="\t")
    return train, valid, test


def _run(cmd, timeout=300):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    return out


def _metric_lines(out, tag):
    return [l for l in out.split("\n") if re.match(r"^\[0\]%s average " % tag, l)]


def _oracle_lines(model, save, trip, known, tag, gamma, hidden, n_cand, chunk, seed=0):
    """today's single-table evaluation on the saved tables, with the arguments the sharded trainers pass"""
    from dglke_amd import eval as kev
    stem = os.path.join(save, "toy_%s_" % model)
    ent = torch.from_numpy(np.load(stem + "entity.npy")).to(DEV)
    rel = torch.from_numpy(np.load(stem + "relation.npy")).to(DEV)
    proj = torch.from_numpy(np.load(stem[:-1] + "projection.npy")).to(DEV) if model == "TransR" else None
    h, r, t = trip[:, 0], trip[:, 1], trip[:, 2]
    Eb = int(max(1, min(4096, (1 << 31) // (4 * ent.shape[0]), len(h))))
    if proj is not None:
        Eb = min(Eb, 64)
    m = kev.evaluate(model, ent, rel, gamma, (gamma + 2.0) / hidden, (h, r, t), known, batch=Eb, proj=proj, n_cand=n_cand,
                     chunk=chunk, seed=seed + 29)
    return ['[0]{} average {}: {}'.format(tag, k, v) for k, v in m.items()]


E2E = [(m, mode, ncand) for ncand in (None, 50) for m in ("TransE_l2", "RotatE", "TransR") for mode in ("a2a", "p2p")]


@pytest.mark.parametrize("model,mode,ncand", E2E, ids=["%s_%s_%s" % (m, d, "sampled" if n else "all") for m, d, n in E2E])
def test_sharded_trainers_print_the_single_table_metrics(tmp_path, model, mode, ncand):
    """`dglke_train --gpu 0 0` validates, tests and saves on the shards: the printed [0]Valid / [0]Test lines are
    kev.evaluate's on the saved tables, as strings (all entities; --neg_sample_size_eval 50)"""
    data = str(tmp_path / "kg")
    train, valid, test = _planted(data)
    extra = {"TransE_l2": [], "RotatE": ["-de"], "TransR": ["--lr", "0.05"]}[model]
    if ncand:
        extra = extra + ["--neg_sample_size_eval", str(ncand), "--batch_size_eval", "16"]
    cmd = [sys.executable, os.path.join(ROOT, "dgl-ke_amd", "dglke_train"), "--model_name", model, "--format", "udd_hrt",
           "--dataset", "toy", "--data_path", data, "--data_files", "e.dict", "r.dict", "train.txt", "valid.txt", "test.txt",
           "--save_path", str(tmp_path / "ckpts"), "--gpu", "0", "0", "--dist_mode", mode, "--batch_size", "256",
           "--neg_sample_size", "64", "--hidden_dim", "32", "-g", "8", "-adv", "--max_step", "200", "--log_interval", "100",
           "--eval_interval", "200", "--valid", "--test", "--graph_steps", "50"] + extra
    out = _run(cmd)
    save = os.path.join(str(tmp_path / "ckpts"), "%s_toy_0" % model)
    known = tuple(np.concatenate([train[:, k], valid[:, k], test[:, k]]) for k in range(3))
    chunk = 16 if ncand else 8
    for tag, trip in (("Valid", valid), ("Test", test)):
        got = _metric_lines(out, tag)
        assert len(got) == 5, out[-2000:]
        assert got == _oracle_lines(model, save, trip, known, tag, 8.0, 32, ncand, chunk), (tag, got)


@pytest.mark.parametrize("protocol", ["filtered", "raw", "sampled"])
def test_multi_gpu_dglke_eval_prints_the_single_gpu_metrics(tmp_path, protocol):
    """`dglke_eval --gpu 0 0` and `--gpu 0 0 0` (one process per entry, each ranking against its row range) print the metric
    lines of `--gpu 0`"""
    data = str(tmp_path / "kg")
    _planted(data, n_ent=401)
    rng = np.random.RandomState(2)
    save = str(tmp_path / "model")
    os.makedirs(save)
    np.save(os.path.join(save, "toy_DistMult_entity.npy"), ((rng.rand(401, 32) - 0.5) * 0.6).astype(np.float32))
    np.save(os.path.join(save, "toy_DistMult_relation.npy"), ((rng.rand(6, 32) - 0.5) * 0.6).astype(np.float32))
    base = [sys.executable, os.path.join(ROOT, "dgl-ke_amd", "dglke_eval"), "--model_name", "DistMult", "--format", "udd_hrt",
            "--dataset", "toy", "--data_path", data, "--data_files", "e.dict", "r.dict", "train.txt", "valid.txt", "test.txt",
            "--model_path", save, "--hidden_dim", "32", "-g", "8"]
    base += {"filtered": [], "raw": ["--no_eval_filter"], "sampled": ["--neg_sample_size_eval", "40", "--batch_size_eval", "24"]}[protocol]
    want = _metric_lines(_run(base + ["--gpu", "0"]), "Test")
    assert len(want) == 5
    for world in (2, 3):
        out = _run(base + ["--gpu"] + ["0"] * world)
        assert _metric_lines(out, "Test") == want, (world, out[-2000:])
        rows = [(401 + world - 1) // world] * (world - 1) + [401 - (world - 1) * ((401 + world - 1) // world)]
        assert "sharded evaluation: world size %d, entity rows per rank %s" % (world, rows) in out


def _memory_worker(rank, world, port, path, ret):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        from dglke_amd import dist as kd
        from dglke_amd import eval as E
        n_ent, d, n_rel = 1 << 17, 512, 50                    # 256 MB entity table
        spec = kd.ShardSpec(n_ent, world, rank)
        torch.manual_seed(rank)
        shard = torch.empty(spec.n_local, d, device=DEV).uniform_(-0.1, 0.1)
        rel = torch.empty(n_rel, d, device=DEV).uniform_(-0.1, 0.1)
        rng = np.random.RandomState(0)
        known = (rng.randint(0, n_ent, 200000), rng.randint(0, n_rel, 200000), rng.randint(0, n_ent, 200000))
        test = tuple(k[:64] for k in known)
        comm = kd.HostStagedComm()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        staged = kd.write_npy_sharded(path, shard, spec.lo, n_ent, max_copy_bytes=32 << 20)
        Eb = int(max(1, min(4096, (1 << 31) // (4 * n_ent), len(test[0]))))
        E.evaluate_sharded("DistMult", shard, spec.lo, n_ent, rel, 12.0, 0.1, test,
                           lambda ids: E.allgather_rows(shard, spec.lo, spec.bounds(), ids, comm), known, batch=Eb)
        torch.cuda.synchronize()
        ret[rank] = (torch.cuda.max_memory_allocated() - base, staged, spec.n_local * d * 4)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_save_and_filtered_test_hold_no_table_copy(tmp_path, world):
    """save + filtered test on a 256 MB table at 2 and 4 ranks (sharing one GPU): each rank's device memory grows by less than
    BOUND above its shard (filter lists, one query block, the ranking workspace) - under half the table, so no rank ever holds a
    copy of it - and the host staging of the writer is one copy buffer of at most the requested 32 MB"""
    import torch.multiprocessing as mp
    BOUND = 48 << 20
    table = (1 << 17) * 512 * 4
    assert BOUND < table // 2
    with __import__("socket").socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(_memory_worker, args=(world, port, str(tmp_path / "ent.npy"), ret), nprocs=world, join=True)
    for rank in range(world):
        grow, staged, shard_bytes = ret[rank]
        assert grow < BOUND, (rank, grow)
        assert 0 < staged <= 32 << 20 and staged < shard_bytes
    assert os.path.getsize(str(tmp_path / "ent.npy")) == table + 128
