"""the sharded evaluation (eval.evaluate_sharded: every rank ranks against its own rows, counts summed) next to kev.evaluate on the
whole table, FB15k-shaped and filtered: 14 951 x 400 entities, 50 000 test triples x 2 modes, 592 k known triples.
World 1 runs in this process; world W > 1 as W processes on the listed GPUs (the same GPU may repeat: rows then travel
through the gloo group, as in `dglke_train --gpu 0 0`).  Each configuration: 3 cached calls; the wall time with and without the
row all-gather (`rows_of` replaced by a local lookup into a full copy made beforehand, which only a test can afford).
usage: python tools/sharded_eval_timing.py [--only whole|sharded] [gpu ...]      (default: 0, then 0 0)
--only: one of the two paths (per-kernel profiles of each, e.g. under rocprofv3 --kernel-trace --stats)"""
import os
import socket
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))

MODEL, N_ENT, N_REL, D, GAMMA, BATCH = "TransE_l2", 14951, 1345, 400, 19.9, 4096


def _data():
    rng = np.random.RandomState(0)
    known = tuple(rng.randint(0, n, 592213) for n in (N_ENT, N_REL, N_ENT))
    test = tuple(k[:50000] for k in known)
    g = torch.Generator().manual_seed(0)
    emb_init = (GAMMA + 2.0) / D
    ent = torch.empty(N_ENT, D).uniform_(-emb_init, emb_init, generator=g)
    rel = torch.empty(N_REL, D).uniform_(-emb_init, emb_init, generator=g)
    return known, test, ent, rel, emb_init


def _sharded(rank, world, gpus, port, calls=3):
    import torch.distributed as dist
    from dglke_amd import dist as kd
    from dglke_amd import eval as E
    if world > 1:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    dev = torch.device("cuda", gpus[rank])
    torch.cuda.set_device(dev)
    known, test, ent, rel, emb_init = _data()
    spec = kd.ShardSpec(N_ENT, world, rank)
    shard = ent[spec.lo:spec.hi].to(dev).contiguous()
    rel = rel.to(dev)
    comm = None
    if world > 1:
        comm = kd.make_comm() if len(set(gpus)) == world else kd.HostStagedComm()
        rows_of = lambda ids: E.allgather_rows(shard, spec.lo, spec.bounds(), ids, comm)      # noqa: E731
    else:
        rows_of = lambda ids: shard[ids]                                                         # noqa: E731
    full = ent.to(dev)
    for label, fn in (("with row all-gather", rows_of), ("rows local (no exchange)", lambda ids: full[ids])):
        cache = {}
        for it in range(calls):
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = E.evaluate_sharded(MODEL, shard, spec.lo, N_ENT, rel, GAMMA, emb_init, test, fn, known, batch=BATCH, cache=cache)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rank == 0:
                print("sharded world %d (%s) call %d: %.4f s  MRR %.6f%s" % (world, label, it, dt, m["MRR"],
                                                                           "  (filter lists built)" if it == 0 else ""))
        if world == 1:
            break                       # world 1 has nothing to exchange
    if comm is not None and hasattr(comm, "close"):
        comm.close()
    if world > 1:
        dist.destroy_process_group()


def main():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import eval as E
    argv = sys.argv[1:]
    only = None
    if argv[:1] == ["--only"]:
        only, argv = argv[1], argv[2:]
    gpus = [int(x) for x in argv] or None
    dev = torch.device("cuda", gpus[0] if gpus else 0)
    torch.cuda.set_device(dev)
    known, test, ent, rel, emb_init = _data()
    ent, rel = ent.to(dev), rel.to(dev)
    cache = {}
    for it in range(3 if only != "sharded" else 0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = E.evaluate(MODEL, ent, rel, GAMMA, emb_init, test, known, batch=BATCH, cache=cache)
        torch.cuda.synchronize()
        print("kev.evaluate (whole table) call %d: %.4f s  MRR %.6f%s" % (it, time.perf_counter() - t0, m["MRR"],
                                                                          "  (filter lists built)" if it == 0 else ""))
    del ent
    if only == "whole":
        return
    for world_gpus in ([gpus] if gpus else [[0], [0, 0]]):
        if len(world_gpus) == 1:
            _sharded(0, 1, world_gpus, 0)
            continue
        import torch.multiprocessing as mp
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        mp.spawn(_sharded, args=(len(world_gpus), world_gpus, port), nprocs=len(world_gpus), join=True)


if __name__ == "__main__":
    main()
