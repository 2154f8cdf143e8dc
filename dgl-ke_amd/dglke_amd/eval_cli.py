"""dglke_eval: rank the test triples of a dataset with saved embeddings - the reference's evaluation entry point
(python/dglke/eval.py:39-110 flags; test() of train_pytorch.py:199-253 and KEModel.forward_test,
general_models.py:436-485, replaced by the on-device filtered ranking kge_rank_eval).  Reads the files dglke_train
(this one or the reference's) writes: <model_path>/<dataset>_<model>_{entity,relation}.npy (+ ...projection.npy for
TransR)."""
import argparse
import os
import sys
import time

import numpy as np
import torch as th

from ._lib import KgeError
from .kgdataset import get_dataset


class ArgParser(argparse.ArgumentParser):
    def __init__(self):
        super(ArgParser, self).__init__()
        a = self.add_argument
        a('--model_name', default='TransE', choices=['TransE', 'TransE_l1', 'TransE_l2', 'TransR', 'RESCAL', 'DistMult',
                                                     'ComplEx', 'RotatE', 'SimplE'])
        a('--data_path', type=str, default='data')
        a('--dataset', type=str, default='FB15k')
        a('--format', type=str, default='built_in')
        a('--data_files', type=str, default=None, nargs='+')
        a('--delimiter', type=str, default='\t')
        a('--model_path', type=str, default='ckpts')
        a('--batch_size_eval', type=int, default=8)
        a('--neg_sample_size_eval', type=int, default=-1)
        a('--neg_deg_sample_eval', action='store_true')
        a('--hidden_dim', type=int, default=256)
        a('-g', '--gamma', type=float, default=12.0)
        a('--eval_percent', type=float, default=1)
        a('--no_eval_filter', action='store_true')
        a('--gpu', type=int, default=[-1], nargs='+')    # several entries: one process per entry, each ranking against its rows
        a('--mix_cpu_gpu', action='store_true')           # accepted, no effect: the tables live in HBM
        a('-de', '--double_ent', action='store_true')
        a('-dr', '--double_rel', action='store_true')
        a('--num_proc', type=int, default=1)              # accepted, no effect: one process ranks on the GPU
        a('--num_thread', type=int, default=1)
        a('--seed', type=int, default=0)
        # this build: rank every test triple against ITS OWN candidates - two .npy id matrices [test triples, n] (corrupted
        # heads, corrupted tails; -1 pads a row; `none` leaves a side out), the ogbl-wikikg2 / ogbl-biokg protocol
        a('--eval_candidates', type=str, default=None, nargs=2, metavar=('HEAD.npy', 'TAIL.npy'))
        # this build: after the entity metrics, rank the true RELATION of every test triple among all relations (h, ?, t) and
        # print REL_MRR / REL_MR / REL_HITS@k; filtered unless --no_eval_filter
        a('--eval_relation', action='store_true')


def main(argv=None):
    from . import eval as kev
    args = ArgParser().parse_args(argv)
    args.eval_filter = not args.no_eval_filter
    if args.neg_deg_sample_eval and args.eval_filter:
        raise KgeError("if negative sampling based on degree, we can't filter positive edges.")
    if args.eval_candidates and (args.neg_sample_size_eval > 0 or args.neg_deg_sample_eval):
        raise KgeError("--eval_candidates ranks against the given lists: --neg_sample_size_eval / --neg_deg_sample_eval do not apply")
    if len(args.gpu) > 1 and args.neg_deg_sample_eval:
        raise KgeError("--neg_deg_sample_eval is not available on sharded tables")
    if len(args.gpu) > 1 and args.eval_candidates:
        raise KgeError("--eval_candidates is not available on sharded tables")
    if len(args.gpu) > 1 and args.eval_relation:
        raise KgeError("--eval_relation is not available on sharded tables")
    if args.eval_relation and args.eval_candidates:
        raise KgeError("--eval_relation ranks against all relations: the lists of --eval_candidates are entity lists")
    if args.gpu[0] < 0:
        raise KgeError("dglke_eval ranks on the GPU only: pass --gpu <id> (there is no CPU fallback)")
    if not os.path.isdir(args.model_path):
        raise KgeError("No existing model_path: {}".format(args.model_path))
    if len(args.gpu) > 1:
        return launch_sharded(args)
    dev = th.device("cuda", args.gpu[0])
    th.cuda.set_device(dev)
    ds = get_dataset(args.data_path, args.dataset, args.format, args.delimiter, args.data_files)
    if ds.test is None:
        raise KgeError("the dataset has no test split")
    model = 'TransE_l2' if args.model_name == 'TransE' else args.model_name
    stem = os.path.join(args.model_path, '{}_{}_'.format(args.dataset, args.model_name))

    def load(name):
        f = stem + name + '.npy' if name != 'projection' else stem[:-1] + 'projection.npy'
        if not os.path.exists(f):
            raise KgeError("missing embedding file {}".format(f))
        return th.from_numpy(np.load(f)).to(dev, th.float32).contiguous()
    ent, rel = load('entity'), load('relation')
    proj = load('projection') if model == 'TransR' else None
    d_e = args.hidden_dim * (2 if args.double_ent else 1)
    if ent.shape != (ds.n_entities, d_e):
        raise KgeError("entity embeddings are {} but the dataset / flags say {}".format(tuple(ent.shape), (ds.n_entities, d_e)))
    emb_init = (args.gamma + 2.0) / args.hidden_dim
    h, r, t = (np.asarray(x) for x in ds.test[:3])
    cands = [None, None]
    if args.eval_candidates:
        for k, f in enumerate(args.eval_candidates):
            if f.lower() == 'none':
                continue
            if not os.path.exists(f):
                raise KgeError("missing candidate file {}".format(f))
            c = np.load(f)
            if c.ndim != 2 or c.shape[0] != len(h) or not np.issubdtype(c.dtype, np.integer):
                raise KgeError("candidate file {} holds {} {}: expected an integer matrix with one row for each of the {} test "
                               "triples".format(f, c.dtype, tuple(c.shape), len(h)))
            cands[k] = c
        if cands[0] is None and cands[1] is None:
            raise KgeError("--eval_candidates: at least one of the two files must be given")
    if args.eval_percent < 1:
        keep = np.random.RandomState(args.seed + 17).permutation(len(h))[:max(1, int(len(h) * args.eval_percent))]
        h, r, t = h[keep], r[keep], t[keep]
        cands = [c[keep] if c is not None else None for c in cands]
    known = None
    if args.eval_filter:
        parts = [p for p in (ds.train, ds.valid, ds.test) if p is not None]
        known = tuple(np.concatenate([np.asarray(p[k]) for p in parts]) for k in range(3))
    Eb = int(max(1, min(max(args.batch_size_eval, 4096), (1 << 31) // (4 * ds.n_entities), len(h))))
    if proj is not None:
        Eb = min(Eb, 64)
    start = time.time()
    if args.eval_candidates:
        metrics = kev.evaluate_candidates(model, ent, rel, args.gamma, emb_init, (h, r, t), cands[0], cands[1], known, batch=Eb,
                                          proj=proj)
    else:
        metrics = kev.evaluate(model, ent, rel, args.gamma, emb_init, (h, r, t), known, batch=Eb, proj=proj,
                               n_cand=args.neg_sample_size_eval if args.neg_sample_size_eval > 0 else None,
                               chunk=args.batch_size_eval, seed=args.seed + 29, neg_deg_sample=args.neg_deg_sample_eval)
    for k, v in metrics.items():
        print('[{}]{} average {}: {}'.format(0, 'Test', k, v))          # train_pytorch.py:236-247 format
    if args.eval_relation:
        rel_metrics = kev.evaluate_relations(model, ent, rel, args.gamma, emb_init, (h, r, t), known, batch=Eb, proj=proj)
        for k, v in rel_metrics.items():
            print('[{}]{} average REL_{}: {}'.format(0, 'Test', k, v))
            metrics['REL_' + k] = v
    print('Test takes {:.3f} seconds'.format(time.time() - start))
    return metrics


def _sharded_worker(rank, args, port):
    """one of the `--gpu g0 g1 ...` processes: maps only its row range of the entity file, loads the relation-side tables whole
    and ranks the test triples against its rows (eval.evaluate_sharded); the row exchange goes through RCCL when every process
    has its own GPU, through the gloo group when they share one (like dglke_train's trainers)."""
    import torch.distributed as dist
    from . import dist as kd
    from . import eval as kev
    world = len(args.gpu)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    comm = None
    try:
        dev = th.device("cuda", args.gpu[rank])
        th.cuda.set_device(dev)
        if rank != 0:                            # one copy of the loader messages is enough
            sys.stdout = open(os.devnull, "w")
        ds = get_dataset(args.data_path, args.dataset, args.format, args.delimiter, args.data_files)
        sys.stdout = sys.__stdout__
        if ds.test is None:
            raise KgeError("the dataset has no test split")
        model = 'TransE_l2' if args.model_name == 'TransE' else args.model_name
        stem = os.path.join(args.model_path, '{}_{}_'.format(args.dataset, args.model_name))

        def path(name):
            f = stem + name + '.npy' if name != 'projection' else stem[:-1] + 'projection.npy'
            if not os.path.exists(f):
                raise KgeError("missing embedding file {}".format(f))
            return f
        full = np.load(path('entity'), mmap_mode='r')
        d_e = args.hidden_dim * (2 if args.double_ent else 1)
        if full.shape != (ds.n_entities, d_e):
            raise KgeError("entity embeddings are {} but the dataset / flags say {}".format(tuple(full.shape), (ds.n_entities, d_e)))
        spec = kd.ShardSpec(ds.n_entities, world, rank)
        shard = th.from_numpy(np.ascontiguousarray(full[spec.lo:spec.hi])).to(dev, th.float32).contiguous()
        del full
        rel = th.from_numpy(np.load(path('relation'))).to(dev, th.float32).contiguous()
        proj = th.from_numpy(np.load(path('projection'))).to(dev, th.float32).contiguous() if model == 'TransR' else None
        comm = kd.make_comm() if len(set(args.gpu)) == world else kd.HostStagedComm()
        emb_init = (args.gamma + 2.0) / args.hidden_dim
        h, r, t = (np.asarray(x) for x in ds.test[:3])
        if args.eval_percent < 1:
            keep = np.random.RandomState(args.seed + 17).permutation(len(h))[:max(1, int(len(h) * args.eval_percent))]
            h, r, t = h[keep], r[keep], t[keep]
        known = None
        if args.eval_filter:
            parts = [p for p in (ds.train, ds.valid, ds.test) if p is not None]
            known = tuple(np.concatenate([np.asarray(p[k]) for p in parts]) for k in range(3))
        Eb = int(max(1, min(max(args.batch_size_eval, 4096), (1 << 31) // (4 * ds.n_entities), len(h))))
        if proj is not None:
            Eb = min(Eb, 64)
        start = time.time()
        metrics = kev.evaluate_sharded(model, shard, spec.lo, ds.n_entities, rel, args.gamma, emb_init, (h, r, t),
                                       lambda ids: kev.allgather_rows(shard, spec.lo, spec.bounds(), ids, comm), known, batch=Eb,
                                       proj=proj, n_cand=args.neg_sample_size_eval if args.neg_sample_size_eval > 0 else None,
                                       chunk=args.batch_size_eval, seed=args.seed + 29)
        if rank == 0:
            for k, v in metrics.items():
                print('[{}]{} average {}: {}'.format(0, 'Test', k, v))          # train_pytorch.py:236-247 format
            print('Test takes {:.3f} seconds'.format(time.time() - start))
            print('sharded evaluation: world size {}, entity rows per rank {}'.format(
                world, [int(b - a) for a, b in zip(spec.bounds()[:-1], spec.bounds()[1:])]))
            sys.stdout.flush()
    finally:
        if comm is not None and hasattr(comm, "close"):
            comm.close()
        dist.destroy_process_group()


def launch_sharded(args):
    """`--gpu g0 g1 ...`: one process per entry (the same GPU may be listed twice: the processes then share it), the gloo
    bootstrap of dglke_train's trainers (train._mp_worker)."""
    import socket
    import torch.multiprocessing as mp
    if min(args.gpu) < 0:
        raise KgeError("dglke_eval ranks on the GPU only: pass --gpu <ids> (there is no CPU fallback)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_sharded_worker, args=(args, port), nprocs=len(args.gpu), join=True)
    return None


if __name__ == '__main__':
    try:
        main()
    except KgeError as e:
        sys.exit("dglke_eval: %s" % e)
