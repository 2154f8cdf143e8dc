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

from . import dist as kd
from . import eval as kev
from . import models
from ._lib import KgeError


class ArgParser(argparse.ArgumentParser):
    def __init__(self):
        super(ArgParser, self).__init__()
        a = self.add_argument
        a('--model_name', default=models.DEFAULT, choices=models.NAMES)
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


def load_tables(args, ds, dev, rows=None):
    """the saved tables on `dev`: (entity, relation, projection or None).  rows = (lo, hi): only that row range of the entity
    file, read through a memory map.  The entity file's shape is checked against the dataset and the flags."""
    if ds.test is None:                 # (refused here: before any file is read)
        raise KgeError("the dataset has no test split")
    stem = os.path.join(args.model_path, '{}_{}'.format(args.dataset, args.model_name))

    def load(name, mmap=None):
        f = stem + name + '.npy'
        if not os.path.exists(f):
            raise KgeError("missing embedding file {}".format(f))
        return np.load(f, mmap_mode=mmap)

    def put(a):
        return th.from_numpy(a).to(dev, th.float32).contiguous()
    ent = load('_entity', 'r' if rows else None)
    d_e = args.hidden_dim * (2 if args.double_ent else 1)
    if ent.shape != (ds.n_entities, d_e):
        raise KgeError("entity embeddings are {} but the dataset / flags say {}".format(tuple(ent.shape), (ds.n_entities, d_e)))
    if rows:
        ent = np.ascontiguousarray(ent[rows[0]:rows[1]])
    return put(ent), put(load('_relation')), put(load('projection')) if models.MODELS[args.model_name].projection else None


def main(argv=None):
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
    from .train import check_model_widths     # before anything is loaded
    check_model_widths(args.model_name, args.hidden_dim, args.double_ent, args.double_rel)
    m = models.MODELS[args.model_name]
    if m.single_gpu_only and len(args.gpu) > 1:
        raise KgeError("%s is not available on sharded tables (--gpu takes one entry)" % m.name)
    if m.no_relation_ranking and args.eval_relation:
        raise KgeError("%s has no relation ranking (--eval_relation): %s" % (m.name, m.no_relation_ranking))
    if args.gpu[0] < 0:
        raise KgeError("dglke_eval ranks on the GPU only: pass --gpu <id> (there is no CPU fallback)")
    if not os.path.isdir(args.model_path):
        raise KgeError("No existing model_path: {}".format(args.model_path))
    if len(args.gpu) > 1:
        if min(args.gpu) < 0:
            raise KgeError("dglke_eval ranks on the GPU only: pass --gpu <ids> (there is no CPU fallback)")
        kd.spawn_ranks(_sharded_worker, args)
        return None
    dev = th.device("cuda", args.gpu[0])
    th.cuda.set_device(dev)
    ds = kd.load_dataset(0, args)
    ent, rel, proj = load_tables(args, ds, dev)
    model = models.MODELS[args.model_name].alias_of or args.model_name
    emb_init = (args.gamma + 2.0) / args.hidden_dim
    cands = None
    if args.eval_candidates:
        cands = [None, None]
        for k, f in enumerate(args.eval_candidates):
            if f.lower() == 'none':
                continue
            if not os.path.exists(f):
                raise KgeError("missing candidate file {}".format(f))
            c = np.load(f)
            if c.ndim != 2 or c.shape[0] != len(ds.test[0]) or not np.issubdtype(c.dtype, np.integer):
                raise KgeError("candidate file {} holds {} {}: expected an integer matrix with one row for each of the {} test "
                               "triples".format(f, c.dtype, tuple(c.shape), len(ds.test[0])))
            cands[k] = c
        if cands[0] is None and cands[1] is None:
            raise KgeError("--eval_candidates: at least one of the two files must be given")
    test, known, Eb, cands = kev.eval_setup(ds, 'test', args, cands)
    start = time.time()
    if cands:
        metrics = kev.evaluate_candidates(model, ent, rel, args.gamma, emb_init, test, cands[0], cands[1], known, batch=Eb, proj=proj)
    else:
        metrics = kev.evaluate(model, ent, rel, args.gamma, emb_init, test, known, batch=Eb, proj=proj,
                               n_cand=args.neg_sample_size_eval, chunk=args.batch_size_eval, seed=args.seed + 29,
                               neg_deg_sample=args.neg_deg_sample_eval)
    kev.print_metrics('Test', metrics)
    if args.eval_relation:
        rel_metrics = kev.evaluate_relations(model, ent, rel, args.gamma, emb_init, test, known, batch=Eb, proj=proj)
        rel_metrics = {'REL_' + k: v for k, v in rel_metrics.items()}
        kev.print_metrics('Test', rel_metrics)
        metrics.update(rel_metrics)
    print('Test takes {:.3f} seconds'.format(time.time() - start))
    return metrics


def _sharded_worker(rank, args):
    """one of the `--gpu g0 g1 ...` processes: maps only its row range of the entity file, loads the relation-side tables whole
    and ranks the test triples against its rows (eval.evaluate_sharded); the row exchange goes through RCCL when every process
    has its own GPU, through the gloo group when they share one (like dglke_train's trainers)."""
    world = len(args.gpu)
    dev = th.device("cuda", args.gpu[rank])
    th.cuda.set_device(dev)
    ds = kd.load_dataset(rank, args)
    spec = kd.ShardSpec(ds.n_entities, world, rank)
    shard, rel, proj = load_tables(args, ds, dev, rows=(spec.lo, spec.hi))
    model = models.MODELS[args.model_name].alias_of or args.model_name
    comm = kd.make_comm() if len(set(args.gpu)) == world else kd.HostStagedComm()
    try:
        test, known, Eb, _ = kev.eval_setup(ds, 'test', args)
        start = time.time()
        metrics = kev.evaluate_sharded(model, shard, spec.lo, ds.n_entities, rel, args.gamma, (args.gamma + 2.0) / args.hidden_dim,
                                       test, lambda ids: kev.allgather_rows(shard, spec.lo, spec.bounds(), ids, comm), known,
                                       batch=Eb, proj=proj, n_cand=args.neg_sample_size_eval, chunk=args.batch_size_eval,
                                       seed=args.seed + 29)
        if rank == 0:
            kev.print_metrics('Test', metrics)
            print('Test takes {:.3f} seconds'.format(time.time() - start))
            print('sharded evaluation: world size {}, entity rows per rank {}'.format(
                world, [int(b - a) for a, b in zip(spec.bounds()[:-1], spec.bounds()[1:])]))
            sys.stdout.flush()
    finally:
        if hasattr(comm, "close"):
            comm.close()


if __name__ == '__main__':
    try:
        main()
    except KgeError as e:
        sys.exit("dglke_eval: %s" % e)
