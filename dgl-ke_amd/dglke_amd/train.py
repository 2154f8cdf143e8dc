"""`dglke_train`-compatible entry point (reference: python/dglke/train.py:40-330 + the common flags of
python/dglke/utils.py:199-297): same flag names, same dataset formats, same log-line formats, same
output files (`<save_path>/<model>_<dataset>_<n>/<dataset>_<model>_{entity,relation}.npy` +
config.json, utils.py:35-49) so that `dglke_eval`, `dglke_predict` and `dglke_emb_sim` (ours in dgl-ke_amd/, or the
reference's) can consume the embeddings.

What is different underneath: the per-step loop `sample -> forward -> backward -> update`
(train_pytorch.py:132-152) is ONE fused HIP step (`kge_step_fused`) fed by the on-device sampler,
replayed from a hipGraph; validation / test are one `kge_rank_eval` call per corruption mode instead
of the per-triple Python loop.  There is no CPU training path: `--gpu` must name a GPU.

One training loop (`_Trainer.train`) drives the three trainers: `Trainer` (one GPU; `--num_proc` lanes = streams) and, one process
per entry of `--gpu g0 g1 ...`, `A2ATrainer` (range-sharded entity table, all-to-all exchanges) or `ShardedTrainer` (peer-to-peer
mapped tables).

    python -m dglke_amd.train --model_name TransE_l2 --dataset FB15k --data_path data --gpu 0 \\
        --batch_size 1000 --neg_sample_size 200 --hidden_dim 400 --gamma 19.9 --lr 0.25 \\
        --max_step 24000 --log_interval 1000 --batch_size_eval 16 -adv --regularization_coef 1e-9 --test
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch as th

from . import _lib
from . import checkpoint as ckpt
from . import dist as kd
from . import eval as kev
from . import models
from ._lib import KgeError
from .dataloader import DeviceSampler, UniformChunkedSampler
from .engine import StepEngine


class ArgParser(argparse.ArgumentParser):
    """flags of utils.py:199-297 (CommonArgParser) + train.py:40-60 (ArgParser)."""

    def __init__(self):
        super(ArgParser, self).__init__(prog="dglke_train")
        a = self.add_argument
        a('--model_name', default=models.DEFAULT, choices=models.NAMES)
        a('--data_path', type=str, default='data')
        a('--dataset', type=str, default='FB15k')
        a('--format', type=str, default='built_in')
        a('--data_files', type=str, default=None, nargs='+')
        a('--delimiter', type=str, default='\t')
        a('--save_path', type=str, default='ckpts')
        a('--no_save_emb', action='store_true')
        a('--max_step', type=int, default=80000)
        a('--batch_size', type=int, default=1024)
        a('--batch_size_eval', type=int, default=8)
        a('--neg_sample_size', type=int, default=256)
        a('--neg_deg_sample', action='store_true')
        a('--neg_deg_sample_eval', action='store_true')
        a('--neg_sample_size_eval', type=int, default=-1)
        a('--eval_relation', action='store_true')    # this build: REL_MRR / REL_MR / REL_HITS@k of (h, ?, t) after the entity metrics
        a('--eval_percent', type=float, default=1)
        a('--no_eval_filter', action='store_true')
        a('-log', '--log_interval', type=int, default=1000)
        a('--eval_interval', type=int, default=10000)
        a('--test', action='store_true')
        a('--num_proc', type=int, default=1)
        a('--num_thread', type=int, default=1)
        a('--force_sync_interval', type=int, default=-1,
          help='multi-GPU: every trainer waits at a barrier every this many steps (reference flag; -1: never)')
        a('--hidden_dim', type=int, default=400)
        a('--lr', type=float, default=0.01)
        a('-g', '--gamma', type=float, default=12.0)
        a('-de', '--double_ent', action='store_true')
        a('-dr', '--double_rel', action='store_true')
        a('-adv', '--neg_adversarial_sampling', action='store_true')
        a('-a', '--adversarial_temperature', default=1.0, type=float)
        a('-rc', '--regularization_coef', type=float, default=0.000002)
        a('-rn', '--regularization_norm', type=int, default=3)
        a('-pw', '--pairwise', action='store_true')
        a('--loss_genre', default='Logsigmoid', choices=['Hinge', 'Logistic', 'Logsigmoid', 'BCE', 'Softmax'])
        a('-m', '--margin', type=float, default=1.0)
        a('--gpu', type=int, default=[-1], nargs='+')
        a('--mix_cpu_gpu', action='store_true')
        a('--valid', action='store_true')
        a('--rel_part', action='store_true',
          help='multi-GPU a2a mode: split the training triples BY RELATION over the trainers (see --rel_part_policy); while every '
               'relation lives on one trainer its row is updated only there - no relation exchange')
        a('--rel_part_policy', default='auto', choices=['auto', 'soft', 'whole'],
          help='whole: whole relations, most frequent first, to the trainer with the fewest edges (never split: a relation with more '
               'than 1 / trainers of the edges unbalances the split).  soft: the reference\'s partition (SoftRelationPartition: '
               'relations with more than min(5 %%, 1 / trainers) of the edges are dealt evenly over all trainers) - even edge shares; '
               'the relation gradients are then all-gathered and applied by every trainer.  auto (default): whole while the fullest '
               'trainer stays within 1.1 x the mean edge share, soft otherwise')
        a('--async_update', action='store_true')
        a('--has_edge_importance', action='store_true',
          help='train.txt carries a 4th column of edge weights (reference flag).  Batches then come from the host sampler; with several '
               'GPUs both modes take them step by step (eager launches)')
        # additions of this build
        a('--async_update_rel', action='store_true',
          help='with --async_update: defer the relation-table update by one step as well (the reference defers the entity '
               'table only); the next step\'s gather then shares a launch with this step\'s backward (fastest mode)')
        a('--async_update_pipeline', action='store_true',
          help='with --async_update (entity table only, the reference\'s semantics): run the one-step-stale pipeline anyway.  By '
               'default the flag maps onto the STRICT step, which is faster on this GPU than a pipeline that must still land the '
               'relation trace between two steps (profiles/r03_v3_workloads_kernels.txt: 32.9 vs 30.7 us per cfg-T step) and is '
               'within the licence of the flag (staleness <= 1 step; here 0)')
        a('--exclude_positive', action='store_true',
          help='leave known training triples out of the negatives: a sampled entity whose corrupted triple (n, r, t) / (h, r, n) is in '
               'the training split contributes neither loss nor gradient nor self-adversarial weight (the reference sampler\'s '
               'exclude_positive parameter, which its CLI never sets; "filtered negatives" elsewhere).  One GPU; not with '
               '--neg_deg_sample, --async_update_pipeline or --async_update_rel')
        a('-sw', '--subsampling_weight', action='store_true',
          help='weight every training triple by 1 / sqrt(count(h, r) + count(t, r^-1)), the counts over the training split and both '
               'started at 3 (the subsampling weights of the RotatE, OGB and PairRE code bases), normalised to mean 1 over the split.  '
               'Computed once on the device; the batches come from the weighted device sampler (captured graphs).  One GPU; not with '
               '--has_edge_importance, --async_update_pipeline or --async_update_rel; batches the device sampler cannot build are '
               'refused')
        a('--edge_importance_on_device', action='store_true',
          help='with --has_edge_importance: hand the weight column of train.txt to the weighted device sampler instead of the host '
               'sampler (same refusals as --subsampling_weight)')
        a('--optimizer', default='Adagrad', choices=['Adagrad', 'Adam'],
          help='Adagrad: the reference\'s row-sparse Adagrad.  Adam: lazy row-sparse Adam with a per-row step count (the rule of '
               'DGL\'s sparse Adam) in the strict step\'s update launch; --lr is its step size (1e-4 ... 1e-3 in the published Adam '
               'recipes).  Moment tables take twice the embedding tables\' memory.  One GPU; not for RESCAL / TransR, not with '
               '--async_update_pipeline or --async_update_rel; row widths multiples of 4, at most 1024 floats')
        a('--adam_beta1', type=float, default=0.9, help='--optimizer Adam: decay of the first moment')
        a('--adam_beta2', type=float, default=0.999, help='--optimizer Adam: decay of the second moment')
        a('--adam_eps', type=float, default=1e-8, help='--optimizer Adam: the term added to the root of the second moment')
        a('--ent_norm', default='none', choices=list(models.NORM_MODES),
          help='norm constraint of radius 1 on the entity rows every step has updated, applied by one more launch behind the update: '
               'clip scales a row onto the unit sphere only when its norm exceeds 1 (TransH / TransR / TransD: |e| <= 1), unit every '
               'non-zero row (TransE: |e| = 1).  TransD: the halves [e | e_p] each on their own.  Fresh tables are projected once, whole.  '
               'One GPU; not with --async_update_pipeline or --async_update_rel')
        a('--rel_norm', default='none', choices=list(models.NORM_MODES),
          help='the same on the relation rows.  PairRE [rH | rT] and TransD [r | r_p]: the halves each on their own; TransH [d | w]: d '
               'by the mode, w always to length 1.  Not for RotatE (the row holds phases), RESCAL and TransR (their relation-side '
               'tables are updated by kernels of their own)')
        a('--dist_slack', type=float, default=None,
          help='--dist_mode a2a: initial capacity of an owner bucket as a multiple of the mean share of a batch\'s unique entities '
               '(default 1.5, or KGE_DIST_SLACK); buckets grow by themselves when a group of batches needs more')
        a('--dist_mode', default='a2a', choices=['a2a', 'p2p'],
          help='multi-GPU training (--gpu g0 g1 ...): a2a = entity table range-sharded, relation table replicated, RCCL '
               'all-to-all pull / push with owner-side Adagrad (parameter-server semantics); p2p = both tables sharded and '
               'mapped peer to peer (hipIpc), Hogwild across the trainers, no collective.  TransR and RESCAL train in both modes '
               'with the entity table sharded, relation rows / matrices and the projection table local to the trainers and the '
               'triples partitioned by relation (the reference\'s --rel_part layout)')
        a('--dist_schedule', default=None, choices=['sync', 'pull', 'overlap'],
          help='--dist_mode a2a: where a step\'s exchanges run.  sync: on the compute stream, every step pulls after its predecessor\'s '
               'update has landed (default without --async_update); pull / overlap (need --async_update: one-step-stale entity rows): the '
               'next step\'s pull, or every exchange, on a side stream next to the compute (overlap: default with --async_update).  '
               'With --graph_steps > 0 the group - kernels and RCCL collectives - replays from one hipGraph; --graph_steps 0 launches '
               'eagerly (the way out if a recorded schedule ever stalls on a new software stack)')
        a('--checkpoint_interval', type=int, default=0,
          help='write a checkpoint to <run directory>/checkpoint every this many steps and at --max_step (0: none): the tables, the '
               'optimizer state (Adam: the moment tables too), every trainer\'s sampler state and loss sums - what --resume needs to '
               'continue the run bit for bit.  Only the newest is kept; the directory is also a model directory for dglke_eval / '
               'dglke_predict.  One GPU; not with --async_update_pipeline or --async_update_rel')
        a('--resume', type=str, default=None, metavar='PATH',
          help='continue the run whose checkpoint PATH holds (a run directory with checkpoint/, or a checkpoint directory) at its '
               'step + 1 up to --max_step, in a new run directory.  "latest": the newest checkpoint of this model and dataset under '
               '--save_path, a fresh run if there is none.  Model, widths, optimizer, --num_proc, batch geometry, --seed, the '
               'weighting flags and the dataset must be the checkpointed run\'s; every other flag may change (--lr, --max_step, ...)')
        a('--seed', type=int, default=0, help='seed of the table initialisation and of the device sampler')
        a('--graph_steps', type=int, default=100, help='steps per captured hipGraph (0: eager launches)')
        a('--target_mrr', type=float, default=None,
          help='with --valid: stop as soon as the validation MRR reaches this value and report the time')


def get_compatible_batch_size(batch_size, neg_sample_size, quiet=False):
    """utils.py:27-33"""
    if neg_sample_size < batch_size and batch_size % neg_sample_size != 0:
        old = batch_size
        batch_size = int(math.ceil(batch_size / neg_sample_size) * neg_sample_size)
        if not quiet:
            print('batch size ({}) is incompatible to the negative sample size ({}). Change the batch size to {}'.format(
            old, neg_sample_size, batch_size))
    return batch_size


def prepare_save_path(args):
    """train.py:62-72"""
    os.makedirs(args.save_path, exist_ok=True)
    folder = '{}_{}_'.format(args.model_name, args.dataset)
    n = len([x for x in os.listdir(args.save_path) if x.startswith(folder)])
    args.save_path = os.path.join(args.save_path, folder + str(n))
    os.makedirs(args.save_path, exist_ok=True)


def write_config(args, emap_file, rmap_file, path=None):
    """config.json of utils.py:35-49 (same keys, including the reference's 'emp_file' spelling); path: the directory it goes to
    (default: args.save_path)"""
    conf = dict(vars(args))
    conf.update({'emp_file': emap_file, 'rmap_file': rmap_file})
    with open(os.path.join(path or args.save_path, 'config.json'), 'w') as f:
        json.dump(conf, f, indent=4)


def save_model(args, model, emap_file=None, rmap_file=None):
    """utils.py:35-49"""
    os.makedirs(args.save_path, exist_ok=True)
    print('Save model to {}'.format(args.save_path))
    model.save_emb(args.save_path, args.dataset)
    write_config(args, emap_file, rmap_file)


def step_marks(max_step, log_interval, eval_interval, valid, force_sync_interval=-1, force_sync=False, checkpoint_interval=0,
               start_step=0):
    """the sorted steps at which the training loop stops enqueueing: every multiple of --log_interval, with --valid of
    --eval_interval, where the trainers wait for each other (force_sync) of --force_sync_interval, of --checkpoint_interval, and
    max_step; start_step (a resumed run): only the marks above it"""
    marks = {max_step}
    for iv in (log_interval, eval_interval if valid else 0, force_sync_interval if force_sync else 0, checkpoint_interval):
        if iv and iv > 0:
            marks.update(range(iv, max_step + 1, iv))
    return sorted(m for m in marks if m > start_step) if start_step else sorted(marks)


def plan_enqueue(n, G, host_step, have_group_graph, n_slots, rem_keys):
    """what `_Lane.enqueue(n)` does on the device sampler, as a list of (kind, k, parity) and the sampler's host step afterwards:
    k steps that start at a host step of that parity (1: the first of them corrupts tails), kind one of
      'eager'         one sampler launch + k steps, launched;
      'capture_group' the same recorded as THE group graph (k = G) - a capture runs nothing: the host step does not move;
      'replay_group'  the group graph replayed;
      'capture_rem'   recorded as the remainder graph of the key (k, parity);
      'replay_rem'    the remainder graph of the key (k, parity) replayed.
    The corruption side of slot j is baked into a recorded graph (DeviceBatch.neg_head) while the ids of the slot follow the device's
    own step counter, so a graph may only be replayed at the parity it was recorded at: the group graph (even G only) at odd host
    steps, a remainder graph under its key.  G = --graph_steps, have_group_graph: the lane holds the group graph, n_slots: the
    sampler's slots, rem_keys: the keys of the remainder graphs the lane holds (at most eight are recorded, and none before the
    group graph exists: a run too short for that one does not pay for captures)."""
    acts, hs, done, rem_keys = [], host_step, 0, set(rem_keys)
    if G >= 2 and G % 2 == 0 and n >= G and hs % 2 == 1:
        if not have_group_graph:
            acts.append(('eager', G, hs % 2))             # eager warm-up (also allocates the workspace)
            hs, done = hs + G, done + G
            if n - done >= G:
                acts.append(('capture_group', G, hs % 2))
                have_group_graph = True
        while have_group_graph and n - done >= G:
            acts.append(('replay_group', G, hs % 2))
            hs, done = hs + G, done + G
    while done < n:                                       # remainder (< G steps, or the parity of a full group is off)
        k = min(n_slots, n - done)
        key = (k, hs % 2)
        if key not in rem_keys and have_group_graph and len(rem_keys) < 8:
            # the log / eval marks repeat: record [1 sampler launch + k steps] once instead of paying
            # ~6 eager launches per step every time (56 -> 44 us/step at log_interval 1000, eval 500)
            acts.append(('capture_rem', k, hs % 2))
            rem_keys.add(key)
        acts.append(('replay_rem' if key in rem_keys else 'eager', k, hs % 2))
        hs, done = hs + k, done + k
    return acts, hs


class _Lane(object):
    """one trainer: a StepEngine (sharing the tables), its sampler over its share of the training triples,
    its HIP stream and - device sampler - a hipGraph of [1 sampler launch + G steps].  `--num_proc K` on
    one GPU = K lanes running concurrently, lock-free on the same tables: the reference's multi-process
    Hogwild training (train.py:298-317, RandomPartition of the edges sampler.py:256-290) with the
    processes replaced by streams."""

    def __init__(self, trainer, k, engine, part):
        self.t, self.k, self.engine = trainer, k, engine
        self.stream = th.cuda.current_stream() if trainer.n_lanes == 1 else th.cuda.Stream(device=trainer.dev)
        self.sampler = trainer.make_sampler(k, part)
        self._graph = None
        self._rem_graphs = {}
        # --async_update (reference: tensor_models.py:136-175, general_models.py:639-647): the one-step-stale pipeline of
        # kge_step_async - the entity update of step s-1 shares a launch with the backward of step s; every captured /
        # enqueued group of steps ends with a flush
        self.async_update = trainer.async_update

    def _steps(self, batches):
        eng = self.engine
        if self.async_update:
            eng.steps_async(batches)
        else:
            for b in batches:
                eng.step(b)

    def timed_step(self):
        """one strict step with the reference's four timers (train_pytorch.py:132-152): returns seconds per phase"""
        with th.cuda.stream(self.stream):
            t0 = time.time()
            if self.t.device_sampler:
                e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                e0.record()
                b = self.sampler.sample(1)[0]
                e1.record()
                d = self.engine.step_timed(b)
                # one sampler launch builds a whole group of batches in the training loop (its latency does not depend on the
                # count): this step's share of a launch is 1 / group
                smp = e0.elapsed_time(e1) * 1e-3 / max(1, self.t.args.graph_steps)
            else:
                b = self.sampler.next_batches(1)[0]
                smp = time.time() - t0
                d = self.engine.step_timed(b)
        if d is not None:
            d['sample'] = smp
        return d

    def enqueue(self, n):
        """enqueue n steps on this lane's stream (no synchronisation)."""
        t = self.t
        with th.cuda.stream(self.stream):
            if not t.device_sampler:
                self._steps(self.sampler.next_batches(n))
                return
            smp = self.sampler
            acts, _ = plan_enqueue(n, t.args.graph_steps, smp.host_step, self._graph is not None, smp.n_slots, self._rem_graphs)
            for kind, k, parity in acts:
                if kind == 'eager':
                    self._steps(smp.sample(k))
                elif kind in ('capture_group', 'capture_rem'):
                    self.stream.synchronize()
                    g = th.cuda.CUDAGraph()
                    with _lib.graph_capture(g, stream=self.stream if t.n_lanes > 1 else None):
                        self._steps(smp.sample(k))
                    smp.host_step -= k                # the capture itself did not run the steps
                    if kind == 'capture_group':
                        self._graph = g
                    else:
                        self._rem_graphs[(k, parity)] = g
                else:
                    (self._graph if kind == 'replay_group' else self._rem_graphs[(k, parity)]).replay()
                    smp.host_step += k


class _Trainer(object):
    """what the three trainers share: the device, the batch geometry, the split of the training triples, the samplers, the
    engines and the training loop of train_pytorch.py:105-196 over the fused step.  A trainer says how n steps are enqueued
    (`enqueue`), whose loss sums it prints (`loss_engines`), and - one process per GPU - how the processes meet (`barrier`) and
    what a validation needs first (`sync_tables`)."""

    def __init__(self, args, dataset, rank=0, world=1):
        self.args, self.dataset, self.rank, self.world = args, dataset, rank, world
        if args.gpu[rank] < 0:
            raise KgeError("dglke_amd trains on the GPU only: pass --gpu <id> (there is no CPU fallback)")
        th.cuda.set_device(args.gpu[rank])
        self.dev = th.device("cuda", args.gpu[rank])
        B, N = args.batch_size, args.neg_sample_size
        self.chunk = N if N <= B else B
        self.C = B // self.chunk
        self.d_e = args.hidden_dim * (2 if args.double_ent else 1)
        self.d_r = args.hidden_dim * (2 if args.double_rel else 1)
        self.emb_init = (args.gamma + 2.0) / args.hidden_dim
        # the on-device sampler builds the batches of a whole group ahead; batches it cannot build - edge importance, or more ids
        # than its launch handles - come from the host sampler (plans built on the host, step by step)
        self.device_sampler = not args.has_edge_importance and 2 * B + self.C * N <= DeviceSampler.MAX_ELEMENTS
        # weights the DEVICE sampler carries (--subsampling_weight, --has_edge_importance --edge_importance_on_device): one float per
        # triple of the training split, set by the trainer before its lanes make their samplers
        self.weighted = weighted_device_sampler(args)
        if self.weighted:
            self.device_sampler = True                # (check_weighted_device_sampler has refused what the sampler cannot build)
        self.edge_weights = None
        self.n_lanes, self.async_update, self.known = 1, False, None

    def make_engine(self, n_entities=None, **tables):
        """a StepEngine of the flags on this trainer's device; tables= / shards=: the tables it trains (default: its own)"""
        return StepEngine.from_args(self.args, self.args.model_name, n_entities or self.dataset.n_entities,
                                    self.dataset.n_relations, self.dev, **tables)

    def split(self, n, edge_rank=None, refusal=None):
        """the rows of the training split of each of n trainers: those a relation partition assigns (edge_rank[i] = the trainer
        of triple i), else a random partition by --seed (RandomPartition, sampler.py:256-290; one trainer: every row, in order).
        Both samplers work on whole batches (the reference drops partial ones, dataloader/sampler.py:503-504), so a trainer whose
        share is smaller than one batch could never step: refused here - the partition is the same on every rank, so every rank
        raises, before any collective.  refusal: the caller's wording, a template over the names below."""
        n_trip, B = len(self.dataset.train[0]), self.args.batch_size
        if edge_rank is not None:
            parts = [np.nonzero(edge_rank == k)[0] for k in range(n)]
        elif n > 1:
            parts = np.array_split(np.random.RandomState(self.args.seed).permutation(n_trip), n)
        else:
            parts = [slice(None)]               # (a view: a large split is not copied)
        share = [len(range(n_trip)[p]) if isinstance(p, slice) else len(p) for p in parts]
        if min(share) < B:
            refusal = refusal or ("--batch_size %(batch)d is larger than a trainer's share of the training triples (%(triples)d "
                                  "over %(n)d trainers)")
            raise KgeError(refusal % dict(trainer=int(np.argmin(share)), share=min(share), batch=B, triples=n_trip, n=n))
        return parts

    def make_sampler(self, k, part):
        """trainer k's sampler over the rows `part` of the training split"""
        a, tr = self.args, self.dataset.train
        h, r, t = (np.asarray(x)[part] for x in tr[:3])
        if self.device_sampler:
            w = None
            if self.weighted:                         # the rows of this lane's part; the counts behind them are the whole split's
                w = self.edge_weights if isinstance(part, slice) else self.edge_weights[th.as_tensor(np.asarray(part), device=self.dev)]
            return DeviceSampler(h, r, t, self.dataset.n_entities, a.batch_size, a.neg_sample_size, self.dev,
                                 n_slots=max(2, a.graph_steps or 2), neg_chunk_size=self.chunk, seed=a.seed + 1000 * k,
                                 edge_importance=w)
        w = np.asarray(tr[3])[part] if a.has_edge_importance else None
        return UniformChunkedSampler(h, r, t, self.dataset.n_entities, a.batch_size, a.neg_sample_size, self.dev,
                                     neg_chunk_size=self.chunk, seed=a.seed + 1000 * k, edge_importance=w)

    def loss_engines(self):
        """(proc number, engine) of the loss sums this process prints at a log mark"""
        return [(self.rank, self.engine)]

    def barrier(self):
        pass

    def sync_tables(self):
        pass

    def train(self, start_step=0, start_since_log=0):
        """start_step, start_since_log (a resumed run, whose state the caller has put back): the steps already trained and how many
        of them the lanes' loss sums hold - the loop goes on with step start_step + 1"""
        args = self.args
        keys = ['loss'] if args.pairwise or args.loss_genre == 'Softmax' else ['pos_loss', 'neg_loss', 'loss']
        if args.regularization_coef > 0 and args.regularization_norm > 0:
            keys.append('regularization')
        idx = {'pos_loss': 0, 'neg_loss': 1, 'loss': 2, 'regularization': 3}
        # --force_sync_interval (reference train_pytorch.py:181-187: every trainer waits at a barrier every so many steps, so that no
        # trainer of the lock-free shared-table modes runs far ahead of the others; the all-to-all mode is in step by construction).
        # --num_proc K lanes on one GPU are streams of this process: the synchronise at a mark IS their barrier
        fsi = args.force_sync_interval
        force_sync = fsi > 0 and (self.world > 1 or self.n_lanes > 1)
        # the reference's four timers (train_pytorch.py:127-177), one GPU, one lane, strict step: the LAST step before a log mark
        # runs as four phase groups with HIP events in between (same kernels, same result).  That one step is launched eagerly and
        # synchronised, so its absolute times are not those of the graph-replayed steps: only the SPLIT is taken from it - the
        # printed totals are the interval's measured training time divided in that step's proportions
        phase_timers = self.world == 1 and self.n_lanes == 1 and not self.lanes[0].async_update
        th.cuda.synchronize()
        self.barrier()
        train_start = start = time.time()
        step, since_log = int(start_step), int(start_since_log)
        t_train = t_interval = 0.0
        timed = reached = None
        ckpt_iv = getattr(args, 'checkpoint_interval', 0) or 0
        for nxt in step_marks(args.max_step, args.log_interval, args.eval_interval, args.valid, fsi, force_sync, ckpt_iv, step):
            n = nxt - step
            at_log = args.log_interval > 0 and nxt % args.log_interval == 0
            if n > 0:
                t0 = time.time()
                want_timers = at_log and phase_timers
                self.enqueue(n - 1 if want_timers else n)
                if want_timers:
                    th.cuda.synchronize()
                    timed = self.lanes[0].timed_step()
                th.cuda.synchronize()
                t_train += time.time() - t0
                t_interval += time.time() - t0
                step, since_log = nxt, since_log + n
            if force_sync and step % fsi == 0:
                self.barrier()
            if at_log and since_log:
                for proc, eng in self.loss_engines():
                    sums = eng.read_loss_sums()
                    for k in keys:
                        print('[proc {}][Train]({}/{}) average {}: {}'.format(proc, step, args.max_step, k, sums[idx[k]] / since_log))
                    print('[proc {}][Train] {} steps take {:.3f} seconds'.format(proc, since_log, time.time() - start))
                if timed is not None:
                    tot = sum(timed[k] for k in ('sample', 'forward', 'backward', 'update')) or 1.0
                    sc = t_interval / tot
                    print('[proc {}]sample: {:.3f}, forward: {:.3f}, backward: {:.3f}, update: {:.3f}'.format(
                        0, timed['sample'] * sc, timed['forward'] * sc, timed['backward'] * sc, timed['update'] * sc))
                    print('[proc {}](split of {:.3f} s over {} steps in the proportions of one phase-timed step)'.format(
                        0, t_interval, since_log))
                    timed = None
                t_interval = 0.0
                if self.world == 1:
                    norms = getattr(self, 'norms', (None, None))
                    print('[proc {}]sample+forward+backward+update (fused HIP step, {}{}{}{}{}{}): {:.3f}'.format(
                        0, args.optimizer, ', --async_update pipeline' if self.lanes[0].async_update else '',
                        ''.join(', --%s_norm %s' % (t, v) for t, v in zip(('ent', 'rel'), norms) if v),
                        ', known training triples excluded' if self.known is not None else '',
                        {None: '', 'subsampling': ', subsampling weights', 'file': ', edge importance on the device'}[self.weighted],
                        '' if self.n_lanes == 1 else ', %d concurrent trainers' % self.n_lanes, t_train))
                since_log, start = 0, time.time()
            if args.valid and step % args.eval_interval == 0 and step > 1 and self.dataset.valid is not None:
                self.barrier()                   # like the reference: all trainers stop for the validation
                self.sync_tables()
                valid_start = time.time()
                m = self.evaluate('valid', 'Valid')      # (several processes: every rank ranks against its own shard)
                if self.rank == 0:
                    print('[proc {}]validation take {:.3f} seconds:'.format(0, time.time() - valid_start))
                # --target_mrr stops a single-GPU run only: the multi-GPU trainers ignore the flag (their ranks would have to
                # agree on the stop and leave the loop's collectives together)
                if self.world == 1 and args.target_mrr is not None and m['MRR'] >= args.target_mrr:
                    reached = (step, t_train)
                    print('[proc 0]validation MRR {:.4f} >= {:.4f} after {} steps, {:.3f} s of training'.format(
                        m['MRR'], args.target_mrr, step, t_train))
                    break
                self.barrier()
                # (no reset of `start` here: the reference's '[Train] N steps take' interval includes a validation that falls
                #  inside it, train_pytorch.py:168-176)
            if ckpt_iv > 0 and (step % ckpt_iv == 0 or step == args.max_step):
                # between two steps, behind the mark's synchronize, its [Train] lines and its validation: only reads
                self.write_checkpoint(step, since_log)
        th.cuda.synchronize()
        print('proc {} takes {:.3f} seconds'.format(self.rank, time.time() - train_start))
        self.barrier()
        return reached


class Trainer(_Trainer):
    """one GPU: `--num_proc` lanes on the tables of one KEModel."""

    def __init__(self, args, dataset):
        from .general_models import KEModel
        super(Trainer, self).__init__(args, dataset)
        th.manual_seed(args.seed)
        # (the model's own engine is lane 0's: built from the same flags as the other lanes' - --neg_deg_sample runs on the fused
        # step for every model, the reference's concat-and-mask is model-agnostic, general_models.py:396-402, 417-432)
        self.model = m = KEModel(args, args.model_name, dataset.n_entities, dataset.n_relations, args.hidden_dim,
                                 args.gamma, double_entity_emb=args.double_ent, double_relation_emb=args.double_rel)
        self.step_flags = int(m.engine.hp.flags)
        self.norms = norm_constraints(args)
        if any(self.norms):
            # fresh tables, whole, once: rows no step has touched yet satisfy the constraint too (a --resume puts its tables back
            # over them and they are not projected again)
            m.engine.project_tables()
            print('[Train] --ent_norm {}, --rel_norm {}: every step projects the rows it has updated (radius 1); the fresh tables '
                  'were projected once'.format(self.norms[0] or 'none', self.norms[1] or 'none'))
        self.n_lanes = max(1, int(args.num_proc))
        # entity-only deferral (the reference's --async_update) runs as the strict step unless the pipeline is asked for: with the
        # relation trace landing between two steps the pipeline needs one more launch than it hides
        async_ok = not models.own_relation_update(models.MODELS[args.model_name])
        pipeline = args.async_update_rel or args.async_update_pipeline
        self.async_update = bool(args.async_update and async_ok and pipeline)
        if args.async_update and not async_ok:
            print('--async_update: not available for this model / option combination; running the strict step')
        elif args.async_update and not pipeline:
            print('--async_update: running the strict step (no staleness; faster on this GPU than the entity-only one-step-stale '
                  'pipeline - pass --async_update_rel to defer the relation trace too, or --async_update_pipeline to force it)')
        if self.weighted == 'subsampling':
            # ONE weight per triple of the whole training split, computed on the device once; every lane's sampler takes its rows
            from .dataloader import subsampling_weights
            check_weighted_device_sampler(args)
            self.edge_weights = subsampling_weights(dataset.train[0], dataset.train[1], dataset.train[2], dataset.n_entities,
                                                    dataset.n_relations, self.dev)
            print('[Train] --subsampling_weight: subsampling weights of {} training triples, mean 1, between {:.4f} and {:.4f}'.format(
                self.edge_weights.numel(), float(self.edge_weights.min()), float(self.edge_weights.max())))
        elif self.weighted == 'file':
            check_weighted_device_sampler(args)
            self.edge_weights = th.as_tensor(np.asarray(dataset.train[3], np.float32)).to(self.dev)
            print('[Train] --edge_importance_on_device: the edge importance of {} training triples goes through the device '
                  'sampler'.format(self.edge_weights.numel()))
        # the lanes share the tables (TransR: the projection table too); every lane trains on its own random share of the triples
        parts = self.split(self.n_lanes, refusal="every trainer needs at least batch_size training triples: %(triples)d triples over "
                           "%(n)d trainer(s) < batch_size %(batch)d - lower --batch_size or --num_proc")
        # (... and, under --optimizer Adam, the moment tables, exactly as they share the state)
        shared = dict(tables=m.tables())
        if m.engine.opt is not None:
            shared['moments'] = (m.engine.ent_mom, m.engine.rel_mom)
        self.lanes = [_Lane(self, k, m.engine if k == 0 else self.make_engine(**shared), parts[k])
                      for k in range(self.n_lanes)]
        if args.exclude_positive:
            # ONE index of the whole training split, sorted on the device once; the lanes' engines only read it
            from .known import KnownIndex
            check_exclude_positive(args)
            self.known = KnownIndex(tuple(np.asarray(x) for x in dataset.train[:3]), dataset.n_entities, dataset.n_relations,
                                    self.dev)
            for lane in self.lanes:
                lane.engine.attach_known(self.known)
            print('[Train] --exclude_positive: {} training triples are never a negative of their own (h, r) / (r, t)'.format(
                len(self.known)))

    def enqueue(self, n):
        """n steps on every lane, concurrently (no synchronisation here)."""
        for lane in self.lanes:
            lane.enqueue(n)

    def loss_engines(self):
        return [(lane.k, lane.engine) for lane in self.lanes]

    def write_checkpoint(self, step, since_log):
        """--checkpoint_interval: <run directory>/checkpoint as of `step` (checkpoint.save_trainer)"""
        nbytes, secs = ckpt.save_trainer(self, step, since_log, getattr(self, 'args_parsed', None))
        print('[proc 0]checkpoint at step {}: {} bytes in {:.3f} s'.format(step, nbytes, secs))

    def evaluate(self, which, mode):
        args, m = self.args, self.model
        test, known, Eb, _ = kev.eval_setup(self.dataset, which, args)
        proj = m.score_func.projection_emb.emb if models.MODELS[args.model_name].projection else None
        # (the split and the known set do not change during a run: filter lists and test ids stay on the device between validations)
        cache = self.__dict__.setdefault('_eval_cache', {}).setdefault(which, {})
        metrics = kev.evaluate(args.model_name, m.entity_emb.emb, m.relation_emb.emb, args.gamma, m.emb_init, test, known,
                               batch=Eb, proj=proj, n_cand=args.neg_sample_size_eval, chunk=args.batch_size_eval,
                               seed=args.seed + 29, cache=cache, neg_deg_sample=args.neg_deg_sample_eval)
        kev.print_metrics(mode, metrics)
        if args.eval_relation:
            rel_metrics = kev.evaluate_relations(args.model_name, m.entity_emb.emb, m.relation_emb.emb, args.gamma, m.emb_init,
                                                 test, known, batch=Eb, proj=proj, cache=cache)
            rel_metrics = {'REL_' + k: v for k, v in rel_metrics.items()}
            kev.print_metrics(mode, rel_metrics)
            metrics.update(rel_metrics)
        return metrics


class ShardedTrainer(_Trainer):
    """one of the `--gpu g0 g1 ...` trainer processes (reference: train.py:298-317, one process per GPU on
    tables in shared host memory).  Here the shared tables are the union of the GPUs' HBM, mapped peer to peer
    (dglke_amd/p2p.py): every process trains on its random share of the triples with the fused step
    (`kge_step_sharded`), lock-free across processes like the reference; the process group (gloo) is only
    used to exchange the hipIpc handles and for barriers.  What every multi-process trainer does the same way - barriers,
    evaluation and saving on the shards in place - is here too; `build` is this mode's own part."""

    def __init__(self, args, dataset, rank, world):
        super(ShardedTrainer, self).__init__(args, dataset, rank, world)
        # TransR / RESCAL: the entity table is spread over the GPUs like every model's; the relation side - relation rows / matrices
        # and TransR's projection table - is LOCAL to the trainer that holds the relation's edges, so the triples are partitioned
        # BY RELATION (whole relations): the reference's --rel_part layout, which its own multi-GPU TransR recipe passes
        # (examples/freebase/multi_gpu.sh:80-89, general_models.py:590-637).  The owners' rows are collected by sync_tables.
        self.rel_side_local = models.own_relation_update(models.MODELS[args.model_name])
        if self.rel_side_local and args.neg_deg_sample:
            raise KgeError("--neg_deg_sample is not available for %s on more than one GPU" % args.model_name)
        self.rel_owner = None
        self.build()

    def build(self):
        from . import p2p
        args, dataset, rank, world = self.args, self.dataset, self.rank, self.world
        edge_rank = refusal = None
        if self.rel_side_local:
            self.rel_owner, edge_rank = kd.relation_partition(dataset.train[1], world)
            refusal = "relation partition: trainer %(trainer)d gets %(share)d training triples, fewer than --batch_size %(batch)d"
            if rank == 0:
                print("%s on %d GPUs: entity table sharded peer to peer, relation-side tables local, triples partitioned by relation "
                      "(whole relations; edges per trainer %s)" % (args.model_name, world, np.bincount(edge_rank, minlength=world).tolist()))
        part = self.split(world, edge_rank, refusal)[rank]
        self.tabs = p2p.ShardedTables(dataset.n_entities, dataset.n_relations, self.d_e,
                                      self.d_r * self.d_e if models.MODELS[args.model_name].relation_matrix else self.d_r, self.dev, world, rank,
                                      rel_local=self.rel_side_local,
                                      proj_dim=self.d_e * self.d_r if models.MODELS[args.model_name].projection else 0)
        if not self.tabs.probe():
            raise KgeError("peer mappings do not reach the other GPUs' memory")
        self.tabs.init_uniform(self.emb_init, args.seed)
        self.engine = self.make_engine(shards=self.tabs)
        self.lane = _Lane(self, rank, self.engine, part)

    def enqueue(self, n):
        self.lane.enqueue(n)

    def barrier(self):
        import torch.distributed as dist
        dist.barrier()

    def sync_tables(self):
        """collective point in front of a validation / test / save: the peer-mapped tables need nothing; relation-side tables
        that are local to the trainers (TransR / RESCAL) are collected from the relations' owners into every rank's (every rank
        ranks against its own shard)."""
        if self.rel_side_local:
            th.cuda.synchronize()
            self.tabs.collect_relations(self.rel_owner, everywhere=True)

    def close(self):
        self.tabs.close()

    def projection(self):
        """TransR: the projection table as every rank holds it after sync_tables()"""
        return self.tabs.proj_tab

    def entity_shard(self):
        """(lo, rows [lo, hi) of the entity table that this rank holds)"""
        per, n = self.tabs.ent_per, self.dataset.n_entities
        lo = min(self.rank * per, n)
        return lo, self.tabs.ent()[:min(lo + per, n) - lo]

    def entity_rows(self, ids):
        """rows of the sorted unique global ids `ids` on this rank (collective in the all-to-all trainer)"""
        return self.tabs.gather("ent", ids)

    def relation_table(self):
        """the whole relation table on this rank"""
        if self.tabs.rel_local:
            return self.tabs.rel_tab
        return self.tabs.gather("rel", th.arange(self.dataset.n_relations, device=self.dev))

    def save(self, emap_file, rmap_file):
        """<dataset>_<model>_entity.npy written shard by shard into one file (dist.write_npy_sharded), the relation-side tables
        and config.json from rank 0.  Collective: every rank calls it after sync_tables()."""
        args = self.args
        rel = self.relation_table()
        lo, shard = self.entity_shard()
        kd.write_npy_sharded(os.path.join(args.save_path, '%s_%s_entity.npy' % (args.dataset, args.model_name)), shard, lo,
                             self.dataset.n_entities)
        if self.rank == 0:
            np.save(os.path.join(args.save_path, '%s_%s_relation.npy' % (args.dataset, args.model_name)), rel.cpu().numpy())
            if models.MODELS[args.model_name].projection:      # TransRScore.save (score_fun.py:190-191): <dataset>_<model>projection.npy
                np.save(os.path.join(args.save_path, '%s_%sprojection.npy' % (args.dataset, args.model_name)),
                        self.projection().cpu().numpy())
            write_config(args, emap_file, rmap_file)
        self.barrier()

    def evaluate(self, which, mode):
        """`--valid` / `--test` on the sharded table, collective: every rank ranks the split against the entities it holds
        (eval.evaluate_sharded); rank 0 prints the metrics."""
        args, ds = self.args, self.dataset
        test, known, Eb, _ = kev.eval_setup(ds, which, args)
        lo, shard = self.entity_shard()
        cache = self.__dict__.setdefault('_eval_cache', {}).setdefault(which, {})
        metrics = kev.evaluate_sharded(args.model_name, shard, lo, ds.n_entities, self.relation_table(), args.gamma, self.emb_init,
                                       test, self.entity_rows, known, batch=Eb,
                                       proj=self.projection() if models.MODELS[args.model_name].projection else None,
                                       n_cand=args.neg_sample_size_eval, chunk=args.batch_size_eval, seed=args.seed + 29, cache=cache)
        if self.rank == 0:
            kev.print_metrics(mode, metrics)
        return metrics


class A2ATrainer(ShardedTrainer):
    """`--gpu g0 g1 ... --dist_mode a2a`: the partitioning BASELINE.json's north_star names - the entity table range-sharded
    over the GPUs, the relation table REPLICATED (every relation row local to every trainer: what the reference's relation
    partitioning is after, general_models.py:590-637), parameter-server semantics as collectives (dglke_amd/dist.py
    DistEngine: pull -> compute -> push, the owner applies the sparse Adagrad in rank order; reference:
    general_models.py:650-680, kvserver.py:41-51).  Collectives: librccl called directly when every rank has its own GPU;
    ranks that share a GPU (`--gpu 0 0`) exchange through the gloo group (dist.HostStagedComm).  Validation, test and saving
    run on the shards in place (eval.evaluate_sharded, dist.write_npy_sharded)."""

    def build(self):
        args, dataset, rank, world = self.args, self.dataset, self.rank, self.world
        B, N = args.batch_size, args.neg_sample_size
        tr = dataset.train
        # --rel_part (the reference's multi-GPU recipes pass it, examples/freebase/multi_gpu.sh; always for TransR / RESCAL, whose
        # relation side is applied IN PLACE on the trainer that holds the relation's edges): the triples are split BY RELATION
        # (dist.choose_relation_partition: whole relations while that balances, else the reference's SoftRelationPartition with its
        # large relations dealt over all trainers).  While every relation lives on ONE trainer its row is updated there and nowhere
        # else - no relation exchange (dist.DistEngine rel_local); with split relations the relation gradients are all-gathered
        # and applied by every trainer like without --rel_part (exact for any edge split), only the edge shares are the reference's
        self.rel_part = args.rel_part or self.rel_side_local
        self.rel_local, edge_rank, refusal = False, None, None
        if self.rel_part:
            mode, edge_rank, self.rel_owner, cross = kd.choose_relation_partition(
                tr[1], world, 'whole' if self.rel_side_local else args.rel_part_policy)
            self.rel_local = len(cross) == 0
            n_rel = int((self.rel_owner != -1).sum())
            cnt = np.bincount(edge_rank, minlength=world)
            if rank == 0:
                print("relation partition (%s): %d relations over %d trainers, edges per trainer %s%s" % (
                    mode, n_rel, world, cnt.tolist(),
                    "" if self.rel_local else "; %d relations split over the trainers: relation gradients all-gathered" % len(cross)))
                if cnt.max() > 1.5 * cnt.mean():
                    # (--rel_part_policy whole only: a relation with more than 1 / world of the edges unbalances the trainers; every
                    # trainer runs max_step steps, so the light trainers revisit their edges more often than under the reference's split)
                    print("WARNING: --rel_part leaves trainer %d with %.2f x the mean edge share (whole relations only; the most "
                          "frequent relation holds %.1f %% of the edges; --rel_part_policy soft splits it)"
                          % (int(cnt.argmax()), cnt.max() / cnt.mean(), 100.0 * np.bincount(np.asarray(tr[1])).max() / len(tr[1])))
            refusal = ("--rel_part: trainer %%(trainer)d gets %%(share)d training triples, fewer than --batch_size %%(batch)d "
                       "(%d relations over %%(n)d trainers)" % n_rel)
        part = self.split(world, edge_rank, refusal)[rank]
        self.spec = kd.ShardSpec(dataset.n_entities, world, rank)
        th.manual_seed(args.seed + 7919 * (rank + 1))
        self.ent = th.empty(self.spec.n_local, self.d_e, dtype=th.float32, device=self.dev).uniform_(-self.emb_init, self.emb_init)
        self.ent_state = th.zeros(self.spec.n_local, dtype=th.float32, device=self.dev)
        th.manual_seed(args.seed)                       # identical relation replicas on every rank
        self.engine = self.make_engine(n_entities=1)    # (the entity rows of a step come from the shards: DistEngine's row cache)
        self.comm = kd.make_comm() if len(set(args.gpu)) == world else kd.HostStagedComm()
        slack = args.dist_slack or float(os.environ.get("KGE_DIST_SLACK", "1.5"))
        self.de = kd.DistEngine(self.engine, self.spec, self.ent, self.ent_state, comm=self.comm, slack=slack,
                                rel_local=self.rel_local, ue_bound=None if self.device_sampler else 2 * B + self.C * N)
        # exchanges may overlap the steps only under the staleness --async_update licenses (tensor_models.py:136-175): then push,
        # owner-side apply and the pull of step s+2 run on a side stream next to step s+1 (DistEngine._steps_overlapped: entity rows
        # exactly one step stale, relation rows current; KGE_DIST_PIPELINE=1: the pull only, the same tables bit for bit);
        # without the flag every step gathers after its predecessor's update has landed, like the reference
        self.pipelined = args.async_update
        if self.pipelined and os.environ.get("KGE_DIST_PIPELINE", "overlap") == "overlap":
            self.pipelined = "overlap"
        # --dist_schedule: sync = every step pulls after its predecessor's update (what runs without --async_update), pull = the pull
        # of step s+1 next to step s, overlap = every exchange on a side stream (the default with --async_update); the two stale
        # schedules need the flag's licence
        if args.dist_schedule:
            if args.dist_schedule != 'sync' and not args.async_update:
                raise KgeError("--dist_schedule %s computes on one-step-stale entity rows: it needs --async_update" % args.dist_schedule)
            self.pipelined = {'sync': False, 'pull': True, 'overlap': 'overlap'}[args.dist_schedule]
        self.sampler = self.make_sampler(rank, part)
        if rank == 0:
            print("multi-GPU mode a2a: entity rows %d per GPU, relations replicated, collectives: %s"
                  % (self.spec.shard, type(self.comm).__name__))
            if self.rel_side_local:
                print("%s on %d GPUs (a2a): entity messages exchanged, relation-side tables (relation rows%s) applied in place on the "
                      "trainer that holds the relation's edges" % (args.model_name, world,
                                                                    ", projection matrices" if models.MODELS[args.model_name].projection else " = matrices"))

    def enqueue(self, n):
        """n sharded steps, eagerly (every rank issues the same collectives in the same order); inside a group of sampled
        batches the pull of step s+1 overlaps step s."""
        smp, done = self.sampler, 0
        log = (lambda m: print('[proc {}] {}'.format(self.rank, m))) if self.rank == 0 else None
        while not self.device_sampler and done < n:          # host-built plans: groups of <= 16 steps, each routed by its own step
            k = min(16, n - done)
            bs = smp.next_batches(k)
            self.de.ensure_capacity(bs, log)                 # (one device read per group; every rank decides alike)
            self.de.run_steps(bs, self.pipelined)
            done += k
        while done < n:
            k = min(smp.n_slots, n - done)
            dbs = smp.sample(k)
            # owner buckets are sized BEFORE the group runs (one small device read per group; every rank takes the same decision);
            # then the routing of the whole group, ONE exchange of its request ids and its steps - with their collectives - replay
            # from one hipGraph (dist.DistEngine.run_group; --graph_steps 0 or a host-staged transport: eager launches)
            self.de.run_group(dbs, log=log, graph=bool(self.args.graph_steps), pipelined=self.pipelined)
            done += k
        lost = self.de.check_overflow()
        if lost:                                 # cannot happen behind ensure_capacity: a bug, not a tuning matter
            raise KgeError('[proc {}] {} entities did not fit their owner bucket although the capacity was checked'.format(self.rank, lost))

    def sync_tables(self):
        """collective point in front of a validation / test / save: every step's update has landed in the shards once the device
        is idle (the pipelined and overlapped schedules included); relation rows that live with their owner are collected into
        every rank's replica."""
        th.cuda.synchronize()
        if self.rel_local:                   # every replica holds the current rows of ITS relations only: collect them everywhere
            kd.relation_rows_from_owners(self.engine.rel, self.engine.rel_state, self.rel_owner, everywhere=True)
            if self.engine.proj is not None:     # TransR: the projection rows live with their relation
                kd.relation_rows_from_owners(self.engine.proj, self.engine.proj_state, self.rel_owner, everywhere=True)

    def entity_shard(self):
        return self.spec.lo, self.ent

    def entity_rows(self, ids):
        return kev.allgather_rows(self.ent, self.spec.lo, self.spec.bounds(), ids, self.comm)

    def relation_table(self):
        return self.engine.rel

    def projection(self):
        return self.engine.proj

    def close(self):
        self.de.close()              # the group graphs first, then the communicator (dist.RcclComm.close)


def _mp_worker(rank, args):
    import torch.distributed as dist
    init_time_start = time.time()
    dataset = kd.load_dataset(rank, args)
    trainer = (A2ATrainer if args.dist_mode == 'a2a' else ShardedTrainer)(args, dataset, rank, len(args.gpu))
    if rank == 0:
        print('Total initialize time {:.3f} seconds'.format(time.time() - init_time_start))
    start = time.time()
    trainer.train()
    failure = None
    trainer.sync_tables()
    # saving and testing are collective: every rank writes its rows of the entity file and ranks against its own shard
    try:
        if rank == 0:
            print('training takes {} seconds'.format(time.time() - start))
        if not args.no_save_emb:
            if rank == 0:
                print('Save model to {}'.format(args.save_path))
            trainer.save(dataset.emap_fname, dataset.rmap_fname)
        if args.test:
            start = time.time()
            trainer.evaluate('test', 'Test')
            if rank == 0:
                print('testing takes {:.3f} seconds'.format(time.time() - start))
    except Exception as e:      # noqa: BLE001 - re-raised after the barrier
        failure = e
    dist.barrier()
    trainer.close()
    if failure is not None:
        raise failure


def check_exclude_positive(args):
    """--exclude_positive runs on the strict single-table step (kge_step_fused_known): refuse what has no such step"""
    if not args.exclude_positive:
        return
    if len(args.gpu) > 1:
        raise KgeError("--exclude_positive is not available on more than one GPU (sharded tables)")
    if args.neg_deg_sample:
        raise KgeError("--exclude_positive is not available with --neg_deg_sample")
    if args.async_update_pipeline or args.async_update_rel:
        raise KgeError("--exclude_positive is not available in the one-step-stale pipeline (--async_update_pipeline / "
                       "--async_update_rel); plain --async_update runs the strict step and is fine")


def weighted_device_sampler(args):
    """which weights the device sampler carries: 'subsampling' (--subsampling_weight), 'file' (--has_edge_importance
    --edge_importance_on_device) or None"""
    if getattr(args, 'subsampling_weight', False):
        return 'subsampling'
    if getattr(args, 'edge_importance_on_device', False):
        return 'file'
    return None


def check_weighted_device_sampler(args):
    """--subsampling_weight and --edge_importance_on_device train on batches of the weighted device sampler, on the strict step of
    one GPU's tables: refuse what has no such batch or step, before anything is loaded"""
    if args.edge_importance_on_device and not args.has_edge_importance:
        raise KgeError("--edge_importance_on_device needs --has_edge_importance (the weight column of train.txt)")
    which = weighted_device_sampler(args)
    if which is None:
        return
    flag = "--subsampling_weight" if which == 'subsampling' else "--edge_importance_on_device"
    if args.subsampling_weight and args.has_edge_importance:
        raise KgeError("--subsampling_weight cannot be combined with --has_edge_importance (two weightings of the same edges)")
    if len(args.gpu) > 1:
        raise KgeError("%s is not available on more than one GPU (--gpu takes one entry)" % flag)
    if args.async_update_pipeline or args.async_update_rel:
        raise KgeError("%s is not available in the one-step-stale pipeline (--async_update_pipeline / --async_update_rel); "
                       "plain --async_update runs the strict step and is fine" % flag)
    B, N = get_compatible_batch_size(args.batch_size, args.neg_sample_size, quiet=True), args.neg_sample_size
    chunk = N if N <= B else B
    if 2 * B + (B // chunk) * N > DeviceSampler.MAX_ELEMENTS:
        raise KgeError("%s: the device sampler builds batches of 2 * batch_size + chunks * neg_sample_size <= %d ids (got %d); "
                       "there is no host sampler for this flag" % (flag, DeviceSampler.MAX_ELEMENTS, 2 * B + (B // chunk) * N))


def check_optimizer(args):
    """--optimizer Adam runs in the strict single-table step's update launch (kge_step_optim); refused here, before anything is
    loaded: what that step does not cover"""
    if getattr(args, 'optimizer', 'Adagrad') != 'Adam':
        return
    if models.own_relation_update(models.MODELS[args.model_name]):
        raise KgeError("--optimizer Adam is not available for %s (RESCAL / TransR update their relation-side tables with kernels of "
                       "their own)" % args.model_name)
    if len(args.gpu) > 1:
        raise KgeError("--optimizer Adam is not available on more than one GPU (--gpu takes one entry)")
    if args.async_update_pipeline or args.async_update_rel:
        raise KgeError("--optimizer Adam is not available in the one-step-stale pipeline (--async_update_pipeline / "
                       "--async_update_rel); plain --async_update runs the strict step and is fine")
    d_e = args.hidden_dim * (2 if args.double_ent else 1)
    d_r = args.hidden_dim * (2 if args.double_rel else 1)
    if d_e % 4 or d_r % 4 or max(d_e, d_r) > _lib.ADAM_MAX_DIM:
        raise KgeError("--optimizer Adam: row widths must be multiples of 4 and at most %d floats (entity %d, relation %d)"
                       % (_lib.ADAM_MAX_DIM, d_e, d_r))
    if not (0.0 <= args.adam_beta1 < 1.0 and 0.0 <= args.adam_beta2 < 1.0):
        raise KgeError("--optimizer Adam: --adam_beta1 and --adam_beta2 must be in [0, 1) (got %g, %g)"
                       % (args.adam_beta1, args.adam_beta2))
    if not args.adam_eps > 0.0:
        raise KgeError("--optimizer Adam: --adam_eps must be positive (got %g)" % args.adam_eps)


def norm_constraints(args):
    """(--ent_norm, --rel_norm) with 'none' as None"""
    return tuple(None if getattr(args, k, 'none') in (None, 'none') else getattr(args, k) for k in ('ent_norm', 'rel_norm'))


def check_norm_constraints(args):
    """--ent_norm / --rel_norm run as a launch behind the update launch of the strict single-table step: refused here, before
    anything is loaded, what has no such launch and the relation rows that have no slices (models.py)"""
    ent_norm, rel_norm = norm_constraints(args)
    if not ent_norm and not rel_norm:
        return
    flag = "--ent_norm" if ent_norm else "--rel_norm"
    if len(args.gpu) > 1:
        raise KgeError("%s is not available on more than one GPU (--gpu takes one entry): sharded tables have no constraint launch"
                       % flag)
    if args.async_update_pipeline:
        raise KgeError("%s is not available with --async_update_pipeline (the one-step-stale pipeline has no launch behind its "
                       "update); plain --async_update runs the strict step and is fine" % flag)
    if args.async_update_rel:
        raise KgeError("%s is not available with --async_update_rel (the one-step-stale pipeline has no launch behind its "
                       "update); plain --async_update runs the strict step and is fine" % flag)
    m = models.MODELS[args.model_name]
    if rel_norm and m.norm_rel == 0:
        raise KgeError("--rel_norm is not available for %s (%s)" % (m.name, m.no_rel_norm))


def check_loss_flags(args):
    """--loss_genre Softmax (cross-entropy of the positive against its row): the softmax is the weighting and the row is the pairing"""
    if args.loss_genre != 'Softmax':
        return
    if args.neg_adversarial_sampling:
        raise KgeError("--loss_genre Softmax cannot be combined with -adv (the softmax is the weighting)")
    if args.pairwise:
        raise KgeError("--loss_genre Softmax cannot be combined with -pw")


def check_model_widths(model_name, hidden_dim, double_ent, double_rel):
    """the -de / -dr / --hidden_dim rules of the model's record (models.py); the texts are the record's"""
    m = models.MODELS[model_name]
    said = dict(de=" -de" if double_ent else " no -de", dr=" -dr" if double_rel else ", no -dr", cdr=", -dr" if double_rel else ", no -dr",
                x2=" x 2 with -de" if double_ent else "", width=hidden_dim * (2 if double_ent else 1), hidden=hidden_dim)

    def flags():
        if m.de == 'tied':
            bad = bool(double_rel) != bool(double_ent)
        else:
            bad = any(want is not None and bool(got) != want for want, got in ((m.de, double_ent), (m.dr, double_rel)))
        if bad:
            raise KgeError(m.flags_text % said)

    def multiple():
        v = said['width'] if m.cli_of == 'width' else hidden_dim
        if m.cli_multiple and (v % m.cli_multiple or (m.cli_of == 'hidden_dim' and v < m.cli_multiple)):
            raise KgeError(m.multiple_text % said)
    for check in ((multiple, flags) if m.multiple_first else (flags, multiple)):
        check()


def check_model_flags(args):
    """a model that trains on the strict step of one GPU's tables: refuse what has no such step, before anything is loaded"""
    m = models.MODELS[args.model_name]
    check_model_widths(args.model_name, args.hidden_dim, args.double_ent, args.double_rel)
    if m.single_gpu_only and len(args.gpu) > 1:
        raise KgeError("%s is not available on more than one GPU (--gpu takes one entry)" % m.name)
    if m.no_stale_pipeline and (args.async_update_pipeline or args.async_update_rel):
        raise KgeError("%s is not available in the one-step-stale pipeline (--async_update_pipeline / --async_update_rel); "
                       "plain --async_update runs the strict step and is fine" % m.name)
    if m.no_relation_ranking and args.eval_relation:
        raise KgeError("%s has no relation ranking (--eval_relation): %s" % (m.name, m.no_relation_ranking))


def main(argv=None, before_train=None):
    """before_train (one GPU): called with the built Trainer in front of its first step - the tests take the initial tables there"""
    args = ArgParser().parse_args(argv)
    check_loss_flags(args)                       # before anything is loaded or created
    check_exclude_positive(args)                 # before anything is loaded or created
    check_model_flags(args)                      # before anything is loaded or created
    check_weighted_device_sampler(args)          # before anything is loaded or created
    check_optimizer(args)                        # before anything is loaded or created
    check_norm_constraints(args)                 # before anything is loaded or created
    ckpt.check_flags(args)                       # before anything is loaded or created
    if args.neg_deg_sample_eval:                # before anything is loaded or created
        if len(args.gpu) > 1:
            raise KgeError("--neg_deg_sample_eval is not available on sharded tables")
        assert args.no_eval_filter, "if negative sampling based on degree, we can't filter positive edges."   # train.py:878
    if args.eval_relation and len(args.gpu) > 1:
        raise KgeError("--eval_relation is not available on sharded tables")
    args_parsed = dict(vars(args))               # the command line as given: what a later --resume reports changes against
    # --resume reads its checkpoint's description, checks the flags against it and --max_step against its step here: before the
    # dataset is loaded and before this run's own directory is made (None: --resume latest found nothing, a fresh run)
    resume = ckpt.open_resume(args) if args.resume else None
    prepare_save_path(args)
    init_time_start = time.time()
    multi = len(args.gpu) > 1                    # one trainer process per listed GPU (the same GPU may be listed twice)
    if multi and min(args.gpu) < 0:
        raise KgeError("dglke_amd trains on the GPU only: pass --gpu <ids> (there is no CPU fallback)")
    if args.log_interval <= 0:
        raise KgeError("--log_interval must be positive")
    if multi and args.num_proc > len(args.gpu):      # reference: several trainer processes per GPU (train.py:94-100, 115-119)
        if args.num_proc % len(args.gpu):
            raise KgeError("--num_proc should be a multiple of the number of GPUs")
        args.gpu = [g for g in args.gpu for _ in range(args.num_proc // len(args.gpu))]
    if not multi:
        dataset = kd.load_dataset(0, args)
        if args.test and dataset.test is None:
            raise KgeError("--test: the dataset has no test split")
        if args.neg_sample_size_eval < 0:
            args.neg_sample_size_eval = dataset.n_entities
    args.batch_size = get_compatible_batch_size(args.batch_size, args.neg_sample_size)
    if not multi:
        args.batch_size_eval = get_compatible_batch_size(args.batch_size_eval, args.neg_sample_size_eval)
    args.eval_filter = not args.no_eval_filter
    args.soft_rel_part = args.strict_rel_part = False     # one replicated HBM relation table
    if multi:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        kd.spawn_ranks(_mp_worker, args)
        return None
    trainer = Trainer(args, dataset)
    trainer.args_parsed = args_parsed
    if resume is not None:
        ckpt.restore_trainer(trainer, resume)     # (in place, and before the hook: it sees the restored state)
    if before_train is not None:
        before_train(trainer)
    print('Total initialize time {:.3f} seconds'.format(time.time() - init_time_start))
    start = time.time()
    if resume is not None:
        trainer.train(start_step=resume.step, start_since_log=resume.since_log)
    else:
        trainer.train()
    print('training takes {} seconds'.format(time.time() - start))
    if not args.no_save_emb:
        save_model(args, trainer.model, emap_file=dataset.emap_fname, rmap_file=dataset.rmap_fname)
    if args.test:
        start = time.time()
        trainer.evaluate('test', 'Test')
        print('testing takes {:.3f} seconds'.format(time.time() - start))
    return trainer


if __name__ == '__main__':
    try:
        main()
    except KgeError as e:
        sys.exit("dglke_train: %s" % e)
