"""What one checkpoint of dglke_train costs (--checkpoint_interval) and what a restore costs (--resume), in seconds and bytes, against
the yardstick the tool already had: `save_model`, the final save, of the same tables in the same process.

Shapes: FB15k's tables (14 951 entities x 1 345 relations, hidden 400, TransE_l2) under Adagrad and under Adam; with --big also
2.5 M entities x 400 under Adam (4 GB of rows, 8 GB of moments: needs that much disk under --dir).  The triples are uniform random
ones - nothing here trains; the trainer is built the way dglke_train builds it, takes a few steps so that every table has been
touched, and is then written and restored REPS times.
  checkpoint   checkpoint.save_trainer: tables, state (and moments) in row blocks through one 64 MiB host buffer, sampler state,
               loss sums, config.json, checkpoint.json, the rename into place;
  final save   train.save_model: np.save of table.cpu().numpy() per table + config.json (no state, no moments);
  restore      checkpoint.restore_trainer into the standing trainer: memory-mapped files -> the live tensors in row blocks.
The file system's cache is not dropped between the write and the read: the restore is the page cache's.
usage: python tools/checkpoint_timing.py [--big] [--dir DIR] [out.txt]     (default profiles/checkpoint_timing.txt)"""
import argparse
import contextlib
import io
import os
import shutil
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, ROOT)

REPS = 3
SHAPES = [("FB15k shape, Adagrad", 14951, 1345, 483142, "Adagrad"),
          ("FB15k shape, Adam", 14951, 1345, 483142, "Adam")]
BIG = ("2.5 M x 400, Adam", 2500000, 1345, 2000000, "Adam")


def dataset(n_ent, n_rel, n_train):
    r = np.random.RandomState(0)
    train = (r.randint(0, n_ent, n_train), r.randint(0, n_rel, n_train), r.randint(0, n_ent, n_train))
    return types.SimpleNamespace(n_entities=n_ent, n_relations=n_rel, train=train, valid=None, test=None, emap_fname=None,
                                 rmap_fname=None)


def dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def measure(name, n_ent, n_rel, n_train, optimizer, root, say):
    import torch as th
    from dglke_amd import checkpoint as ckpt
    from dglke_amd import train as T
    run = os.path.join(root, "run")
    os.makedirs(run)
    args = T.ArgParser().parse_args(["--model_name", "TransE_l2", "--dataset", "timing", "--gpu", "0", "--batch_size", "1000",
                                     "--neg_sample_size", "200", "--hidden_dim", "400", "-g", "19.9", "-adv", "--optimizer", optimizer,
                                     "--lr", "0.25" if optimizer == "Adagrad" else "0.001", "--save_path", run, "--graph_steps", "0"])
    tr = T.Trainer(args, dataset(n_ent, n_rel, n_train))
    tr.enqueue(20)
    th.cuda.synchronize()
    quiet = io.StringIO()
    t_ck, t_save, t_rest = [], [], []
    for _ in range(REPS):
        nbytes, secs = ckpt.save_trainer(tr, 20, 20)
        t_ck.append(secs)
        final = os.path.join(root, "final")
        t0 = time.time()
        with contextlib.redirect_stdout(quiet):
            T.save_model(types.SimpleNamespace(**dict(vars(args), save_path=final)), tr.model)
        t_save.append(time.time() - t0)
        final_bytes = dir_bytes(final)
        shutil.rmtree(final)
        res = ckpt.Resume(*ckpt.locate(run))
        t0 = time.time()
        ckpt.restore_trainer(tr, res)
        t_rest.append(time.time() - t0)
    fmt = lambda x: "%8.3f s (min %8.3f max %8.3f)" % (float(np.median(x)), min(x), max(x))
    say("%s: %d x 400 entity rows, %d x 400 relation rows" % (name, n_ent, n_rel))
    say("  checkpoint  %s  %13d bytes  %7.2f GB/s" % (fmt(t_ck), nbytes, nbytes / np.median(t_ck) / 1e9))
    say("  final save  %s  %13d bytes  %7.2f GB/s" % (fmt(t_save), final_bytes, final_bytes / np.median(t_save) / 1e9))
    say("  restore     %s  %13d bytes  %7.2f GB/s" % (fmt(t_rest), nbytes, nbytes / np.median(t_rest) / 1e9))
    del tr
    shutil.rmtree(run)
    th.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--big", action="store_true")
    p.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    p.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "checkpoint_timing.txt"))
    a = p.parse_args()
    import torch as th
    import __graft_entry__
    __graft_entry__.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/checkpoint_timing.py%s: %s; medians of %d repetitions; host staging %d MiB"
        % (" --big" if a.big else "", th.cuda.get_device_name(0), REPS, 64))
    with tempfile.TemporaryDirectory(dir=a.dir) as root:
        for shape in SHAPES + ([BIG] if a.big else []):
            measure(*shape, root=root, say=say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
