"""What per-edge weights from the device sampler cost per step at the cfg-T shape (TransE_l2, d 400, batch 1000, 200 negatives in
chunks of 200), on the planted FB15k-shaped graph of bench.py's time_to_mrr leg (tools/make_planted_fb15k.py), whether the default
step moved, and what the host route it replaces costs (tools/softmax_loss_timing.py's method).

Every graph variant is a hipGraph of [one sampler launch + G strict steps] over a device sampler.  Each measurement is a child
process of its own under `timeout`: it builds the engine, captures the graph, times REPLAYS replays MEAS times and prints one JSON
line.  The driver runs the variants in alternation, REPS rounds; the first child that fails ends the run.  The figure of a variant is
the median over all its measurements; its spread the range of its per-process medians.
  default    Logsigmoid -adv, the benchmark's configuration, unweighted device sampler
  parent     (--baseline_lib PATH: libkge_hip.so built from the parent commit) the same, run by that library - the two must agree
             within the spread: no kernel on that path changes
  weighted   the same step on batches of the WEIGHTED device sampler (the split's subsampling weights): kge_batch.edge_w set,
             edge_w_mean 0 - every wavefront that needs the batch's mean weight sums the B weights itself
  host       the route --has_edge_importance takes without --edge_importance_on_device: UniformChunkedSampler batches (plans built
             on the host, uploaded) and eager steps, sampling included, wall clock per step
Once: dataloader.subsampling_weights (two sorts, two launches, the float64 mean) at FB15k's 483 142 triples.
--mrr: for information only, dglke_train with bench.py's planted-graph recipe cut at 2 000 steps, validation MRR with and without
--subsampling_weight.
usage: python tools/subsampling_timing.py [--baseline_lib PATH] [--mrr] [--quick] [out.txt]   (default profiles/subsampling_timing.txt)"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, ROOT)

N_ENT, N_REL = 14951, 1345
HIDDEN, GAMMA, LR, B, N = 400, 19.9, 0.25, 1000, 200
G, REPS, REPLAYS, MEAS = 100, 9, 30, 3
HOST_STEPS = 200
FB15K_TRIPLES = 483142
CHILD_LIMIT_S = 150
VARIANTS = ("default", "parent", "weighted", "host")
NEW_ENTRIES = ("kge_sampler_slot_bytes_weighted", "kge_sample_batches_weighted", "kge_batch_from_slot_weighted", "kge_subsampling_weights")


def load_train(data):
    t = np.loadtxt(os.path.join(data, "train.txt"), dtype=np.int64)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()


def child(variant, data, quick):
    """one variant, timed in this process; prints one JSON line"""
    import torch as th
    from dglke_amd import _lib
    if variant == "parent":                   # the parent commit's library has none of the new entries: not bound, not called
        for name in NEW_ENTRIES:
            _lib._SIGNATURES.pop(name, None)
    from dglke_amd.dataloader import DeviceSampler, UniformChunkedSampler, subsampling_weights
    from dglke_amd.engine import StepEngine
    trip = load_train(data)
    dev = th.device("cuda", 0)
    th.manual_seed(0)
    eng = StepEngine("TransE_l2", N_ENT, N_REL, HIDDEN, GAMMA, LR, dev, False, False, True, 1.0, 1e-9, 3)
    if variant == "weights":
        n = FB15K_TRIPLES
        sel = np.arange(n) % len(trip[0])
        h, r, t = (th.as_tensor(x[sel]).to(dev) for x in trip)
        subsampling_weights(h, r, t, N_ENT, N_REL, dev)              # warm-up: torch.sort's buffers, the kernel's code object
        th.cuda.synchronize()
        ts = []
        for _ in range(MEAS):
            t0 = time.time()
            w = subsampling_weights(h, r, t, N_ENT, N_REL, dev)
            th.cuda.synchronize()
            ts.append((time.time() - t0) * 1e6)
        k = []                                                       # the kernel alone, on sorted keys made outside the timing
        khr, ktr = th.sort(h * N_REL + r)[0], th.sort(t * N_REL + r)[0]
        out = th.empty(n, device=dev)
        for _ in range(MEAS):
            a, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(_lib.lib().kge_subsampling_weights(_lib.ptr(khr), n, _lib.ptr(ktr), n, _lib.ptr(h), _lib.ptr(r), _lib.ptr(t), n,
                                                          N_ENT, N_REL, 1.0, _lib.ptr(out), _lib.stream_ptr()))
            e.record()
            th.cuda.synchronize()
            k.append(a.elapsed_time(e) * 1e3)
        print(json.dumps(dict(us=ts, kernel_us=k, finite=bool(th.isfinite(w).all()), mean=float(w.double().mean()))))
        return
    if variant == "host":
        w = subsampling_weights(trip[0], trip[1], trip[2], N_ENT, N_REL, dev).cpu().numpy()
        smp = UniformChunkedSampler(trip[0], trip[1], trip[2], N_ENT, B, N, dev, neg_chunk_size=N, seed=5, edge_importance=w)
        for b in smp.next_batches(20):        # warm-up: allocates the workspace
            eng.step(b)
        th.cuda.synchronize()
        steps = 20 if quick else HOST_STEPS
        ts = []
        for _ in range(MEAS):
            t0 = time.time()
            for b in smp.next_batches(steps):
                eng.step(b)
            th.cuda.synchronize()
            ts.append((time.time() - t0) * 1e6 / steps)
        print(json.dumps(dict(us=ts, finite=bool(np.isfinite(eng.read_loss_sums()[2])))))
        return
    w = subsampling_weights(trip[0], trip[1], trip[2], N_ENT, N_REL, dev) if variant == "weighted" else None
    kw = dict(edge_importance=w) if variant == "weighted" else {}
    smp = DeviceSampler(trip[0], trip[1], trip[2], N_ENT, B, N, dev, n_slots=G, neg_chunk_size=N, seed=5, **kw)
    for b in smp.sample(G):                   # eager warm-up: allocates the workspace
        eng.step(b)
    th.cuda.synchronize()
    g = th.cuda.CUDAGraph()
    with _lib.graph_capture(g):
        for b in smp.sample(G):
            eng.step(b)
    replays = 2 if quick else REPLAYS
    ts = []
    for _ in range(MEAS):
        a, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        g.replay()                            # the first kernels after a pause of the queue run late: one untimed replay in front
        a.record()
        for _ in range(replays):
            g.replay()
        e.record()
        th.cuda.synchronize()
        ts.append(a.elapsed_time(e) * 1e3 / (replays * G))
    loss = eng.read_loss_sums()
    print(json.dumps(dict(us=ts, finite=bool(np.isfinite(loss[2])))))
    del g, smp, eng


def run_child(variant, data, quick, lib):
    env = dict(os.environ)
    env.pop("KGE_LIB", None)
    if lib:
        env["KGE_LIB"] = lib
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", variant, data]
    p = subprocess.run(cmd + (["--quick"] if quick else []), env=env, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("%s: the timed child ended with status %d - nothing further is started" % (variant, p.returncode))
    r = json.loads(p.stdout.strip().split("\n")[-1])
    if not r["finite"]:
        raise SystemExit("%s: the result is not finite" % variant)
    return r


def mrr_after(data, tmp, extra, steps=2000):
    cli = os.path.join(ROOT, "dgl-ke_amd", "dglke_train")
    cmd = ["timeout", "-k", "10", "240", sys.executable, cli, "--format", "udd_hrt", "--dataset", "fb15k_planted", "--data_path", data,
           "--data_files", "entities.dict", "relations.dict", "train.txt", "valid.txt", "test.txt", "--save_path",
           os.path.join(tmp, "ckpts"), "--model_name", "TransE_l2", "--no_save_emb", "--gpu", "0", "--batch_size", "1000",
           "--neg_sample_size", "200", "--hidden_dim", "400", "--gamma", "19.9", "--lr", "0.25", "--regularization_coef", "1e-9",
           "--max_step", str(steps), "--log_interval", "1000", "--eval_interval", str(steps), "--valid", "--graph_steps", "100",
           "--batch_size_eval", "16", "-adv"] + extra
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode:
        raise SystemExit("dglke_train %s ended with status %d:\n%s" % (" ".join(extra), p.returncode, p.stdout[-1500:]))
    v = re.findall(r"\]Valid average MRR: ([0-9.eE+-]+)", p.stdout)
    return float(v[-1]) if v else float("nan")


def main():
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in flags
    if "--child" in flags:
        return child(argv[0], argv[1], quick)
    base = None
    if "--baseline_lib" in flags:
        base, argv = os.path.abspath(argv[0]), argv[1:]
        if not os.path.isfile(base):
            raise SystemExit("--baseline_lib %s: no such file" % base)
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "subsampling_timing.txt")
    import __graft_entry__
    __graft_entry__.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    order = [v for v in VARIANTS if v != "parent" or base]
    per = {v: [] for v in order}
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "fb15k_planted")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_planted_fb15k.py"), data], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode:
            raise SystemExit(r.stdout)
        for _ in range(2 if quick else REPS):
            for v in order:
                per[v].append(run_child(v, data, quick, base if v == "parent" else None)["us"])
        wt = run_child("weights", data, quick, None)
        mrr = None
        if "--mrr" in flags:
            mrr = (mrr_after(data, tmp, ["--subsampling_weight"]), mrr_after(data, tmp, []))
    med = lambda v: float(np.median(np.concatenate(per[v])))
    spread = lambda v: float(np.ptp([np.median(x) for x in per[v]]))
    fmt = lambda v: "%8.2f us (processes' medians %8.2f .. %8.2f, spread %.2f)" % (
        med(v), min(np.median(x) for x in per[v]), max(np.median(x) for x in per[v]), spread(v))
    say("# cfg-T: TransE_l2 d %d, batch %d, %d negatives in chunks of %d; planted FB15k-shaped graph; per step of a replayed group of %d"
        % (HIDDEN, B, N, N, G))
    say("default step     %s   Logsigmoid -adv, unweighted device sampler, this build" % fmt("default"))
    if base:
        s = max(spread("default"), spread("parent"))
        d = med("default") - med("parent")
        say("default, parent  %s   the parent commit's library (KGE_LIB) under this package" % fmt("parent"))
        say("this - parent    %+.2f us; the larger spread of one library is %.2f us: %s" % (
            d, s, "within it" if abs(d) <= s else "OUTSIDE it"))
    else:
        say("default, parent  not measured (no --baseline_lib)")
    s = max(spread("default"), spread("weighted"))
    d = med("weighted") - med("default")
    say("weighted step    %s   weighted device sampler, edge_w_mean summed by the kernels" % fmt("weighted"))
    say("weighted - default  %+.2f us; the larger spread of the two is %.2f us: %s" % (d, s, "within it" if abs(d) <= s else "OUTSIDE it"))
    say("host route       %s   UniformChunkedSampler + eager steps, sampling included (wall clock, %d steps per measurement)"
        % (fmt("host"), 20 if quick else HOST_STEPS))
    say("host / weighted device step  %.1f x" % (med("host") / med("weighted")))
    say("subsampling_weights at %d triples (two sorts, two launches, the float64 mean; wall clock, synchronised): %s us; "
        "kge_subsampling_weights alone: %s us; mean of the weights %.9f"
        % (FB15K_TRIPLES, ", ".join("%.0f" % x for x in wt["us"]), ", ".join("%.1f" % x for x in wt["kernel_us"]), wt["mean"]))
    if mrr is not None:
        say("validation MRR after 2 000 steps of the planted-graph recipe (information only): --subsampling_weight %.4f, without %.4f" % mrr)
    else:
        say("validation MRR after 2 000 steps: not measured (no --mrr)")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# tools/subsampling_timing.py%s: %d alternating rounds, one process per measurement, %d x %d replays each\n" % (
            " --quick" if quick else "", 2 if quick else REPS, MEAS, 2 if quick else REPLAYS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
