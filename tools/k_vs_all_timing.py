"""What a K-vs-all step costs next to the 1-vs-all softmax step, measured in the same run (the method of tools/one_vs_all_timing.py).
Shape: batch 1000, hidden 400, the planted FB15k-shaped graph of tools/make_planted_fb15k.py (14 951 entities, 1 345 relations): the
batches are rows of its training split, the label lists its training split's index (known.KnownIndex).  Batches are host-built
plans uploaded before the timed region; steps are launched eagerly (neither mode has a captured form), K steps between two events,
one untimed group in front.  Each measurement is a child process of its own under `timeout`; the driver runs the variants in
alternation, REPS rounds, and the first child that fails ends the run.  Figure of a variant: the median over all its measurements;
spread: the range of its per-process medians.
  kva_distmult / kva_complex   StepEngine(k_vs_all=True, label_smoothing=0.1).step: edge_fwd, kva_prep, kva_bwd_a, kva_loss, edge_bwd,
                               kva_bwd_e, update
  kva_empty                    DistMult with an EMPTY index (1-vs-all BCE): what the label lists cost is the difference
  kva_dense                    DistMult, the planted index plus DENSE random extra answers for every batch row's query: the planted
                               graph is nearly one-to-one (its lists hold one or two entities), this one shows lists of ~50
  ova_distmult / ova_complex   the yardstick: StepEngine(one_vs_all=True).step on the same batches
  default / parent             TransE_l2 at cfg-T (Logsigmoid -adv, 200 negatives), a replayed graph of G strict steps over the device
                               sampler, by this build and (--baseline_lib PATH) by the parent commit's library: no existing kernel's
                               source changed, the two must agree within the spread
FLOP figure: 2 B n_ent d per product; the K-vs-all step counts four (GA 2, owner 2), the softmax step five (forward 1, GA 2, owner 2).
--trace: one more child each of kva_empty, kva_distmult and kva_dense under `rocprofv3 --kernel-trace --stats`, in runs of their own behind the
timed ones; the mean duration of every kernel of the step is written under the timings.
usage: python tools/k_vs_all_timing.py [--baseline_lib PATH] [--trace] [--quick] [out.txt]   (default profiles/k_vs_all_timing.txt)"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, ROOT)

N_ENT, N_REL, HIDDEN, GAMMA, LR, B, N = 14951, 1345, 400, 19.9, 0.1, 1000, 200
K, MEAS, REPS, CHILD_LIMIT_S = 20, 5, 3, 150
G, REPLAYS = 100, 30
# variant -> (model, mode)
DENSE = 50
VARIANTS = {"kva_distmult": ("DistMult", "kva"), "kva_complex": ("ComplEx", "kva"), "kva_empty": ("DistMult", "kva_empty"),
            "kva_dense": ("DistMult", "kva_dense"),
            "ova_distmult": ("DistMult", "ova"), "ova_complex": ("ComplEx", "ova"),
            "default": ("TransE_l2", "cfgT"), "parent": ("TransE_l2", "cfgT")}
PRODUCTS = {"kva": 4, "kva_empty": 4, "kva_dense": 4, "ova": 5}


def load_train(data):
    t = np.loadtxt(os.path.join(data, "train.txt"), dtype=np.int64)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()


def child_cfgt(trip, quick):
    import torch as th
    from dglke_amd import _lib
    from dglke_amd.dataloader import DeviceSampler
    from dglke_amd.engine import StepEngine
    dev = th.device("cuda", 0)
    eng = StepEngine("TransE_l2", N_ENT, N_REL, HIDDEN, GAMMA, 0.25, dev, False, False, True, 1.0, 1e-9, 3)
    smp = DeviceSampler(trip[0], trip[1], trip[2], N_ENT, B, N, dev, n_slots=G, neg_chunk_size=N, seed=5)
    for b in smp.sample(G):                   # eager warm-up: allocates the workspace
        eng.step(b)
    th.cuda.synchronize()
    g = th.cuda.CUDAGraph()
    with _lib.graph_capture(g):
        for b in smp.sample(G):
            eng.step(b)
    replays, ts = (2 if quick else REPLAYS), []
    for _ in range(MEAS):
        a, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        g.replay()                            # the first kernels after a pause of the queue run late: one untimed replay in front
        a.record()
        for _ in range(replays):
            g.replay()
        e.record()
        th.cuda.synchronize()
        ts.append(a.elapsed_time(e) * 1e3 / (replays * G))
    return ts, eng


def child(variant, data, quick):
    import torch as th
    from dglke_amd import plan
    from dglke_amd.engine import StepEngine
    from dglke_amd.known import KnownIndex
    model, mode = VARIANTS[variant]
    trip = load_train(data)
    dev = th.device("cuda", 0)
    th.manual_seed(0)
    if mode == "cfgT":
        ts, eng = child_cfgt(trip, quick)
    else:
        rng = np.random.RandomState(1)
        rows = [rng.randint(0, len(trip[0]), B) for _ in range(K)]
        if mode == "ova":
            eng = StepEngine(model, N_ENT, N_REL, HIDDEN, GAMMA, LR, dev, loss_genre='Softmax', one_vs_all=True)
        else:
            eng = StepEngine(model, N_ENT, N_REL, HIDDEN, GAMMA, LR, dev, loss_genre='BCE', k_vs_all=True, label_smoothing=0.1)
            idx = trip if mode != "kva_empty" else tuple(np.zeros(0, np.int64) for _ in range(3))
            if mode == "kva_dense":                  # (step k corrupts heads when k is even: the extra answers go to that side)
                hh, rr, tt = ([np.repeat(trip[c][r], DENSE) for r in rows] for c in range(3))
                for k in range(K):
                    (hh if k % 2 == 0 else tt)[k] = rng.randint(0, N_ENT, B * DENSE)
                idx = tuple(np.concatenate([trip[c]] + x) for c, x in enumerate((hh, rr, tt)))
            eng.attach_known(KnownIndex(idx, N_ENT, N_REL, dev))
        plans = [plan.build_plan(trip[0][r], trip[2][r], trip[1][r], np.zeros(0, np.int64), B, 0, k % 2 == 0) for k, r in enumerate(rows)]
        batches = plan.upload(plans, dev)
        ts = []
        for m in range((1 if quick else MEAS) + 1):
            a, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            a.record()
            for b in batches:
                eng.step(b)
            e.record()
            th.cuda.synchronize()
            if m:                                     # (the first group allocates the workspace and ramps the clocks)
                ts.append(a.elapsed_time(e) * 1e3 / K)
    print(json.dumps(dict(us=ts, finite=bool(np.isfinite(eng.read_loss_sums()[2])))))


def run_child(variant, data, quick, lib=None, trace_dir=None):
    env = dict(os.environ)
    env.pop("KGE_LIB", None)
    if lib:
        env["KGE_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, data] + (["--quick"] if quick else [])
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + cmd
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S)] + cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("child %s failed (%d): nothing more is run" % (variant, r.returncode))
    d = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"us"')][-1]
    assert d["finite"], variant
    return d["us"]


def kernel_means(trace_dir):
    """kernel name -> (calls, mean us) from the kernel_stats.csv of a rocprofv3 --stats run"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            if name.startswith(("kva_", "edge_", "update_", "finalize_")):      # the step's own launches
                out[name] = (int(row["Calls"]), float(row["AverageNs"]) * 1e-3)
    return out


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
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "k_vs_all_timing.txt")
    import __graft_entry__
    __graft_entry__.build()
    order = [v for v in VARIANTS if v != "parent" or base]
    res, traces, trace_note = {v: [] for v in order}, {}, "no --trace"
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "fb15k_planted")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_planted_fb15k.py"), data], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode:
            raise SystemExit(r.stdout)
        for rep in range(1 if quick else REPS):
            for v in order:
                res[v].append(run_child(v, data, quick, base if v == "parent" else None))
                print(v, rep, ["%.1f" % x for x in res[v][-1]], flush=True)
        if "--trace" in flags:                        # behind the timed runs, each a run of its own
            try:
                for v in ("kva_empty", "kva_distmult", "kva_dense"):
                    td = os.path.join(tmp, "trace_" + v)
                    run_child(v, data, True, trace_dir=td)
                    traces[v] = kernel_means(td)
                    if not traces[v]:
                        raise KeyError("no kernel_stats.csv under the trace directory")
            except (SystemExit, KeyError, ValueError, OSError) as e:      # the timings stand without the trace
                traces, trace_note = {}, "failed: %r" % (e,)
    med = lambda v: float(np.median(np.concatenate(res[v])))
    per = lambda v: [float(np.median(r)) for r in res[v]]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("one MI355X; batch %d, hidden %d, planted FB15k-shaped graph (%d entities); N == 0 steps: eager launches, %d steps per "
                "measurement, %d measurements per process; %d processes per variant in alternation\n"
                % (B, HIDDEN, N_ENT, K, 1 if quick else MEAS, len(res["ova_distmult"])))
        for v in order:
            mode = VARIANTS[v][1]
            line = "%-13s median %9.1f us/step   per-process medians %9.1f .. %9.1f" % (v, med(v), min(per(v)), max(per(v)))
            if mode in PRODUCTS:
                gflop = PRODUCTS[mode] * 2.0 * B * N_ENT * HIDDEN * 1e-9
                line += "   %d products, %.1f GFLOP counted -> %.1f TFLOP/s over the whole step" % (PRODUCTS[mode], gflop, gflop / med(v) * 1e3)
            else:
                line += "   cfg-T strict step, per step of a replayed group of %d" % G
            f.write(line + "\n")
        for m in ("distmult", "complex"):
            f.write("kva_%s - ova_%s: %+.1f us (%.3f x the yardstick of the same run)\n"
                    % (m, m, med("kva_" + m) - med("ova_" + m), med("kva_" + m) / med("ova_" + m)))
        f.write("kva_distmult - kva_empty (what the planted graph's label lists cost in the whole step): %+.1f us\n"
                % (med("kva_distmult") - med("kva_empty")))
        f.write("kva_dense - kva_empty (lists of ~%d answers per row): %+.1f us\n" % (DENSE + 1, med("kva_dense") - med("kva_empty")))
        if base:
            s = max(np.ptp(per("default")), np.ptp(per("parent")))
            d = med("default") - med("parent")
            f.write("default - parent: %+.2f us; the larger process-to-process spread of one library is %.2f us: %s\n"
                    % (d, s, "within it" if abs(d) <= s else "OUTSIDE it"))
        else:
            f.write("default against the parent commit's library: not measured (no --baseline_lib)\n")
        if traces:
            f.write("kernel trace (rocprofv3 --kernel-trace --stats, runs of their own): mean us per call [calls], empty | planted | dense index\n")
            for name in sorted(traces["kva_distmult"]):
                cols = [traces[v].get(name, (0, float("nan"))) for v in ("kva_empty", "kva_distmult", "kva_dense")]
                f.write("  %-32s %s\n" % (name[:32], " | ".join("%8.1f [%d]" % (c[1], c[0]) for c in cols)))
        else:
            f.write("kernel trace: not measured (%s)\n" % trace_note)
        f.write("not measured: validation MRR\n")
    print(open(out).read())


if __name__ == "__main__":
    main()
