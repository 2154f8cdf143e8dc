"""What a 1-vs-all step costs (the method of tools/transd_timing.py, cut down).  Shape: batch 1000, hidden 400, 14 951 entities,
1 345 relations, uniform random triples; batches are host-built plans uploaded before the timed region; steps are launched eagerly
(the mode has no captured form), K steps between two events, one untimed group in front.
Each measurement is a child process of its own under `timeout`; the driver runs the variants in alternation, REPS rounds, and the
first child that fails ends the run.  Figure of a variant: the median over all its measurements; spread: the range of its
per-process medians.
  ova_distmult / ova_complex   StepEngine(one_vs_all=True).step: edge_fwd, ova_fwd, ova_lse, ova_bwd_a, edge_bwd, ova_bwd_e, update
  softmax200                   DistMult, --loss_genre Softmax at 200 sampled negatives per chunk of 200, the same eager loop
FLOP figure of a 1-vs-all step: 2 B n_ent d per product, five products (forward 1, GA 2, owner 2), as the issue counts them; the owner
kernel runs half a product more than it uses - that work is not counted.
NOT here: the default step against the parent commit's library, the per-kernel split of a rocprofv3 run, validation MRR.
usage: python tools/one_vs_all_timing.py [--quick] [out.txt]   (default profiles/one_vs_all_timing.txt)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))

N_ENT, N_REL, HIDDEN, GAMMA, LR, B, N = 14951, 1345, 400, 19.9, 0.1, 1000, 200
K, MEAS, REPS, CHILD_LIMIT_S = 20, 5, 3, 150
VARIANTS = {"ova_distmult": ("DistMult", True), "ova_complex": ("ComplEx", True), "softmax200": ("DistMult", False)}


def child(variant, quick):
    import torch as th
    from dglke_amd import plan
    from dglke_amd.engine import StepEngine
    model, ova = VARIANTS[variant]
    dev = th.device("cuda", 0)
    th.manual_seed(0)
    rng = np.random.RandomState(1)
    eng = StepEngine(model, N_ENT, N_REL, HIDDEN, GAMMA, LR, dev, loss_genre='Softmax', one_vs_all=ova)
    n = 0 if ova else N
    plans = [plan.build_plan(rng.randint(0, N_ENT, B), rng.randint(0, N_ENT, B), rng.randint(0, N_REL, B),
                             rng.randint(0, N_ENT, (B // (n or B)) * n), n or B, n, k % 2 == 0) for k in range(K)]
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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:
        return child(args[0], quick)
    out = args[0] if args else os.path.join(ROOT, "profiles", "one_vs_all_timing.txt")
    res = {v: [] for v in VARIANTS}
    for rep in range(1 if quick else REPS):
        for v in VARIANTS:
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", v] +
                               (["--quick"] if quick else []), stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                sys.exit("child %s failed (%d): nothing more is run" % (v, r.returncode))
            d = json.loads(r.stdout.strip().splitlines()[-1])
            assert d["finite"], v
            res[v].append(d["us"])
            print(v, rep, ["%.1f" % x for x in d["us"]], flush=True)
    gflop = 5 * 2.0 * B * N_ENT * HIDDEN * 1e-9
    with open(out, "w") as f:
        f.write("one MI355X; batch %d, hidden %d, %d entities; eager launches, %d steps per measurement, %d measurements per process, "
                "%d processes per variant in alternation\n" % (B, HIDDEN, N_ENT, K, 1 if quick else MEAS, len(res["softmax200"])))
        for v, runs in res.items():
            med, per = float(np.median(np.concatenate(runs))), [float(np.median(r)) for r in runs]
            line = "%-13s median %9.1f us/step   per-process medians %9.1f .. %9.1f" % (v, med, min(per), max(per))
            if VARIANTS[v][1]:
                line += "   %.1f GFLOP counted -> %.1f TFLOP/s over the whole step" % (gflop, gflop / med * 1e3)
            f.write(line + "\n")
        f.write("not measured: the default step against the parent commit's library, the three product kernels one by one "
                "(rocprofv3), validation MRR\n")
    print(open(out).read())


if __name__ == "__main__":
    main()
