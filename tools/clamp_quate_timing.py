"""What the SimplE and QuatE all-entity steps cost next to DistMult's (the method of tools/one_vs_all_timing.py).  Shape: batch 1000,
hidden 400, 14 951 entities, 1 345 relations, uniform random triples (K-vs-all: the same triples are the index); host-built plans
uploaded before the timed region; eager launches, K steps between two events, one untimed group in front.
Each measurement is a child process of its own under `timeout`; the driver runs the variants in alternation, REPS rounds, and the
first child that fails ends the run.  Figure of a variant: the median over all its measurements; spread: the range of its
per-process medians.
  ova_* / kva_*        StepEngine(one_vs_all / k_vs_all).step of DistMult (the yardstick), SimplE (clamped kernels) and QuatE
  --parent_lib PATH    adds ova_distmult and the default sampled step (TransE_l2, 200 negatives, Logsigmoid) on the library at PATH,
                       in the same alternation, and the latter on this build: differences against the process-to-process spread
usage: python tools/clamp_quate_timing.py [--quick] [--parent_lib PATH] [out.txt]   (default profiles/clamp_quate_timing.txt)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))

N_ENT, N_REL, HIDDEN, GAMMA, LR, B, N = 14951, 1345, 400, 19.9, 0.1, 1000, 200
K, MEAS, REPS, CHILD_LIMIT_S = 20, 5, 3, 150
VARIANTS = {"%s_%s" % (crit, m.lower()): (m, crit) for crit in ("ova", "kva") for m in ("DistMult", "SimplE", "QuatE")}
VARIANTS["sampled_transe_l2"] = ("TransE_l2", None)
PARENT = ("ova_distmult", "sampled_transe_l2")                    # measured on the parent's library too


def child(variant, quick):
    import torch as th
    from dglke_amd import plan
    from dglke_amd.engine import StepEngine
    from dglke_amd.known import KnownIndex
    model, crit = VARIANTS[variant]
    dev = th.device("cuda", 0)
    th.manual_seed(0)
    rng = np.random.RandomState(1)
    kw = {None: {}, "ova": dict(loss_genre='Softmax', one_vs_all=True), "kva": dict(loss_genre='BCE', k_vs_all=True, label_smoothing=0.1)}[crit]
    eng = StepEngine(model, N_ENT, N_REL, HIDDEN, GAMMA, LR, dev, **kw)
    n = N if crit is None else 0
    trip = [(rng.randint(0, N_ENT, B), rng.randint(0, N_REL, B), rng.randint(0, N_ENT, B)) for _ in range(K)]
    if crit == "kva":
        eng.attach_known(KnownIndex(tuple(np.concatenate([t[i] for t in trip]) for i in range(3)), N_ENT, N_REL, dev))
    plans = [plan.build_plan(h, t, r, rng.randint(0, N_ENT, (B // (n or B)) * n), n or B, n, k % 2 == 0) for k, (h, r, t) in enumerate(trip)]
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
    argv = sys.argv[1:]
    parent = argv[argv.index("--parent_lib") + 1] if "--parent_lib" in argv else None
    args = [a for a in argv if not a.startswith("--") and a != parent]
    quick = "--quick" in argv
    if "--child" in argv:
        return child(args[0], quick)
    out = args[0] if args else os.path.join(ROOT, "profiles", "clamp_quate_timing.txt")
    runs = [(v, None) for v in VARIANTS] + ([(v, parent) for v in PARENT] if parent else [])
    res = {r: [] for r in runs}
    for rep in range(1 if quick else REPS):
        for v, lib in runs:
            env = dict(os.environ, KGE_LIB=os.path.abspath(lib)) if lib else os.environ
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", v] +
                               (["--quick"] if quick else []), stdout=subprocess.PIPE, text=True, env=env)
            if r.returncode != 0:
                sys.exit("child %s failed (%d): nothing more is run" % (v, r.returncode))
            d = json.loads(r.stdout.strip().splitlines()[-1])
            assert d["finite"], v
            res[(v, lib)].append(d["us"])
            print(v, "parent" if lib else "", rep, ["%.1f" % x for x in d["us"]], flush=True)
    with open(out, "w") as f:
        f.write("one MI355X; batch %d, hidden %d, %d entities; eager launches, %d steps per measurement, %d measurements per process, "
                "%d processes per variant in alternation\n" % (B, HIDDEN, N_ENT, K, 1 if quick else MEAS, 1 if quick else REPS))
        for (v, lib), rr in res.items():
            med, per = float(np.median(np.concatenate(rr))), [float(np.median(r)) for r in rr]
            f.write("%-28s median %9.1f us/step   per-process medians %9.1f .. %9.1f\n"
                    % (v + (" (parent library)" if lib else ""), med, min(per), max(per)))
    print(open(out).read())


if __name__ == "__main__":
    main()
