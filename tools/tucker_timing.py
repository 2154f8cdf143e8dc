"""What a TuckER K-vs-all step costs, next to the DistMult K-vs-all step at the same widths in the same run (the method and the
helpers of tools/k_vs_all_timing.py: separate child processes under `timeout` in alternation, REPS rounds, the first child that fails
ends the run; figure of a variant: the median over all its measurements; spread: the range of its per-process medians).
Shape: batch 1000, d_e = d_r = 200, the planted FB15k-shaped graph of tools/make_planted_fb15k.py (14 951 entities); batches are
host-built plans uploaded before the timed region, steps are launched eagerly, K steps between two events, one untimed group in front.
  tucker_kva     StepEngine('TuckER', k_vs_all=True, label_smoothing=0.1).step: operand + combine, kva_prep, kva_bwd_a, kva_loss, u,
                 backward + gxr, core owner, kva_bwd_e, update
  distmult_kva   the same step of DistMult at hidden 200: what the candidate side and the traces cost without the core
  default / parent   TransE_l2 at cfg-T by this build and (--baseline_lib PATH) by the parent commit's library: no existing kernel's
                 source changed, the two must agree within the spread the tool measures between processes of one library
The new launches on their own: one more tucker_kva child under `rocprofv3 --kernel-trace --stats`, a run of its own behind the timed
ones; the mean duration of every tk_* kernel of the step and their sum are written under the timings.
FLOP figure: 2 B d_r d_e^2 per contraction with the core, three of them; arithmetic, not a measurement.
usage: python tools/tucker_timing.py [--baseline_lib PATH] [--quick] [out.txt]   (default profiles/tucker_timing.txt)"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-ke_amd"), os.path.join(ROOT, "tools")]
import k_vs_all_timing as KT      # noqa: E402 - load_train, child_cfgt and the shape of the planted graph

D = 200
VARIANTS = ("tucker_kva", "distmult_kva", "default", "parent")


def child(variant, data, quick):
    import torch as th
    from dglke_amd import plan
    from dglke_amd.engine import StepEngine
    from dglke_amd.known import KnownIndex
    trip = KT.load_train(data)
    dev = th.device("cuda", 0)
    th.manual_seed(0)
    if variant in ("default", "parent"):
        ts, eng = KT.child_cfgt(trip, quick)
    else:
        rng = np.random.RandomState(1)
        rows = [rng.randint(0, len(trip[0]), KT.B) for _ in range(KT.K)]
        kw = dict(relation_dim=D) if variant == "tucker_kva" else {}
        eng = StepEngine("TuckER" if variant == "tucker_kva" else "DistMult", KT.N_ENT, KT.N_REL, D, KT.GAMMA, KT.LR, dev,
                         loss_genre='BCE', k_vs_all=True, label_smoothing=0.1, **kw)
        eng.attach_known(KnownIndex(trip, KT.N_ENT, KT.N_REL, dev))
        batches = plan.upload([plan.build_plan(trip[0][r], trip[2][r], trip[1][r], np.zeros(0, np.int64), KT.B, 0, k % 2 == 0)
                               for k, r in enumerate(rows)], dev)
        ts = []
        for m in range((1 if quick else KT.MEAS) + 1):
            a, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            a.record()
            for b in batches:
                eng.step(b)
            e.record()
            th.cuda.synchronize()
            if m:                                     # (the first group allocates the workspace and ramps the clocks)
                ts.append(a.elapsed_time(e) * 1e3 / KT.K)
    print(json.dumps(dict(us=ts, finite=bool(np.isfinite(eng.read_loss_sums()[2])))))


def run_child(variant, data, quick, lib=None, trace_dir=None):
    env = dict(os.environ)
    env.pop("KGE_LIB", None)
    if lib:
        env["KGE_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, data] + (["--quick"] if quick else [])
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + cmd
    r = subprocess.run(["timeout", "-k", "10", str(KT.CHILD_LIMIT_S)] + cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("child %s failed (%d): nothing more is run" % (variant, r.returncode))
    d = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"us"')][-1]
    assert d["finite"], variant
    return d["us"]


def tk_kernel_means(trace_dir):
    """tk_* kernel name -> (calls, mean us) from the kernel_stats.csv of a rocprofv3 --stats run"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            if name.startswith("tk_"):
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
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "tucker_timing.txt")
    import __graft_entry__
    __graft_entry__.build()
    order = [v for v in VARIANTS if v != "parent" or base]
    res, trace, trace_note = {v: [] for v in order}, {}, ""
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "fb15k_planted")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_planted_fb15k.py"), data], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode:
            raise SystemExit(r.stdout)
        for rep in range(1 if quick else KT.REPS):
            for v in order:
                res[v].append(run_child(v, data, quick, base if v == "parent" else None))
                print(v, rep, ["%.1f" % x for x in res[v][-1]], flush=True)
        try:                                          # behind the timed runs, a run of its own; the timings stand without it
            td = os.path.join(tmp, "trace")
            run_child("tucker_kva", data, True, trace_dir=td)
            trace = tk_kernel_means(td)
            if not trace:
                raise KeyError("no kernel_stats.csv under the trace directory")
        except (SystemExit, KeyError, ValueError, OSError) as e:
            trace, trace_note = {}, "failed: %r" % (e,)
    med = lambda v: float(np.median(np.concatenate(res[v])))
    per = lambda v: [float(np.median(r)) for r in res[v]]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("one MI355X; batch %d, d_e = d_r = %d, planted FB15k-shaped graph (%d entities); N == 0 steps: eager launches, %d steps per "
                "measurement, %d measurements per process; %d processes per variant in alternation\n"
                % (KT.B, D, KT.N_ENT, KT.K, 1 if quick else KT.MEAS, len(res["tucker_kva"])))
        for v in order:
            f.write("%-13s median %9.1f us/step   per-process medians %9.1f .. %9.1f\n" % (v, med(v), min(per(v)), max(per(v))))
        gflop = 3 * 2.0 * KT.B * D * D * D * 1e-9
        f.write("tucker_kva - distmult_kva: %+.1f us for three contractions with the core, %.1f GFLOP counted (arithmetic)\n"
                % (med("tucker_kva") - med("distmult_kva"), gflop))
        if base:
            s = max(np.ptp(per("default")), np.ptp(per("parent")))
            d = med("default") - med("parent")
            f.write("default - parent: %+.2f us; the larger process-to-process spread of one library is %.2f us: %s\n"
                    % (d, s, "within it" if abs(d) <= s else "OUTSIDE it"))
        else:
            f.write("default against the parent commit's library: not measured (no --baseline_lib)\n")
        if trace:
            f.write("the new launches (rocprofv3 --kernel-trace --stats, a run of its own): mean us per call [calls]\n")
            for name in sorted(trace):
                f.write("  %-40s %9.1f [%d]\n" % (name[:40], trace[name][1], trace[name][0]))
            # (both corruption sides alternate: a step runs one instance of each kernel, half of the calls of either side's)
            steps = max(c for c, _ in trace.values())
            f.write("  sum over the tk_* kernels per step: %.1f us\n" % (sum(c * u for c, u in trace.values()) / steps))
        else:
            f.write("the new launches on their own: not measured (%s)\n" % trace_note)
    print(open(out).read())


if __name__ == "__main__":
    main()
