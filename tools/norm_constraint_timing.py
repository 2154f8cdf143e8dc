"""What --ent_norm / --rel_norm cost per step, and whether the default step moved (tools/adam_timing.py's method), on the planted
FB15k-shaped graph of bench.py's time_to_mrr leg (tools/make_planted_fb15k.py).

Every step variant is a hipGraph of [one sampler launch + G strict steps] over a device sampler.  Each measurement is a child
process of its own under `timeout`: it builds the engine, captures the graph, times REPLAYS replays MEAS times and prints one JSON
line.  The driver runs the variants in alternation, REPS rounds; the first child that fails ends the run.  The figure of a variant is
the median over all its measurements; its spread the range of its per-process medians.
  default      cfg-T (TransE_l2, d 400, batch 1000, 200 negatives in chunks of 200), Logsigmoid -adv, Adagrad, no constraint
  parent       (--baseline_lib PATH: libkge_hip.so built from the parent commit) the same, run by that library - the two must agree
               within the spread: the kernels the step launches are compiled from the same source
  ent_clip     the cfg-T step with ent_norm='clip' (one more launch behind the update)
  transd       TransD at the recipe shape (hidden 400: rows of 800 floats in two slices), no constraint
  transd_norm  the same with ent_norm='clip', rel_norm='clip'
  upd          the update launch alone: gather, forward and backward of one cfg-T batch once, then a hipGraph of G update phase groups
  upd_norm     (kge_step_phase, KGE_PHASE_UPDATE) on that batch, back to back; per group.  With ent_norm='clip' a group is the update
               launch followed by the constraint launch: the library has no entry that issues the constraint launch by itself, so its
               time is the difference of the two figures - with the spreads of both - and the same batch is updated and clipped G times
               in a row, so the share of slices that take the store path is not a training step's (both are said in the output)
--mrr: for information only, dglke_train TransD on the planted graph cut at 2 000 steps, validation MRR with --ent_norm clip
--rel_norm clip and without.
usage: python tools/norm_constraint_timing.py [--baseline_lib PATH] [--mrr] [--quick] [out.txt]
       (default profiles/norm_constraint_timing.txt)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, ROOT)

N_ENT, N_REL = 14951, 1345
HIDDEN, GAMMA, LR, B, N = 400, 19.9, 0.25, 1000, 200
G, REPS, REPLAYS, MEAS = 100, 3, 30, 3
CHILD_LIMIT_S = 150
VARIANTS = ("default", "parent", "ent_clip", "transd", "transd_norm", "upd", "upd_norm")


def load_train(data):
    t = np.loadtxt(os.path.join(data, "train.txt"), dtype=np.int64)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()


def child(variant, data, quick):
    """one variant, timed in this process; prints one JSON line"""
    import torch as th
    from dglke_amd import _lib
    from dglke_amd.dataloader import DeviceSampler
    from dglke_amd.engine import StepEngine
    trip = load_train(data)
    dev = th.device("cuda", 0)
    th.manual_seed(0)
    norms = dict(ent_clip=dict(ent_norm="clip"), upd_norm=dict(ent_norm="clip"), transd_norm=dict(ent_norm="clip", rel_norm="clip")).get(variant, {})
    if variant.startswith("transd"):
        eng = StepEngine("TransD", N_ENT, N_REL, HIDDEN, GAMMA, LR, dev, True, True, True, 1.0, 1e-9, 3, **norms)
    else:
        eng = StepEngine("TransE_l2", N_ENT, N_REL, HIDDEN, GAMMA, LR, dev, False, False, True, 1.0, 1e-9, 3, **norms)
    smp = DeviceSampler(trip[0], trip[1], trip[2], N_ENT, B, N, dev, n_slots=G, neg_chunk_size=N, seed=5)
    for b in smp.sample(G):                   # eager warm-up: allocates the workspace
        eng.step(b)
    th.cuda.synchronize()
    g = th.cuda.CUDAGraph()
    if variant.startswith("upd"):
        b = smp.sample(1)[0]
        out = _lib.KgeStepOut()
        out.loss_accum, out.tickets = _lib.ptr(eng.loss_accum), _lib.ptr(eng.tickets)
        ws = eng.workspace_for(b)

        def phases(ph):
            _lib.check(_lib.lib().kge_step_phase(C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(ws), eng._ws_bytes,
                                                 ph, _lib.stream_ptr()))
        for ph in (_lib.PHASE_GATHER, _lib.PHASE_FORWARD, _lib.PHASE_BACKWARD):
            phases(ph)
        th.cuda.synchronize()
        with _lib.graph_capture(g):
            for _ in range(G):
                phases(_lib.PHASE_UPDATE)
    else:
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
    print(json.dumps(dict(us=ts, finite=bool(np.isfinite(loss[2]) and th.isfinite(eng.ent).all()))))
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
    cmd = ["timeout", "-k", "10", "300", sys.executable, cli, "--format", "udd_hrt", "--dataset", "fb15k_planted", "--data_path", data,
           "--data_files", "entities.dict", "relations.dict", "train.txt", "valid.txt", "test.txt", "--save_path",
           os.path.join(tmp, "ckpts"), "--model_name", "TransD", "-de", "-dr", "--no_save_emb", "--gpu", "0", "--batch_size", "1000",
           "--neg_sample_size", "200", "--hidden_dim", "200", "--gamma", "6.0", "--lr", "0.1", "--max_step", str(steps), "--log_interval", "1000",
           "--eval_interval", str(steps), "--valid", "--graph_steps", "100", "--batch_size_eval", "16", "-adv"] + extra
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
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "norm_constraint_timing.txt")
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
        for rnd in range(2 if quick else REPS):
            for v in order:
                per[v].append(run_child(v, data, quick, base if v == "parent" else None)["us"])
                print("round %d %-12s %s" % (rnd + 1, v, " ".join("%.2f" % t for t in per[v][-1])), flush=True)
        mrr = None
        if "--mrr" in flags:
            mrr = (mrr_after(data, tmp, ["--ent_norm", "clip", "--rel_norm", "clip"]), mrr_after(data, tmp, []))
    med = lambda v: float(np.median(np.concatenate(per[v])))
    spread = lambda v: float(np.ptp([np.median(x) for x in per[v]]))
    fmt = lambda v: "%8.2f us (processes' medians %8.2f .. %8.2f, spread %.2f)" % (
        med(v), min(np.median(x) for x in per[v]), max(np.median(x) for x in per[v]), spread(v))
    say("# cfg-T: TransE_l2 d %d, batch %d, %d negatives in chunks of %d; planted FB15k-shaped graph; per step of a replayed group of %d"
        % (HIDDEN, B, N, N, G))
    say("default step            %s   Logsigmoid -adv, Adagrad, no constraint, this build" % fmt("default"))
    if base:
        s = max(spread("default"), spread("parent"))
        d = med("default") - med("parent")
        say("default, parent         %s   the parent commit's library (KGE_LIB) under this package" % fmt("parent"))
        say("this - parent           %+.2f us; the larger spread of one library is %.2f us: %s" % (
            d, s, "within it" if abs(d) <= s else "OUTSIDE it"))
    else:
        say("default, parent         not measured (no --baseline_lib)")
    say("cfg-T, --ent_norm clip  %s" % fmt("ent_clip"))
    say("  - default             %+.2f us per step (%.3f x); the larger spread of the two is %.2f us" % (
        med("ent_clip") - med("default"), med("ent_clip") / med("default"), max(spread("ent_clip"), spread("default"))))
    say("TransD, hidden %d      %s   rows of %d floats, no constraint" % (HIDDEN, fmt("transd"), 2 * HIDDEN))
    say("TransD, both flags clip %s   four slices of %d" % (fmt("transd_norm"), HIDDEN))
    say("  - TransD              %+.2f us per step (%.3f x); the larger spread of the two is %.2f us" % (
        med("transd_norm") - med("transd"), med("transd_norm") / med("transd"), max(spread("transd_norm"), spread("transd"))))
    say("update launch alone            %s   %d update phase groups of one cfg-T batch back to back" % (fmt("upd"), G))
    say("update + constraint launch     %s   the same with ent_norm='clip'" % fmt("upd_norm"))
    con = med("upd_norm") - med("upd")
    cs = spread("upd_norm") + spread("upd")
    verdict = "SLOWER than" if con - cs > med("upd") else "faster than" if con + cs < med("upd") else "NOT SEPARABLE from"
    say("constraint launch (difference) %+.2f us +- %.2f us (a difference of two medians: it carries the spreads of both, summed here); "
        "the update launch alone is %.2f us: the constraint launch is %s that yardstick" % (con, cs, med("upd"), verdict))
    say("  caveat: the groups update and clip the SAME batch %d times in a row, so the share of slices that are scaled and stored (norm > 1 "
        "after an update that follows a clip) is not that of a training step, whose rows come from different batches" % G)
    if mrr is not None:
        say("validation MRR after 2 000 steps of TransD (hidden 200) on the planted graph (information only): --ent_norm clip --rel_norm "
            "clip %.4f, without %.4f" % mrr)
    else:
        say("validation MRR after 2 000 steps: not measured (no --mrr)")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# tools/norm_constraint_timing.py%s: %d alternating rounds, one process per measurement, %d x %d replays each\n" % (
            " --quick" if quick else "", 2 if quick else REPS, MEAS, 2 if quick else REPLAYS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
