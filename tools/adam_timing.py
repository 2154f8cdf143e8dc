"""What --optimizer Adam costs per step at the cfg-T shape (TransE_l2, d 400, batch 1000, 200 negatives in chunks of 200) on the
planted FB15k-shaped graph of bench.py's time_to_mrr leg (tools/make_planted_fb15k.py), and whether the default Adagrad step moved
(tools/subsampling_timing.py's method).

Every step variant is a hipGraph of [one sampler launch + G strict steps] over a device sampler.  Each measurement is a child
process of its own under `timeout`: it builds the engine, captures the graph, times REPLAYS replays MEAS times and prints one JSON
line.  The driver runs the variants in alternation, REPS rounds; the first child that fails ends the run.  The figure of a variant is
the median over all its measurements; its spread the range of its per-process medians.
  default      Logsigmoid -adv, the benchmark's configuration, Adagrad (kge_step_fused)
  parent       (--baseline_lib PATH: libkge_hip.so built from the parent commit) the same, run by that library - the two must agree
               within the spread: the kernels the Adagrad step launches are compiled from the same source
  adam         the same step with optimizer='Adam' (kge_step_optim, KGE_OPT_ADAM), lr 1e-3
  upd_adagrad  the update launch alone: gather, forward and backward of one batch once, then a hipGraph of G update phase groups
  upd_adam     (kge_step_optim, phase mask KGE_PHASE_UPDATE) on that batch, back to back; per launch
--mrr: for information only, dglke_train PairRE on the planted graph cut at 2 000 steps, validation MRR under Adam (lr 1e-3) and
under Adagrad (the README's PairRE recipe: -g 6.0 --lr 0.1 -adv, hidden 200).
usage: python tools/adam_timing.py [--baseline_lib PATH] [--mrr] [--quick] [out.txt]   (default profiles/adam_timing.txt)"""
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
HIDDEN, GAMMA, LR, ADAM_LR, B, N = 400, 19.9, 0.25, 1e-3, 1000, 200
G, REPS, REPLAYS, MEAS = 100, 5, 30, 3
CHILD_LIMIT_S = 150
VARIANTS = ("default", "parent", "adam", "upd_adagrad", "upd_adam")


def load_train(data):
    t = np.loadtxt(os.path.join(data, "train.txt"), dtype=np.int64)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()


def child(variant, data, quick):
    """one variant, timed in this process; prints one JSON line"""
    import torch as th
    from dglke_amd import _lib
    if variant == "parent":                   # the parent commit's library has no kge_step_optim: not bound, not called
        _lib._SIGNATURES.pop("kge_step_optim", None)
    from dglke_amd.dataloader import DeviceSampler
    from dglke_amd.engine import StepEngine
    trip = load_train(data)
    dev = th.device("cuda", 0)
    th.manual_seed(0)
    adam = variant in ("adam", "upd_adam")
    eng = StepEngine("TransE_l2", N_ENT, N_REL, HIDDEN, GAMMA, ADAM_LR if adam else LR, dev, False, False, True, 1.0, 1e-9, 3,
                     **(dict(optimizer="Adam") if adam else {}))
    smp = DeviceSampler(trip[0], trip[1], trip[2], N_ENT, B, N, dev, n_slots=G, neg_chunk_size=N, seed=5)
    for b in smp.sample(G):                   # eager warm-up: allocates the workspace
        eng.step(b)
    th.cuda.synchronize()
    g = th.cuda.CUDAGraph()
    if variant.startswith("upd_"):
        opt = eng.opt
        if opt is None:
            opt = _lib.KgeOptim()
            opt.kind = _lib.OPT_ADAGRAD
        b = smp.sample(1)[0]
        out = _lib.KgeStepOut()
        out.loss_accum, out.tickets = _lib.ptr(eng.loss_accum), _lib.ptr(eng.tickets)
        ws = eng.workspace_for(b)

        def phases(ph):
            _lib.check(_lib.lib().kge_step_optim(C.byref(eng.hp), C.byref(opt), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(ws),
                                                 eng._ws_bytes, ph, None, None, 0, _lib.stream_ptr()))
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
           os.path.join(tmp, "ckpts"), "--model_name", "PairRE", "-dr", "--no_save_emb", "--gpu", "0", "--batch_size", "1000",
           "--neg_sample_size", "200", "--hidden_dim", "200", "--gamma", "6.0", "--max_step", str(steps), "--log_interval", "1000",
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
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "adam_timing.txt")
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
        mrr = None
        if "--mrr" in flags:
            mrr = (mrr_after(data, tmp, ["--optimizer", "Adam", "--lr", "0.001"]), mrr_after(data, tmp, ["--lr", "0.1"]))
    med = lambda v: float(np.median(np.concatenate(per[v])))
    spread = lambda v: float(np.ptp([np.median(x) for x in per[v]]))
    fmt = lambda v: "%8.2f us (processes' medians %8.2f .. %8.2f, spread %.2f)" % (
        med(v), min(np.median(x) for x in per[v]), max(np.median(x) for x in per[v]), spread(v))
    say("# cfg-T: TransE_l2 d %d, batch %d, %d negatives in chunks of %d; planted FB15k-shaped graph; per step of a replayed group of %d"
        % (HIDDEN, B, N, N, G))
    say("default step     %s   Logsigmoid -adv, Adagrad, this build" % fmt("default"))
    if base:
        s = max(spread("default"), spread("parent"))
        d = med("default") - med("parent")
        say("default, parent  %s   the parent commit's library (KGE_LIB) under this package" % fmt("parent"))
        say("this - parent    %+.2f us; the larger spread of one library is %.2f us: %s" % (
            d, s, "within it" if abs(d) <= s else "OUTSIDE it"))
    else:
        say("default, parent  not measured (no --baseline_lib)")
    say("Adam step        %s   optimizer Adam, lr %g, betas 0.9 / 0.999, eps 1e-8" % (fmt("adam"), ADAM_LR))
    say("Adam - Adagrad   %+.2f us per step (%.2f x); the larger spread of the two is %.2f us" % (
        med("adam") - med("default"), med("adam") / med("default"), max(spread("adam"), spread("default"))))
    say("update launch alone, Adagrad  %s   %d update phase groups of one batch back to back" % (fmt("upd_adagrad"), G))
    say("update launch alone, Adam     %s   the same, KGE_OPT_ADAM" % fmt("upd_adam"))
    say("Adam - Adagrad update launch  %+.2f us; the whole Adagrad step is %.2f us: the Adam update launch costs %s than that" % (
        med("upd_adam") - med("upd_adagrad"), med("default"), "MORE" if med("upd_adam") > med("default") else "less"))
    if mrr is not None:
        say("validation MRR after 2 000 steps of PairRE on the planted graph (information only): Adam lr 1e-3 %.4f, Adagrad lr 0.1 %.4f" % mrr)
    else:
        say("validation MRR after 2 000 steps: not measured (no --mrr)")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# tools/adam_timing.py%s: %d alternating rounds, one process per measurement, %d x %d replays each\n" % (
            " --quick" if quick else "", 2 if quick else REPS, MEAS, 2 if quick else REPLAYS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
