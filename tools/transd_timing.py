"""What a TransD step costs, and whether the default step moved (the method of tools/transh_timing.py).  Shapes: the FB15k recipe shape (batch 1000, 200 negatives in chunks
of 200) on the planted FB15k-shaped graph of bench.py's time_to_mrr leg (tools/make_planted_fb15k.py).

Every step variant is a hipGraph of [one sampler launch + G strict steps] over a device sampler (tools/pairre_timing.py's method).
Each measurement is a child process of its own under `timeout`: it builds the engine, captures the graph, times REPLAYS replays
MEAS times and prints one JSON line.  The driver runs the variants in alternation, REPS rounds; the first child that fails ends
the run.  The figure of a variant is the median over all its measurements; its spread the range of its per-process medians.
  default    TransE_l2 at cfg-T (hidden 400), Logsigmoid -adv, the benchmark's configuration: the 4-launch step
  parent     (--baseline_lib PATH: libkge_hip.so built from the parent commit) the same, run by that library - the two must agree
             within the spread: no existing kernel instance changed
  transd     TransD (-de -dr, hidden 400: rows 800 wide on both tables): edge forward / stacked forward product over the first
             halves / scores / loss / coefficients / stacked backward products / edge backward / update
  transh     TransH (-dr, hidden 400): the same launch sequence, relation rows 800 wide, entity rows 400
  l2_split   TransE_l2 (hidden 400) forced onto the split launch sequence (KGE_FLAG_SPLIT_FWD | KGE_FLAG_NO_TRANSE_FAST): edge forward,
             forward product, loss, backward products, edge backward, update - one product where TransD runs two
  transd200  TransD at hidden 200
  transr200  TransR at hidden 200 (relation width 200): the model whose d_e x d_r matrix per relation TransD's two vectors replace
For information, in one more child: one Ranker.ranks call of 2 x 50 000 triples against the 14 951 entities (hidden 400), TransD next
to TransH.
usage: python tools/transd_timing.py [--baseline_lib PATH] [--quick] [out.txt]   (default profiles/transd_timing.txt)"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, ROOT)

N_ENT, N_REL = 14951, 1345
WIDTH, GAMMA, LR, B, N = 400, 19.9, 0.25, 1000, 200
G, REPS, REPLAYS, MEAS = 100, 3, 30, 3
RANK_E = 50000
CHILD_LIMIT_S = 150
# variant -> (model, hidden, -de, -dr, flags)
SPLIT = 128 | 2             # KGE_FLAG_SPLIT_FWD | KGE_FLAG_NO_TRANSE_FAST
VARIANTS = {"default": ("TransE_l2", WIDTH, False, False, 0), "parent": ("TransE_l2", WIDTH, False, False, 0),
            "transd": ("TransD", WIDTH, True, True, 0), "transh": ("TransH", WIDTH, False, True, 0),
            "l2_split": ("TransE_l2", WIDTH, False, False, SPLIT),
            "transd200": ("TransD", 200, True, True, 0), "transr200": ("TransR", 200, False, False, 0)}


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
    if variant == "rank":
        return rank_child(trip, dev, quick)
    model, hidden, de, dr, flags = VARIANTS[variant]
    eng = StepEngine(model, N_ENT, N_REL, hidden, GAMMA, LR, dev, de, dr, True, 1.0, 1e-9, 3, flags=flags)
    assert eng.d_e == hidden * (2 if de else 1)
    smp = DeviceSampler(trip[0], trip[1], trip[2], N_ENT, B, N, dev, n_slots=G, neg_chunk_size=N, seed=5)
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


def rank_child(trip, dev, quick):
    """one Ranker.ranks call per side over RANK_E test triples against every entity, per model; the second call of each is timed"""
    import torch as th
    from dglke_amd import eval as kev
    E = 2000 if quick else RANK_E
    rng = np.random.RandomState(3)
    sel = rng.randint(0, len(trip[0]), E)
    h, r, t = (x[sel] for x in trip)
    out = {}
    for model, de_, dr in (("TransH", 1, 2), ("TransD", 2, 2)):
        ent = (th.rand(N_ENT, de_ * WIDTH, device=dev) - 0.5)
        rel = (th.rand(N_REL, dr * WIDTH, device=dev) - 0.5)
        rk = kev.Ranker(model, ent, rel, GAMMA, 1.0)
        ms = []
        for rep_ in range(2):
            a, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            a.record()
            for neg_head in (False, True):
                ranks = rk.ranks(h, r, t, neg_head)
            e.record()
            th.cuda.synchronize()
            ms.append(a.elapsed_time(e))
        out[model] = ms[1]
        assert int(ranks.min()) >= 1
    print(json.dumps(dict(us=[out["TransH"] * 1e3, out["TransD"] * 1e3], finite=True)))


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
        raise SystemExit("%s: the loss is not finite" % variant)
    return r["us"]


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
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "transd_timing.txt")
    import __graft_entry__
    __graft_entry__.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    order = ["default"] + (["parent"] if base else []) + ["transd", "transh", "l2_split", "transd200", "transr200"]
    per = {v: [] for v in order}
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "fb15k_planted")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_planted_fb15k.py"), data], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode:
            raise SystemExit(r.stdout)
        for _ in range(2 if quick else REPS):
            for v in order:
                per[v].append(run_child(v, data, quick, base if v == "parent" else None))
        rank = run_child("rank", data, quick, None)
    med = lambda v: float(np.median(np.concatenate(per[v])))
    spread = lambda v: float(np.ptp([np.median(x) for x in per[v]]))
    fmt = lambda v: "%7.2f us (processes' medians %7.2f .. %7.2f, spread %.2f)" % (
        med(v), min(np.median(x) for x in per[v]), max(np.median(x) for x in per[v]), spread(v))
    say("# batch %d, %d negatives in chunks of %d, entity width %d; planted FB15k-shaped graph; per step of a replayed group of %d"
        % (B, N, N, WIDTH, G))
    say("default step     %s   TransE_l2, Logsigmoid -adv, this build" % fmt("default"))
    if base:
        s = max(spread("default"), spread("parent"))
        d = med("default") - med("parent")
        say("default, parent  %s   the parent commit's library (KGE_LIB) under this package" % fmt("parent"))
        say("this - parent    %+.2f us; the larger spread of one library is %.2f us: %s" % (
            d, s, "within it" if abs(d) <= s else "OUTSIDE it"))
    else:
        say("default, parent  not measured (no --baseline_lib)")
    say("TransD step      %s   hidden 400, entity and relation rows 800 wide" % fmt("transd"))
    say("TransH step      %s   hidden 400, relation rows 800 wide" % fmt("transh"))
    say("TransE_l2 split  %s   hidden 400, KGE_FLAG_SPLIT_FWD | KGE_FLAG_NO_TRANSE_FAST: the same launch sequence, one product" % fmt("l2_split"))
    say("TransD / TransH  %.2f x;  TransD / TransE_l2 split  %.2f x; the largest spread of the three is %.2f us" % (
        med("transd") / med("transh"), med("transd") / med("l2_split"), max(spread("transd"), spread("transh"), spread("l2_split"))))
    say("TransD step      %s   hidden 200" % fmt("transd200"))
    say("TransR step      %s   hidden 200, relation width 200" % fmt("transr200"))
    say("TransR / TransD at hidden 200  %.1f x (%s)" % (med("transr200") / med("transd200"),
                                                        "TransD is below TransR" if med("transd200") < med("transr200") else "TransD is NOT below TransR"))
    say("Ranker.ranks, 2 x %d triples against %d entities, hidden %d, one call:  TransH %.1f ms   TransD %.1f ms" % (
        2000 if quick else RANK_E, N_ENT, WIDTH, rank[0] / 1e3, rank[1] / 1e3))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# tools/transd_timing.py%s: %d alternating rounds, one process per measurement, %d x %d replays each\n" % (
            " --quick" if quick else "", 2 if quick else REPS, MEAS, 2 if quick else REPLAYS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
