"""What dglke_train --exclude_positive costs per step at the cfg-T shape (TransE_l2, d 400, batch 1000, 200 negatives in chunks of
200, -adv), on the planted FB15k-shaped graph of bench.py's time_to_mrr leg (tools/make_planted_fb15k.py; uniform synthetic
triples almost never collide with uniform negatives, a graph at least has the positives' own lists).

Every variant is a hipGraph of [one sampler launch + G strict steps] over a device sampler, replayed in alternation with the other
variants; the time is the median over the repetitions of (replay time / G):
  off        no index attached: kge_step_fused, the 4-launch step with the LEAN loss kernel;
  on         the training split attached (StepEngine.attach_known): kge_step_fused_known - one mask launch in front of the loss launch
             and the loss kernel's full instance;
  parent     (--baseline_tree DIR: a built checkout of the parent commit) the same `off` graph run by that tree's package and library
             in a child process of its own.
Also: the mask kernel alone (a hipGraph of G back-to-back launches over the group's batches) and the share of known pairs among the
B * N pairs of those batches.
usage: python tools/exclude_positive_timing.py [--baseline_tree DIR] [--quick] [out.txt]     (default profiles/exclude_positive_timing.txt)"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("KGE_TIMING_TREE") or ROOT          # the child of --baseline_tree imports the package of that tree
sys.path.insert(0, os.path.join(TREE, "dgl-ke_amd"))
sys.path.insert(0, TREE)

N_ENT, N_REL = 14951, 1345
HIDDEN, GAMMA, LR, B, N = 400, 19.9, 0.25, 1000, 200
G, REPS, REPLAYS = 100, 7, 50


def load_train(data):
    t = np.loadtxt(os.path.join(data, "train.txt"), dtype=np.int64)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()


def group(trip, known, seed=5):
    """engine + sampler + the captured graph of one variant.  The graph holds the ADDRESSES of the engine's tables and workspace and of
    the sampler's triples, state and slots: the caller keeps all three objects for as long as it replays the graph."""
    import torch as th
    from dglke_amd import _lib
    from dglke_amd.dataloader import DeviceSampler
    from dglke_amd.engine import StepEngine
    dev = th.device("cuda", 0)
    th.manual_seed(0)
    eng = StepEngine("TransE_l2", N_ENT, N_REL, HIDDEN, GAMMA, LR, dev, False, False, True, 1.0, 1e-9, 3)
    if known is not None:
        eng.attach_known(known)
    smp = DeviceSampler(trip[0], trip[1], trip[2], N_ENT, B, N, dev, n_slots=G, neg_chunk_size=N, seed=seed)
    for b in smp.sample(G):                   # eager warm-up: allocates the workspace
        eng.step(b)
    th.cuda.synchronize()
    g = th.cuda.CUDAGraph()
    with _lib.graph_capture(g):
        for b in smp.sample(G):
            eng.step(b)
    return eng, smp, g


def replay_us(g, replays):
    import torch as th
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    g.replay()                                # the first kernels after a pause of the queue run late: one untimed replay in front
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (replays * G)


def child(data, quick):
    """the parent tree's plain step, timed the same way; prints one JSON line"""
    trip = load_train(data)
    eng, smp, g = group(trip, None)           # (eng, smp: kept alive, see group)
    ts = [replay_us(g, 2 if quick else REPLAYS) for _ in range(REPS)]
    print(json.dumps(dict(us=ts)))
    del g, smp, eng


def main():
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in flags
    if "--child" in flags:
        return child(argv[0], quick)
    base = None
    if "--baseline_tree" in flags:
        base, argv = os.path.abspath(argv[0]), argv[1:]
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "exclude_positive_timing.txt")
    import ctypes as C
    import torch as th
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib
    from dglke_amd.known import KnownIndex
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as data:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_planted_fb15k.py"), data], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode:
            raise SystemExit(r.stdout)
        trip = load_train(data)
        parent = None
        if base:       # a fresh child process: that tree's package and library, nothing of this one's
            env = dict(os.environ, KGE_TIMING_TREE=base)
            env.pop("KGE_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", data] + (["--quick"] if quick else []), env=env,
                               stdout=subprocess.PIPE, text=True, timeout=300)
            if p.returncode:
                raise SystemExit("the baseline child failed (exit %d)" % p.returncode)
            parent = json.loads(p.stdout.strip().split("\n")[-1])["us"]
    dev = th.device("cuda", 0)
    say("# %s; cfg-T: TransE_l2 d %d, batch %d, %d negatives in chunks of %d, -adv; planted FB15k-shaped graph, %d training triples"
        % (th.cuda.get_device_name(0), HIDDEN, B, N, N, len(trip[0])))
    idx = KnownIndex(trip, N_ENT, N_REL, dev)
    (kt, _), (kh, _) = idx.side(False), idx.side(True)
    say("# index: %d (key, tail) pairs, %d (key, head) pairs, sorted on the device once" % (kt.numel(), kh.numel()))
    eng_off, smp_off, g_off = group(trip, None)     # (eng_off, smp_off: kept alive, see group)
    eng_on, smp_on, g_on = group(trip, idx)
    reps = 2 if quick else REPLAYS
    t_off, t_on = [], []
    for _ in range(REPS):
        t_off.append(replay_us(g_off, reps))
        t_on.append(replay_us(g_on, reps))
    # the mask kernel alone, and the share of known pairs, over the batches the sampler's slots hold now
    bs = [smp_on._batches[(k, (k + 1) % 2 == 0)] for k in range(G)]       # (groups start at an odd step: slot k corrupts heads for odd k)
    W = (N + 31) // 32
    masks = th.zeros(G, B, W, dtype=th.int32, device=dev)
    k = eng_on._known[0]
    L = _lib.lib()

    def mask_all():
        for j, b in enumerate(bs):
            _lib.check(L.kge_known_neg_mask(C.byref(b.c), C.byref(k), masks[j].data_ptr(), B * W * 4, _lib.stream_ptr()))
    mask_all()
    th.cuda.synchronize()
    bits = masks.cpu().numpy().view(np.uint32)
    n_known = int(np.unpackbits(bits.view(np.uint8)).sum())
    gm = th.cuda.CUDAGraph()
    with _lib.graph_capture(gm):
        mask_all()
    t_mask = [replay_us(gm, reps) for _ in range(REPS)]
    med = lambda x: float(np.median(x))
    fmt = lambda x: "%7.2f us (min %7.2f max %7.2f)" % (med(x), min(x), max(x))
    say("step, flag off   %s   per step of a replayed group of %d" % (fmt(t_off), G))
    say("step, flag on    %s   +%.2f us: one mask launch + the loss kernel's full instance instead of the LEAN one" % (fmt(t_on), med(t_on) - med(t_off)))
    if parent is not None:
        say("step, parent     %s   the parent commit's package and library in a child process; flag off - parent = %+.2f us"
            % (fmt(parent), med(t_off) - med(parent)))
    else:
        say("step, parent     not measured (no --baseline_tree)")
    say("mask kernel      %s   per launch, %d launches back to back in a hipGraph" % (fmt(t_mask), G))
    say("known pairs      %d of %d pairs of one group = %.4f %%" % (n_known, G * B * N, 100.0 * n_known / (G * B * N)))
    del g_off, smp_off, eng_off
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# tools/exclude_positive_timing.py%s: %d alternating repetitions of %d replays, medians\n" % (" --quick" if quick else "", REPS, reps))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
