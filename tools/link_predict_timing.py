"""Device time of link prediction with known-edge exclusion (dglke_amd/ke_model.py -> kge_topk_select_filtered,
kge_triples_known) at FB15k's shape: 1000 heads x 14 951 candidates, d 400, K 10, batch_head, for DistMult, TransE_l2 and
TransE_l1.  The known graph is 592 213 triples with FB15k's heavy-tailed hub proportions (bench.synth_triples, skew) plus a
planted hub (h, r) with 5 000 known tails.
usage: python tools/link_predict_timing.py [--unfiltered | --kernels] [out.txt]    (default profiles/link_predict_timing.txt)
  (no flag)     per model: exclude_mode None / 'mask' / 'exclude' as whole Python calls (device events, after a warm-up),
                for rows whose lists are all empty, for typical rows, for typical rows + the hub row, and for a row block
                made of the hub row only; the one-off
                index build per side; torch matmul + masked_fill + topk on the full block as context (DistMult form)
  --unfiltered  only ScoreInfer.topK (the unfiltered path), every repetition printed: the A/B leg.  KGE_LIB may point at
                another build of the library (one that lacks the two new entry points is accepted in this mode only)
  --kernels     the cases of the default run, 1 warm-up + 3 calls each and nothing else: the run to put under
                rocprofv3 --kernel-trace --stats --output-format csv (kernel-only times: profiles/link_predict_kernel_stats.txt)"""
import ctypes
import os
import sys
import tempfile
import time

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, ROOT)

N_ENT, N_REL, H, K, HIDDEN, GAMMA = 14951, 1345, 1000, 10, 400, 12.0
MODELS = ("DistMult", "TransE_l2", "TransE_l1")


def times(fn, reps):
    fn()
    th.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        th.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def fmt(ms):
    return "median %8.3f ms  min %8.3f  max %8.3f  (n %d)" % (float(np.median(ms)), min(ms), max(ms), len(ms))


def tables(model, tmp, rng):
    ent = rng.uniform(-0.1, 0.1, (N_ENT, HIDDEN)).astype(np.float32)
    rel = rng.uniform(-0.1, 0.1, (N_REL, HIDDEN)).astype(np.float32)
    d = os.path.join(tmp, model)
    os.makedirs(d)
    np.save(os.path.join(d, "entity.npy"), ent)
    np.save(os.path.join(d, "relation.npy"), rel)
    np.save(os.path.join(d, "fb_%s_entity.npy" % model), ent)
    np.save(os.path.join(d, "fb_%s_relation.npy" % model), rel)
    return d


def main():
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "link_predict_timing.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.RandomState(0)
    tmp = tempfile.mkdtemp()
    if "--unfiltered" in flags:
        from dglke_amd import _lib
        handle = ctypes.CDLL(_lib.LIB_PATH)
        for name in ("kge_topk_select_filtered", "kge_triples_known"):      # an older build of the library: this leg only
            if not hasattr(handle, name):
                _lib._SIGNATURES.pop(name)
        from dglke_amd.infer import ScoreInfer
        say("# library: %s" % _lib.LIB_PATH)
        for model in MODELS:
            d = tables(model, tmp, rng)
            m = ScoreInfer(0, {"model_name": model, "dataset": "fb", "hidden_dim": HIDDEN, "gamma": GAMMA}, d, "none")
            m.load_model()
            h = rng.randint(0, N_ENT, H)
            ms = times(lambda: m.topK(h, [1], None, "batch_head", K), 20)
            say("unfiltered ScoreInfer.topK batch_head %-10s %s   all: %s" % (model, fmt(ms), " ".join("%.3f" % x for x in ms)))
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return

    import bench
    from dglke_amd import ke_model as KM
    kernels = "--kernels" in flags
    reps = 3 if kernels else 20
    kh, kr, kt = bench.synth_triples({"n_train": 592213, "n_ent": N_ENT, "n_rel": N_REL}, 1, skew=True)
    top_rel = int(np.bincount(kr).argmax())
    hub_h = int(np.bincount(kh[kr == top_rel]).argmax())
    hub_t = rng.permutation(N_ENT)[:5000]
    kh = np.concatenate([kh, np.full(5000, hub_h)])
    kr = np.concatenate([kr, np.full(5000, top_rel)])
    kt = np.concatenate([kt, hub_t])
    heads = rng.permutation(N_ENT)
    heads = heads[heads != hub_h][:H]
    lens = np.array([np.unique(kt[(kh == a) & (kr == top_rel)]).size for a in heads[:200]])
    say("# known graph: %d triples (skewed ids, bench.synth_triples) + a hub (h, r) with %d known tails; relation %d (the most "
        "frequent: %d triples); list length of the first 200 query rows: mean %.1f, max %d, empty %d"
        % (len(kh) - 5000, np.unique(kt[(kh == hub_h) & (kr == top_rel)]).size, top_rel, int((kr == top_rel).sum()), lens.mean(),
           lens.max(), int((lens == 0).sum())))
    listed = set(kh[kr == top_rel].tolist())
    no_list = np.array([a for a in rng.permutation(N_ENT).tolist() if a not in listed][:H])      # (h, r) without a known tail
    with_hub = heads.copy()
    with_hub[500] = hub_h
    hub_block = np.full(128, hub_h)
    for model in MODELS:
        d = tables(model, tmp, rng)
        m = getattr(KM, model + "Model")(0, GAMMA) if model != "DistMult" else KM.DistMultModel(0)
        m.load(d)
        m.attach_graph((kh, kr, kt))
        if not kernels:
            for side in (False, True):
                th.cuda.synchronize()
                th.cuda.reset_peak_memory_stats()
                base = th.cuda.memory_allocated()
                t0 = time.time()
                m._known._sides.pop(side, None)
                m._known.side(side)
                th.cuda.synchronize()
                say("%-10s index build, %s side: %7.1f ms, peak %.1f x 16 M bytes over what was allocated, %.2f x 16 M kept (M = %d)"
                    % (model, "head" if side else "tail", (time.time() - t0) * 1e3,
                       (th.cuda.max_memory_allocated() - base) / (16.0 * len(kh)),
                       (th.cuda.memory_allocated() - base) / (16.0 * len(kh)), len(kh)))
        for rows_name, hh in (("empty lists only %d" % len(no_list), no_list), ("typical rows 1000", heads),
                              ("typical + hub row 1000", with_hub), ("hub row x 128", hub_block)):
            base_ms = None
            for emode in (None, "mask", "exclude"):
                ms = times(lambda: m.link_predict(hh, [top_rel], None, "batch_head", "none", K, emode), reps)
                if emode is None:
                    base_ms = float(np.median(ms))
                say("%-10s %-24s exclude_mode %-9s %s  x%.3f of None" % (model, rows_name, emode, fmt(ms), float(np.median(ms)) / base_ms))
        if model == "DistMult" and not kernels:
            E, R = m.entity_embed, m.relation_embed
            q = (E[th.as_tensor(heads, device=E.device)] * R[top_rel]).contiguous()
            mask = th.zeros(H, N_ENT, dtype=th.bool, device=E.device)
            ms = times(lambda: th.topk((q @ E.T).masked_fill(mask, float("-inf")), K, dim=1), reps)
            say("context: torch matmul + masked_fill + topk on the full 1000 x 14951 block (DistMult form, mask given) %s" % fmt(ms))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# tools/link_predict_timing.py%s (device events around whole Python calls, after one warm-up call)\n"
                 % (" --kernels" if kernels else ""))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
