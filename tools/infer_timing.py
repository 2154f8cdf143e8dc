"""Device time of the inference path (dglke_amd/infer.py -> csrc/kge_topk.hip) at FB15k's and wikikg2's shapes, with
kge_rank_eval's GEMM and torch matmul + topk in the same process as yardsticks (context only: they are not the product).
One GPU call; device events around each case after a warm-up.
usage: python tools/infer_timing.py [--fb15k] [out.txt]   (stdout + the file, default profiles/infer_timing.txt)
  --fb15k: only the seven FB15k-shaped predict cases - the run to put under
           rocprofv3 --kernel-trace --stats --output-format csv (kernel-only times: profiles/infer_kernel_stats.txt)"""
import os
import sys
import tempfile

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, ROOT)

PEAK_TF = 157.3           # fp32 MFMA peak of the MI355X, TFLOP/s


def timed(fn, reps=3):
    fn()
    th.cuda.synchronize()
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) / reps / 1e3


def main():
    from dglke_amd import eval as E
    from dglke_amd.infer import EmbSimInfer, ScoreInfer
    argv = [a for a in sys.argv[1:] if a != "--fb15k"]
    fb_only = "--fb15k" in sys.argv
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "infer_timing.txt")
    lines = []

    def row(name, sec, scores, flops=None):
        s = "%-58s %9.3f ms  %9.3e scores/s" % (name, sec * 1e3, scores / sec)
        if flops:
            s += "  %6.1f TFLOP/s (%4.1f %% of fp32 MFMA peak)" % (flops / sec / 1e12, 100 * flops / sec / 1e12 / PEAK_TF)
        print(s, flush=True)
        lines.append(s)

    rng = np.random.RandomState(0)
    n_ent, H, K = 14951, 1000, 10
    tmp = tempfile.mkdtemp()
    for model in ("TransE_l2", "DistMult", "ComplEx", "SimplE", "RESCAL", "TransE_l1", "RotatE"):
        hidden = {"ComplEx": 200, "SimplE": 200, "RotatE": 200, "RESCAL": 64}.get(model, 400)
        d_e = hidden * (2 if model in ("ComplEx", "SimplE", "RotatE") else 1)
        d_r = hidden * hidden if model == "RESCAL" else (d_e if model != "RotatE" else hidden)
        ent = rng.uniform(-0.1, 0.1, (n_ent, d_e)).astype(np.float32)
        rel = rng.uniform(-0.1, 0.1, (4, d_r)).astype(np.float32)
        np.save(os.path.join(tmp, "fb_%s_entity.npy" % model), ent)
        np.save(os.path.join(tmp, "fb_%s_relation.npy" % model), rel)
        cfg = {"model_name": model, "dataset": "fb", "hidden_dim": hidden, "gamma": 12.0, "double_ent": d_e > hidden,
               "double_rel": model in ("ComplEx", "SimplE")}
        m = ScoreInfer(0, cfg, tmp, "none")
        m.load_model()
        h = rng.randint(0, n_ent, H)
        sec = timed(lambda: m.topK(h, [1], None, "batch_head", K))
        gemm = model not in ("TransE_l1", "RotatE")
        row("predict h_r_* batch_head %s 1000x14951 d%d K%d" % (model, d_e, K), sec, H * n_ent,
            2.0 * H * n_ent * d_e if gemm else None)
        if model == "TransE_l2" and not fb_only:
            # yardstick: kge_rank_eval's GEMM (mask-bit epilogue) at 1024 x 14 951 x 400, unfiltered, tail side
            ent_t, rel_t = m.ent, m.rel
            rk = E.Ranker("TransE_l2", ent_t, rel_t, 12.0, 14.0 / hidden, 1024)
            tri = [th.as_tensor(rng.randint(0, n, 1024), device="cuda:0") for n in (n_ent, 4, n_ent)]
            sec_r = timed(lambda: rk.ranks(tri[0], tri[1], tri[2], False))
            row("yardstick: kge_rank_eval TransE_l2 1024x14951 d400", sec_r, 1024 * n_ent, 2.0 * 1024 * n_ent * d_e)
            q = (ent_t[th.as_tensor(h, device="cuda:0")] + rel_t[1]).contiguous()
            sec_t = timed(lambda: th.topk(q @ ent_t.T, K, dim=1))
            row("yardstick: torch matmul + topk (DistMult form) 1000x14951", sec_t, H * n_ent, 2.0 * H * n_ent * d_e)
    if fb_only:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    emb = rng.uniform(-1, 1, (n_ent, 400)).astype(np.float32)
    f = os.path.join(tmp, "emb.npy")
    np.save(f, emb)
    for sim in ("cosine", "l2", "l1"):
        e = EmbSimInfer(0, f, sim)
        e.load_emb()
        sec = timed(lambda: e.topK(None, None, bcast=True, k=K), reps=1)
        row("emb_sim * batch_left %s 14951x14951 d400 K%d" % (sim, K), sec, n_ent * n_ent,
            2.0 * n_ent * n_ent * 400 if sim != "l1" else None)
    big = th.empty(2500604, 400, dtype=th.float32, device="cuda:0").uniform_(-1, 1)
    e = EmbSimInfer(0, f, "cosine")
    e.emb = big
    left = np.arange(4096)
    sec = timed(lambda: e.topK(left, None, bcast=True, k=K), reps=1)
    row("emb_sim l_* batch_left cosine 4096x2500604 d400 K%d" % K, sec, 4096 * 2500604, 2.0 * 4096 * 2500604 * 400)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# tools/infer_timing.py (device events, after one warm-up call; the whole Python call incl. id lists)\n")
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
