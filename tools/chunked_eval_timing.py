"""Chunked-candidate ranking (kge_rank_eval_chunked through Ranker.chunked_ranks) against the host loop it stands beside
(eval.sampled_ranks: one draw, one kge_rank_eval_ex call and - filtered - one eval.filter_columns per chunk), at the shapes of the
reference's large-graph recipes:
  TransE_l2 d 400, chunk 1000, 1000 candidates, 2 500 604 entities     (wikikg2 --neg_sample_size_eval 1000 style)
  ComplEx   d 400, chunk 8 and 16, 500 candidates, 2 500 604 entities  (wikikg2 / biokg: 500 candidates, default and doubled chunk)
  TransE_l2 d 400, chunk 8, 1000 candidates, 14 951 entities, 59 071 triples   (FB15k's test split at the default chunk)
Both paths get the same candidates, one side (tails), raw and filtered; whole calls that end in a synchronise, wall clock, one
warm-up each, then the two paths alternating in one process.  The filter lists are built once outside the timed calls (entity-id
lists on the device for the new entry, the same lists on the host for the loop, as eval.evaluate hands them over).
usage: python tools/chunked_eval_timing.py [--kernels] [--quick] [out.txt]     (default profiles/chunked_eval_timing.txt)
  --kernels  one warm-up + one call of the new entry per case and nothing else: the run to put under
             rocprofv3 --kernel-trace --stats (kernel-only times: profiles/chunked_eval_kernel_stats.txt)
  --quick    a tenth of the triples (a smoke run of the tool itself)"""
import os
import sys
import time

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, ROOT)

BIG = 2500604
#        name                        model        hidden n_ent  n_rel  E      chunk n_cand
CASES = [("wikikg2 TransE_l2 c1000", "TransE_l2", 400, BIG, 535, 20000, 1000, 1000),
         ("wikikg2 ComplEx c8", "ComplEx", 200, BIG, 535, 8000, 8, 500),
         ("wikikg2 ComplEx c16", "ComplEx", 200, BIG, 535, 8000, 16, 500),
         ("FB15k TransE_l2 c8", "TransE_l2", 400, 14951, 1345, 59071, 8, 1000)]
REPS = 3


def wall(fn):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    th.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "chunked_eval_timing.txt")
    kernels, quick = "--kernels" in flags, "--quick" in flags
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import eval as kev
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tables = {}
    for name, model, hidden, n_ent, n_rel, E, chunk, n_cand in CASES:
        if quick:
            E = max(chunk, E // 10)
        d = 2 * hidden if model == "ComplEx" else hidden
        gamma = 19.9
        emb_init = (gamma + 2.0) / hidden
        key = (n_ent, d)
        if key not in tables:
            tables.clear()                                   # one big table at a time
            th.manual_seed(0)
            tables[key] = (th.empty(n_ent, d, device="cuda").uniform_(-emb_init, emb_init),
                           th.empty(n_rel, d, device="cuda").uniform_(-emb_init, emb_init))
        ent, rel = tables[key]
        rng = np.random.RandomState(1)
        n_known = max(600000, 2 * E)
        known = tuple(rng.randint(0, n, n_known) for n in (n_ent, n_rel, n_ent))
        h, r, t = (k[:E].copy() for k in known)
        n_chunks = (E + chunk - 1) // chunk
        cands = rng.randint(0, n_ent, (n_chunks, n_cand)).astype(np.int64)
        rk = kev.Ranker(model, ent, rel, gamma, emb_init, batch=4096)
        fdev = kev.build_filter_device(known, (h, r, t), False, n_rel, n_ent, ent.device)
        fhost = (fdev[0].cpu().numpy(), fdev[1].cpu().numpy())
        say("# %s: %s d %d, %d entities, %d triples in %d chunks of %d, %d candidates per chunk, tails; %d known triples"
            % (name, model, d, n_ent, E, n_chunks, chunk, n_cand, n_known))
        for label, fd, fh_ in (("raw", None, None), ("filtered", fdev, fhost)):
            new = lambda: rk.chunked_ranks(h, r, t, False, chunk, cand=cands, filt=fd)
            old = lambda: kev.sampled_ranks(rk, h, r, t, False, fh_, n_ent, n_cand, chunk, None, cand_of_chunk=lambda k: cands[k])
            if kernels:
                wall(new)
                wall(new)
                continue
            _, a = wall(new)
            _, b = wall(old)
            diff = int((a != b).sum())
            tn, to = [], []
            for _ in range(REPS):
                tn.append(wall(new)[0])
                to.append(wall(old)[0])
            mn, mo = float(np.median(tn)), float(np.median(to))
            say("%-26s %-8s one call %9.2f ms (min %9.2f max %9.2f)   host loop %10.2f ms (min %10.2f max %10.2f)   loop / call %7.1fx   "
                "ranks differing %d of %d" % (name, label, mn * 1e3, min(tn) * 1e3, max(tn) * 1e3, mo * 1e3, min(to) * 1e3, max(to) * 1e3,
                                              mo / mn, diff, E))
            if mn >= mo:
                say("  NOT FASTER: the single call takes %.2f x the loop's time at this shape" % (mn / mo))
    if not kernels:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("# tools/chunked_eval_timing.py%s: wall clock of whole calls ending in a synchronise, 1 warm-up + %d alternating repetitions, "
                     "medians\n" % (" --quick" if quick else "", REPS))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
