"""Relation ranking (kge_rank_rel_eval through Ranker.relation_ranks) against the route a user had before it: a host loop of one
kge_score_pos call per relation (the relation's row expanded over the triples) plus a torch compare against the positive scores
and a dense [triples, relations] "listed" mask.  FB15k-shaped random tables: 14 951 entities, 1 345 relations, d 400, 59 071 test
triples, filtered against 592 213 random known triples (random pairs repeat far less than FB15k's, so the lists are short).
RESCAL is timed at d 64 and TransR at d 200, both with 4 096 triples: they cost d_e * d_r multiply-adds per (triple, relation).
kge_score_pos refuses TransR, which is timed on its own.
Whole calls between two events on the stream, one warm-up each, then REPS alternating repetitions, medians.
usage: python tools/relation_rank_timing.py [--kernels] [--quick] [out.txt]     (default profiles/relation_rank_timing.txt)
  --kernels  one warm-up + one call of the new entry per model and nothing else: the run to put under
             rocprofv3 --kernel-trace --stats (profiles/relation_rank_kernel_stats.txt)
  --quick    a tenth of the triples and relations (a smoke run of the tool itself)"""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, ROOT)

N_ENT, N_REL, N_KNOWN = 14951, 1345, 592213
#        model        hidden  triples
CASES = [("TransE_l1", 400, 59071), ("TransE_l2", 400, 59071), ("DistMult", 400, 59071), ("ComplEx", 200, 59071),
         ("RotatE", 200, 59071), ("SimplE", 200, 59071), ("RESCAL", 64, 4096), ("TransR", 200, 4096)]
REPS = 3


def timed(fn):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    th.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def host_loop(model_id, ent, rel, h, r, t, gamma, emb_init, listed):
    """rank = 1 + #{j not listed : s(h, j, t) >= s(h, r, t)}, one kge_score_pos call per relation"""
    from dglke_amd import _lib
    L = _lib.lib()
    H, T = ent[h].contiguous(), ent[t].contiguous()
    E, d_e, d_r = H.shape[0], ent.shape[1], rel.shape[1]
    p, s = th.empty(E, device=ent.device), th.empty(E, device=ent.device)
    _lib.check(L.kge_score_pos(model_id, _lib.ptr(H), _lib.ptr(rel[r].contiguous()), _lib.ptr(T), E, d_e, d_r, gamma, emb_init,
                               _lib.ptr(p), _lib.stream_ptr()))
    cnt = th.zeros(E, dtype=th.int32, device=ent.device)
    for j in range(rel.shape[0]):
        R = rel[j].expand(E, d_r).contiguous()
        _lib.check(L.kge_score_pos(model_id, _lib.ptr(H), _lib.ptr(R), _lib.ptr(T), E, d_e, d_r, gamma, emb_init, _lib.ptr(s),
                                   _lib.stream_ptr()))
        cnt += ((s >= p) & ~listed[:, j]).to(th.int32)
    return cnt + 1


def main():
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "relation_rank_timing.txt")
    kernels, quick = "--kernels" in flags, "--quick" in flags
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib
    from dglke_amd import eval as kev
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n_rel = N_REL // 10 if quick else N_REL
    dev = th.device("cuda")
    say("# %s, %d entities, %d relations, filtered against %d random known triples + the test triples"
        % (th.cuda.get_device_name(0), N_ENT, n_rel, N_KNOWN))
    for model, hidden, E in CASES:
        if quick:
            E = max(64, E // 10)
        d_e = 2 * hidden if model in ("ComplEx", "SimplE", "RotatE") else hidden
        d_r = hidden if model == "RotatE" else hidden * hidden if model == "RESCAL" else d_e
        gamma = 19.9
        emb_init = (gamma + 2.0) / hidden
        th.manual_seed(0)
        ent = th.empty(N_ENT, d_e, device=dev).uniform_(-emb_init, emb_init)
        rel = th.empty(n_rel, d_r, device=dev).uniform_(-emb_init, emb_init)
        proj = th.empty(n_rel, d_e * d_r, device=dev).uniform_(-0.3, 0.3) if model == "TransR" else None
        rng = np.random.RandomState(1)
        known = tuple(rng.randint(0, n, N_KNOWN) for n in (N_ENT, n_rel, N_ENT))
        h, r, t = (th.as_tensor(k[:E].copy()).to(dev) for k in known)
        filt = kev.build_relation_filter(tuple(k[E:] for k in known), (h, r, t), N_ENT, n_rel, dev)
        rk = kev.Ranker(model, ent, rel, gamma, emb_init, batch=4096, proj=proj)
        new = lambda: rk.relation_ranks(h, r, t, filt)
        if kernels:
            timed(new)
            timed(new)
            continue
        _, a = timed(new)
        tn = [timed(new)[0] for _ in range(REPS)] if model == "TransR" else []
        if model == "TransR":
            say("%-10s d_e %4d d_r %6d %6d triples  one call %9.2f ms (min %9.2f max %9.2f)   host loop: kge_score_pos refuses TransR"
                % (model, d_e, d_r, E, float(np.median(tn)) * 1e3, min(tn) * 1e3, max(tn) * 1e3))
            continue
        # the dense listed mask of the loop, built once outside the timed calls like the lists of the new entry
        frng, fids = filt
        listed = th.zeros(E, n_rel, dtype=th.bool, device=dev)
        lens = frng[:, 1] - frng[:, 0]
        rows = th.repeat_interleave(th.arange(E, device=dev), lens)
        offs = th.arange(int(lens.sum()), device=dev) - th.repeat_interleave(th.cumsum(lens, 0) - lens, lens)
        listed[rows, fids[th.repeat_interleave(frng[:, 0], lens) + offs]] = True
        mid = _lib.model_id(model)
        old = lambda: host_loop(mid, ent, rel, h, r, t, gamma, emb_init, listed)
        _, b = timed(old)
        diff = int((a != b).sum())
        to = []
        for _ in range(REPS):
            tn.append(timed(new)[0])
            to.append(timed(old)[0])
        mn, mo = float(np.median(tn)), float(np.median(to))
        say("%-10s d_e %4d d_r %6d %6d triples  one call %9.2f ms (min %9.2f max %9.2f)   host loop %10.2f ms (min %10.2f max %10.2f)   "
            "loop / call %7.1fx   ranks differing %d of %d" % (model, d_e, d_r, E, mn * 1e3, min(tn) * 1e3, max(tn) * 1e3, mo * 1e3,
                                                              min(to) * 1e3, max(to) * 1e3, mo / mn, diff, E))
        if mn >= mo:
            say("  NOT FASTER: the single call takes %.2f x the loop's time at this shape" % (mn / mo))
        del listed
    if not kernels:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("# tools/relation_rank_timing.py%s: whole calls between two stream events, 1 warm-up + %d alternating repetitions, "
                     "medians\n" % (" --quick" if quick else "", REPS))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
