"""Case table of the subsampling-weight tests (test infrastructure; a plain module, not a conftest): the float64 statement of the
weights, the graphs they are computed on and the geometries of the weighted sampler launch.  Shared by
  tests/test_subsampling_inputs.py   (CPU): holds the table to what the comments say;
  tests/test_gpu_subsampling.py      (GPU): the weighted sampler, kge_subsampling_weights, the step, the loop and the flags.

The weights (dglke_train --subsampling_weight): RotatE's `count_frequency` counts every (h, r) and every (t, r^-1) pair of the
training split with both counters started at 4 - a pair seen n times counts n + 3, a triple present twice counts twice - and
weights a triple by 1 / sqrt(count(h, r) + count(t, r^-1)); this build normalises them to mean 1 over the split.
"""
import numpy as np

N_ENT, N_REL, N_TRIPLES = 300, 5, 3000
LONE_REL, UNUSED_REL = 3, 4             # one relation with a single triple, one relation id without any
TRIPLED = 17                            # index (into the graph) of the triple that is present three times


def counts(h, r, t, n_rel):
    """(n_hr, n_tr) per triple: how many triples of the split share its (h, r), how many its (t, r) - with multiplicity"""
    h, r, t = (np.asarray(x, np.int64) for x in (h, r, t))

    def per_key(key):
        _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        return cnt[inv]
    return per_key(h * n_rel + r), per_key(t * n_rel + r)


def raw_weights64(h, r, t, n_rel):
    """1 / sqrt(n_hr + n_tr + 6) in float64: the + 6 is the start value 4 of both counters (a pair seen n times counts n + 3)"""
    n_hr, n_tr = counts(h, r, t, n_rel)
    return 1.0 / np.sqrt((n_hr + n_tr + 6).astype(np.float64))


def weights64(h, r, t, n_rel):
    """the float64 statement of dataloader.subsampling_weights: the raw weights divided by their mean"""
    raw = raw_weights64(h, r, t, n_rel)
    return raw / raw.mean()


def _zipf_ids(rng, n_ids, n):
    p = 1.0 / (1.0 + np.arange(n_ids))
    return rng.choice(n_ids, size=n, p=p / p.sum()).astype(np.int64)


def graph(n_ent=N_ENT, seed=0):
    """(h, r, t): N_TRIPLES triples over n_ent entities with Zipf-distributed heads and tails (no h == t: TransR's gradient of such
    an edge has no digits to compare, tests/loss_option_cases.py) in relations 0 .. 2, one triple in LONE_REL, none in UNUSED_REL,
    and the triple at index TRIPLED present three times (its two copies are the last two triples)"""
    rng = np.random.RandomState(7100 + seed)
    n = N_TRIPLES - 3
    h, t = _zipf_ids(rng, n_ent, n), _zipf_ids(rng, n_ent, n)
    r = rng.randint(0, 3, size=n).astype(np.int64)
    # the tripled triple: a pair of entities from the tail of the distribution in its own combination, so that it is present
    # exactly three times and a count without multiplicity would give it another weight
    h[TRIPLED], r[TRIPLED], t[TRIPLED] = n_ent - 2, 1, n_ent - 1
    same = h == t
    t[same] = (t[same] + 1) % n_ent
    clash = (h == h[TRIPLED]) & (r == 1) & (t == t[TRIPLED])
    clash[TRIPLED] = False
    t[clash] = 0
    lone = (np.int64(n_ent // 2), np.int64(LONE_REL), np.int64(n_ent // 2 + 1))
    h = np.concatenate([h, [lone[0], h[TRIPLED], h[TRIPLED]]])
    r = np.concatenate([r, [lone[1], r[TRIPLED], r[TRIPLED]]])
    t = np.concatenate([t, [lone[2], t[TRIPLED], t[TRIPLED]]])
    return h, r, t


def weight_graphs():
    """name -> (h, r, t, n_ent, n_rel) of the graphs test 2 computes weights on: the table's graph, one relation only, and ids
    whose keys h * R + r exceed 2^40 (1 500 000 entities x 1 000 000 relations)"""
    h, r, t = graph()
    one = (h, np.zeros_like(r), t, N_ENT, 1)
    big_e, big_r = 1500000, 1000000
    rng = np.random.RandomState(7200)
    sel = rng.randint(big_e - 40, big_e, size=400).astype(np.int64)       # 40 entities at the top of the id range: counts repeat
    bh, bt = sel[:200].copy(), sel[200:].copy()
    br = (big_r - 1 - rng.randint(0, 3, size=200)).astype(np.int64)
    return {"table": (h, r, t, N_ENT, N_REL), "one_relation": one, "keys_above_2^40": (bh, br, bt, big_e, big_r)}


# ---- the weighted sampler launch ----------------------------------------------------------------------------------------------
SP_MAXE, SP_CODE_BITS, SP_CODE_BITS_BIG = 4096, 12, 13        # csrc/kge_sampler_common.hpp

# (id, B, N, n_train, n_ent, slots per launch, the instance the geometry names: (wide, 64-bit keys)); chunk = N, 3 launches each
GEOMETRIES = [
    ("B8-N4-four-epochs", 8, 4, 50, 40, 7, (False, False)),           # 6 whole batches per epoch, 21 batches: epochs 0 .. 3 (re-keying)
    ("B1000-N200", 1000, 200, 2503, 14951, 2, (False, False)),
    ("B2048-N256-wide", 2048, 256, 5123, 14951, 2, (True, False)),
    ("B64-N16-key64", 64, 16, 163, (1 << 20) + 5, 2, (False, True)),
    ("B2048-N256-wide-key64", 2048, 256, 5123, (1 << 19) + 5, 2, (True, True)),      # (the fourth instance; not in the issue's list)
]
N_LAUNCHES = 3


def instance(B, C, N, n_ent):
    """(wide, 64-bit keys): the instance launch_sample_batches picks (csrc/kge_sampler.hip)"""
    wide = 2 * B + C * N > SP_MAXE or B > SP_MAXE // 2
    bits = SP_CODE_BITS_BIG if wide else SP_CODE_BITS
    return wide, n_ent > (1 << (32 - bits))


def al32(x):
    return (x + 31) & ~31


def slot_bytes(B, CN, weighted=False):
    """the slot layout as include/kge_hip.h and DeviceSampler.slot_arrays document it: every array 32-byte aligned, edge_w behind
    counts in a weighted slot only"""
    NE = 2 * B + CN
    o = 0
    for nbytes in (8 * B, 8 * B, 8 * B, 8 * CN, 8 * NE, 8 * B, 4 * (NE + 1), 4 * 2 * B, 4 * (NE + 1), 4 * CN, 4 * (B + 1), 4 * B,
                   32 * NE, 32 * B, 16) + ((4 * B,) if weighted else ()):
        o = al32(o + nbytes)
    return o


def unique_triples(n_train, n_ent, n_rel=3, seed=0):
    """n_train DISTINCT triples (h, r, t) and one distinct float32 weight per triple (exact multiples of 2^-10)"""
    rng = np.random.RandomState(7300 + seed)
    total = n_ent * n_rel * n_ent
    code = np.unique(rng.randint(0, total, size=3 * n_train, dtype=np.int64))
    assert len(code) >= n_train
    code = rng.permutation(code)[:n_train]
    h, rest = code // (n_rel * n_ent), code % (n_rel * n_ent)
    r, t = rest // n_ent, rest % n_ent
    w = ((1 + rng.permutation(n_train)) * 2.0 ** -10).astype(np.float32)
    return h, r, t, w
