"""CPU guard of tests/test_gpu_sampler_statement.py: the statement of the device sampler's ids (tests/sampler_statement.py) is not a copy
of a mistake - it meets a published test vector, big-integer arithmetic and the properties the epoch order needs - and the RNG it
states is uniform, serially uncorrelated and free of overlapping streams, at sample sizes no GPU test could afford.  The GPU file
pins the kernels to the statement bit for bit, so what holds here holds for the kernels.

Seeds are fixed (0, 1, 3, 12345): nothing here is random from run to run.  The bounds are those of the distributions (chi-square,
the correlation coefficient of independent pairs, the binomial), not measured margins; what these seeds gave stands next to each.

`python tests/test_sampler_statement_inputs.py` rewrites profiles/sampler_epoch_cobatch.txt (see cobatch_report).
"""
import math
import os
import random

import numpy as np
import pytest

import sampler_statement as S

SEEDS = (0, 1, 3, 12345)
EPOCHS = (0, 1, 2, 7, 8, 9, 10 ** 6, 1 << 40)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COBATCH_FILE = os.path.join(ROOT, "profiles", "sampler_epoch_cobatch.txt")


# ---- the hashes -----------------------------------------------------------------------------------------------------------------
def test_mix64_meets_the_published_vector():
    """splitmix64 seeded with 0: the state advances by GOLD and is finalised - its first output is 0xE220A8397B1DCDAF"""
    assert S.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert S.mix64(0) == 0
    x = [0, 1, S.GOLD, S.M64, 1 << 63, 0x123456789ABCDEF]
    assert [int(v) for v in S.mix64_np(np.array(x, np.uint64))] == [S.mix64(v) for v in x]
    rng = random.Random(1)
    x = [rng.getrandbits(64) for _ in range(1000)]
    assert [int(v) for v in S.mix64_np(np.array(x, np.uint64))] == [S.mix64(v) for v in x]


@pytest.mark.parametrize("n_ent", [1, 9, 14951, 86054151, (1 << 40) + 7, (1 << 51) - 1])
def test_umulhi_by_halves_equals_big_integers(n_ent):
    rng = random.Random(n_ent)
    x = [0, 1, S.M64, S.M64 - 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63] + [rng.getrandbits(64) for _ in range(5000)]
    got = S.umulhi_np(np.array(x, np.uint64), n_ent)
    assert [int(v) for v in got] == [(v * n_ent) >> 64 for v in x]
    assert int(got.max()) < n_ent
    for seed in SEEDS:                                       # and the whole chain, vectorised against Python integers
        ids = S.negative_ids(seed, 7, 50, n_ent)
        key = S.mix64(seed ^ (7 * S.GOLD & S.M64))
        assert ids.tolist() == [S.umulhi(S.mix64(key + j), n_ent) for j in range(50)]


def test_negative_ids_take_the_whole_seed_and_step():
    """bit 63 of the seed and the bits of the step beyond 2^32 reach the ids"""
    for seed in SEEDS:
        a = S.negative_ids(seed, 5, 100, 14951)
        assert not np.array_equal(a, S.negative_ids(seed | 1 << 63, 5, 100, 14951))
        assert not np.array_equal(a, S.negative_ids(seed, 5 + (1 << 32), 100, 14951))
        assert not np.array_equal(a, S.negative_ids(seed, 6, 100, 14951))


# ---- the epoch order ------------------------------------------------------------------------------------------------------------
BIJECTION_N = (1, 2, 3, 64, 4096, 30030)
GCD_N = (483142, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 15, 3 << 33, (1 << 62) + 57)


@pytest.mark.parametrize("n", BIJECTION_N + GCD_N)
def test_epoch_affine_is_a_bijection(n):
    for seed in SEEDS:
        for ep in EPOCHS:
            mul, add = S.epoch_affine(seed, ep, n)
            if ep == 0:
                assert (mul, add) == (1, 0)
                continue
            assert math.gcd(mul, n) == 1 and 0 <= add < n and mul >= 3 and mul & 1, (seed, ep, mul, add)
            assert mul < (1 << 32) + 2 * 64 if n < (1 << 32) else mul < n + 2 * 64      # (the search moves a few steps at the most)
            assert S.epoch_affine(seed, ep, n, shuffled=False) == (1, 0)
            if n in BIJECTION_N:
                assert sorted(S.epoch_index(p, mul, add, n) for p in range(n)) == list(range(n)), (seed, ep)


def test_epochs_differ_in_both_constants():
    """the multiplier's key is epoch + 1, the offset's the epoch: no two of the test epochs share either"""
    for n in (483142, (1 << 32) + 15):
        for seed in SEEDS:
            c = [S.epoch_affine(seed, ep, n) for ep in EPOCHS[1:]]
            assert len({m for m, _ in c}) == len(c) and len({a for _, a in c}) == len(c)
            assert all(S.epoch_affine(seed, ep, n) != S.epoch_affine(seed + 1, ep, n) for ep in EPOCHS[1:])


def test_reciprocal_remainder_is_exact_with_at_most_two_subtractions():
    rng = random.Random(3)
    ns = [(1 << 32) - 1, (1 << 32) - 5, (1 << 31) + 11, 483142, 3, 1] + [rng.randrange(1, 1 << 32) for _ in range(2000)]
    worst = 0
    for n in ns:
        rinv = S.reciprocal(n)
        for k in range(50):
            pos, add = rng.randrange(n), rng.randrange(n)
            mul = (rng.getrandbits(32) | 1) if k else (1 << 32) - 1
            if k == 1:
                pos, add = n - 1, n - 1
            x = pos * mul + add
            assert x < 1 << 64
            r, subs = S.reciprocal_remainder(x, n, rinv)
            assert r == x % n and subs <= 2, (n, pos, mul, add, r, subs)
            worst = max(worst, subs)
    assert worst >= 1                                        # (the correction is needed: the estimate alone is not the remainder)


# ---- the quality of the negatives -----------------------------------------------------------------------------------------------
STEPS, CN = 400, 1000
_DRAWS = {}


def _draws(seed, n_ent):
    """[STEPS, CN] ids of steps 1 .. STEPS, computed once"""
    if (seed, n_ent) not in _DRAWS:
        _DRAWS[(seed, n_ent)] = np.stack([S.negative_ids(seed, s, CN, n_ent) for s in range(1, STEPS + 1)])
    return _DRAWS[(seed, n_ent)]


@pytest.mark.parametrize("n_ent,bins", [(50, 50), (14951, 14951), (1000003, 1000)])
@pytest.mark.parametrize("seed", SEEDS)
def test_negatives_are_uniform(seed, n_ent, bins):
    """chi-square of 400 000 draws over `bins` cells of (almost) equal size: |chi^2 - df| / sqrt(2 df) < 4, a two-sided tail of about
    6e-5 of the chi-square distribution at these degrees of freedom.  These seeds: within +-1.8"""
    ids = _draws(seed, n_ent).reshape(-1)
    cell = ids * bins // n_ent
    size = np.bincount(np.arange(n_ent, dtype=np.int64) * bins // n_ent, minlength=bins)      # ids per cell: differ by one at the most
    expected = size * (ids.size / float(n_ent))
    observed = np.bincount(cell, minlength=bins)
    chi2, df = float(((observed - expected) ** 2 / expected).sum()), bins - 1
    z = (chi2 - df) / math.sqrt(2 * df)
    print("seed %d n_ent %d: chi^2 %.1f, df %d, z %+.2f" % (seed, n_ent, chi2, df, z))
    assert abs(z) < 4, (chi2, df, z)


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("n_ent", [50, 14951, 1000003])
@pytest.mark.parametrize("seed", SEEDS)
def test_negatives_are_serially_uncorrelated(seed, n_ent):
    """the correlation coefficient of id / n_ent between slots j and j + 1 of a step (399 600 pairs) and between steps s and s + 1 at
    the same slot (399 000 pairs): |r| < 5 / sqrt(pairs) - r of independent pairs has standard deviation 1 / sqrt(pairs).
    These seeds: 0.0040 at the worst, the bound is 0.0079"""
    u = _draws(seed, n_ent) / float(n_ent)
    for what, a, b in (("slots", u[:, :-1], u[:, 1:]), ("steps", u[:-1], u[1:])):
        r = _corr(a.reshape(-1), b.reshape(-1))
        print("seed %d n_ent %d %s: r %+.5f over %d pairs" % (seed, n_ent, what, r, a.size))
        assert abs(r) < 5 / math.sqrt(a.size), (what, r)


@pytest.mark.parametrize("n_ent", [50, 14951, 1000003])
@pytest.mark.parametrize("seed", SEEDS)
def test_consecutive_steps_repeat_an_id_at_a_slot_as_often_as_chance(seed, n_ent):
    """equal ids at the same slot of consecutive steps: a fraction within 5 binomial standard deviations of 1 / n_ent"""
    d = _draws(seed, n_ent)
    pairs, p = d[:-1].size, 1.0 / n_ent
    frac = float((d[:-1] == d[1:]).sum()) / pairs
    sd = math.sqrt(p * (1 - p) / pairs)
    print("seed %d n_ent %d: %.3g against %.3g (sd %.2g)" % (seed, n_ent, frac, p, sd))
    assert abs(frac - p) < 5 * sd, (frac, p, sd)


@pytest.mark.parametrize("base", SEEDS)
def test_lane_streams_do_not_overlap(base):
    """trainer lane k samples with seed base + 1000 k (dglke_amd/train.py); slot j of a step hashes key + j with
    key = mix64(seed ^ step * GOLD).  Over 8 lanes and 2 000 000 steps the 16 M keys are distinct: no two (lane, step) pairs draw the
    same negatives.  With dglke_train's default --seed 0 they are, sorted, more than 8192 apart (a batch has at most 8192 slots): no
    two streams are shifted windows of one another.  Smallest gap: 204 902 (base 0), 4 744 (1), 38 015 (3), 88 946 (12345).

    The gap is a property of the seed, not of the construction: 16 M uniform 64-bit values lie 2^64 / (16 M)^2 = 72 000 apart at the
    closest on average, so a gap of 8192 or less turns up for about one base seed in nine - as it does for base 1, where one pair of
    (lane, step) streams would share its ids from slot 4 744 on if a step drew that many negatives (the recipes draw 256 to 4 096).
    That is measured and printed, not asserted: distinct keys are what a good hash guarantees (a collision has probability 7e-6
    per base seed), and keys further apart than a batch would need another construction than key + j, which changes every batch."""
    steps = np.arange(1, 2 * 10 ** 6 + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        walk = steps * np.uint64(S.GOLD)
    keys = np.sort(np.concatenate([S.mix64_np(np.uint64(base + 1000 * k) ^ walk) for k in range(8)]))
    gap = int(np.diff(keys).min())
    print("base %d: smallest gap %d" % (base, gap))
    assert keys.size == 16 * 10 ** 6 and gap > 0, "two (lane, step) pairs share a key"
    if base == 0:
        assert gap > 8192, gap
    assert S.step_key(base + 3000, 77) == int(S.mix64_np(np.uint64(base + 3000) ^ walk[76:77])[0])


# ---- the GPU test's own cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.CASES + S.TAIL_CASES[-1:], ids=lambda c: c["id"])
def test_the_gpu_cases_reach_what_they_are_for(c):
    """every geometry multiplies an edge position by a multiplier beyond 2^32 (a 32-bit product would differ) or says why it cannot;
    entity ids beyond 2^32 occur among the triples of every case whose n_ent allows them; every case crosses an epoch boundary"""
    H, R, T, W = S.triples(c)
    B, n = c["B"], c["n_train"]
    assert len(H) == n >= B and B % c["chunk"] == 0 and int(H.max()) < c["n_ent"] and int(R.max()) < c["n_rel"]
    assert (W is not None) == c["weighted"] and (W is None or float(W.min()) > 0)
    steps = [s for tail in ((False, True) if c["tail"] else (False,)) for s0, k, _ in S.steps_of(c, tail) for s in range(s0, s0 + k)]
    epochs = {S.step_position(s, B, n)[1] for s in steps}
    assert len(epochs) > 1, "no epoch boundary"
    widest = 0
    for s in steps:
        _, ep, pos1 = S.step_position(s, B, n)
        mul, _ = S.epoch_affine(c["seed"], ep, n, c["shuffle"])
        widest = max(widest, (pos1 + B - 1) * mul)
    if c["no_wide_product"] is None:
        assert widest >= 1 << 32, widest
    else:
        assert widest < 1 << 32 and c["no_wide_product"].strip()
    if c["n_ent"] > 1 << 32:
        hi = np.concatenate([H, T]) >> 32
        assert int((hi > 0).sum()) > n and int(S.negative_ids(c["seed"], c["step0"], 64, c["n_ent"]).max()) >> 32 > 0
    if c["id"] == "wide":
        assert 2 * B + (B // c["chunk"]) * c["N"] > 4096
    if c["id"] == "far":
        assert min(steps) > 1 << 32 and min(epochs) > 1 << 32
    if c["id"] == "every-step-an-epoch":
        assert n // B == 1
    if c["id"] == "no-trailing":
        assert n % B == 0 and c["seed"] >> 63 == 1


def test_state_after():
    assert S.state_after(0, 1, 5, 1000, 3017) == (5000 % 3017, 6, 0)
    assert S.state_after(3000, 10 ** 12 + 1, 3, 256, 769) == ((3000 + 768) % 769, 10 ** 12 + 4, 0)


# ---- measured, not asserted: how much two epochs' batches share -----------------------------------------------------------------
def _shared_pairs(b1, b2, nb):
    """edge pairs that share a batch in both of two epochs, from every edge's batch number in each"""
    c = np.bincount(b1 * nb + b2)
    return int((c * (c - 1) // 2).sum())


def cobatch_report(seeds=(0, 5, 11), n_train=40000, B=200, n_epochs=10):
    """The per-epoch order is an affine map of ONE base permutation, so two epochs are far from independent shuffles: an edge pair
    at distance d in the base order is at distance d * mul1 in one epoch and d * mul2 in the other, and small multiples stay inside a
    batch in both.  The count of edge pairs co-batched in both epochs, for every pair of the first `n_epochs` epochs, next to what
    independent uniform shuffles give (numpy) and their expectation.  A record, without a threshold: replacing the permutation scheme
    changes every sampled batch."""
    nb = n_train // B
    expect = nb * (B * (B - 1) // 2) * (B - 1) / float(n_train - 1)
    lines = ["edge pairs co-batched in BOTH of two epochs: n_train %d, B %d (%d batches), epochs 0..%d, every pair of epochs" % (n_train, B, nb, n_epochs - 1),
             "independent uniform shuffles, expectation: %.0f" % expect]
    pos = np.arange(n_train, dtype=np.int64)
    for seed in seeds:
        label = []
        for ep in range(n_epochs):
            mul, add = S.epoch_affine(seed, ep, n_train)
            at = np.empty(n_train, np.int64)
            at[(pos * mul + add) % n_train] = pos                # position of every base-order edge in this epoch (mul < 2^32)
            label.append(at // B)
        affine = sorted(_shared_pairs(label[a], label[b], nb) for a in range(n_epochs) for b in range(a + 1, n_epochs))
        rs = np.random.RandomState(seed)
        shuf = [np.argsort(rs.permutation(n_train)) // B for _ in range(n_epochs)]
        uniform = sorted(_shared_pairs(shuf[a], shuf[b], nb) for a in range(n_epochs) for b in range(a + 1, n_epochs))
        lines.append("seed %2d  affine epochs: min %d  median %d  mean %.0f (%.2fx)  max %d (%.1fx)   numpy shuffles: min %d  mean %.0f  max %d"
                     % (seed, affine[0], affine[len(affine) // 2], np.mean(affine), np.mean(affine) / expect, affine[-1], affine[-1] / expect,
                        uniform[0], np.mean(uniform), uniform[-1]))
    return "\n".join(lines) + "\n"


def test_the_cobatch_record_is_what_the_statement_gives():
    """profiles/sampler_epoch_cobatch.txt is this file's measurement (no bound on the figures themselves)"""
    assert open(COBATCH_FILE).read() == cobatch_report()


if __name__ == "__main__":
    with open(COBATCH_FILE, "w") as f:
        f.write(cobatch_report())
    print(open(COBATCH_FILE).read())
