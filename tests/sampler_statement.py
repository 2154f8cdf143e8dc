"""The device sampler's choice of ids, restated in Python integers and numpy uint64 from DESIGN.md (section 3.3, the sampler row of
section 3.2) and the comments of csrc/kge_sampler_common.hpp / kge_sampler_kernel.hpp.  It neither imports nor calls the library:
tests/test_gpu_sampler_statement.py pins the kernels to it bit for bit, tests/test_sampler_statement_inputs.py (CPU) checks the
statement itself against published values and big-integer arithmetic and tests the quality of the RNG on it.

  negative j of step s   umulhi(mix64(mix64(seed ^ s * GOLD) + j), n_ent)                 (counter-based: no state but the step number)
  edge i of step s       perm[((pos1 + i) * mul + add) mod n_train],  nb = n_train // B whole batches per epoch,
                         ep = (s - 1) // nb,  pos1 = ((s - 1) mod nb) * B,  (mul, add) hashed from (seed, ep); epoch 0 and a sampler
                         without a base permutation: (1, 0)
  corrupted side         tails on odd steps, heads on even steps

All arithmetic is modulo 2^64 where the device's is (the hashes), and exact where the device's must be ((pos * mul + add) mod n).
The plan arrays are not restated: dglke_amd.plan.build_plan is their host statement.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15            # 2^64 / golden ratio: the step's stride in the negatives' key
HASH_ADD = 0xD6E8FEB86659FD93        # the epoch's stride in the key of the affine map's offset ...
HASH_MUL = 0xA0761D6478BD642F        # ... and (epoch + 1)'s in the key of its multiplier


# ---- hashes ---------------------------------------------------------------------------------------------------------------------
def mix64(x):
    """the splitmix64 finaliser on a Python int (modulo 2^64)"""
    x &= M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x


def mix64_np(x):
    """the same on a numpy uint64 array (unsigned products wrap)"""
    x = np.asarray(x, np.uint64).copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def umulhi(x, n):
    """the high 64 bits of the 128-bit product (Python ints)"""
    return (x * n) >> 64


def umulhi_np(x, n):
    """the same for a uint64 array x and one integer n < 2^64, by 32-bit halves (no partial sum reaches 2^64)"""
    x = np.asarray(x, np.uint64)
    lo32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    xl, xh = x & lo32, x >> s32
    nl, nh = np.uint64(n & 0xFFFFFFFF), np.uint64(n >> 32)
    ll, lh, hl, hh = xl * nl, xl * nh, xh * nl, xh * nh
    mid = (ll >> s32) + (lh & lo32) + (hl & lo32)
    return hh + (lh >> s32) + (hl >> s32) + (mid >> s32)


def step_key(seed, step):
    """the key of a step's negatives: slot j hashes key + j"""
    return mix64((seed & M64) ^ (step * GOLD & M64))


def negative_ids(seed, step, CN, n_ent):
    """the CN uniform ids of [0, n_ent) of 1-based step `step`, int64"""
    with np.errstate(over="ignore"):
        x = mix64_np(np.uint64(step_key(seed, step)) + np.arange(CN, dtype=np.uint64))
    return umulhi_np(x, n_ent).astype(np.int64)


# ---- the epoch order ------------------------------------------------------------------------------------------------------------
def epoch_affine(seed, ep, n_train, shuffled=True):
    """(mul, add) of epoch `ep`: gcd(mul, n_train) = 1, add < n_train.  Below 2^32 triples the multiplier keeps 32 bits of its hash
    (pos * mul + add then fits 64 bits), from there on it is the hash modulo n_train; made odd, at least 3, then raised by 2 until
    it is coprime to n_train"""
    if not shuffled or ep <= 0:
        return 1, 0
    n, seed = int(n_train), seed & M64
    add = mix64(seed ^ (HASH_ADD * ep & M64)) % n
    m = mix64(seed ^ (HASH_MUL * (ep + 1) & M64))
    m = m & 0xFFFFFFFF if n < (1 << 32) else m % n
    m |= 1
    if m < 3:
        m = 3
    while math.gcd(m, n) != 1:
        m += 2
    return m, add


def epoch_index(pos, mul, add, n_train):
    return (pos * mul + add) % n_train


def reciprocal(n_train):
    """what the tail jobs cache next to (mul, add): floor((2^64 - 1) / n_train)"""
    return M64 // n_train


def reciprocal_remainder(x, n, rinv=None):
    """x mod n for x < 2^64 the way the tail jobs take it (n < 2^32): the quotient estimated with the cached reciprocal, then
    corrected; -> (remainder, corrective subtractions)"""
    rinv = reciprocal(n) if rinv is None else rinv
    r = x - ((x * rinv) >> 64) * n
    k = 0
    while r >= n:
        r -= n
        k += 1
    return r, k


def epoch_consts(seed, ep, n_train, shuffled=True):
    """state[5..7] of a sampler whose state[4] is `ep`"""
    mul, add = epoch_affine(seed, ep, n_train, shuffled)
    return mul, add, reciprocal(n_train)


def step_position(step, B, n_train):
    """(batches per epoch, epoch, position of the batch's first edge in its epoch) of 1-based step `step`"""
    nb = n_train // B
    return nb, (step - 1) // nb, ((step - 1) % nb) * B


def edge_indices(seed, step, B, n_train, perm=None):
    """the B training-triple indices of step `step`, int64; perm: the base permutation or None (a sampler that does not shuffle)"""
    _, ep, pos1 = step_position(step, B, n_train)
    mul, add = epoch_affine(seed, ep, n_train, perm is not None)
    idx = np.array([epoch_index(pos1 + i, mul, add, n_train) for i in range(B)], np.int64)
    return idx if perm is None else np.asarray(perm, np.int64)[idx]


def batch_ids(H, R, T, perm, W, n_ent, B, N, chunk, seed, step):
    """the ids of 1-based step `step`: h_gid, t_gid, rel_ids [B], neg_ids [(B / chunk) * N], edge_w [B] (None without weights W) and
    neg_head"""
    e = edge_indices(seed, step, B, len(H), perm)
    return dict(h_gid=np.asarray(H, np.int64)[e], t_gid=np.asarray(T, np.int64)[e], rel_ids=np.asarray(R, np.int64)[e],
                neg_ids=negative_ids(seed, step, (B // chunk) * N, n_ent), edge_w=None if W is None else np.asarray(W, np.float32)[e],
                neg_head=step % 2 == 0, edges=e)


def state_after(pos, step, n, B, n_train):
    """state[0..2] = {position, next step, ticket} after a launch (or a group of tail jobs) of n batches"""
    return (pos + n * B) % n_train, step + n, 0


# ---- the geometries of tests/test_gpu_sampler_statement.py -----------------------------------------------------------------------
# launches: [(batches, first slot)]; tail: this geometry also runs as tail jobs (three groups of three); no_wide_product: why no edge
# position times the multiplier passes 2^32 in this case (None: one does - tests/test_sampler_statement_inputs.py checks either)
def _case(name, n_ent, n_rel, B, N, chunk, n_train, seed, launches, shuffle=True, step0=1, weighted=False, tail=False, no_wide_product=None):
    return dict(id=name, n_ent=n_ent, n_rel=n_rel, B=B, N=N, chunk=chunk, n_train=n_train, seed=seed, launches=launches, shuffle=shuffle,
                step0=step0, weighted=weighted, tail=tail, no_wide_product=no_wide_product)


_CFGT = (14951, 1345, 1000, 200, 200, 3 * 1000 + 17, 3, [(2, 0), (3, 1), (1, 0), (4, 0)])
_HI = ((1 << 40) + 7, 14824, 1024, 256, 256, 2 * 1024 + 9, 3, [(2, 0), (2, 0)])
_SMALL = (3000, 30, 256, 64, 64, 3 * 256 + 1, 9)
IDENTITY_WHY = "a sampler that does not shuffle: mul = 1 in every epoch, and positions stay below n_train = 769"
CASES = [
    _case("cfgT", *_CFGT, tail=True),                                          # two epoch boundaries, one inside a launch
    _case("every-step-an-epoch", 9, 2, 16, 4, 4, 16, 0, [(3, 0), (3, 0), (2, 0)], tail=True),              # nb = 1
    _case("no-trailing", 500, 7, 120, 24, 40, 2 * 120, (1 << 63) + 5, [(3, 0), (3, 0)], tail=True),      # n_train % B == 0, seed bit 63
    _case("hi-ids", *_HI),                                                     # 64-bit keys, the high id word of ue_rec
    _case("wide", 40943, 18, 2048, 256, 256, 2 * 2048 + 5, 7, [(2, 0), (2, 0)]),                           # 8 keys per thread
    _case("identity", *_SMALL, launches=[(4, 0)], shuffle=False, no_wide_product=IDENTITY_WHY),
    _case("far", *_SMALL, launches=[(3, 0), (2, 0)], step0=10 ** 12 + 1, tail=True),                      # 64-bit step and epoch arithmetic
    _case("cfgT-weighted", *_CFGT, weighted=True),
    _case("hi-ids-weighted", *_HI, weighted=True),
]
# the tail jobs' 64-bit-key case (entity ids beyond 2^20; the launch-only cases above go beyond what a tail job's step can carry)
TAIL_CASES = [c for c in CASES if c["tail"]] + [_case("tail-key64", 86054151, 14824, 1024, 256, 256, 2 * 1024 + 9, 3, [], tail=True)]
TAIL_GROUPS, TAIL_GROUP_JOBS = 3, 3


def triples(c):
    """(H, R, T, W) of a case: ids drawn over the whole range (first triple: the largest ids), weights in [0.25, 4) or None"""
    rng = np.random.RandomState(len(c["id"]) + c["B"])
    n = c["n_train"]
    H, R, T = (rng.randint(0, hi, n, dtype=np.int64) for hi in (c["n_ent"], c["n_rel"], c["n_ent"]))
    H[0], R[0], T[0] = c["n_ent"] - 1, c["n_rel"] - 1, c["n_ent"] - 1
    W = rng.uniform(0.25, 4.0, n).astype(np.float32) if c["weighted"] else None
    return H, R, T, W


def steps_of(c, tail=False):
    """[(first step, batches, first slot)] of a case's launches (tail: of its groups of jobs)"""
    out, step = [], c["step0"]
    for n, slot0 in ([(TAIL_GROUP_JOBS, 0)] * TAIL_GROUPS if tail else c["launches"]):
        out.append((step, n, slot0))
        step += n
    return out
