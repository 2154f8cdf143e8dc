// kge_known.hip - which (positive, negative) pairs of a training batch are KNOWN triples (dglke_train --exclude_positive; the
// reference sampler's `exclude_positive`, dataloader/sampler.py:377, 396, 418, which its CLI hard-wires to False).
//
// Row i of the batch is the positive (h_i, r_i, t_i) of chunk c = i / chunk, column j holds entity n = neg_ids[c * N + j].  The pair
// is known when the corrupted triple - (n, r_i, t_i) when the step corrupts heads, (h_i, r_i, n) when it corrupts tails - is in the
// index: the (key, entity) pairs of eval.sort_known_device, sorted by key then entity, key = t * R + r with heads as values (head
// side) or h * R + r with tails as values (tail side).  Output: one bit per pair, uint32 mask[B][ceil(N / 32)], bit j & 31 of word
// j >> 5 of row i; the bits beyond column N of a row's last word are 0.  The stand-alone loss kernel (kge_rowwise.hip) reads it.
//
// One wavefront per positive row.  The row's list [f0, f1) is found by a wave-uniform search over the keys - uniform addresses in
// read-only memory: scalar loads, no vector register or lane is involved - a binary search for f0, then a gallop from f0 for f1
// (the lists are short next to the array: ~2 log2(length) probes instead of another log2(M)).  Every lane then searches its
// columns' entity ids in vals[f0, f1) and a ballot packs 64 columns into two words.  Offsets are 64-bit throughout.
#include "kge_common.hpp"
#include "kge_update_body.hpp"      // LANE()

using namespace kge;

__global__ __launch_bounds__(KGE_BLOCK) void known_mask_kernel(KnownMaskArgs a) {
    const int i = (int)blockIdx.x * KGE_WAVES_PER_BLOCK + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= a.B) return;
    const int lane = LANE();
    const int nh = (a.counts_dev ? a.counts_dev[2] : a.neg_head) != 0 ? 1 : 0;
    // (selects, not an indexed read of the argument block: the pointers stay in scalar registers)
    const int64_t *keys = nh ? a.keys[1] : a.keys[0], *vals = nh ? a.vals[1] : a.vals[0];
    const int64_t M = nh ? a.m[1] : a.m[0];
    const int64_t key = (nh ? a.t[i] : a.h[i]) * a.n_rel + a.r[i];
    int64_t f0 = 0, f1 = M;
    while (f0 < f1) {                                    // first position with keys[p] >= key
        const int64_t mid = f0 + ((f1 - f0) >> 1);
        if (keys[mid] < key) f0 = mid + 1; else f1 = mid;
    }
    f1 = f0;
    if (f0 < M && keys[f0] == key) {                     // first position with keys[p] > key: gallop, then bisect the last stride
        int64_t lo = f0 + 1, hi = M;
        for (int64_t step = 1; f0 + step < M; step <<= 1) {
            if (keys[f0 + step] > key) { hi = f0 + step; break; }
            lo = f0 + step + 1;
        }
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] <= key) lo = mid + 1; else hi = mid;
        }
        f1 = lo;
    }
    const int N = a.N, W = (N + 31) >> 5;
    const int64_t *neg = a.neg + (int64_t)(i / a.chunk) * N;
    uint32_t *mrow = a.mask + (int64_t)i * W;
    for (int base = 0; base < N; base += 64) {
        const int j = base + lane;
        const bool hit = j < N && f1 > f0 && in_sorted(vals, f0, f1, neg[j]);
        const unsigned long long bits = __ballot(hit);
        if (lane == 0) {
            const int wd = base >> 5;                    // (wd < W: base < N)
            mrow[wd] = (uint32_t)bits;
            if (wd + 1 < W) mrow[wd + 1] = (uint32_t)(bits >> 32);
        }
    }
}

int launch_known_mask(const KnownMaskArgs &a, hipStream_t s) {
    if (a.B <= 0 || a.N <= 0 || a.chunk <= 0) return KGE_ERR_ARG;
    const int nb = (a.B + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK;
    hipLaunchKernelGGL(known_mask_kernel, dim3(nb), dim3(KGE_BLOCK), 0, s, a);
    return check_launch();
}
