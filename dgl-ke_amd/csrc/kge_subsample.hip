// kge_subsample.hip - frequency ("subsampling") weights of the training triples (dglke_train --subsampling_weight): the weighting of
// the RotatE, OGB and PairRE code bases, word2vec's subsampling carried over to triples.  Their `count_frequency` counts every (h, r)
// pair and every (t, r^-1) pair of the training split, both counters starting at 4 - a pair seen n times counts n + 3 - and weights a
// triple by 1 / sqrt(count(h, r) + count(t, r^-1)).
//
// Here the two counters are the training split's keys h * R + r and t * R + r, each sorted ascending WITH multiplicity (a triple that
// is present twice counts twice): the count of a pair is the length of its run of equal keys, upper bound minus lower bound.
//     out[i] = scale * (1 / sqrtf((float)(n_hr + n_tr + 6)))
// with IEEE sqrtf and a true division: three correctly rounded fp32 operations behind an exact conversion (the sum stays far below
// 2^24 for every graph whose keys fit the device).  One thread per triple, 64-bit keys and offsets throughout.
#include "kge_common.hpp"

using namespace kge;

namespace {

// [first position with keys[p] >= key, first position with keys[p] > key) in keys[0, m): the length of key's run
__device__ __forceinline__ int64_t run_length(const int64_t *keys, int64_t m, int64_t key) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int64_t first = lo;
    hi = m;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo - first;
}

__global__ __launch_bounds__(256) void subsampling_weights_kernel(const int64_t *keys_hr, int64_t m_hr, const int64_t *keys_tr, int64_t m_tr,
                                                                  const int64_t *heads, const int64_t *rels, const int64_t *tails, int64_t n,
                                                                  int64_t n_rel, float scale, float *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = rels[i];
    const int64_t n_hr = run_length(keys_hr, m_hr, heads[i] * n_rel + r);
    const int64_t n_tr = run_length(keys_tr, m_tr, tails[i] * n_rel + r);
    out[i] = scale * (1.f / sqrtf((float)(n_hr + n_tr + 6)));
}

}  // namespace

extern "C" int kge_subsampling_weights(const int64_t *keys_hr, int64_t m_hr, const int64_t *keys_tr, int64_t m_tr, const int64_t *heads,
                                       const int64_t *rels, const int64_t *tails, int64_t n, int64_t n_ent, int64_t n_rel, float scale,
                                       float *out, void *stream) {
    if (m_hr < 0 || m_tr < 0 || n < 0 || n_ent <= 0 || n_rel <= 0 || (m_hr && !keys_hr) || (m_tr && !keys_tr) ||
        (n && (!heads || !rels || !tails || !out)) || !(scale > 0.f))
        return kge_fail(KGE_ERR_ARG, "kge_subsampling_weights: bad argument");
    if ((unsigned __int128)n_ent * (unsigned __int128)n_rel >= ((unsigned __int128)1 << 62))
        return kge_fail(KGE_ERR_ARG, "kge_subsampling_weights: n_ent * n_rel >= 2^62 - the keys h * n_rel + r do not fit 64 bits");
    if (n == 0) return KGE_OK;
    if ((n + 255) / 256 > 0x7fffffffll) return kge_fail(KGE_ERR_ARG, "kge_subsampling_weights: more triples than one launch takes");
    hipLaunchKernelGGL(subsampling_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keys_hr, m_hr,
                       keys_tr, m_tr, heads, rels, tails, n, n_rel, scale, out);
    return check_launch();
}
