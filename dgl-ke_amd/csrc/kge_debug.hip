// kge_debug.hip - test support (include/kge_hip.h, "test support"): the sampler's epoch order evaluated for ANY n_train.
//
// The epoch order of the device sampler is perm[(pos * mul + add) mod n_train] with (mul, add) hashed from (seed, epoch)
// (kge_sampler_common.hpp).  The sampler kernels reach those functions only through real triples, so a graph of 2^32 triples or more -
// the shift-and-add product of epoch_index, the `m % n` branch of epoch_affine - cannot be reached by a test of a few seconds.  This
// kernel evaluates the SAME inline functions, one thread per (epoch, position) pair, without any triple: tests compare its five
// outputs with a statement in Python integers (tests/sampler_statement.py, tests/test_gpu_sampler_statement.py).
#include "kge_common.hpp"
#include "kge_sampler_common.hpp"

using namespace kge;

namespace {

__global__ __launch_bounds__(256) void debug_epoch_order_kernel(int64_t n_train, uint64_t seed, int shuffled, const int64_t *epoch,
                                                                const int64_t *pos, int64_t n, int64_t *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    SamplerArgs a{};
    a.n_train = n_train; a.seed = seed;
    a.perm = shuffled ? out : nullptr;       // a non-null dummy: the epoch functions only ask whether there IS a base permutation
    const int64_t ep = epoch[i];
    const uint64_t p = (uint64_t)pos[i];
    uint64_t mul, add;
    epoch_affine(a, ep, mul, add);
    const EpochConst c = epoch_consts_slow(a, ep);
    int64_t *o = out + 5 * i;
    o[0] = (int64_t)epoch_index(p, mul, add, (uint64_t)n_train);
    o[1] = (int64_t)epoch_index_fast(p, c, (uint64_t)n_train);
    o[2] = (int64_t)mul; o[3] = (int64_t)add; o[4] = (int64_t)c.rinv;
}

}  // namespace

extern "C" int kge_debug_epoch_order(int64_t n_train, uint64_t seed, int shuffled, const int64_t *epoch, const int64_t *pos, int64_t n,
                                     int64_t *out, void *stream) {
    if (n_train <= 0 || n < 0 || !epoch || !pos || !out) return kge_fail(KGE_ERR_ARG, "kge_debug_epoch_order: bad argument");
    if (n == 0) return KGE_OK;
    if ((n + 255) / 256 > 0x7fffffffll) return kge_fail(KGE_ERR_ARG, "kge_debug_epoch_order: more pairs than one launch takes");
    hipLaunchKernelGGL(debug_epoch_order_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_train, seed,
                       shuffled, epoch, pos, n, out);
    return check_launch();
}
