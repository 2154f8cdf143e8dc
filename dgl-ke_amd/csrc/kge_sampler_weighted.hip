// kge_sampler_weighted.hip - the weighted twins of the sampler launch's four instances (kge_sample_batches_weighted): the kernel of
// kge_sampler_kernel.hpp with WGT = true, in a translation unit of their own (why: see that header).
#include "kge_sampler_kernel.hpp"

int launch_sample_batches_weighted(const SamplerArgs &a, int n_slots, hipStream_t s) {
    return launch_sample_batches_t<true>(a, n_slots, s);
}
