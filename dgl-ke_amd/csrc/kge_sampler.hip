// kge_sampler.hip - on-device mini-batch sampler + plan builder.
//
// Restates, on the GPU, what the reference gets from DGL's C++ EdgeSampler and its Python wrappers
// (dataloader/sampler.py:376-419 call site: batch_size positives, chunked uniform negatives over
// all entities with replacement, positives not excluded; :853-859 odd steps corrupt tails / even
// steps heads; :503-504 whole batches only) and the duplicate-grouping "plan" that
// dglke_amd/plan.py builds on the host (include/kge_hip.h `kge_batch`).  DGL's RNG stream cannot
// be reproduced (no dgl here), so parity is defined structurally: tests rebuild the plan on the
// host from the ids the kernel sampled and compare every array.
//
// One workgroup (1024 threads) builds one batch entirely in LDS:
//   1. positives: whole batches of the epoch's edge order (base permutation re-keyed per epoch) -> (h, r, t);  negatives: counter-based hash
//      RNG keyed by (seed, step, j) -> uniform id in [0, n_ent)
//   2. sort of <= 4096 keys (wide instance: 8192)  (entity id << 12 (13) | element code), code = edge*2+side  (a stable block radix sort over the id bits:
//      the codes are the positions; the relation plan keeps the register bitonic network)
//      for positive edge ends, 2B + slot for negatives  -> elements grouped by entity, ascending
//      code inside a group (= the order of the host plan and of index_add_)
//   3. one block-wide scan of packed (unique, positive, negative) flags -> unique entity list,
//      CSR pointers and lists, 32-byte plan records
//   4. same for the relations (sort of rel id << 12 | edge).
// Many batches are built concurrently (grid = number of slots), ahead of the training steps, so the
// sampler is off the critical path exactly like the reference's prefetching sampler threads.
#include <cstring>
#include "kge_common.hpp"
KGE_TL_DEFINE(sampler)

#include "kge_sampler_common.hpp"
#include "kge_sampler_kernel.hpp"

int launch_sample_batches_weighted(const SamplerArgs &a, int n_slots, hipStream_t s);      // kge_sampler_weighted.hip

int launch_sample_batches(const SamplerArgs &a, int n_slots, hipStream_t s, bool weighted = false) {
    return weighted ? launch_sample_batches_weighted(a, n_slots, s) : launch_sample_batches_t<false>(a, n_slots, s);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

size_t kge_sampler_slot_bytes(int B, int C, int N) {
    return (size_t)slot_layout(B, C * N).total;
}
size_t kge_sampler_slot_bytes_weighted(int B, int C, int N) {
    return (size_t)slot_layout(B, C * N, true).total;
}

// the checks and the launch of both sampler entries; `weights` non-null: the weighted instances and the weighted slot layout
static int sample_batches(const char *short_msg, const int64_t *heads, const int64_t *rels, const int64_t *tails, const int64_t *perm,
                          const float *weights, int64_t n_train, int64_t n_ent, int B, int C, int chunk, int N, uint64_t seed,
                          int64_t *state, void *slots, size_t slot_bytes, int n_slots, void *stream) {
    if (n_train < B) return kge_fail(KGE_ERR_ARG, short_msg);
    if (!heads || !rels || !tails || !state || !slots || n_train <= 0 || n_ent <= 0 || B <= 0 || C <= 0 ||
        chunk <= 0 || N <= 0 || C * chunk != B)
        return KGE_ERR_ARG;
    if (2 * B + C * N > SP_MAXE_BIG || B > SP_MAXE_BIG / 2 || n_ent >= ((int64_t)1 << (64 - SP_CODE_BITS_BIG)))
        return KGE_ERR_ARG;                      // larger batches: build the plan on the host
    if (slot_bytes < (weights ? kge_sampler_slot_bytes_weighted(B, C, N) : kge_sampler_slot_bytes(B, C, N))) return KGE_ERR_WORKSPACE;
    SamplerArgs a{};
    a.H = heads; a.R = rels; a.T = tails; a.perm = perm; a.n_train = n_train; a.n_ent = n_ent;
    a.B = B; a.C = C; a.chunk = chunk; a.N = N; a.seed = seed; a.state = state;
    a.slots = (char *)slots; a.slot_bytes = (int64_t)slot_bytes;
    if (weights) a.W = weights;              // (after the rest: W lies over preperm, which the launch does not read)
    return launch_sample_batches(a, n_slots, (hipStream_t)stream, weights != nullptr);
}

int kge_sample_batches(const int64_t *heads, const int64_t *rels, const int64_t *tails, const int64_t *perm,
                       int64_t n_train, int64_t n_ent, int B, int C, int chunk, int N, uint64_t seed,
                       int64_t *state, void *slots, size_t slot_bytes, int n_slots, void *stream) {
    return sample_batches("kge_sample_batches: fewer training triples than one batch (n_train < batch)", heads, rels, tails, perm, nullptr, n_train, n_ent, B, C, chunk, N, seed, state, slots,
                          slot_bytes, n_slots, stream);
}

// the same launch with one weight per training triple: slot k also gets edge_w[i] = weights[e_i] of its B edges.  Ids, plan and
// state are those of kge_sample_batches from the same state.
int kge_sample_batches_weighted(const int64_t *heads, const int64_t *rels, const int64_t *tails, const int64_t *perm,
                                const float *weights, int64_t n_train, int64_t n_ent, int B, int C, int chunk, int N, uint64_t seed,
                                int64_t *state, void *slots, size_t slot_bytes, int n_slots, void *stream) {
    if (!weights) return kge_fail(KGE_ERR_ARG, "kge_sample_batches_weighted: weights is null (one float per training triple; unweighted: kge_sample_batches)");
    return sample_batches("kge_sample_batches_weighted: fewer training triples than one batch (n_train < batch)", heads, rels, tails, perm, weights, n_train, n_ent, B, C, chunk, N, seed, state,
                          slots, slot_bytes, n_slots, stream);
}

// fill a kge_batch whose arrays live in sampler slot `slot` (host-side pointer arithmetic only).
// UE / UR are set to their upper bounds; the kernels read the actual counts from counts_dev.
static int batch_from_slot(void *slots, size_t slot_bytes, int slot, int B, int C, int chunk, int N, int neg_head, bool weighted,
                           kge_batch *out) {
    if (!slots || !out || C * chunk != B) return KGE_ERR_ARG;
    const SlotLayout L = slot_layout(B, C * N, weighted);
    char *sb = (char *)slots + (size_t)slot * slot_bytes;
    memset(out, 0, sizeof(*out));
    out->B = B; out->C = C; out->chunk = chunk; out->N = N; out->neg_head = neg_head;
    out->U = 0; out->UE = 2 * B + C * N; out->UR = B;
    out->h_gid = (const int64_t *)(sb + L.h_gid); out->t_gid = (const int64_t *)(sb + L.t_gid);
    out->rel_ids = (const int64_t *)(sb + L.rel_ids); out->neg_ids = (const int64_t *)(sb + L.neg_ids);
    // weighted: edge_w_mean stays 0 (the batch is built on the device) - the step's kernels sum the weights themselves (mean_edge_weight)
    out->edge_w = weighted ? (const float *)(sb + L.edge_w) : nullptr;
    out->ue_id = (const int64_t *)(sb + L.ue_id);
    out->ue_pos_ptr = (const int32_t *)(sb + L.ue_pos_ptr); out->ue_pos_adj = (const int32_t *)(sb + L.ue_pos_adj);
    out->ue_neg_ptr = (const int32_t *)(sb + L.ue_neg_ptr); out->ue_neg_slot = (const int32_t *)(sb + L.ue_neg_slot);
    out->ur_id = (const int64_t *)(sb + L.ur_id);
    out->ur_ptr = (const int32_t *)(sb + L.ur_ptr); out->ur_edge = (const int32_t *)(sb + L.ur_edge);
    out->ue_rec = (const int32_t *)(sb + L.ue_rec); out->ur_rec = (const int32_t *)(sb + L.ur_rec);
    out->counts_dev = (const int32_t *)(sb + L.counts);
    return KGE_OK;
}
int kge_batch_from_slot(void *slots, size_t slot_bytes, int slot, int B, int C, int chunk, int N, int neg_head,
                        kge_batch *out) {
    return batch_from_slot(slots, slot_bytes, slot, B, C, chunk, N, neg_head, false, out);
}
int kge_batch_from_slot_weighted(void *slots, size_t slot_bytes, int slot, int B, int C, int chunk, int N, int neg_head,
                                 kge_batch *out) {
    if (slot_bytes < kge_sampler_slot_bytes_weighted(B, C, N))
        return kge_fail(KGE_ERR_WORKSPACE, "kge_batch_from_slot_weighted: slot_bytes is smaller than kge_sampler_slot_bytes_weighted()");
    return batch_from_slot(slots, slot_bytes, slot, B, C, chunk, N, neg_head, true, out);
}

}  // extern "C"
