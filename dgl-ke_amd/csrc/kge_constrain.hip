// kge_constrain.hip - the norm constraints of the translation family's papers (TransE |e| = 1; TransH |e| <= 1, |w| = 1; TransR / TransD
// |e|, |r|, |e_p|, |r_p| <= 1) as a projection of exactly the rows a step has just updated: ONE launch behind the update launch of the
// strict step (KGE_FLAG_ENT_NORM_* / KGE_FLAG_REL_NORM_*, include/kge_hip.h).  A translation unit of its own: no
// existing kernel is compiled from anything that changed.
//
// Per slice x of a row (a row is `parts` equal slices): n = sqrtf(sum x^2) in fp32, s = 1.0f / n, x <- x * s
//   clip: only when n > 1 (a NaN norm compares false: the slice is left alone);   unit: when n > 0 and n != 1.
// A slice that is not scaled is not written.  Only row values change - never optimizer state.
//
// One wavefront per plan record (the update launch's convention and layout), entity and relation records in one launch; every row
// is named by one record only, so nothing races.  The reduction stays inside the wavefront (DPP, kge_common.hpp wave_sum): no LDS,
// no atomics, a fixed summation order.
#include "kge_common.hpp"
#include "kge_constrain.hpp"

namespace {

using kge::wave_sum;

__device__ __forceinline__ bool constrain_scales(float n, bool unit) { return unit ? (n > 0.f && n != 1.f) : (n > 1.f); }

// one slice of p floats at x.  NIT > 0: the slice stays in registers between the reduction and the store (p <= 256 * NIT; VEC: one
// 16-byte access per lane and round, else four 4-byte ones); NIT == 0: two streaming passes, any p.  VEC needs p % 4 == 0 and a
// 16-byte aligned x.  Every index is tested against p: nothing beyond the slice is read or written.
template <int NIT, bool VEC>
__device__ __forceinline__ void constrain_slice(float *x, int p, bool unit, int lane) {
    if constexpr (NIT == 0) {
        float ss = 0.f;
        if constexpr (VEC) {
            for (int i = lane * 4; i < p; i += KGE_WAVE * 4) {
                const f32x4 v = *(const f32x4 *)(x + i);
                ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
            }
        } else {
            for (int i = lane; i < p; i += KGE_WAVE) ss += x[i] * x[i];
        }
        const float n = sqrtf(wave_sum(ss));
        if (!constrain_scales(n, unit)) return;
        const float s = 1.0f / n;
        if constexpr (VEC) {
            for (int i = lane * 4; i < p; i += KGE_WAVE * 4) {
                f32x4 v = *(const f32x4 *)(x + i);
                v.x *= s; v.y *= s; v.z *= s; v.w *= s;
                *(f32x4 *)(x + i) = v;
            }
        } else {
            for (int i = lane; i < p; i += KGE_WAVE) x[i] *= s;
        }
    } else if constexpr (VEC) {
        f32x4 v[NIT];
        float ss = 0.f;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = (it * KGE_WAVE + lane) * 4;
            v[it] = i < p ? *(const f32x4 *)(x + i) : f32x4{0.f, 0.f, 0.f, 0.f};
            ss += v[it].x * v[it].x + v[it].y * v[it].y + v[it].z * v[it].z + v[it].w * v[it].w;
        }
        const float n = sqrtf(wave_sum(ss));
        if (!constrain_scales(n, unit)) return;
        const float s = 1.0f / n;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = (it * KGE_WAVE + lane) * 4;
            if (i < p) *(f32x4 *)(x + i) = f32x4{v[it].x * s, v[it].y * s, v[it].z * s, v[it].w * s};
        }
    } else {
        float v[4 * NIT];
        float ss = 0.f;
#pragma unroll
        for (int it = 0; it < 4 * NIT; ++it) {
            const int i = it * KGE_WAVE + lane;
            v[it] = i < p ? x[i] : 0.f;
            ss += v[it] * v[it];
        }
        const float n = sqrtf(wave_sum(ss));
        if (!constrain_scales(n, unit)) return;
        const float s = 1.0f / n;
#pragma unroll
        for (int it = 0; it < 4 * NIT; ++it) {
            const int i = it * KGE_WAVE + lane;
            if (i < p) x[i] = v[it] * s;
        }
    }
}

// workgroups [0, nb_ent): entity records, four per workgroup; the rest: relation records
template <int NIT, bool VEC>
__global__ __launch_bounds__(KGE_BLOCK) void constrain_kernel(ConstrainArgs a, int nb_ent) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const bool is_ent = (int)blockIdx.x < nb_ent;
    const int u = ((int)blockIdx.x - (is_ent ? 0 : nb_ent)) * KGE_WAVES_PER_BLOCK + wave;
    // beyond the bound there is no record; beyond the actual count of a device-built plan the record is stale: no table access
    if (u >= (is_ent ? a.UE : a.UR)) return;
    if (a.counts_dev && u >= a.counts_dev[is_ent ? 0 : 1]) return;
    const int32_t *rec = (is_ent ? a.ue_rec : a.ur_rec) + 8 * (int64_t)u;
    const int64_t id = (int64_t)(((uint64_t)(uint32_t)rec[1] << 32) | (uint64_t)(uint32_t)rec[0]);
    const int width = is_ent ? a.d_e : a.d_r, parts = is_ent ? a.ent_parts : a.rel_parts;
    const unsigned unit = is_ent ? a.ent_unit : a.rel_unit;
    float *row = (is_ent ? a.ent : a.rel) + id * (int64_t)width;
    const int p = width / parts;
    for (int k = 0; k < parts; ++k) constrain_slice<NIT, VEC>(row + (int64_t)k * p, p, (unit >> k) & 1u, lane);
}

}  // namespace

int launch_constrain(const ConstrainArgs &a, hipStream_t s) {
    const int nbE = (a.UE + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK, nbR = (a.UR + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK;
    if (nbE + nbR == 0) return KGE_OK;
    if ((a.UE > 0 && (!a.ent || !a.ue_rec || a.ent_parts < 1 || a.d_e < 1 || a.d_e % a.ent_parts)) ||
        (a.UR > 0 && (!a.rel || !a.ur_rec || a.rel_parts < 1 || a.d_r < 1 || a.d_r % a.rel_parts)))
        return KGE_ERR_ARG;
    // the instance: by the widest slice of the constrained tables; 16-byte accesses where every constrained slice allows them
    const int pe = a.UE > 0 ? a.d_e / a.ent_parts : 0, pr = a.UR > 0 ? a.d_r / a.rel_parts : 0;
    const int pmax = pe > pr ? pe : pr;
    const bool vec = pe % 4 == 0 && pr % 4 == 0;
    const dim3 g(nbE + nbR), b(KGE_BLOCK);
#define KGE_CONSTRAIN(N) do { if (vec) hipLaunchKernelGGL((constrain_kernel<N, true>), g, b, 0, s, a, nbE); \
                              else hipLaunchKernelGGL((constrain_kernel<N, false>), g, b, 0, s, a, nbE); } while (0)
    if (pmax <= KGE_CONSTRAIN_REG_NARROW) KGE_CONSTRAIN(1);
    else if (pmax <= KGE_CONSTRAIN_REG_WIDE) KGE_CONSTRAIN(4);
    else KGE_CONSTRAIN(0);
#undef KGE_CONSTRAIN
    return kge::check_launch();
}
