// kge_allent.hpp - device pieces shared by the all-entity steps' translation units (kge_kvsall.hip, kge_allent_clamp.hip): the
// K-vs-all criterion's terms and label bits, and the 128 x 64 tile loop of the owner kernels.  Everything here is inlined into its
// callers: moving it out of kge_kvsall.hip left that file's kernels as they were.
#pragma once
#include "kge_tile_gemm.hpp"

#define KVA_LDG 132                                // dwords per staged row of a G tile: 4 x odd, as TILE_LD
#define KVA_EB 64                                  // entity rows a workgroup of an owner kernel owns = candidates of its score tile

namespace kge {

typedef float TileLds[2][(TILE_BM + TILE_BN) * TILE_LD];      // tile_gemm_128x128's stage buffers: 18432 floats, free between tiles
typedef float Tile64Lds[2][(TILE_BM + KVA_EB) * TILE_LD];     // tile_gemm_128x64's: 13824 floats

// softplus(s) and sigma(s) from one exponential
__device__ __forceinline__ void bce_terms(float s, float &sp, float &sg) {
    const float e = __expf(-fabsf(s)), r = __builtin_amdgcn_rcpf(1.f + e);
    sp = fmaxf(s, 0.f) + __logf(1.f + e);
    sg = s >= 0.f ? r : e * r;
}

// a tile row's cursor into its sorted list: `cur` the position, `nxt` the entity there (loaded ahead; meaningless once cur == f1)
struct ListCursor { int64_t cur, f1, nxt, own; };

// a row's list range and own end as kva_prep_kernel left them (rows beyond the batch: an empty list, no own end)
struct ListRange { int64_t f0, f1, own; };
__device__ __forceinline__ ListRange range_of(const KvaArgs &a, int row) {
    ListRange g{0, 0, -1};
    if (row < a.B) { g.f0 = a.rng[2 * row]; g.f1 = a.rng[2 * row + 1]; g.own = a.own[row]; }
    return g;
}

// the cursor of the list at its first entity >= first
__device__ __forceinline__ ListCursor cursor_at(const KvaArgs &a, const ListRange &g, int64_t first) {
    ListCursor c{0, g.f1, 0, g.own};
    int64_t lo = g.f0, hi = g.f1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.vals[mid] < first) lo = mid + 1; else hi = mid;
    }
    c.cur = lo;
    if (lo < c.f1) c.nxt = a.vals[lo];
    return c;
}

// bits of the entities [c0, c0 + 64 W) of the cursor's list and the row's own end; the cursor moves past them.  W = 1 or 2 words of 64
template <int W>
__device__ __forceinline__ void label_bits(const KvaArgs &a, ListCursor &c, int64_t c0, unsigned long long (&bits)[W]) {
    const int64_t cend = c0 + 64 * W;
#pragma unroll
    for (int k = 0; k < W; ++k) bits[k] = 0ull;
    while (c.cur < c.f1 && c.nxt < cend) {
        const int b = (int)(c.nxt - c0);
        if (W == 1 || b < 64) bits[0] |= 1ull << b;
        else bits[W - 1] |= 1ull << (b - 64);
        ++c.cur;
        c.nxt = a.vals[c.cur < c.f1 ? c.cur : c.f1 - 1];
    }
    if (c.own >= c0 && c.own < cend) {
        const int b = (int)(c.own - c0);
        if (W == 1 || b < 64) bits[0] |= 1ull << b;
        else bits[W - 1] |= 1ull << (b - 64);
    }
}

// ---- the 128 x 64 tile loop of the owner kernels ----------------------------------------------------------------------------------
// acc = A_tile . B_tile^T over k = 0 .. D (D % 4 == 0, D >= 4) for one workgroup of 256 threads: 128 pos-side rows x 64 candidates.
// row_a(i) / row_b(j): readable global row pointers for every 0 <= i < 128, 0 <= j < 64 (the callers clamp).  lds is free again when
// the function returns (it ends in a __syncthreads()).  Wavefront w owns rows [32 w, +32) x all 64 candidates (2 x 4 MFMA tiles:
// six fragment reads feed eight MFMAs), and with m = lane & 15, q = lane >> 4
//   acc[i][j][r] = (row 32 w + 16 i + 4 q + r, candidate 16 j + m).
// k runs in stages of 32 through LDS, double-buffered as in tile_gemm_128x128: 192 rows x 8 float4 per stage, 6 per thread, the same
// conflict-free row stride, the same clamped (unconditional) loads of a last partial stage, stored as zeros.
template <class RowA, class RowB>
__device__ __forceinline__ void tile_gemm_128x64(Tile64Lds &lds, int D, int wave, const RowA &row_a, const RowB &row_b, f32x4 (&acc)[2][4]) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nst = (D + TILE_BK - 1) / TILE_BK;
    const int c4t = (tid & 7) * 4;
    const float *gp[6];
    int lo[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int row = (tid + 256 * i) >> 3;      // (< 128: pos-side, else candidate; the piece is tid & 7 for every i)
        if (row < TILE_BM) gp[i] = row_a(row) + c4t;
        else gp[i] = row_b(row - TILE_BM) + c4t;
        lo[i] = row * TILE_LD + c4t;
    }
    f32x4 g[6];
    const bool tail = (D % TILE_BK) != 0 && (nst - 1) * TILE_BK + c4t >= D;
    auto gload = [&](int s) {
        const int off = min(s * TILE_BK, D - 4 - c4t);
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = *reinterpret_cast<const f32x4 *>(gp[i] + off);
    };
    auto lstore = [&](int bf, bool last) {
        if (last && (D % TILE_BK) != 0) {                          // (wave-uniform)
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = tail ? (f32x4){0.f, 0.f, 0.f, 0.f} : g[i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) *reinterpret_cast<f32x4 *>(&lds[bf][lo[i]]) = g[i];
    };
    const int m = lane & 15, q = lane >> 4;
    const int aoff = (wave * 32 + m) * TILE_LD + 4 * q, boff = (TILE_BM + m) * TILE_LD + 4 * q;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    gload(0);
    lstore(0, nst == 1);
    __syncthreads();
    for (int s = 0; s < nst; ++s) {
        const int bf = s & 1;
        if (s + 1 < nst) gload(s + 1);
        f32x4 af[2][2], bfr[2][4];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int i = 0; i < 2; ++i) af[kb][i] = *reinterpret_cast<const f32x4 *>(&lds[bf][aoff + i * 16 * TILE_LD + kb * 16]);
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[kb][j] = *reinterpret_cast<const f32x4 *>(&lds[bf][boff + j * 16 * TILE_LD + kb * 16]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = MFMA16(af[0][i][e], bfr[0][j][e], acc[i][j]);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < nst) lstore(bf ^ 1, s + 2 == nst);             // the other buffer, under the second half's MFMAs
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = MFMA16(af[1][i][e], bfr[1][j][e], acc[i][j]);
        __syncthreads();
    }
}

}  // namespace kge
