// kge_tile_gemm.hpp - the 128 x 128 x 32 LDS-tiled fp32-MFMA product shared by full-table ranking (rank_gemm_kernel,
// kge_rank_gemm.hip) and top-K selection (topk_select_kernel<ACC_MFMA>, kge_topk.hip), and the score form that both and the
// chunked ranking (rank_chunk_gemm_kernel, kge_rank_chunk.hip) put on a raw product.
#pragma once
#include "kge_common.hpp"

#define TILE_BM 128                               // pos-side (query) rows of a workgroup tile
#define TILE_BN 128                               // candidates of a workgroup tile
#define TILE_BK 32                                // k per stage (the stage loop below is written for two 16-k halves)
#define TILE_LD (TILE_BK + 4)                     // dwords per staged row: 4 x odd, the fragment reads (16 rows x one float4) are conflict-free

namespace kge {

// gamma - |a - b|_2 from the product x = a . b and the squared norms, exactly as the training forward tiles form it
__device__ __forceinline__ float l2_score(float x, float gamma, float as, float bs) {
    return gamma - sqrtf(fmaxf(fmaf(-2.f, x, as + bs), 1e-30f));
}
// TransH (include/kge_hip.h): |a - n + (w^ . n) w^|^2 from the two products p = a . n and q = w^ . n, the squared norms as = |a|^2,
// bs = |n|^2 and c = w^ . a:  as + bs - 2 p + 2 c q - q^2  (|w^| is 1 or w^ = 0, and then q = 0).  One routine for the step's score
// kernel, its coefficient kernel, ranking and top-K: the same operands give the same bits everywhere
__device__ __forceinline__ float transh_dist2(float p, float q, float as, float bs, float c) {
    return fmaxf(fmaf(q, fmaf(2.f, c, -q), fmaf(-2.f, p, as + bs)), 1e-30f);
}
__device__ __forceinline__ float transh_score(float p, float q, float gamma, float as, float bs, float c) {
    return gamma - sqrtf(transh_dist2(p, q, as, bs, c));
}
// the two operands of a 64-query TransH tile inside the 128 pos-side rows of tile_gemm_128x128: 16-row strips 0, 1 of each
// wavefront's 64 rows are the a vectors of 32 queries and strips 2, 3 the w^ vectors of the same queries, so that with
// acc[i][j][r] as documented below a lane holds p in acc[i][j][r] and q in acc[i + 2][j][r] (i < 2) of ONE (query, candidate) pair:
// query 32 wr + 16 i + 4 q + r of the tile.  Tile row R -> (query of the tile, 0 = a / 1 = w^)
__device__ __forceinline__ int transh_tile_query(int R) { return 32 * (R >> 6) + (R & 31); }
__device__ __forceinline__ int transh_tile_is_w(int R) { return (R >> 5) & 1; }
// TransD (include/kge_hip.h): |a - n - c rho|^2 from the two products p = a . n and q = rho . n, the row scalars as = |a|^2,
// sg = |rho|^2, u = a . rho and the candidate scalars bs = |n|^2, c = m . n:  as + bs + c^2 sg - 2 p + 2 c (q - u).  One routine
// for the step's score kernel, its coefficient kernel, ranking and top-K, as for TransH.  The pair (a, rho) of 64 queries sits in
// a tile exactly as TransH's (transh_tile_query / transh_tile_is_w)
__device__ __forceinline__ float transd_dist2(float p, float q, float as, float sg, float u, float bs, float c) {
    return fmaxf(fmaf(c, fmaf(c, sg, 2.f * (q - u)), fmaf(-2.f, p, as + bs)), 1e-30f);
}
__device__ __forceinline__ float transd_score(float p, float q, float gamma, float as, float sg, float u, float bs, float c) {
    return gamma - sqrtf(transd_dist2(p, q, as, sg, u, bs, c));
}
// the score of a (pos-side row, candidate) pair from its raw product: TransE_l2 (l2; as / bs = |a|^2 / |b|^2), SimplE (clampv > 0:
// clamp), the other matrix forms (the product itself)
__device__ __forceinline__ float tile_score(float x, int l2, float gamma, float as, float bs, float clampv) {
    if (l2) return l2_score(x, gamma, as, bs);
    if (clampv > 0.f) return fminf(fmaxf(x, -clampv), clampv);
    return x;
}

// acc = A_tile . B_tile^T over k = 0 .. D (D % 4 == 0, D >= 4) for one workgroup of 256 threads.
//   row_a(i): global pointer of the tile's pos-side row i, row_b(j): of its candidate j (0 <= i, j < 128).  Both must be readable
//   for every i / j: the callers clamp rows beyond their matrix to its last valid row and ignore those products afterwards.
//   lds: the workgroup's two stage buffers; free again when the function returns (it ends in a __syncthreads()).
//   wave: the caller's readfirstlane(threadIdx.x >> 6) (an argument: a second readfirstlane in here is not merged with the caller's
//   inside topk_select_kernel's candidate loop and costs that kernel 4 VGPRs).
// Four wavefronts of 64 x 64 (4 x 4 MFMA tiles: one fragment read feeds four MFMAs): wavefront (wr, wc) = (wave >> 1, wave & 1)
// owns rows [64 wr, +64) x candidates [64 wc, +64), and with m = lane & 15, q = lane >> 4
//   acc[i][j][r] = (row 64 wr + 16 i + 4 q + r, candidate 64 wc + 16 j + m).
// k runs in stages of 32 through LDS, double-buffered: 128-byte global segments, the next stage's global loads in flight under the
// stage's 128 MFMAs per wavefront.
template <class RowA, class RowB>
__device__ __forceinline__ void tile_gemm_128x128(float (&lds)[2][(TILE_BM + TILE_BN) * TILE_LD], int D, int wave, const RowA &row_a,
                                                  const RowB &row_b, f32x4 (&acc)[4][4]) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nst = (D + TILE_BK - 1) / TILE_BK;
    const int c4t = (tid & 7) * 4;
    // ---- staging: float4 f = tid + 256 i of the stage's 2 x 1024: row f >> 3 (< 128: pos-side, else candidate), piece f & 7 ------
    const float *gp[8];
    int lo[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = tid + 256 * i, row = f >> 3, c4 = (f & 7) * 4;
        if (row < TILE_BM) gp[i] = row_a(row) + c4;
        else gp[i] = row_b(row - TILE_BM) + c4;
        lo[i] = row * TILE_LD + c4;
    }
    f32x4 g[8];
    // (D % 4 == 0: this thread's float4 of a stage is whole or beyond the row.  Only the LAST stage can reach beyond: its loads are
    //  clamped in-bounds re-reads like every prefetch here - unconditional, no exec-masked branch around a load - and stored as zeros)
    const bool tail = (D % TILE_BK) != 0 && (nst - 1) * TILE_BK + c4t >= D;
    auto gload = [&](int s) {
        const int off = min(s * TILE_BK, D - 4 - c4t);
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = *reinterpret_cast<const f32x4 *>(gp[i] + off);
    };
    auto lstore = [&](int bf, bool last) {
        if (last && (D % TILE_BK) != 0) {                          // (wave-uniform)
#pragma unroll
            for (int i = 0; i < 8; ++i) g[i] = tail ? (f32x4){0.f, 0.f, 0.f, 0.f} : g[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4 *>(&lds[bf][lo[i]]) = g[i];
    };
    // ---- compute ----------------------------------------------------------------------------------------------------------------
    const int wr = wave >> 1, wc = wave & 1;
    const int m = lane & 15, q = lane >> 4;
    const int aoff = (wr * 64 + m) * TILE_LD + 4 * q, boff = (TILE_BM + wc * 64 + m) * TILE_LD + 4 * q;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    gload(0);
    lstore(0, nst == 1);
    __syncthreads();
    for (int s = 0; s < nst; ++s) {
        const int bf = s & 1;
        if (s + 1 < nst) gload(s + 1);
        // both 16-k halves' fragments are requested up front; the next stage goes to the other LDS buffer BETWEEN the two halves'
        // MFMAs (its global loads were issued a half-stage = 64 MFMAs ago), so that the stores sit under the second half's MFMAs
        f32x4 af[2][4], bfr[2][4];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                af[kb][i] = *reinterpret_cast<const f32x4 *>(&lds[bf][aoff + i * 16 * TILE_LD + kb * 16]);
                bfr[kb][i] = *reinterpret_cast<const f32x4 *>(&lds[bf][boff + i * 16 * TILE_LD + kb * 16]);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = MFMA16(af[0][i][e], bfr[0][j][e], acc[i][j]);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < nst) lstore(bf ^ 1, s + 2 == nst);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = MFMA16(af[1][i][e], bfr[1][j][e], acc[i][j]);
        __syncthreads();
    }
}

}  // namespace kge
