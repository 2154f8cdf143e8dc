// kge_onevsall.hip - 1-vs-all softmax cross-entropy (kge_step_fused on a batch with N == 0, include/kge_hip.h): every entity of the
// table is a candidate of every positive edge, s_ij = a_i . e_j.  The [B, n_ent] score matrix is never stored:
//   ova_fwd_kernel    128 x 128 score tiles (tile_gemm_128x128, rows of A x rows of the table) folded into a running (max, sum-exp)
//                     pair per row; one pair per (row, split of the entity range) leaves the kernel
//   ova_lse_kernel    the splits' pairs of a row, in split order -> lse_i, the row's loss term, coef_i = w_i / B
//   ova_bwd_a_kernel  recomputes the score tile, G = coef_i exp(s - lse_i) goes through LDS as the first operand of a second product
//                     G [128 x 128] . E_tile [128 x d]: GA = dL/da in one part per split, no atomics
//   ova_bwd_e_kernel  a workgroup OWNS 64 entity rows: it walks every row tile of the batch, accumulates G^T . A_tile into its
//                     register-resident [64, d] gradient and applies the Adagrad rule to its rows itself - no gradient buffer
// Every sum has a fixed order: the results are bit-reproducible.  Matrix products are fp32 MFMA (16 x 16 x 4).
#include <cmath>
#include "kge_tile_gemm.hpp"

#define OVA_LDG 132                                // dwords per staged row of a G tile: 4 x odd, as TILE_LD
#define OVA_EB 64                                  // entity rows a workgroup of ova_bwd_e_kernel owns

namespace {
using namespace kge;

typedef float TileLds[2][(TILE_BM + TILE_BN) * TILE_LD];      // tile_gemm_128x128's stage buffers: 18432 floats, free between tiles

// ---- forward: running (max, sum-exp) per row, scores never stored ---------------------------------------------------------------
__global__ __launch_bounds__(KGE_BLOCK) void ova_fwd_kernel(OvaArgs a) {
    __shared__ __attribute__((aligned(16))) TileLds lds;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int wc = wave & 1, m = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x * TILE_BM, sp = blockIdx.y;
    const int t0 = sp * a.g.tps, t1 = min(t0 + a.g.tps, a.g.NT);
    float mx[4][4], z[4][4];                       // [i][r]: row 64 wr + 16 i + 4 q + r of the tile, over this lane's columns
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) { mx[i][r] = -INFINITY; z[i][r] = 0.f; }
    auto row_a = [&](int i) { return a.A + (int64_t)min(r0 + i, a.B - 1) * a.d; };
    for (int t = t0; t < t1; ++t) {
        const int64_t c0 = (int64_t)t * TILE_BN;
        auto row_b = [&](int j) { return a.ent + min(c0 + j, a.n_ent - 1) * (int64_t)a.d; };
        f32x4 acc[4][4];
        tile_gemm_128x128(lds, a.d, wave, row_a, row_b, acc);
        bool ok[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ok[j] = c0 + 64 * wc + 16 * j + m < a.n_ent;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float tm = -INFINITY;
#pragma unroll
                for (int j = 0; j < 4; ++j) tm = ok[j] ? fmaxf(tm, acc[i][j][r]) : tm;
                const float mn = fmaxf(mx[i][r], tm);
                float zz = mx[i][r] == mn ? z[i][r] : z[i][r] * __expf(mx[i][r] - mn);
#pragma unroll
                for (int j = 0; j < 4; ++j) zz += ok[j] ? __expf(acc[i][j][r] - mn) : 0.f;
                mx[i][r] = mn; z[i][r] = zz;
            }
    }
    // the 16 lanes of a row group (one DPP row), then the two column wavefronts through the stage buffers (free: the loop ends in a barrier)
    float *red = &lds[0][0];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float M = row_max16(mx[i][r]);
            const float Z = row_sum16(mx[i][r] == M ? z[i][r] : z[i][r] * __expf(mx[i][r] - M));
            if (m == 0) { red[(wave * 64 + 16 * i + 4 * q + r) * 2] = M; red[(wave * 64 + 16 * i + 4 * q + r) * 2 + 1] = Z; }
        }
    __syncthreads();
    const int row = threadIdx.x;
    if (row < TILE_BM && r0 + row < a.B) {
        const float *p0 = red + ((row >> 6) * 2 * 64 + (row & 63)) * 2, *p1 = p0 + 64 * 2;
        const float M0 = p0[0], Z0 = p0[1], M1 = p1[0], Z1 = p1[1];
        const float M = fmaxf(M0, M1);
        const float Z = (M0 == M ? Z0 : Z0 * __expf(M0 - M)) + (M1 == M ? Z1 : Z1 * __expf(M1 - M));
        float *o = a.part + ((int64_t)sp * a.B + r0 + row) * 2;
        o[0] = M; o[1] = Z;
    }
}

// ---- the splits of a row in split order: lse, loss term, coefficient.  Every entity is in the sum, so Z >= 1 at the row's maximum:
// the small-loss series of the sampled softmax (log1p of a tiny sum) has no case here - one logf per row
__global__ __launch_bounds__(KGE_BLOCK) void ova_lse_kernel(OvaArgs a) {
    const int i = blockIdx.x * KGE_BLOCK + threadIdx.x;
    if (i >= a.B) return;
    float M = -INFINITY;
    for (int s = 0; s < a.g.S; ++s) M = fmaxf(M, a.part[((int64_t)s * a.B + i) * 2]);
    float Z = 0.f;
    for (int s = 0; s < a.g.S; ++s) {
        const float ms = a.part[((int64_t)s * a.B + i) * 2], zs = a.part[((int64_t)s * a.B + i) * 2 + 1];
        Z += ms == M ? zs : zs * __expf(ms - M);
    }
    const float lse = M + logf(Z);
    const float cf = (a.w ? a.w[i] : 1.f) / (float)a.B;
    const float l = (lse - a.pos[i]) * cf;
    a.lse[i] = lse; a.coef[i] = cf; a.dpos[i] = -cf;
    if (a.row_pos) { a.row_pos[i] = 0.f; a.row_neg[i] = l; }
    if (a.acc) atomicAdd(&a.acc[2 * KGE_ACC_SLOTS + (i & (KGE_ACC_SLOTS - 1))], l);      // (one add per slot while B <= KGE_ACC_SLOTS)
}

// ---- GA = G . E without atomics: one part per split ------------------------------------------------------------------------------
// grid (row tile, split, column group).  A workgroup's 128 x (64 NJ) block of GA stays in registers over its split's column tiles:
// wavefront w owns the 16 NJ columns d0 + 16 NJ w .. of all 128 rows, ga[ib][j][r] = (row 16 ib + 4 q + r, column dw + 16 j + m).
// Rows wider than 256 floats take two column groups, each recomputing the score tiles: 128 x 512 accumulators would be 256 registers
// per lane beside the score tile's 64.
template <int NJ>
__global__ __launch_bounds__(KGE_BLOCK) void ova_bwd_a_kernel(OvaArgs a) {
    __shared__ __attribute__((aligned(16))) TileLds lds;
    __shared__ float sl[TILE_BM], sc[TILE_BM];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int wr = wave >> 1, wc = wave & 1, m = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x * TILE_BM, sp = blockIdx.y, dw = blockIdx.z * 64 * NJ + wave * 16 * NJ;
    const int t0 = sp * a.g.tpa, t1 = min(t0 + a.g.tpa, a.g.NT);
    if (threadIdx.x < TILE_BM) {
        const int row = r0 + threadIdx.x;
        sl[threadIdx.x] = a.lse[min(row, a.B - 1)];
        sc[threadIdx.x] = row < a.B ? a.coef[row] : 0.f;
    }
    int dcl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) dcl[j] = min(dw + 16 * j + m, a.d - 1);
    f32x4 ga[8][NJ];
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int j = 0; j < NJ; ++j) ga[ib][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float *G = &lds[0][0];                         // [128 rows][OVA_LDG]: the G tile, first operand of the second product
    auto row_a = [&](int i) { return a.A + (int64_t)min(r0 + i, a.B - 1) * a.d; };
    for (int t = t0; t < t1; ++t) {
        const int64_t c0 = (int64_t)t * TILE_BN;
        auto row_b = [&](int j) { return a.ent + min(c0 + j, a.n_ent - 1) * (int64_t)a.d; };
        {
            f32x4 acc[4][4];
            tile_gemm_128x128(lds, a.d, wave, row_a, row_b, acc);      // (its first barrier also publishes sl / sc)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 64 * wr + 16 * i + 4 * q + r;
                    const float l = sl[row], c = sc[row];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int col = 64 * wc + 16 * j + m;
                        G[row * OVA_LDG + col] = c0 + col < a.n_ent ? c * __expf(acc[i][j][r] - l) : 0.f;
                    }
                }
        }
        __syncthreads();
#pragma unroll 1
        for (int kb = 0; kb < TILE_BN / 16; ++kb) {      // 16 candidates: k = 4 q + e of four MFMAs
            f32x4 bf[NJ];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float *er = a.ent + min(c0 + kb * 16 + 4 * q + e, a.n_ent - 1) * (int64_t)a.d;      // (G is 0 beyond the table)
#pragma unroll
                for (int j = 0; j < NJ; ++j) bf[j][e] = er[dcl[j]];
            }
#pragma unroll
            for (int ib = 0; ib < 8; ++ib) {
                const f32x4 af = *reinterpret_cast<const f32x4 *>(&G[(16 * ib + m) * OVA_LDG + kb * 16 + 4 * q]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) ga[ib][j] = MFMA16(af[e], bf[j][e], ga[ib][j]);
            }
        }
        __syncthreads();                           // the next tile's staging overwrites G
    }
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + 16 * ib + 4 * q + r;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int dc = dw + 16 * j + m;
                if (row < a.B && dc < a.d) a.GAp[((int64_t)sp * a.B + row) * a.d + dc] = ga[ib][j][r];
            }
        }
}

// ---- owner-computes dense gradient with the Adagrad update fused -----------------------------------------------------------------
// A workgroup owns the entity rows e0 .. e0 + 64.  Per row tile of the batch: the score tile (the owned rows are candidates 0 .. 63
// of tile_gemm_128x128; its other 64 candidate columns repeat them and are dropped - the shared tile loop is kept whole at the price
// of half of this product), G^T staged in LDS [entity][edge], then G^T . A_tile into gn[ib][j][r] = (entity 16 ib + 4 q + r, column
// 16 NJ wave + 16 j + m): wavefront w holds the columns 16 NJ w .. of all 64 rows, NJ = ceil(d / 64) <= 8 - 128 registers at d = 512.
// No other workgroup reads these rows in this launch (each reads A and its own rows), so the update at the end races with nothing.
template <int NJ>
__global__ __launch_bounds__(KGE_BLOCK) void ova_bwd_e_kernel(OvaArgs a) {
    __shared__ __attribute__((aligned(16))) TileLds lds;
    __shared__ float sq[KGE_WAVES_PER_BLOCK][OVA_EB], kk[OVA_EB];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int wr = wave >> 1, wc = wave & 1, m = lane & 15, q = lane >> 4;
    const int64_t e0 = (int64_t)blockIdx.x * OVA_EB;
    const int dw = wave * 16 * NJ;
    int dcl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) dcl[j] = min(dw + 16 * j + m, a.d - 1);
    f32x4 gn[4][NJ];
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int j = 0; j < NJ; ++j) gn[ib][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float *Gt = &lds[0][0];                        // [64 entities][OVA_LDG]: G transposed, first operand of the second product
    auto row_b = [&](int j) { return a.ent + min(e0 + (j & (OVA_EB - 1)), a.n_ent - 1) * (int64_t)a.d; };
    for (int rt = 0; rt < a.g.RT; ++rt) {
        const int r0 = rt * TILE_BM;
        auto row_a = [&](int i) { return a.A + (int64_t)min(r0 + i, a.B - 1) * a.d; };
        {
            f32x4 acc[4][4];
            tile_gemm_128x128(lds, a.d, wave, row_a, row_b, acc);
            if (wc == 0) {                         // (wave-uniform) candidates 0 .. 63: the owned rows
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float l[4], c[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = r0 + 64 * wr + 16 * i + 4 * q + r;
                        l[r] = a.lse[min(row, a.B - 1)];
                        c[r] = row < a.B ? a.coef[row] : 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool ok = e0 + 16 * j + m < a.n_ent;
                        f32x4 g;
#pragma unroll
                        for (int r = 0; r < 4; ++r) g[r] = ok ? c[r] * __expf(acc[i][j][r] - l[r]) : 0.f;
                        *reinterpret_cast<f32x4 *>(&Gt[(16 * j + m) * OVA_LDG + 64 * wr + 16 * i + 4 * q]) = g;
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int kb = 0; kb < TILE_BM / 16; ++kb) {      // 16 edges: k = 4 q + e of four MFMAs
            f32x4 bf[NJ];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float *ar = a.A + (int64_t)min(r0 + kb * 16 + 4 * q + e, a.B - 1) * a.d;      // (G is 0 beyond the batch)
#pragma unroll
                for (int j = 0; j < NJ; ++j) bf[j][e] = ar[dcl[j]];
            }
#pragma unroll
            for (int ib = 0; ib < 4; ++ib) {
                const f32x4 af = *reinterpret_cast<const f32x4 *>(&Gt[(16 * ib + m) * OVA_LDG + kb * 16 + 4 * q]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) gn[ib][j] = MFMA16(af[e], bf[j][e], gn[ib][j]);
            }
        }
        __syncthreads();
    }
    // ---- Adagrad on the owned rows: state += mean(G^2), row -= lr G / (sqrt(state) + eps) - the update launch's rule ----
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) ss = dw + 16 * j + m < a.d ? fmaf(gn[ib][j][r], gn[ib][j][r], ss) : ss;
            ss = row_sum16(ss);
            if (m == 0) sq[wave][16 * ib + 4 * q + r] = ss;
        }
    __syncthreads();
    if (threadIdx.x < OVA_EB && e0 + threadIdx.x < a.n_ent) {
        const int er = threadIdx.x;
        const float tot = ((sq[0][er] + sq[1][er]) + sq[2][er]) + sq[3][er];
        const float sn = a.ent_state[e0 + er] + tot / (float)a.d;
        a.ent_state[e0 + er] = sn;
        kk[er] = -a.lr / (sqrtf(sn) + a.eps);
    }
    __syncthreads();
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int er = 16 * ib + 4 * q + r;
            if (e0 + er >= a.n_ent) continue;
            const float k = kk[er];
            float *row = a.ent + (e0 + er) * (int64_t)a.d;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int dc = dw + 16 * j + m;
                if (dc < a.d) row[dc] = fmaf(gn[ib][j][r], k, row[dc]);
            }
        }
}

inline bool ova_ok(const OvaArgs &a) { return a.B > 0 && a.n_ent > 0 && a.d >= 4 && a.d % 4 == 0 && a.d <= 512; }

}  // namespace

int launch_ova_fwd(const OvaArgs &a, hipStream_t s) {
    if (!ova_ok(a)) return KGE_ERR_ARG;
    hipLaunchKernelGGL(ova_fwd_kernel, dim3(a.g.RT, a.g.S), dim3(KGE_BLOCK), 0, s, a);
    return kge::check_launch();
}

int launch_ova_lse(const OvaArgs &a, hipStream_t s) {
    if (!ova_ok(a)) return KGE_ERR_ARG;
    hipLaunchKernelGGL(ova_lse_kernel, dim3((a.B + KGE_BLOCK - 1) / KGE_BLOCK), dim3(KGE_BLOCK), 0, s, a);
    return kge::check_launch();
}

int launch_ova_bwd_a(const OvaArgs &a, hipStream_t s) {
    if (!ova_ok(a)) return KGE_ERR_ARG;
    const dim3 g(a.g.RT, a.g.Sa, a.g.nslab), b(KGE_BLOCK);
    switch (a.g.nj) {
        case 1: hipLaunchKernelGGL(ova_bwd_a_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(ova_bwd_a_kernel<2>, g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL(ova_bwd_a_kernel<3>, g, b, 0, s, a); break;
        default: hipLaunchKernelGGL(ova_bwd_a_kernel<4>, g, b, 0, s, a); break;
    }
    return kge::check_launch();
}

int launch_ova_bwd_e(const OvaArgs &a, hipStream_t s) {
    if (!ova_ok(a)) return KGE_ERR_ARG;
    const dim3 g((unsigned)((a.n_ent + OVA_EB - 1) / OVA_EB)), b(KGE_BLOCK);
    switch ((a.d + 63) / 64) {
        case 1: hipLaunchKernelGGL(ova_bwd_e_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(ova_bwd_e_kernel<2>, g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL(ova_bwd_e_kernel<3>, g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL(ova_bwd_e_kernel<4>, g, b, 0, s, a); break;
        case 5: hipLaunchKernelGGL(ova_bwd_e_kernel<5>, g, b, 0, s, a); break;
        case 6: hipLaunchKernelGGL(ova_bwd_e_kernel<6>, g, b, 0, s, a); break;
        case 7: hipLaunchKernelGGL(ova_bwd_e_kernel<7>, g, b, 0, s, a); break;
        default: hipLaunchKernelGGL(ova_bwd_e_kernel<8>, g, b, 0, s, a); break;
    }
    return kge::check_launch();
}
