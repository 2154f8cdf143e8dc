// kge_allent_clamp.hip - the all-entity criteria over CLAMPED scores (SimplE on kge_step_fused / kge_step_fused_known with N == 0;
// DESIGN.md 3.21): s_ij = clamp(a_i . e_j, -20, 20) for every entity j of the table, and no gradient reaches a raw product that the
// clamp saturates (|a_i . e_j| >= 20: the sampled step's convention, kge_loss_body.hpp).  The scores are never stored; clamp and mask
// act on the MFMA accumulators in registers, between the product and what the unclamped kernels do with it - no LDS pass, no barrier
// and no global access is added.  One kernel family serves both criteria (BCE = false: softmax, true: K-vs-all BCE), so that the
// softmax owner kernel, too, runs the 128 x 64 score tile of the K-vs-all one instead of a 128 x 128 tile whose second half repeats
// the first:
//   ace_fwd_kernel        softmax: 128 x 128 score tiles folded into a running (max, sum-exp) pair per row and split.  The maximum of a
//                         row is one of its clamped scores, so Z >= 1 there as without a clamp
//   ace_lse_kernel        softmax: the splits' pairs in split order -> lse_i, the loss term, coef_i = w_i / B, and dL/dp_i = -coef_i or
//                         0 where the positive is saturated (edge_fwd left p_i = +-20 exactly then)
//   ace_bwd_a_kernel      128 x 128 score tiles recomputed, G = mask . dL/ds through LDS as the first operand of G . E_tile:
//                         GA = dL/da in one part per split; BCE: label bits from the rows' list cursors, and the loss summed on the way
//   ace_bwd_e_kernel      a workgroup OWNS 64 entity rows: per row tile of the batch the 128 x 64 score tile, G^T staged in LDS,
//                         G^T . A_tile into its register-resident [64, d] gradient, then the Adagrad rule on its rows
// kva_prep_kernel / kva_loss_kernel (kge_kvsall.hip) do not look at a score and serve the clamped BCE as they are.  The unclamped
// kernels of kge_onevsall.hip / kge_kvsall.hip are not touched: a translation unit of its own keeps their code objects as they were.
// Every sum has a fixed order: the results are bit-reproducible.  Matrix products are fp32 MFMA (16 x 16 x 4).
#include <cmath>
#include "kge_allent.hpp"

namespace {
using namespace kge;

// the clamped score of a raw product and whether a gradient passes (false on the bound itself, as in the sampled step's loss kernels)
__device__ __forceinline__ float clamp_score(float raw, bool &open) {
    open = fabsf(raw) < KGE_SIMPLE_CLAMP;
    return fminf(fmaxf(raw, -KGE_SIMPLE_CLAMP), KGE_SIMPLE_CLAMP);
}

// ---- softmax forward: running (max, sum-exp) per row over clamped scores ------------------------------------------------------------
__global__ __launch_bounds__(KGE_BLOCK) void ace_fwd_kernel(AceArgs aa) {
    const KvaArgs &a = aa.k;
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
                float sv[4], tm = -INFINITY;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bool open;
                    sv[j] = clamp_score(acc[i][j][r], open);
                    tm = ok[j] ? fmaxf(tm, sv[j]) : tm;
                }
                const float mn = fmaxf(mx[i][r], tm);
                float zz = mx[i][r] == mn ? z[i][r] : z[i][r] * __expf(mx[i][r] - mn);
#pragma unroll
                for (int j = 0; j < 4; ++j) zz += ok[j] ? __expf(sv[j] - mn) : 0.f;
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
        float *o = aa.part + ((int64_t)sp * a.B + r0 + row) * 2;
        o[0] = M; o[1] = Z;
    }
}

// ---- softmax: the splits of a row in split order -> lse, loss term, coefficient, the positive's masked gradient --------------------
__global__ __launch_bounds__(KGE_BLOCK) void ace_lse_kernel(AceArgs aa) {
    const KvaArgs &a = aa.k;
    const int i = blockIdx.x * KGE_BLOCK + threadIdx.x;
    if (i >= a.B) return;
    float M = -INFINITY;
    for (int s = 0; s < a.g.S; ++s) M = fmaxf(M, aa.part[((int64_t)s * a.B + i) * 2]);
    float Z = 0.f;
    for (int s = 0; s < a.g.S; ++s) {
        const float ms = aa.part[((int64_t)s * a.B + i) * 2], zs = aa.part[((int64_t)s * a.B + i) * 2 + 1];
        Z += ms == M ? zs : zs * __expf(ms - M);
    }
    const float lse = M + logf(Z), p = aa.pos[i];
    const float cf = (a.w ? a.w[i] : 1.f) / (float)a.B;
    const float l = (lse - p) * cf;
    aa.lse[i] = lse; a.coef[i] = cf;
    a.dpos[i] = fabsf(p) >= KGE_SIMPLE_CLAMP ? 0.f : -cf;      // (p is the clamped score: +-20 exactly where the raw one is saturated)
    if (a.row_pos) { a.row_pos[i] = 0.f; a.row_neg[i] = l; }
    if (a.acc) atomicAdd(&a.acc[2 * KGE_ACC_SLOTS + (i & (KGE_ACC_SLOTS - 1))], l);      // (one add per slot while B <= KGE_ACC_SLOTS)
}

// ---- GA = G . E without atomics: one part per split -----------------------------------------------------------------------------------
// grid (row tile, split, column group).  A workgroup's 128 x (64 NJ) block of GA stays in registers over its split's column tiles:
// wavefront w owns the 16 NJ columns d0 + 16 NJ w .. of all 128 rows, ga[ib][j][r] = (row 16 ib + 4 q + r, column dw + 16 j + m).
// The epilogue of the score tile, all in registers: clamp, then the criterion's dL/ds of the clamped score times the mask.  BCE: one
// thread per tile row keeps a cursor into its sorted list and sets the tile's label bits; column group 0 sums softplus(s) - y' s.
template <bool BCE, int NJ>
__global__ __launch_bounds__(KGE_BLOCK) void ace_bwd_a_kernel(AceArgs aa) {
    const KvaArgs &a = aa.k;
    __shared__ __attribute__((aligned(16))) TileLds lds;
    __shared__ __attribute__((aligned(16))) uint32_t lab[BCE ? TILE_BM : 1][4];      // bit c & 31 of word c >> 5 of a tile row
    __shared__ float sc[TILE_BM], sl[BCE ? 1 : TILE_BM];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int wr = wave >> 1, wc = wave & 1, m = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x * TILE_BM, sp = blockIdx.y, dw = blockIdx.z * 64 * NJ + wave * 16 * NJ;
    const bool first = blockIdx.z == 0;
    const int t0 = sp * a.g.tpa, t1 = min(t0 + a.g.tpa, a.g.NT);
    const float y0 = a.smooth / (float)a.n_ent, y1 = (1.f - a.smooth) + y0;
    ListCursor cu{0, 0, 0, -1};
    if (threadIdx.x < TILE_BM) {                   // (waves 0 and 1, whole)
        const int row = r0 + threadIdx.x;
        sc[threadIdx.x] = row < a.B ? a.coef[row] : 0.f;
        if constexpr (BCE) cu = cursor_at(a, range_of(a, row), (int64_t)t0 * TILE_BN);
        else sl[threadIdx.x] = aa.lse[min(row, a.B - 1)];
    }
    int dcl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) dcl[j] = min(dw + 16 * j + m, a.d - 1);
    f32x4 ga[8][NJ];
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int j = 0; j < NJ; ++j) ga[ib][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float rl[4][4];                                // BCE, [i][r]: loss sum of row 64 wr + 16 i + 4 q + r over this lane's columns
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rl[i][r] = 0.f;
    float *G = &lds[0][0];                         // [128 rows][KVA_LDG]: the G tile, first operand of the second product
    auto row_a = [&](int i) { return a.A + (int64_t)min(r0 + i, a.B - 1) * a.d; };
    for (int t = t0; t < t1; ++t) {
        const int64_t c0 = (int64_t)t * TILE_BN;
        auto row_b = [&](int j) { return a.ent + min(c0 + j, a.n_ent - 1) * (int64_t)a.d; };
        if constexpr (BCE) {
            if (threadIdx.x < TILE_BM) {           // (the previous tile's bits were last read ahead of two barriers)
                unsigned long long bits[2];
                label_bits<2>(a, cu, c0, bits);
                *reinterpret_cast<uint4 *>(&lab[threadIdx.x][0]) =
                    make_uint4((uint32_t)bits[0], (uint32_t)(bits[0] >> 32), (uint32_t)bits[1], (uint32_t)(bits[1] >> 32));
            }
        }
        {
            f32x4 acc[4][4];
            tile_gemm_128x128(lds, a.d, wave, row_a, row_b, acc);      // (its first barrier also publishes sc / sl / lab)
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) ok[j] = c0 + 64 * wc + 16 * j + m < a.n_ent;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 64 * wr + 16 * i + 4 * q + r;
                    const float c = sc[row];
                    float l = 0.f, ls = 0.f;
                    uint2 lw = make_uint2(0u, 0u);
                    if constexpr (BCE) lw = *reinterpret_cast<const uint2 *>(&lab[row][2 * wc]);
                    else l = sl[row];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int col = 64 * wc + 16 * j + m;
                        bool open;
                        const float s = clamp_score(acc[i][j][r], open);
                        float g;
                        if constexpr (BCE) {
                            const uint32_t word = j < 2 ? lw.x : lw.y;
                            const float y = (word >> (16 * (j & 1) + m)) & 1u ? y1 : y0;
                            float spl, sg;
                            bce_terms(s, spl, sg);
                            g = c * (sg - y);
                            if (first) ls += ok[j] ? fmaf(-y, s, spl) : 0.f;
                        } else g = c * __expf(s - l);
                        G[row * KVA_LDG + col] = ok[j] && open ? g : 0.f;
                    }
                    rl[i][r] += ls;
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
                const f32x4 af = *reinterpret_cast<const f32x4 *>(&G[(16 * ib + m) * KVA_LDG + kb * 16 + 4 * q]);
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
    if constexpr (BCE) {
        if (!first) return;                        // (uniform over the workgroup)
        // the 16 lanes of a row group (one DPP row), then the two column wavefronts through the stage buffers (free: the loop ends in a barrier)
        float *red = &lds[0][0];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = row_sum16(rl[i][r]);
                if (m == 0) red[wave * 64 + 16 * i + 4 * q + r] = v;
            }
        __syncthreads();
        const int row = threadIdx.x;
        if (row < TILE_BM && r0 + row < a.B) {
            const float *p = red + (row >> 6) * 2 * 64 + (row & 63);
            a.lpart[(int64_t)sp * a.B + r0 + row] = p[0] + p[64];
        }
    }
}

// ---- owner-computes dense gradient with the Adagrad update fused ---------------------------------------------------------------------
// A workgroup owns the entity rows e0 .. e0 + 64.  Per row tile of the batch: (BCE: label bits of the owned range, one bisection per
// tile row,) the 128 x 64 score tile, clamp and mask in its accumulators, G^T staged in LDS [entity][edge], then G^T . A_tile into
// gn[ib][j][r] = (entity 16 ib + 4 q + r, column 16 NJ wave + 16 j + m): wavefront w holds the columns 16 NJ w .. of all 64 rows,
// NJ = ceil(d / 64) <= 8.  No other workgroup reads these rows in this launch (each reads A and its own rows), so the update at the
// end races with nothing.
template <bool BCE, int NJ>
__global__ __launch_bounds__(KGE_BLOCK) void ace_bwd_e_kernel(AceArgs aa) {
    const KvaArgs &a = aa.k;
    __shared__ __attribute__((aligned(16))) Tile64Lds lds;
    __shared__ __attribute__((aligned(16))) uint32_t lab[BCE ? TILE_BM : 1][2];      // label bits of the owned rows, per edge of the row tile
    __shared__ float sq[KGE_WAVES_PER_BLOCK][KVA_EB], kk[KVA_EB];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int m = lane & 15, q = lane >> 4;
    const int64_t e0 = (int64_t)blockIdx.x * KVA_EB;
    const int dw = wave * 16 * NJ;
    const float y0 = a.smooth / (float)a.n_ent, y1 = (1.f - a.smooth) + y0;
    int dcl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) dcl[j] = min(dw + 16 * j + m, a.d - 1);
    f32x4 gn[4][NJ];
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int j = 0; j < NJ; ++j) gn[ib][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float *Gt = &lds[0][0];                        // [64 entities][KVA_LDG]: G transposed, first operand of the second product
    auto row_b = [&](int j) { return a.ent + min(e0 + j, a.n_ent - 1) * (int64_t)a.d; };
    ListRange lr{0, 0, -1};                        // BCE, of this thread's row of the NEXT row tile: requested a whole product ahead
    if constexpr (BCE) { if (threadIdx.x < TILE_BM) lr = range_of(a, (int)threadIdx.x); }
    for (int rt = 0; rt < a.g.RT; ++rt) {
        const int r0 = rt * TILE_BM;
        auto row_a = [&](int i) { return a.A + (int64_t)min(r0 + i, a.B - 1) * a.d; };
        if constexpr (BCE) {
            if (threadIdx.x < TILE_BM) {           // (the previous row tile's bits were last read ahead of two barriers)
                ListCursor cu = cursor_at(a, lr, e0);
                unsigned long long bits[1];
                label_bits<1>(a, cu, e0, bits);
                *reinterpret_cast<uint2 *>(&lab[threadIdx.x][0]) = make_uint2((uint32_t)bits[0], (uint32_t)(bits[0] >> 32));
                lr = range_of(a, r0 + TILE_BM + (int)threadIdx.x);
            }
        }
        {
            f32x4 acc[2][4];
            tile_gemm_128x64(lds, a.d, wave, row_a, row_b, acc);      // (its first barrier also publishes lab)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float c[4], l[4];
                uint2 lw[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tr = 32 * wave + 16 * i + 4 * q + r;
                    c[r] = r0 + tr < a.B ? a.coef[r0 + tr] : 0.f;
                    if constexpr (BCE) { lw[r] = *reinterpret_cast<const uint2 *>(&lab[tr][0]); l[r] = 0.f; }
                    else { l[r] = aa.lse[min(r0 + tr, a.B - 1)]; lw[r] = make_uint2(0u, 0u); }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = e0 + 16 * j + m < a.n_ent;
                    f32x4 g;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        bool open;
                        const float s = clamp_score(acc[i][j][r], open);
                        float gv;
                        if constexpr (BCE) {
                            const uint32_t word = j < 2 ? lw[r].x : lw[r].y;
                            const float y = (word >> (16 * (j & 1) + m)) & 1u ? y1 : y0;
                            float spl, sg;
                            bce_terms(s, spl, sg);
                            gv = c[r] * (sg - y);
                        } else gv = c[r] * __expf(s - l[r]);
                        g[r] = ok && open ? gv : 0.f;
                    }
                    *reinterpret_cast<f32x4 *>(&Gt[(16 * j + m) * KVA_LDG + 32 * wave + 16 * i + 4 * q]) = g;
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
                const f32x4 af = *reinterpret_cast<const f32x4 *>(&Gt[(16 * ib + m) * KVA_LDG + kb * 16 + 4 * q]);
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
    if (threadIdx.x < KVA_EB && e0 + threadIdx.x < a.n_ent) {
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

inline bool ace_ok(const AceArgs &aa, bool bce) {
    const KvaArgs &a = aa.k;
    if (!(a.B > 0 && a.n_ent > 0 && a.d >= 4 && a.d % 4 == 0 && a.d <= 512 && a.A && a.ent && a.ent_state && a.coef && a.GAp)) return false;
    if (bce) return a.m >= 0 && (a.m == 0 || (a.keys && a.vals)) && a.rng && a.own && a.lpart;
    return aa.part && aa.pos && aa.lse;
}

template <bool BCE>
void run_bwd_a(const AceArgs &a, hipStream_t s) {
    const dim3 g(a.k.g.RT, a.k.g.Sa, a.k.g.nslab), b(KGE_BLOCK);
    switch (a.k.g.nj) {
        case 1: hipLaunchKernelGGL((ace_bwd_a_kernel<BCE, 1>), g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL((ace_bwd_a_kernel<BCE, 2>), g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL((ace_bwd_a_kernel<BCE, 3>), g, b, 0, s, a); break;
        default: hipLaunchKernelGGL((ace_bwd_a_kernel<BCE, 4>), g, b, 0, s, a); break;
    }
}

template <bool BCE>
void run_bwd_e(const AceArgs &a, hipStream_t s) {
    const dim3 g((unsigned)((a.k.n_ent + KVA_EB - 1) / KVA_EB)), b(KGE_BLOCK);
    switch ((a.k.d + 63) / 64) {
        case 1: hipLaunchKernelGGL((ace_bwd_e_kernel<BCE, 1>), g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL((ace_bwd_e_kernel<BCE, 2>), g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL((ace_bwd_e_kernel<BCE, 3>), g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL((ace_bwd_e_kernel<BCE, 4>), g, b, 0, s, a); break;
        case 5: hipLaunchKernelGGL((ace_bwd_e_kernel<BCE, 5>), g, b, 0, s, a); break;
        case 6: hipLaunchKernelGGL((ace_bwd_e_kernel<BCE, 6>), g, b, 0, s, a); break;
        case 7: hipLaunchKernelGGL((ace_bwd_e_kernel<BCE, 7>), g, b, 0, s, a); break;
        default: hipLaunchKernelGGL((ace_bwd_e_kernel<BCE, 8>), g, b, 0, s, a); break;
    }
}

}  // namespace

int launch_ace_fwd(const AceArgs &a, hipStream_t s) {
    if (!ace_ok(a, false)) return KGE_ERR_ARG;
    hipLaunchKernelGGL(ace_fwd_kernel, dim3(a.k.g.RT, a.k.g.S), dim3(KGE_BLOCK), 0, s, a);
    return kge::check_launch();
}

int launch_ace_lse(const AceArgs &a, hipStream_t s) {
    if (!ace_ok(a, false) || !a.k.dpos) return KGE_ERR_ARG;
    hipLaunchKernelGGL(ace_lse_kernel, dim3((a.k.B + KGE_BLOCK - 1) / KGE_BLOCK), dim3(KGE_BLOCK), 0, s, a);
    return kge::check_launch();
}

int launch_ace_bwd_a(const AceArgs &a, bool bce, hipStream_t s) {
    if (!ace_ok(a, bce)) return KGE_ERR_ARG;
    if (bce) run_bwd_a<true>(a, s); else run_bwd_a<false>(a, s);
    return kge::check_launch();
}

int launch_ace_bwd_e(const AceArgs &a, bool bce, hipStream_t s) {
    if (!ace_ok(a, bce)) return KGE_ERR_ARG;
    if (bce) run_bwd_e<true>(a, s); else run_bwd_e<false>(a, s);
    return kge::check_launch();
}
