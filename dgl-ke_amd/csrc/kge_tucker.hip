// kge_tucker.hip - TuckER's edge side (include/kge_hip.h, KGE_TUCKER).  The core W[l][k][m] is ONE tensor for every edge of
// the batch, so each of the step's three contractions is a GEMM over the batch whose first operand is a Kronecker product of two
// gathered rows.  That operand is formed in the LDS stage or in the fragment read and never exists in memory:
//   tk_operand_kernel  A = (x (x) r) . W'   M = B, N = d_e, K = d_r d_e: the x tile is staged once per k-range, the r value multiplies
//                      the fragment as it is read; K is split over l, one part of A per split
//   tk_combine_kernel  the parts in split order -> A, p_i = a_i . y_i
//   tk_u_kernel        u_i = GA_i + dp_i y_i (the GA parts in part order), GY_i = dp_i a_i
//   tk_bwd_kernel      T = U . W'^T, M = B, N = the (l, k) columns, K = d_e, contracted in the tile epilogue: GX += r_il T in registers
//                      over the workgroup's l range (one part per range), GR[i][l] = sum_k x_ik T per l (one part per column group)
//   tk_gxr_kernel      the parts in order -> GX, GR (+ the regulariser's gradient of the relation row)
//   tk_core_kernel     a workgroup OWNS 64 core rows (consecutive k of one l): it walks the row tiles of the batch, stages its 64 x 128
//                      block of X^T in LDS, accumulates X^T . U_tile into a register-resident [64, d_e] gradient and applies the
//                      Adagrad rule to its rows itself - no gradient buffer for the core
// With the heads corrupted the reduction of the first two runs over (l, m) and the output index is k: the same core rows are read with
// the fragment's roles swapped (tk_load_b), there is no second copy of the core.
// Every sum has a fixed order: the results are bit-reproducible.  Matrix products are fp32 MFMA (16 x 16 x 4); no atomics.
#include <cmath>
#include "kge_tucker.hpp"

#define TK_BM 128                                  // edges of a row tile
#define TK_LDX 36                                  // dwords per staged row of a [128 x 32] chunk: 4 x odd, as TILE_LD
#define TK_LDR 33                                  // dwords per staged row of the [128 x 32] block of r values
#define TK_LDT 132                                 // dwords per staged row of the owner kernel's [64 x 128] block of X^T
#define TK_OB 64                                   // core rows a workgroup of tk_core_kernel owns

namespace {
using namespace kge;

// The second operand's fragment for 16 reduction indices of MFMA k-block `k4` = k0 + 4 q (this lane's four) and the lane's output
// columns dcl[j], from the core rows of one l (cl = core + l d_e d_e).
//   ROWRED   the reduction index is the ROW of W[l] (k), the output column its column (m): four rows, one float each per block
//   !ROWRED  the reduction index is the COLUMN of W[l] (m), the output column its row (k): one float4 of row dcl[j] per block
// Indices beyond d_e are clamped in-bounds: the first operand is staged as zeros there (the convention of ova_bwd_a_kernel's clamped
// rows: a NON-FINITE core entry in the last row / column would turn such a 0 . inf into NaN in outputs it does not touch).
// ROWRED costs 4 NJ scalar global loads per 16-row block of MFMA work, !ROWRED NJ float4 loads; neither goes through LDS.
template <int NJ, bool ROWRED>
__device__ __forceinline__ void tk_load_b(const float *cl, int de, int k4, const int (&dcl)[NJ], f32x4 (&bf)[NJ]) {
    if (ROWRED) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float *row = cl + (int64_t)min(k4 + e, de - 1) * de;
#pragma unroll
            for (int j = 0; j < NJ; ++j) bf[j][e] = row[dcl[j]];
        }
    } else {
        const int c = min(k4, de - 4);
#pragma unroll
        for (int j = 0; j < NJ; ++j) bf[j] = *reinterpret_cast<const f32x4 *>(cl + (int64_t)dcl[j] * de + c);
    }
}

// thread t stages 16 floats of row t >> 1 of a [128 x 32] chunk: columns k0 + 16 (t & 1) .. of `rowp`, zeros beyond d_e / the batch
__device__ __forceinline__ void tk_stage(float *xs, const float *rowp, bool valid, int k0, int de) {
    const int sh = (threadIdx.x & 1) * 16;
    float *dst = xs + (threadIdx.x >> 1) * TK_LDX + sh;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = k0 + sh + 4 * i;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (valid && c < de) v = *reinterpret_cast<const f32x4 *>(rowp + c);
        *reinterpret_cast<f32x4 *>(dst + 4 * i) = v;
    }
}
// ... and 16 of the 32 r values l = lc + 16 (t & 1) .. of its row, zeros from l1 on
__device__ __forceinline__ void tk_stage_r(float *rs, const float *rptr, bool valid, int lc, int l1) {
    const int sh = (threadIdx.x & 1) * 16;
    float *dst = rs + (threadIdx.x >> 1) * TK_LDR + sh;
#pragma unroll
    for (int i = 0; i < 16; ++i) dst[i] = (valid && lc + sh + i < l1) ? rptr[lc + sh + i] : 0.f;
}

// ---- the operand: A = (x (x) r) . W' in parts ---------------------------------------------------------------------------------------
// grid (row tile, split of l, column group).  Wavefront w owns the 16 NJ output columns dw .. of all 128 rows:
// ga[ib][j][r] = (row 16 ib + 4 q + r, column dw + 16 j + m).  Per 32 l values the r block is staged once, per 32 reduction indices of
// the inner side (k, heads: m) the x chunk once; the first operand's fragment is x_chunk[row][k] * r[row][l], formed in registers.
template <int NJ, bool HEADS>
__global__ __launch_bounds__(KGE_BLOCK) void tk_operand_kernel(TkArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[TK_BM * TK_LDX];
    __shared__ float rs[TK_BM * TK_LDR];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int m = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x * TK_BM, sp = blockIdx.y, dw = blockIdx.z * 64 * NJ + wave * 16 * NJ;
    const int de = a.de, l0 = sp * a.g.lpo, l1 = min(l0 + a.g.lpo, a.dr);
    const int srow = min(r0 + (int)(threadIdx.x >> 1), a.B - 1);
    const bool svalid = r0 + (int)(threadIdx.x >> 1) < a.B;
    const float *xptr = a.ent + a.xid[srow] * (int64_t)de, *rptr = a.rel + a.rid[srow] * (int64_t)a.dr;
    int dcl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) dcl[j] = min(dw + 16 * j + m, de - 1);
    f32x4 ga[8][NJ];
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int j = 0; j < NJ; ++j) ga[ib][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int lc = l0; lc < l1; lc += 32) {
        const int nl = min(32, l1 - lc);
        __syncthreads();                           // the previous block's fragment reads are done
        tk_stage_r(rs, rptr, svalid, lc, l1);
        for (int k0 = 0; k0 < de; k0 += 32) {
            __syncthreads();
            tk_stage(xs, xptr, svalid, k0, de);
            __syncthreads();
#pragma unroll 1
            for (int l = 0; l < nl; ++l) {
                const float *cl = a.core + (int64_t)(lc + l) * de * de;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    if (k0 + kb * 16 >= de) break;
                    f32x4 bf[NJ];
                    tk_load_b<NJ, !HEADS>(cl, de, k0 + kb * 16 + 4 * q, dcl, bf);
#pragma unroll
                    for (int ib = 0; ib < 8; ++ib) {
                        const float rv = rs[(16 * ib + m) * TK_LDR + l];
                        f32x4 af = *reinterpret_cast<const f32x4 *>(&xs[(16 * ib + m) * TK_LDX + kb * 16 + 4 * q]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float v = af[e] * rv;
#pragma unroll
                            for (int j = 0; j < NJ; ++j) ga[ib][j] = MFMA16(v, bf[j][e], ga[ib][j]);
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + 16 * ib + 4 * q + r;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int dc = dw + 16 * j + m;
                if (row < a.B && dc < de) a.Ap[((int64_t)sp * a.B + row) * de + dc] = ga[ib][j][r];
            }
        }
}

// ---- one wavefront per edge: the parts of A in split order, p = a . y ---------------------------------------------------------------
__global__ __launch_bounds__(KGE_BLOCK) void tk_combine_kernel(TkArgs a) {
    const int row = blockIdx.x * KGE_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.B) return;                        // (wave-uniform)
    const float *y = a.ent + a.yid[row] * (int64_t)a.de;
    float p = 0.f;
    for (int c = lane; c < a.de; c += 64) {
        float v = 0.f;
        for (int s = 0; s < a.g.So; ++s) v += a.Ap[((int64_t)s * a.B + row) * a.de + c];
        a.A[(int64_t)row * a.de + c] = v;
        p = fmaf(v, y[c], p);
    }
    p = wave_sum(p);
    if (lane == 0) a.P[row] = p;
}

// ---- one wavefront per edge: u = GA + dp y (the GA parts in part order), GY = dp a ---------------------------------------------------
__global__ __launch_bounds__(KGE_BLOCK) void tk_u_kernel(TkArgs a) {
    const int row = blockIdx.x * KGE_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.B) return;
    const float *y = a.ent + a.yid[row] * (int64_t)a.de;
    const float dp = a.dP[row];
    for (int c = lane; c < a.de; c += 64) {
        float g = 0.f;
        for (int s = 0; s < a.ga_parts; ++s) g += a.GAp[((int64_t)s * a.B + row) * a.de + c];
        a.U[(int64_t)row * a.de + c] = fmaf(dp, y[c], g);
        a.GY[(int64_t)row * a.de + c] = dp * a.A[(int64_t)row * a.de + c];
    }
}

// ---- the backward: T = U . W'^T contracted in the epilogue, T never stored ----------------------------------------------------------
// grid (row tile, range of l, column group).  Per l: t[ib][j][r] = (row 16 ib + 4 q + r, column c0 + 16 j + m) of the [128 x 64 NJ]
// tile of T over K = d_e (U staged in chunks of 32); then gx += r_il t (registers, over the l range) and GR[i][l] = sum over the
// group's columns of x t (DPP row sum, the four wavefronts through LDS in wavefront order).
template <int NJ, bool HEADS>
__global__ __launch_bounds__(KGE_BLOCK) void tk_bwd_kernel(TkArgs a) {
    __shared__ __attribute__((aligned(16))) float us[TK_BM * TK_LDX];
    __shared__ float rs[TK_BM * TK_LDR];
    __shared__ float red[KGE_WAVES_PER_BLOCK][TK_BM];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int m = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x * TK_BM, sp = blockIdx.y, c0 = blockIdx.z * 64 * NJ + wave * 16 * NJ;
    const int de = a.de, l0 = sp * a.g.lpb, l1 = min(l0 + a.g.lpb, a.dr);
    const int srow = min(r0 + (int)(threadIdx.x >> 1), a.B - 1);
    const bool svalid = r0 + (int)(threadIdx.x >> 1) < a.B;
    const float *uptr = a.U + (int64_t)srow * de, *rptr = a.rel + a.rid[srow] * (int64_t)a.dr;
    int dcl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) dcl[j] = min(c0 + 16 * j + m, de - 1);
    f32x4 xk[8][NJ], gx[8][NJ];                    // x at this lane's (row, column) pairs: zero beyond the batch and beyond d_e
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + 16 * ib + 4 * q + r;
            const float *x = a.ent + a.xid[min(row, a.B - 1)] * (int64_t)de;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                xk[ib][j][r] = (row < a.B && c0 + 16 * j + m < de) ? x[dcl[j]] : 0.f;
                gx[ib][j][r] = 0.f;
            }
        }
    for (int lc = l0; lc < l1; lc += 32) {
        const int nl = min(32, l1 - lc);
        __syncthreads();
        tk_stage_r(rs, rptr, svalid, lc, l1);
#pragma unroll 1
        for (int l = 0; l < nl; ++l) {
            const float *cl = a.core + (int64_t)(lc + l) * de * de;
            f32x4 t[8][NJ];
#pragma unroll
            for (int ib = 0; ib < 8; ++ib)
#pragma unroll
                for (int j = 0; j < NJ; ++j) t[ib][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < de; k0 += 32) {
                __syncthreads();                   // (also: rs is staged, red of the previous l has been read)
                tk_stage(us, uptr, svalid, k0, de);
                __syncthreads();
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    if (k0 + kb * 16 >= de) break;
                    f32x4 bf[NJ];
                    tk_load_b<NJ, HEADS>(cl, de, k0 + kb * 16 + 4 * q, dcl, bf);
#pragma unroll
                    for (int ib = 0; ib < 8; ++ib) {
                        const f32x4 af = *reinterpret_cast<const f32x4 *>(&us[(16 * ib + m) * TK_LDX + kb * 16 + 4 * q]);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int j = 0; j < NJ; ++j) t[ib][j] = MFMA16(af[e], bf[j][e], t[ib][j]);
                    }
                }
            }
#pragma unroll
            for (int ib = 0; ib < 8; ++ib)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float rv = rs[(16 * ib + 4 * q + r) * TK_LDR + l];
                    float g = 0.f;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        gx[ib][j][r] = fmaf(rv, t[ib][j][r], gx[ib][j][r]);
                        g = fmaf(xk[ib][j][r], t[ib][j][r], g);
                    }
                    g = row_sum16(g);
                    if (m == 0) red[wave][16 * ib + 4 * q + r] = g;
                }
            __syncthreads();
            if (threadIdx.x < TK_BM && r0 + threadIdx.x < a.B) {
                const int i = threadIdx.x;
                a.GRp[((int64_t)blockIdx.z * a.B + r0 + i) * a.dr + lc + l] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
            }
        }
    }
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + 16 * ib + 4 * q + r;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int dc = c0 + 16 * j + m;
                if (row < a.B && dc < de) a.GXp[((int64_t)sp * a.B + row) * de + dc] = gx[ib][j][r];
            }
        }
}

// ---- one wavefront per edge: GX from its parts in range order, GR from its parts in group order (+ the regulariser) -------------------
__global__ __launch_bounds__(KGE_BLOCK) void tk_gxr_kernel(TkArgs a) {
    const int row = blockIdx.x * KGE_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.B) return;
    for (int c = lane; c < a.de; c += 64) {
        float v = 0.f;
        for (int s = 0; s < a.g.Sb; ++s) v += a.GXp[((int64_t)s * a.B + row) * a.de + c];
        a.GX[(int64_t)row * a.de + c] = v;
    }
    const float *rr = a.rel + a.rid[row] * (int64_t)a.dr;
    const bool reg = a.reg_coef > 0.f && a.reg_norm > 0;
    for (int l = lane; l < a.dr; l += 64) {
        float v = 0.f;
        for (int s = 0; s < a.g.nslabb; ++s) v += a.GRp[((int64_t)s * a.B + row) * a.dr + l];
        if (reg) v += reg_grad(rr[l], a.reg_coef, a.reg_norm);
        a.GR[(int64_t)row * a.dr + l] = v;
    }
}

// ---- owner-computes core gradient with the Adagrad update fused ------------------------------------------------------------------
// A workgroup owns the core rows (l, k0 .. k0 + 64), k < d_e.  Per row tile of the batch its [64 x 128] block of X^T goes to LDS
// [k][edge]: r_il x_ik (heads: r_il u_ik); the second operand is the tile's rows of U (heads: x) read as ova_bwd_e_kernel reads A.
// gn[ib][j][r] = (core row k0 + 16 ib + 4 q + r, column 16 NJ wave + 16 j + m), NJ = ceil(d_e / 64) <= 8.  No other workgroup reads
// or writes these core rows in this launch.
template <int NJ, bool HEADS>
__global__ __launch_bounds__(KGE_BLOCK) void tk_core_kernel(TkArgs a) {
    __shared__ __attribute__((aligned(16))) float Xt[TK_OB * TK_LDT];
    __shared__ float sq[KGE_WAVES_PER_BLOCK][TK_OB], kk[TK_OB];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int m = lane & 15, q = lane >> 4;
    const int de = a.de, l = blockIdx.x / a.g.NO, k0 = (blockIdx.x % a.g.NO) * TK_OB;
    const int dw = wave * 16 * NJ;
    int dcl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) dcl[j] = min(dw + 16 * j + m, de - 1);
    f32x4 gn[4][NJ];
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int j = 0; j < NJ; ++j) gn[ib][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int si = threadIdx.x & (TK_BM - 1), sk = 32 * (int)(threadIdx.x >> 7);      // staging: edge si, k values k0 + sk .. + 32
    for (int rt = 0; rt < a.g.RT; ++rt) {
        const int r0 = rt * TK_BM;
        {
            const int row = min(r0 + si, a.B - 1);
            const bool valid = r0 + si < a.B;
            const float *src = HEADS ? a.U + (int64_t)row * de : a.ent + a.xid[row] * (int64_t)de;
            const float rl = valid ? a.rel[a.rid[row] * (int64_t)a.dr + l] : 0.f;
            __syncthreads();                       // the previous tile's fragment reads are done
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int k = k0 + sk + 4 * c;
                f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (valid && k < de) v = *reinterpret_cast<const f32x4 *>(src + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) Xt[(sk + 4 * c + e) * TK_LDT + si] = v[e] * rl;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int kb = 0; kb < TK_BM / 16; ++kb) {      // 16 edges: k = 4 q + e of four MFMAs
            f32x4 bf[NJ];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = min(r0 + kb * 16 + 4 * q + e, a.B - 1);      // (X^T is 0 beyond the batch)
                const float *br = HEADS ? a.ent + a.xid[row] * (int64_t)de : a.U + (int64_t)row * de;
#pragma unroll
                for (int j = 0; j < NJ; ++j) bf[j][e] = br[dcl[j]];
            }
#pragma unroll
            for (int ib = 0; ib < 4; ++ib) {
                const f32x4 af = *reinterpret_cast<const f32x4 *>(&Xt[(16 * ib + m) * TK_LDT + kb * 16 + 4 * q]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) gn[ib][j] = MFMA16(af[e], bf[j][e], gn[ib][j]);
            }
        }
    }
    // ---- Adagrad on the owned rows: state += mean(G^2), row -= lr G / (sqrt(state) + eps) - the update launch's rule ----
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) ss = dw + 16 * j + m < de ? fmaf(gn[ib][j][r], gn[ib][j][r], ss) : ss;
            ss = row_sum16(ss);
            if (m == 0) sq[wave][16 * ib + 4 * q + r] = ss;
        }
    __syncthreads();
    const int64_t row0 = (int64_t)l * de + k0;     // the owned rows: row0 + er, k0 + er < d_e (never into the next l)
    if (threadIdx.x < TK_OB && k0 + (int)threadIdx.x < de) {
        const int er = threadIdx.x;
        const float tot = ((sq[0][er] + sq[1][er]) + sq[2][er]) + sq[3][er];
        const float sn = a.core_state[row0 + er] + tot / (float)de;
        a.core_state[row0 + er] = sn;
        kk[er] = -a.lr / (sqrtf(sn) + a.eps);
    }
    __syncthreads();
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int er = 16 * ib + 4 * q + r;
            if (k0 + er >= de) continue;
            const float k = kk[er];
            float *row = a.core + (row0 + er) * de;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int dc = dw + 16 * j + m;
                if (dc < de) row[dc] = fmaf(gn[ib][j][r], k, row[dc]);
            }
        }
}

inline bool tk_width(int d) { return d >= 4 && d <= 512 && d % 4 == 0; }
inline bool tk_ok(const TkArgs &a) { return a.B > 0 && tk_width(a.de) && tk_width(a.dr); }
inline dim3 tk_rows(const TkArgs &a) { return dim3((a.B + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK); }

template <bool HEADS>
void tk_operand_launch(const TkArgs &a, hipStream_t s) {
    const dim3 g(a.g.RT, a.g.So, a.g.nslab), b(KGE_BLOCK);
    switch (a.g.nj) {
        case 1: hipLaunchKernelGGL((tk_operand_kernel<1, HEADS>), g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL((tk_operand_kernel<2, HEADS>), g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL((tk_operand_kernel<3, HEADS>), g, b, 0, s, a); break;
        default: hipLaunchKernelGGL((tk_operand_kernel<4, HEADS>), g, b, 0, s, a); break;
    }
}
template <bool HEADS>
void tk_bwd_launch(const TkArgs &a, hipStream_t s) {
    const dim3 g(a.g.RT, a.g.Sb, a.g.nslabb), b(KGE_BLOCK);
    if (a.g.njb == 1) hipLaunchKernelGGL((tk_bwd_kernel<1, HEADS>), g, b, 0, s, a);
    else hipLaunchKernelGGL((tk_bwd_kernel<2, HEADS>), g, b, 0, s, a);
}
template <bool HEADS>
void tk_core_launch(const TkArgs &a, hipStream_t s) {
    const dim3 g((unsigned)(a.dr * a.g.NO)), b(KGE_BLOCK);
    switch (a.g.NO) {
        case 1: hipLaunchKernelGGL((tk_core_kernel<1, HEADS>), g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL((tk_core_kernel<2, HEADS>), g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL((tk_core_kernel<3, HEADS>), g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL((tk_core_kernel<4, HEADS>), g, b, 0, s, a); break;
        case 5: hipLaunchKernelGGL((tk_core_kernel<5, HEADS>), g, b, 0, s, a); break;
        case 6: hipLaunchKernelGGL((tk_core_kernel<6, HEADS>), g, b, 0, s, a); break;
        case 7: hipLaunchKernelGGL((tk_core_kernel<7, HEADS>), g, b, 0, s, a); break;
        default: hipLaunchKernelGGL((tk_core_kernel<8, HEADS>), g, b, 0, s, a); break;
    }
}

}  // namespace

int launch_tk_operand(const TkArgs &a, hipStream_t s) {
    if (!tk_ok(a)) return KGE_ERR_ARG;
    if (a.heads) tk_operand_launch<true>(a, s); else tk_operand_launch<false>(a, s);
    if (int rc = kge::check_launch()) return rc;
    hipLaunchKernelGGL(tk_combine_kernel, tk_rows(a), dim3(KGE_BLOCK), 0, s, a);
    return kge::check_launch();
}

int launch_tk_u(const TkArgs &a, hipStream_t s) {
    if (!tk_ok(a)) return KGE_ERR_ARG;
    hipLaunchKernelGGL(tk_u_kernel, tk_rows(a), dim3(KGE_BLOCK), 0, s, a);
    return kge::check_launch();
}

int launch_tk_bwd(const TkArgs &a, hipStream_t s) {
    if (!tk_ok(a)) return KGE_ERR_ARG;
    if (a.heads) tk_bwd_launch<true>(a, s); else tk_bwd_launch<false>(a, s);
    if (int rc = kge::check_launch()) return rc;
    hipLaunchKernelGGL(tk_gxr_kernel, tk_rows(a), dim3(KGE_BLOCK), 0, s, a);
    return kge::check_launch();
}

int launch_tk_core(const TkArgs &a, hipStream_t s) {
    if (!tk_ok(a)) return KGE_ERR_ARG;
    if (a.heads) tk_core_launch<true>(a, s); else tk_core_launch<false>(a, s);
    return kge::check_launch();
}
