// kge_pairre.hip - PairRE (Chao et al., ACL 2021; include/kge_hip.h, enum kge_model): paired relation vectors r = [rH | rT] on
// unit-normalised entity rows,  s(h, r, t) = gamma - sum_k |h^_k rH_k - t^_k rT_k|,  x^ = x / |x|_2 (0 where |x|_2 == 0).
//
// The chunked score has ONE form for both corruption sides: per edge a pair of vectors (a, w) -
//     tails corrupted  a = h^ o rH, w = rT;      heads corrupted  a = t^ o rT, w = rH
// - and per candidate row its norm, so that  s_ij = gamma - sum_k |a_ik - w_ik n^_jk|.  The candidate side is scaled per edge:
// no GEMM form; a VALU pairwise reduction like TransE_l1's (kge_neg_pair.hip) with a second per-edge operand.
//
//   pairre_edge_fwd_kernel   one wavefront per edge: row norms, positive score, (a, w); further wavefronts, one per candidate
//                            row: the row's norm (and its dense copy)
//   pairre_fwd_kernel        32 x 32 score tile per workgroup, 2 x 2 per thread, a / w / n^ staged through LDS as [k][row] in
//                            slabs of 32 columns (the candidate slab is normalised while it is staged)
//   pairre_bwd_kernel        [32 rows x 32 k] tiles of (Ga, Gw) and of Gn^ = dL/dn^, the reduction index in slabs of 32 through LDS
//   pairre_row_adj_kernel    Gn^ -> the raw candidate row's gradient through the normalisation (+ regulariser), per occurrence
//   pairre_edge_bwd_kernel   (Ga, Gw, dL/dp) -> per-edge gradients of the head, tail and relation rows
// Every difference is formed as fmaf(-w, n^, a) with a rounded on its own, in every kernel: forward, backward and ranking see the
// same sign for the same operands.  No atomics; every sum has a fixed order.
#include "kge_common.hpp"

using namespace kge;

#define QT 32          // tile edge
#define QK 32          // columns of a backward output tile
#define QS 32          // staged slab: k of the forward tile, reduction index of a backward tile (a multiple of 32).  Measured at the
                       // FB15k shape: 32 -> 143.4 us per step, 128 (51 KB of LDS, a quarter of the load rounds and barriers) -> 187.7 us
#define QLD (QT + 2)   // padded leading dimension (float2 alignment kept, bank aliasing broken)

namespace {

// |x|_2 of a row, in every lane: lane-strided squares, then the fixed-order wavefront sum.  The ONE norm routine: an entity row has
// the same norm bit for bit as a head / tail row (edge kernels) and as a candidate row (norm jobs)
__device__ __forceinline__ float pr_norm(const float *x, int d, int lane) {
    float s = 0.f;
    for (int k = lane; k < d; k += KGE_WAVE) s = fmaf(x[k], x[k], s);
    return sqrtf(wave_sum(s));
}
__device__ __forceinline__ float pr_unit(float x, float n) { return n > 0.f ? x / n : 0.f; }
__device__ __forceinline__ float pr_diff(float a, float w, float n) { return fmaf(-w, n, a); }

__global__ __launch_bounds__(KGE_BLOCK) void pairre_edge_fwd_kernel(PairreEdgeArgs a) {
    const int64_t w = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, D = a.d_e;
    if (w < a.B) {
        const int64_t i = w;
        const float *h = row_ptr(a.src.hbase, a.src.hidx, i, D);
        const float *t = row_ptr(a.src.tbase, a.src.tidx, i, D);
        const float *r = row_ptr(a.src.rbase, a.src.ridx, i, 2 * D);
        const float nh = pr_norm(h, D, lane), nt = pr_norm(t, D, lane);
        // own side: the entity row inside a; other side: the corrupted one
        const float *xo = a.neg_head ? t : h, *xc = a.neg_head ? h : t;
        const float no = a.neg_head ? nt : nh, nc = a.neg_head ? nh : nt;
        const float *ro = a.neg_head ? r + D : r, *rw = a.neg_head ? r : r + D;
        float *A = a.A ? a.A + i * (int64_t)D : nullptr, *W = a.W ? a.W + i * (int64_t)D : nullptr;
        float ps = 0.f;
        for (int k = lane; k < D; k += KGE_WAVE) {
            const float av = pr_unit(xo[k], no) * ro[k], wv = rw[k];
            ps += fabsf(pr_diff(av, wv, pr_unit(xc[k], nc)));
            if (A) A[k] = av;
            if (W) W[k] = wv;
        }
        if (a.pos_score) {
            ps = wave_sum(ps);
            if (lane == 0) a.pos_score[i] = a.gamma - ps;
        }
    } else if (w < (int64_t)a.B + a.n_neg) {
        const int64_t j = w - a.B;
        int64_t jx = j;
        const int64_t *jidx = a.nidx;
        if (a.nd_own) {                  // neg_deg_sample: in-batch rows first, then the sampled ones
            const int Np = a.nd_chunk + a.nd_Ns, c = (int)(j / Np), jj = (int)(j % Np);
            if (jj < a.nd_chunk) { jidx = a.nd_own; jx = (int64_t)c * a.nd_chunk + jj; }
            else jx = (int64_t)c * a.nd_Ns + jj - a.nd_chunk;
        }
        const float *x = row_ptr(a.nbase, jidx, jx, D);
        if (a.Bn) {
            float *cp = a.Bn + j * (int64_t)D;
            for (int k = lane; k < D; k += KGE_WAVE) cp[k] = x[k];
        }
        const float n = pr_norm(x, D, lane);
        if (a.nrm && lane == 0) a.nrm[j] = n;
    }
}

// one operand's [QT rows x QS k] slab, global -> registers -> LDS as dst[k][row]: thread t holds row t / 8, columns
// 32 m + (t % 8) * 4 .. + 3 (m < QS / 32) of the slab.  p: the thread's row or null (row beyond the tile's rows); columns beyond K and
// null rows are zero-filled.  The loads of all operands are issued before the first store (pr_put), one latency per slab
struct PrSlab { float v[QS / 32][4]; };
__device__ __forceinline__ PrSlab pr_get(const float *p, int k0, int K) {
    const int kk = (threadIdx.x & 7) * 4;
    PrSlab s;
#pragma unroll
    for (int m = 0; m < QS / 32; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + 32 * m + kk + e;
            s.v[m][e] = (p && k < K) ? p[k] : 0.f;
        }
    return s;
}
__device__ __forceinline__ void pr_put(float (*dst)[QLD], const PrSlab &s, bool unit, float nrm) {
    const int rr = threadIdx.x >> 3, kk = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int m = 0; m < QS / 32; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[32 * m + kk + e][rr] = unit ? pr_unit(s.v[m][e], nrm) : s.v[m][e];
}

// ------------------------------------------------------------------------------------------
// forward: S[c, i, j] = gamma - sum_k |a_ik - w_ik n^_jk|
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KGE_BLOCK) void pairre_fwd_kernel(PairreNegArgs a, int ti, int tj) {
    __shared__ __attribute__((aligned(16))) float As[QS][QLD];
    __shared__ __attribute__((aligned(16))) float Ws[QS][QLD];
    __shared__ __attribute__((aligned(16))) float Bs[QS][QLD];
    const int tile = blockIdx.x;
    const int jt = tile % tj, it = (tile / tj) % ti, c = tile / (tj * ti);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int D = a.d_e;
    const int i0 = it * QT, j0 = jt * QT;
    const int ni = min(QT, a.chunk - i0), nj = min(QT, a.N - j0);
    // this thread's staging rows (row threadIdx.x / 8 of each operand)
    const int rr = threadIdx.x >> 3;
    const int64_t arow = (int64_t)c * a.chunk + i0 + rr, brow = (int64_t)c * a.N + j0 + rr;
    const float *ap = rr < ni ? a.A + arow * D : nullptr, *wp = rr < ni ? a.W + arow * D : nullptr;
    const float *bp = rr < nj ? row_ptr(a.nbase, a.nidx, brow, D) : nullptr;
    const float bn = rr < nj ? a.nrm[brow] : 0.f;
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    for (int k0 = 0; k0 < D; k0 += QS) {
        const PrSlab sa = pr_get(ap, k0, D), sw = pr_get(wp, k0, D), sb = pr_get(bp, k0, D);
        __syncthreads();
        pr_put(As, sa, false, 0.f);
        pr_put(Ws, sw, false, 0.f);
        pr_put(Bs, sb, true, bn);
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < QS; ++k) {            // (columns beyond d_e are zero in all three slabs: they add |0 - 0 * 0|)
            const float2 av = *reinterpret_cast<const float2 *>(&As[k][2 * ty]);
            const float2 wv = *reinterpret_cast<const float2 *>(&Ws[k][2 * ty]);
            const float2 bv = *reinterpret_cast<const float2 *>(&Bs[k][2 * tx]);
            acc[0][0] += fabsf(pr_diff(av.x, wv.x, bv.x));
            acc[0][1] += fabsf(pr_diff(av.x, wv.x, bv.y));
            acc[1][0] += fabsf(pr_diff(av.y, wv.y, bv.x));
            acc[1][1] += fabsf(pr_diff(av.y, wv.y, bv.y));
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = i0 + 2 * ty + r, j = j0 + 2 * tx + s;
            if (i < a.chunk && j < a.N) a.S[((int64_t)c * a.chunk + i) * a.N + j] = a.gamma - acc[r][s];
        }
}

// ------------------------------------------------------------------------------------------
// backward, with sigma_ijk = sign(a_ik - w_ik n^_jk) and G = dL/ds:
//   row tiles  (r = edge i, reduction s = candidate j):   Ga_ik = -sum_j G sigma,   Gw_ik = +sum_j G sigma n^_jk
//   cand tiles (r = candidate j, reduction s = edge i):    Gn^_jk = +sum_i G sigma w_ik
// A workgroup owns a [32 rows x 32 k] output tile and walks the reduction index in slabs of 32; G and the other side's operands
// go through LDS, the tile's own operands live in registers.  The first C * ti * tk workgroups are row tiles.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KGE_BLOCK) void pairre_bwd_kernel(PairreNegArgs a, int ti, int tj, int tk) {
    __shared__ __attribute__((aligned(16))) float Gs[QS][QLD];      // [s][r]
    __shared__ __attribute__((aligned(16))) float Y0[QS][QLD];      // [s][k]: row tiles n^; cand tiles a
    __shared__ __attribute__((aligned(16))) float Y1[QS][QLD];      // [s][k]: cand tiles w
    const int nGA = a.C * ti * tk;
    int tile = blockIdx.x;
    const bool isGA = tile < nGA;
    if (!isGA) tile -= nGA;
    const int tr = isGA ? ti : tj;
    const int kt = tile % tk, rt = (tile / tk) % tr, c = tile / (tk * tr);
    const int D = a.d_e;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int R = isGA ? a.chunk : a.N;          // rows of this product (per chunk)
    const int S = isGA ? a.N : a.chunk;          // reduction length
    const int r0 = rt * QT, k0 = kt * QK;
    const float *Gc = a.G + (int64_t)c * a.chunk * a.N;
    // the tile's own operands, 2 rows x 2 k: (a, w) or (n^, -)
    float x0[2][2], x1[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = min(r0 + 2 * ty + r, R - 1);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = k0 + 2 * tx + q;
            x0[r][q] = 0.f; x1[r][q] = 0.f;
            if (k < D) {
                if (isGA) {
                    const int64_t o = ((int64_t)c * a.chunk + row) * D + k;
                    x0[r][q] = a.A[o]; x1[r][q] = a.W[o];
                } else {
                    const int64_t j = (int64_t)c * a.N + row;
                    x0[r][q] = pr_unit(row_ptr(a.nbase, a.nidx, j, D)[k], a.nrm[j]);
                }
            }
        }
    }
    float o0[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, o1[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    for (int s0 = 0; s0 < S; s0 += QS) {
        // G tile: Gs[s][r] = G(r0 + r, s0 + s); the other side's slab as [s][k]: thread t -> rows s = 32 m + t / 8, k = (t % 8) * 4 .. + 3.
        // All of a slab's loads are requested before the barrier and the first LDS store
        float gv_[QS / 8];
        {
            const int t = threadIdx.x;
#pragma unroll
            for (int e = 0; e < QS / 8; ++e) {
                const int lin = t + e * KGE_BLOCK;      // 0 .. 32 QS - 1
                int rr, ss;
                if (isGA) { rr = lin / QS; ss = lin % QS; }   // contiguous along s (= j)
                else      { ss = lin >> 5; rr = lin & 31; }   // contiguous along r (= j)
                const int gr = r0 + rr, gs = s0 + ss;
                float v = 0.f;
                if (gr < R && gs < S) {
                    const int i = isGA ? gr : gs, j = isGA ? gs : gr;
                    v = Gc[(int64_t)i * a.N + j];
                }
                gv_[e] = v;
            }
        }
        float v0[QS / 32][4], v1[QS / 32][4];
        {
            const int t = threadIdx.x;
            const int kk = (t & 7) * 4;
#pragma unroll
            for (int m = 0; m < QS / 32; ++m) {
                const int gs = s0 + 32 * m + (t >> 3);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v0[m][e] = 0.f; v1[m][e] = 0.f; }
                if (gs < S) {
                    if (isGA) {
                        const int64_t j = (int64_t)c * a.N + gs;
                        const float *yp = row_ptr(a.nbase, a.nidx, j, D);
                        const float ny = a.nrm[j];
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const int k = k0 + kk + e; if (k < D) v0[m][e] = pr_unit(yp[k], ny); }
                    } else {
                        const int64_t o = ((int64_t)c * a.chunk + gs) * D;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const int k = k0 + kk + e; if (k < D) { v0[m][e] = a.A[o + k]; v1[m][e] = a.W[o + k]; } }
                    }
                }
            }
        }
        __syncthreads();
        {
            const int t = threadIdx.x;
#pragma unroll
            for (int e = 0; e < QS / 8; ++e) {
                const int lin = t + e * KGE_BLOCK;
                if (isGA) Gs[lin % QS][lin / QS] = gv_[e]; else Gs[lin >> 5][lin & 31] = gv_[e];
            }
            const int kk = (t & 7) * 4;
#pragma unroll
            for (int m = 0; m < QS / 32; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) { Y0[32 * m + (t >> 3)][kk + e] = v0[m][e]; Y1[32 * m + (t >> 3)][kk + e] = v1[m][e]; }
        }
        __syncthreads();
        const int smax = min(QS, S - s0);
        for (int s = 0; s < smax; ++s) {
            const float2 gv = *reinterpret_cast<const float2 *>(&Gs[s][2 * ty]);
            const float2 yv = *reinterpret_cast<const float2 *>(&Y0[s][2 * tx]);
            const float2 zv = *reinterpret_cast<const float2 *>(&Y1[s][2 * tx]);
            const float g2[2] = {gv.x, gv.y}, y2[2] = {yv.x, yv.y}, z2[2] = {zv.x, zv.y};
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if (isGA) {
                        const float gs_ = g2[r] * sgnf(pr_diff(x0[r][q], x1[r][q], y2[q]));
                        o0[r][q] -= gs_;
                        o1[r][q] = fmaf(gs_, y2[q], o1[r][q]);
                    } else {
                        const float gs_ = g2[r] * sgnf(pr_diff(y2[q], z2[q], x0[r][q]));
                        o0[r][q] = fmaf(gs_, z2[q], o0[r][q]);
                    }
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = r0 + 2 * ty + r;
        if (row >= R) continue;
        const int64_t grow = (int64_t)c * R + row;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = k0 + 2 * tx + q;
            if (k >= D) continue;
            if (isGA) { a.GA[grow * D + k] = o0[r][q]; a.GW[grow * D + k] = o1[r][q]; }
            else a.GN[grow * D + k] = o0[r][q];
        }
    }
}

// GN[j, :] = dL/dn^_j  ->  dL/dx_j = (g - x^ <x^, g>) / |x| (0 where |x| == 0) + regulariser of the raw row; one wavefront per
// candidate-row occurrence, in place (the adjoint is linear: the update merges duplicate ids afterwards)
__global__ __launch_bounds__(KGE_BLOCK) void pairre_row_adj_kernel(PairreNegArgs a) {
    const int64_t j = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (j >= (int64_t)a.C * a.N) return;
    const int lane = threadIdx.x & 63, D = a.d_e;
    const float *x = row_ptr(a.nbase, a.nidx, j, D);
    const float n = a.nrm[j];
    float *g = a.GN + j * (int64_t)D;
    float pr = 0.f;
    for (int k = lane; k < D; k += KGE_WAVE) pr = fmaf(pr_unit(x[k], n), g[k], pr);
    pr = wave_sum(pr);
    const bool reg = a.reg_coef > 0.f && a.reg_norm > 0;
    for (int k = lane; k < D; k += KGE_WAVE) {
        float v = n > 0.f ? (g[k] - pr_unit(x[k], n) * pr) / n : 0.f;
        if (reg) v += reg_grad(x[k], a.reg_coef, a.reg_norm);
        g[k] = v;
    }
}

// per-edge gradients.  With (x^o, ro) the entity row and relation half inside a, (x^c, w) the corrupted side's, and
// sigma = sign(a - w x^c):   p = gamma - sum |a - w x^c|  and  L reaches (a, w) through (Ga, Gw) -
//   dL/dx^o = (Ga - dp sigma) ro,  dL/dro = (Ga - dp sigma) x^o,  dL/dx^c = dp sigma w,  dL/dw = Gw + dp sigma x^c
// then each entity row through its normalisation; the relation row takes the regulariser of the raw row.
__global__ __launch_bounds__(KGE_BLOCK) void pairre_edge_bwd_kernel(PairreBwdArgs a) {
    const int64_t i = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= a.B) return;
    const int lane = threadIdx.x & 63, D = a.d_e;
    const float *h = row_ptr(a.src.hbase, a.src.hidx, i, D);
    const float *t = row_ptr(a.src.tbase, a.src.tidx, i, D);
    const float *r = row_ptr(a.src.rbase, a.src.ridx, i, 2 * D);
    const float nh = pr_norm(h, D, lane), nt = pr_norm(t, D, lane);
    const float *xo = a.neg_head ? t : h, *xc = a.neg_head ? h : t;
    const float no = a.neg_head ? nt : nh, nc = a.neg_head ? nh : nt;
    const int oo = a.neg_head ? D : 0, ow = a.neg_head ? 0 : D;      // columns of ro / w inside the relation row
    const float dp = a.dpos ? a.dpos[i] : 0.f;
    const float *ga = a.GA ? a.GA + i * (int64_t)D : nullptr, *gw = a.GW ? a.GW + i * (int64_t)D : nullptr;
    float *GO = a.neg_head ? a.GT : a.GH, *GC = a.neg_head ? a.GH : a.GT;      // own / corrupted side's output
    if (GO) GO += i * (int64_t)D;
    if (GC) GC += i * (int64_t)D;
    float *GR = a.GR ? a.GR + i * (int64_t)(2 * D) : nullptr;
    const float *gnd = a.GNd ? a.GNd + ((i / a.nd_chunk) * a.nd_Np + i % a.nd_chunk) * (int64_t)D : nullptr;
    const bool reg = a.reg_coef > 0.f && a.reg_norm > 0;
    // first pass: <x^o, dL/dx^o>, <x^c, dL/dx^c> and the relation row; second pass: the entity rows
    float po = 0.f, pc = 0.f;
    for (int k = lane; k < D; k += KGE_WAVE) {
        const float uo = pr_unit(xo[k], no), uc = pr_unit(xc[k], nc), rov = r[oo + k], wv = r[ow + k];
        const float sg = dp * sgnf(pr_diff(uo * rov, wv, uc));
        const float go = (ga ? ga[k] : 0.f) - sg;
        po = fmaf(uo, go * rov, po);
        pc = fmaf(uc, sg * wv, pc);
        if (GR) {
            float g_ro = go * uo, g_w = (gw ? gw[k] : 0.f) + sg * uc;
            if (reg) { g_ro += reg_grad(rov, a.reg_coef, a.reg_norm); g_w += reg_grad(wv, a.reg_coef, a.reg_norm); }
            GR[oo + k] = g_ro; GR[ow + k] = g_w;
        }
    }
    po = wave_sum(po); pc = wave_sum(pc);
    for (int k = lane; k < D; k += KGE_WAVE) {
        const float uo = pr_unit(xo[k], no), uc = pr_unit(xc[k], nc), rov = r[oo + k], wv = r[ow + k];
        const float sg = dp * sgnf(pr_diff(uo * rov, wv, uc));
        const float go = ((ga ? ga[k] : 0.f) - sg) * rov, gc = sg * wv;
        if (GO) GO[k] = no > 0.f ? (go - uo * po) / no : 0.f;
        if (GC) {
            float v = nc > 0.f ? (gc - uc * pc) / nc : 0.f;
            if (gnd) v += gnd[k];            // neg_deg_sample: the in-batch negative row joins the corrupted side
            GC[k] = v;
        }
    }
}

inline int waves_to_blocks(int64_t waves) { return (int)((waves + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK); }

}  // namespace

int launch_pairre_edge_fwd(const PairreEdgeArgs &a, hipStream_t s) {
    const bool negjob = (a.nrm || a.Bn) && a.n_neg > 0;
    PairreEdgeArgs b = a;
    if (!negjob) b.n_neg = 0;
    const int64_t waves = (int64_t)b.B + b.n_neg;
    if (waves == 0) return KGE_OK;
    hipLaunchKernelGGL(pairre_edge_fwd_kernel, dim3(waves_to_blocks(waves)), dim3(KGE_BLOCK), 0, s, b);
    return check_launch();
}

int launch_pairre_neg_fwd(const PairreNegArgs &a, hipStream_t s) {
    const int ti = (a.chunk + QT - 1) / QT, tj = (a.N + QT - 1) / QT;
    const int nb = a.C * ti * tj;
    if (nb == 0) return KGE_OK;
    hipLaunchKernelGGL(pairre_fwd_kernel, dim3(nb), dim3(KGE_BLOCK), 0, s, a, ti, tj);
    return check_launch();
}

int launch_pairre_neg_bwd(const PairreNegArgs &a, hipStream_t s) {
    const int ti = (a.chunk + QT - 1) / QT, tj = (a.N + QT - 1) / QT, tk = (a.d_e + QK - 1) / QK;
    const int nb = a.C * (ti + tj) * tk;
    if (nb == 0) return KGE_OK;
    hipLaunchKernelGGL(pairre_bwd_kernel, dim3(nb), dim3(KGE_BLOCK), 0, s, a, ti, tj, tk);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(pairre_row_adj_kernel, dim3(waves_to_blocks((int64_t)a.C * a.N)), dim3(KGE_BLOCK), 0, s, a);
    return check_launch();
}

int launch_pairre_edge_bwd(const PairreBwdArgs &a, hipStream_t s) {
    if (a.B == 0) return KGE_OK;
    hipLaunchKernelGGL(pairre_edge_bwd_kernel, dim3(waves_to_blocks(a.B)), dim3(KGE_BLOCK), 0, s, a);
    return check_launch();
}
