// kge_transd.hip - TransD (Ji et al., ACL 2015; include/kge_hip.h, enum kge_model): every entity and every relation carries a
// mapping vector next to its embedding - entity rows [e | e_p], relation rows [r | r_p], both 2 k floats wide - and the
// relation's projection of an entity is the rank-one map  x_perp = x + (x_p . x) r_p  (M_rx = r_p x_p^T + I):
//     s(h, r, t) = gamma - |h_perp + r - t_perp|_2.
//
// The chunked score has ONE form for both corruption sides: per edge the pair (a, rho), rho = r_p of the edge's relation -
//     tails corrupted  a = h_perp + r;      heads corrupted  a = t_perp - r
// - per candidate row [n | m] the scalar c = m . n, and  s_ij = gamma - |a_i - n_j - c_j rho_i|_2,  whose square is, with
// p = a_i . n_j, q = rho_i . n_j, alpha = |a|^2, beta = |n|^2, sigma = |rho|^2, u = a . rho,
//     alpha_i + beta_j + c_j^2 sigma_i - 2 p + 2 c_j (q - u_i)                          (transd_dist2, kge_tile_gemm.hpp).
// So the forward is ONE product of the stacked operand [A ; P] (TransdEdgeArgs, kge_common.hpp) with the candidates' FIRST
// halves, and the backward two: the fp32-MFMA kernels of kge_neg_gemm.hip in their DistMult form run them unchanged (kge_api.hip),
// and this file holds the row-wise kernels around them:
//
//   transd_edge_fwd_kernel   one wavefront per edge: both projections, positive score, the stacked (a, rho), alpha, sigma, u;
//                            further wavefronts, one per candidate row: beta, c (and the dense copies of the row / its first half)
//   transd_score_kernel      raw p | q -> S
//   transd_coef_kernel       dL/dS -> the stacked coefficients P' | Q' of the backward products, with E = -(dL/ds) / (2 dist):
//                            P' = -2 E, Q' = 2 E c_j; row sums of E, E c, E c^2; column sums of E and
//                            Gc_j = sum_i E_ij (2 c_j sigma_i - 2 u_i + 2 q_ij), in a fixed order through LDS
//   transd_edge_bwd_kernel   (Ga | Grho products, row sums, dL/dp) -> per-edge gradients of both halves of the head, tail and
//                            relation rows through the adjoints of the two projections; further wavefronts assemble the
//                            candidates' rows: [product + 2 n sum_i E + Gc m | Gc n] (+ regulariser)
// No atomics; every sum has a fixed order.
#include "kge_tile_gemm.hpp"

using namespace kge;

#define TD_CT 32       // columns of a column-sum workgroup
#define TD_CR 8        // its row groups (TD_CT * TD_CR == KGE_BLOCK)

namespace {

// where the pair of batch row i lives in a stacked operand (rows): a, and rho `m` rows behind it
__device__ __forceinline__ int64_t td_stack_row(int64_t i, int chunk, int B, int &m) {
    const int64_t c = i / chunk;
    const int64_t left = (int64_t)B - c * chunk;
    m = (int)(left < chunk ? left : chunk);
    return 2 * c * chunk + (i - c * chunk);
}

// x_p . x of a row [x | x_p] of 2 K floats, in every lane
__device__ __forceinline__ float td_self_dot(const float *x, int K, int lane) {
    float s = 0.f;
    for (int k = lane; k < K; k += KGE_WAVE) s = fmaf(x[K + k], x[k], s);
    return wave_sum(s);
}

__global__ __launch_bounds__(KGE_BLOCK) void transd_edge_fwd_kernel(TransdEdgeArgs a) {
    const int64_t w = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, D = a.d_e, K = D / 2;
    if (w < a.B) {
        const int64_t i = w;
        const float *h = row_ptr(a.src.hbase, a.src.hidx, i, D);
        const float *t = row_ptr(a.src.tbase, a.src.tidx, i, D);
        const float *r = row_ptr(a.src.rbase, a.src.ridx, i, D);
        const float *rp = r + K;
        const float sh = td_self_dot(h, K, lane), st = td_self_dot(t, K, lane);
        int m = 0;
        const int64_t ar = a.AP ? td_stack_row(i, a.chunk, a.B, m) : 0;
        float *A = a.AP ? a.AP + ar * K : nullptr, *R = a.AP ? a.AP + (ar + m) * K : nullptr;
        if (a.W) { A = a.AP + i * K; R = a.W + i * K; }
        float d2 = 0.f, as = 0.f, sg = 0.f, u = 0.f;
        for (int k = lane; k < K; k += KGE_WAVE) {
            const float rho = rp[k];
            const float hp = fmaf(sh, rho, h[k]), tp = fmaf(st, rho, t[k]);
            const float e = (hp + r[k]) - tp;
            d2 = fmaf(e, e, d2);
            const float av = a.neg_head ? tp - r[k] : hp + r[k];
            as = fmaf(av, av, as); sg = fmaf(rho, rho, sg); u = fmaf(av, rho, u);
            if (A) { A[k] = av; R[k] = rho; }
        }
        if (a.pos_score) {
            d2 = wave_sum(d2);
            if (lane == 0) a.pos_score[i] = a.gamma - sqrtf(d2);
        }
        if (a.AP) {
            as = wave_sum(as); sg = wave_sum(sg); u = wave_sum(u);
            if (lane == 0) { a.alpha[i] = as; a.sig[i] = sg; a.u[i] = u; }
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
        float *cp = a.Bn ? a.Bn + j * (int64_t)D : nullptr;
        float *hf = a.Nh ? a.Nh + j * (int64_t)K : nullptr;
        float s = 0.f, c = 0.f;
        for (int k = lane; k < K; k += KGE_WAVE) {
            const float n = x[k], mm = x[K + k];
            s = fmaf(n, n, s); c = fmaf(mm, n, c);
            if (cp) { cp[k] = n; cp[K + k] = mm; }
            if (hf) hf[k] = n;
        }
        s = wave_sum(s); c = wave_sum(c);
        if (lane == 0) {
            if (a.beta) a.beta[j] = s;
            if (a.cj) a.cj[j] = c;
        }
    }
}

// S[c, i, j] from the stacked raw products: one thread per score, consecutive threads along j
__global__ __launch_bounds__(KGE_BLOCK) void transd_score_kernel(TransdNegArgs a) {
    const int64_t e = (int64_t)blockIdx.x * KGE_BLOCK + threadIdx.x;
    const int64_t per = (int64_t)a.chunk * a.N;
    if (e >= (int64_t)a.C * per) return;
    const int64_t c = e / per, rem = e - c * per;
    const int64_t i = rem / a.N, j = rem - i * a.N;
    const int64_t gi = c * a.chunk + i;
    const float *pq = a.PQ + (2 * c * a.chunk + i) * a.N + j;
    a.S[e] = transd_score(pq[0], pq[(int64_t)a.chunk * a.N], a.gamma, a.alpha[gi], a.sig[gi], a.u[gi], a.beta[c * a.N + j], a.cj[c * a.N + j]);
}

// E_ij = -(dL/ds_ij) / (2 dist_ij), 0 where the distance sits on the guard of transd_dist2 (as the TransE_l2 chain rule does)
__device__ __forceinline__ float td_E(float g, float p, float q, float as, float sg, float u, float bs, float c) {
    const float dist = sqrtf(transd_dist2(p, q, as, sg, u, bs, c));
    return dist > 1e-15f ? -g / (2.f * dist) : 0.f;
}

// The first C * chunk / 4 workgroups: one wavefront per score row (coefficients, row sums).  The others: TD_CT columns of one chunk
// each, the rows split over TD_CR groups and summed through LDS in the groups' order (column sums).  Both read the raw products.
__global__ __launch_bounds__(KGE_BLOCK) void transd_coef_kernel(TransdNegArgs a, int nb_rows, int tct) {
    if ((int)blockIdx.x < nb_rows) {
        const int64_t gi = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
        if (gi >= (int64_t)a.C * a.chunk) return;
        const int lane = threadIdx.x & 63;
        const int64_t c = gi / a.chunk, i = gi - c * a.chunk;
        const int64_t po = (2 * c * a.chunk + i) * a.N, qo = po + (int64_t)a.chunk * a.N;
        const float as = a.alpha[gi], sg = a.sig[gi], u = a.u[gi];
        const float *bs = a.beta + c * a.N, *cj = a.cj + c * a.N, *g = a.G + gi * a.N;
        float se = 0.f, sc = 0.f, sc2 = 0.f;
        for (int j = lane; j < a.N; j += KGE_WAVE) {
            const float p = a.PQ[po + j], q = a.PQ[qo + j], cc = cj[j];
            const float E = td_E(g[j], p, q, as, sg, u, bs[j], cc);
            const float Ec = E * cc;
            a.PQc[po + j] = -2.f * E;
            a.PQc[qo + j] = 2.f * Ec;
            se += E; sc += Ec; sc2 = fmaf(Ec, cc, sc2);
        }
        se = wave_sum(se); sc = wave_sum(sc); sc2 = wave_sum(sc2);
        if (lane == 0) { a.rs[gi] = se; a.rc[gi] = sc; a.rc2[gi] = sc2; }
        return;
    }
    __shared__ float part[2][TD_CR][TD_CT];
    const int b = (int)blockIdx.x - nb_rows;
    const int64_t c = b / tct;
    const int j = (b % tct) * TD_CT + (threadIdx.x & (TD_CT - 1)), rg = threadIdx.x / TD_CT;
    float s = 0.f, gc = 0.f;
    if (j < a.N) {
        const float bs = a.beta[c * a.N + j], cc = a.cj[c * a.N + j];
        for (int i = rg; i < a.chunk; i += TD_CR) {
            const int64_t gi = c * a.chunk + i;
            const int64_t po = (2 * c * a.chunk + i) * a.N + j;
            const float q = a.PQ[po + (int64_t)a.chunk * a.N], sg = a.sig[gi], u = a.u[gi];
            const float E = td_E(a.G[gi * a.N + j], a.PQ[po], q, a.alpha[gi], sg, u, bs, cc);
            s += E;
            gc = fmaf(E, 2.f * (fmaf(cc, sg, q) - u), gc);
        }
    }
    part[0][rg][threadIdx.x & (TD_CT - 1)] = s;
    part[1][rg][threadIdx.x & (TD_CT - 1)] = gc;
    __syncthreads();
    if (rg == 0 && j < a.N) {
        float tot = 0.f, tg = 0.f;
#pragma unroll
        for (int k = 0; k < TD_CR; ++k) { tot += part[0][k][threadIdx.x]; tg += part[1][k][threadIdx.x]; }
        a.cs[c * a.N + j] = tot;
        a.gc[c * a.N + j] = tg;
    }
}

// per-edge gradients.  sa = +1: a = h_perp + r (tails corrupted); sa = -1: a = t_perp - r.  e = h_perp + r - t_perp,
// p = gamma - |e| and Ge = -dp e / |e| = cu e:
//   Ga    = (product) + 2 a sum_j E - 2 rho sum_j E c             Grho = (product) + 2 rho sum_j E c^2 - 2 a sum_j E c
//   Gh_perp = (sa > 0 ? Ga : 0) + Ge,   Gt_perp = (sa < 0 ? Ga : 0) - Ge
//   Gx = Gx_perp + (Gx_perp . r_p) x_p,  Gx_p = (Gx_perp . r_p) x                     (the adjoint of a projection)
//   Gr = sa Ga + Ge,  Gr_p = Grho + (h_p . h) Gh_perp + (t_p . t) Gt_perp;  the relation row takes the regulariser of the raw row.
__global__ __launch_bounds__(KGE_BLOCK) void transd_edge_bwd_kernel(TransdBwdArgs a) {
    const int64_t wf = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, D = a.d_e, K = D / 2;
    if (wf >= a.B) {
        const int64_t j = wf - a.B;
        if (j >= a.n_neg) return;
        const float *x = row_ptr(a.nbase, a.nidx, j, D);
        const float *gp = a.GNp + j * (int64_t)K;
        float *g = a.GN + j * (int64_t)D;
        const float c2 = 2.f * a.cs[j], gc = a.gc[j];
        const bool reg = a.n_reg_coef > 0.f && a.reg_norm > 0;
        for (int k = lane; k < K; k += KGE_WAVE) {
            const float n = x[k], mm = x[K + k];
            float v = fmaf(gc, mm, fmaf(c2, n, gp[k])), vm = gc * n;
            if (reg) { v += reg_grad(n, a.n_reg_coef, a.reg_norm); vm += reg_grad(mm, a.n_reg_coef, a.reg_norm); }
            g[k] = v; g[K + k] = vm;
        }
        return;
    }
    const int64_t i = wf;
    const float *h = row_ptr(a.src.hbase, a.src.hidx, i, D);
    const float *t = row_ptr(a.src.tbase, a.src.tidx, i, D);
    const float *r = row_ptr(a.src.rbase, a.src.ridx, i, D);
    const float *rp = r + K;
    const float sa = a.neg_head ? -1.f : 1.f;
    const float sh = td_self_dot(h, K, lane), st = td_self_dot(t, K, lane);
    const float dp = a.dpos ? a.dpos[i] : 0.f;
    int m = 0;
    const int64_t ar = a.GAP ? td_stack_row(i, a.chunk, a.B, m) : 0;
    const float *ga = a.GAP ? a.GAP + ar * K : nullptr, *gr = a.GAP ? a.GAP + (ar + m) * K : nullptr;
    const float rs2 = a.GAP ? 2.f * a.rs[i] : 0.f, rc2 = a.GAP ? 2.f * a.rc[i] : 0.f, rcc2 = a.GAP ? 2.f * a.rc2[i] : 0.f;
    // the pieces of one column: e_k, a_k, Ga_k (complete)
    auto col = [&](int k, float &e, float &av, float &gav) {
        const float rho = rp[k];
        const float hp = fmaf(sh, rho, h[k]), tp = fmaf(st, rho, t[k]);
        e = (hp + r[k]) - tp;
        av = a.neg_head ? tp - r[k] : hp + r[k];
        gav = ga ? fmaf(-rc2, rho, fmaf(rs2, av, ga[k])) : 0.f;
    };
    float d2 = 0.f, we = 0.f, wga = 0.f;
    for (int k = lane; k < K; k += KGE_WAVE) {
        float e, av, gav; col(k, e, av, gav);
        d2 = fmaf(e, e, d2); we = fmaf(rp[k], e, we); wga = fmaf(rp[k], gav, wga);
    }
    d2 = wave_sum(d2); we = wave_sum(we); wga = wave_sum(wga);
    const float dist = sqrtf(d2);
    const float cu = dist > 1e-15f ? -dp / dist : 0.f;          // Ge = cu e
    const float fh = a.neg_head ? 0.f : 1.f, ft = a.neg_head ? 1.f : 0.f;      // which projection a runs through
    const float dh = fmaf(cu, we, fh * wga), dt = fmaf(-cu, we, ft * wga);     // Gh_perp . r_p, Gt_perp . r_p
    float *GH = a.GH ? a.GH + i * (int64_t)D : nullptr, *GT = a.GT ? a.GT + i * (int64_t)D : nullptr;
    float *GR = a.GR ? a.GR + i * (int64_t)D : nullptr;
    float *GC = a.neg_head ? GH : GT;                            // the corrupted side's output
    const float *gnd = a.GNd ? a.GNd + ((i / a.nd_chunk) * a.nd_Np + i % a.nd_chunk) * (int64_t)D : nullptr;
    const bool reg = a.reg_coef > 0.f && a.reg_norm > 0;
    for (int k = lane; k < K; k += KGE_WAVE) {
        float e, av, gav; col(k, e, av, gav);
        const float ge = cu * e;
        const float ghp = fmaf(fh, gav, ge), gtp = fmaf(ft, gav, -ge);
        if (GH) { GH[k] = fmaf(dh, h[K + k], ghp); GH[K + k] = dh * h[k]; }
        if (GT) { GT[k] = fmaf(dt, t[K + k], gtp); GT[K + k] = dt * t[k]; }
        if (GC && gnd) { GC[k] += gnd[k]; GC[K + k] += gnd[K + k]; }   // neg_deg_sample: the in-batch negative row joins the corrupted side
        if (GR) {
            float g_r = fmaf(sa, gav, ge);
            float g_p = gr ? fmaf(-rc2, av, fmaf(rcc2, rp[k], gr[k])) : 0.f;
            g_p = fmaf(st, gtp, fmaf(sh, ghp, g_p));
            if (reg) { g_r += reg_grad(r[k], a.reg_coef, a.reg_norm); g_p += reg_grad(rp[k], a.reg_coef, a.reg_norm); }
            GR[k] = g_r; GR[K + k] = g_p;
        }
    }
}

inline int waves_to_blocks(int64_t waves) { return (int)((waves + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK); }

}  // namespace

int launch_transd_edge_fwd(const TransdEdgeArgs &a, hipStream_t s) {
    const bool negjob = (a.beta || a.cj || a.Bn || a.Nh) && a.n_neg > 0;
    TransdEdgeArgs b = a;
    if (!negjob) b.n_neg = 0;
    const int64_t waves = (int64_t)b.B + b.n_neg;
    if (waves == 0) return KGE_OK;
    hipLaunchKernelGGL(transd_edge_fwd_kernel, dim3(waves_to_blocks(waves)), dim3(KGE_BLOCK), 0, s, b);
    return check_launch();
}

int launch_transd_score(const TransdNegArgs &a, hipStream_t s) {
    const int64_t n = (int64_t)a.C * a.chunk * a.N;
    if (n == 0) return KGE_OK;
    hipLaunchKernelGGL(transd_score_kernel, dim3((unsigned)((n + KGE_BLOCK - 1) / KGE_BLOCK)), dim3(KGE_BLOCK), 0, s, a);
    return check_launch();
}

int launch_transd_coef(const TransdNegArgs &a, hipStream_t s) {
    static_assert(TD_CT * TD_CR == KGE_BLOCK, "column-sum workgroup shape");
    const int nb_rows = waves_to_blocks((int64_t)a.C * a.chunk), tct = (a.N + TD_CT - 1) / TD_CT;
    const int nb = nb_rows + a.C * tct;
    if (nb == 0) return KGE_OK;
    hipLaunchKernelGGL(transd_coef_kernel, dim3(nb), dim3(KGE_BLOCK), 0, s, a, nb_rows, tct);
    return check_launch();
}

// neg_deg_sample: the edges read GN rows that the candidate jobs complete - those run first, in a launch of their own
int launch_transd_edge_bwd(const TransdBwdArgs &a, hipStream_t s) {
    TransdBwdArgs b = a;
    if (!b.GN || !b.GNp || !b.cs || !b.gc) b.n_neg = 0;
    if (b.GNd && b.n_neg > 0) {
        TransdBwdArgs n = b;
        n.B = 0;
        hipLaunchKernelGGL(transd_edge_bwd_kernel, dim3(waves_to_blocks(n.n_neg)), dim3(KGE_BLOCK), 0, s, n);
        if (int rc = check_launch()) return rc;
        b.n_neg = 0;
    }
    const int64_t waves = (int64_t)b.B + b.n_neg;
    if (waves == 0) return KGE_OK;
    hipLaunchKernelGGL(transd_edge_bwd_kernel, dim3(waves_to_blocks(waves)), dim3(KGE_BLOCK), 0, s, b);
    return check_launch();
}
