// kge_transh.hip - TransH (Wang et al., AAAI 2014; include/kge_hip.h, enum kge_model): a relation is a translation d and a
// hyperplane normal w, r = [d | w];  w^ = w / |w|_2 (0 where |w|_2 == 0),  x_perp = x - (w^ . x) w^,
//     s(h, r, t) = gamma - |h_perp + d - t_perp|_2.
//
// The chunked score has ONE form for both corruption sides: per edge the pair (a, w^) -
//     tails corrupted  a = h_perp + d;      heads corrupted  a = t_perp - d
// - and  s_ij = gamma - |a_i - n_j + (w^_i . n_j) w^_i|_2,  whose square is, with p = a_i . n_j and q = w^_i . n_j,
//     |a_i|^2 + |n_j|^2 - 2 p + 2 (w^_i . a_i) q - q^2                                  (transh_dist2, kge_tile_gemm.hpp).
// So the forward is ONE product of the stacked operand [A ; W^] (TranshEdgeArgs, kge_common.hpp) with the candidate rows, and the
// backward two: the fp32-MFMA kernels of kge_neg_gemm.hip in their DistMult form run them unchanged (kge_api.hip), and this file
// holds the row-wise kernels around them:
//
//   transh_edge_fwd_kernel   one wavefront per edge: w^, the projections, positive score, the stacked (a, w^), |a|^2, w^ . a;
//                            further wavefronts, one per candidate row: |n|^2 (and the row's dense copy)
//   transh_score_kernel      raw p | q -> S
//   transh_coef_kernel       dL/dS -> the stacked coefficients P' | Q' of the backward products, with E = -(dL/ds) / (2 dist):
//                            P' = -2 E, Q' = 2 E (c - q); row sums sum_j E, kappa = sum_j 2 E q; column sums sum_i E
//   transh_edge_bwd_kernel   (Ga | Gw^ products, row terms, dL/dp) -> per-edge gradients of the head, tail and relation rows through
//                            the projections and the normalisation; further wavefronts: GN_j += 2 n_j sum_i E_ij (+ regulariser)
// No atomics; every sum has a fixed order.
#include "kge_tile_gemm.hpp"

using namespace kge;

#define TH_CT 32       // columns of a column-sum workgroup
#define TH_CR 8        // its row groups (TH_CT * TH_CR == KGE_BLOCK)

namespace {

__device__ __forceinline__ float th_unit(float x, float n) { return n > 0.f ? x / n : 0.f; }

// |w|_2 of a row, in every lane: lane-strided squares, then the fixed-order wavefront sum (the ONE norm routine of this file)
__device__ __forceinline__ float th_norm(const float *x, int d, int lane) {
    float s = 0.f;
    for (int k = lane; k < d; k += KGE_WAVE) s = fmaf(x[k], x[k], s);
    return sqrtf(wave_sum(s));
}

// where the pair of batch row i lives in a stacked operand (rows): a, and w^ `m` rows behind it
__device__ __forceinline__ int64_t th_stack_row(int64_t i, int chunk, int B, int &m) {
    const int64_t c = i / chunk;
    const int64_t left = (int64_t)B - c * chunk;
    m = (int)(left < chunk ? left : chunk);
    return 2 * c * chunk + (i - c * chunk);
}

__global__ __launch_bounds__(KGE_BLOCK) void transh_edge_fwd_kernel(TranshEdgeArgs a) {
    const int64_t w = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, D = a.d_e;
    if (w < a.B) {
        const int64_t i = w;
        const float *h = row_ptr(a.src.hbase, a.src.hidx, i, D);
        const float *t = row_ptr(a.src.tbase, a.src.tidx, i, D);
        const float *r = row_ptr(a.src.rbase, a.src.ridx, i, 2 * D);
        const float *dv = r, *wv = r + D;
        const float wn = th_norm(wv, D, lane);
        float sh = 0.f, st = 0.f;
        for (int k = lane; k < D; k += KGE_WAVE) {
            const float u = th_unit(wv[k], wn);
            sh = fmaf(u, h[k], sh); st = fmaf(u, t[k], st);
        }
        sh = wave_sum(sh); st = wave_sum(st);
        int m = 0;
        const int64_t ar = a.AW ? th_stack_row(i, a.chunk, a.B, m) : 0;
        float *A = a.AW ? a.AW + ar * D : nullptr, *W = a.AW ? a.AW + (ar + m) * D : nullptr;
        if (a.W) { A = a.AW + i * D; W = a.W + i * D; }
        float d2 = 0.f, as = 0.f, c = 0.f;
        for (int k = lane; k < D; k += KGE_WAVE) {
            const float u = th_unit(wv[k], wn);
            const float hp = fmaf(-sh, u, h[k]), tp = fmaf(-st, u, t[k]);
            const float e = (hp + dv[k]) - tp;
            d2 = fmaf(e, e, d2);
            const float av = a.neg_head ? tp - dv[k] : hp + dv[k];
            as = fmaf(av, av, as); c = fmaf(u, av, c);
            if (A) { A[k] = av; W[k] = u; }
        }
        if (a.pos_score) {
            d2 = wave_sum(d2);
            if (lane == 0) a.pos_score[i] = a.gamma - sqrtf(d2);
        }
        if (a.AW) {
            as = wave_sum(as); c = wave_sum(c);
            if (lane == 0) { a.alpha[i] = as; a.cw[i] = c; }
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
        float s = 0.f;
        for (int k = lane; k < D; k += KGE_WAVE) {
            const float v = x[k];
            s = fmaf(v, v, s);
            if (cp) cp[k] = v;
        }
        s = wave_sum(s);
        if (a.beta && lane == 0) a.beta[j] = s;
    }
}

// S[c, i, j] from the stacked raw products: one thread per score, consecutive threads along j
__global__ __launch_bounds__(KGE_BLOCK) void transh_score_kernel(TranshNegArgs a) {
    const int64_t e = (int64_t)blockIdx.x * KGE_BLOCK + threadIdx.x;
    const int64_t per = (int64_t)a.chunk * a.N;
    if (e >= (int64_t)a.C * per) return;
    const int64_t c = e / per, rem = e - c * per;
    const int64_t i = rem / a.N, j = rem - i * a.N;
    const int64_t gi = c * a.chunk + i;
    const float *pq = a.PQ + (2 * c * a.chunk + i) * a.N + j;
    a.S[e] = transh_score(pq[0], pq[(int64_t)a.chunk * a.N], a.gamma, a.alpha[gi], a.beta[c * a.N + j], a.cw[gi]);
}

// E_ij = -(dL/ds_ij) / (2 dist_ij), 0 where the distance sits on the guard of transh_dist2 (as the TransE_l2 chain rule does)
__device__ __forceinline__ float th_E(float g, float p, float q, float as, float bs, float c) {
    const float dist = sqrtf(transh_dist2(p, q, as, bs, c));
    return dist > 1e-15f ? -g / (2.f * dist) : 0.f;
}

// The first C * chunk / 4 workgroups: one wavefront per score row (coefficients, row sums).  The others: TH_CT columns of one chunk
// each, the rows split over TH_CR groups and summed through LDS in the groups' order (column sums).  Both read the raw products.
__global__ __launch_bounds__(KGE_BLOCK) void transh_coef_kernel(TranshNegArgs a, int nb_rows, int tct) {
    if ((int)blockIdx.x < nb_rows) {
        const int64_t gi = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
        if (gi >= (int64_t)a.C * a.chunk) return;
        const int lane = threadIdx.x & 63;
        const int64_t c = gi / a.chunk, i = gi - c * a.chunk;
        const int64_t po = (2 * c * a.chunk + i) * a.N, qo = po + (int64_t)a.chunk * a.N;
        const float as = a.alpha[gi], cw = a.cw[gi];
        const float *bs = a.beta + c * a.N, *g = a.G + gi * a.N;
        float se = 0.f, sk = 0.f;
        for (int j = lane; j < a.N; j += KGE_WAVE) {
            const float p = a.PQ[po + j], q = a.PQ[qo + j];
            const float E = th_E(g[j], p, q, as, bs[j], cw);
            a.PQc[po + j] = -2.f * E;
            a.PQc[qo + j] = 2.f * E * (cw - q);
            se += E; sk = fmaf(2.f * E, q, sk);
        }
        se = wave_sum(se); sk = wave_sum(sk);
        if (lane == 0) { a.rs[gi] = se; a.kap[gi] = sk; }
        return;
    }
    __shared__ float part[TH_CR][TH_CT];
    const int b = (int)blockIdx.x - nb_rows;
    const int64_t c = b / tct;
    const int j = (b % tct) * TH_CT + (threadIdx.x & (TH_CT - 1)), rg = threadIdx.x / TH_CT;
    float s = 0.f;
    if (j < a.N) {
        const float bs = a.beta[c * a.N + j];
        for (int i = rg; i < a.chunk; i += TH_CR) {
            const int64_t gi = c * a.chunk + i;
            const int64_t po = (2 * c * a.chunk + i) * a.N + j;
            s += th_E(a.G[gi * a.N + j], a.PQ[po], a.PQ[po + (int64_t)a.chunk * a.N], a.alpha[gi], bs, a.cw[gi]);
        }
    }
    part[rg][threadIdx.x & (TH_CT - 1)] = s;
    __syncthreads();
    if (rg == 0 && j < a.N) {
        float tot = 0.f;
#pragma unroll
        for (int k = 0; k < TH_CR; ++k) tot += part[k][threadIdx.x];
        a.cs[c * a.N + j] = tot;
    }
}

// per-edge gradients.  With xo the entity row inside a (so = w^ . xo, sa = +1: a = h_perp + d; sa = -1: a = t_perp - d),
// u = h_perp + d - t_perp, p = gamma - |u| and Gu = -dp u / |u|:
//   Ga   = (product) + 2 a sum_j E + kappa w^                     Gw^ = (product) + kappa a
//   Gxo  = Ga_perp,  Gd = sa Ga,  Gw^ += -so Ga - (w^ . Ga) xo       (a through the projection of xo)
//   Gh  += Gu_perp,  Gt -= Gu_perp,  Gd += Gu,  Gw^ += -(w^ . (h - t)) Gu - (w^ . Gu) (h - t)
//   Gw   = (Gw^ - (Gw^ . w^) w^) / |w|, 0 where |w| == 0;  the relation row takes the regulariser of the raw row.
__global__ __launch_bounds__(KGE_BLOCK) void transh_edge_bwd_kernel(TranshBwdArgs a) {
    const int64_t wf = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, D = a.d_e;
    if (wf >= a.B) {
        const int64_t j = wf - a.B;
        if (j >= a.n_neg) return;
        const float *x = row_ptr(a.nbase, a.nidx, j, D);
        float *g = a.GN + j * (int64_t)D;
        const float c2 = 2.f * a.cs[j];
        const bool reg = a.n_reg_coef > 0.f && a.reg_norm > 0;
        for (int k = lane; k < D; k += KGE_WAVE) {
            float v = fmaf(c2, x[k], g[k]);
            if (reg) v += reg_grad(x[k], a.n_reg_coef, a.reg_norm);
            g[k] = v;
        }
        return;
    }
    const int64_t i = wf;
    const float *h = row_ptr(a.src.hbase, a.src.hidx, i, D);
    const float *t = row_ptr(a.src.tbase, a.src.tidx, i, D);
    const float *r = row_ptr(a.src.rbase, a.src.ridx, i, 2 * D);
    const float *dv = r, *wv = r + D;
    const float *xo = a.neg_head ? t : h;
    const float sa = a.neg_head ? -1.f : 1.f;
    const float wn = th_norm(wv, D, lane);
    float sh = 0.f, st = 0.f;
    for (int k = lane; k < D; k += KGE_WAVE) {
        const float u = th_unit(wv[k], wn);
        sh = fmaf(u, h[k], sh); st = fmaf(u, t[k], st);
    }
    sh = wave_sum(sh); st = wave_sum(st);
    const float so = a.neg_head ? st : sh;
    const float dp = a.dpos ? a.dpos[i] : 0.f;
    int m = 0;
    const int64_t ar = a.GAW ? th_stack_row(i, a.chunk, a.B, m) : 0;
    const float *ga = a.GAW ? a.GAW + ar * D : nullptr, *gw = a.GAW ? a.GAW + (ar + m) * D : nullptr;
    const float rs2 = a.GAW ? 2.f * a.rs[i] : 0.f, kap = a.GAW ? a.kap[i] : 0.f;
    // the pieces of one column: u_k, a_k, Ga_k (complete), w^_k
    auto col = [&](int k, float &u, float &e, float &av, float &gav) {
        u = th_unit(wv[k], wn);
        const float hp = fmaf(-sh, u, h[k]), tp = fmaf(-st, u, t[k]);
        e = (hp + dv[k]) - tp;
        av = a.neg_head ? tp - dv[k] : hp + dv[k];
        gav = ga ? fmaf(kap, u, fmaf(rs2, av, ga[k])) : 0.f;
    };
    float d2 = 0.f, wu = 0.f, wga = 0.f;
    for (int k = lane; k < D; k += KGE_WAVE) {
        float u, e, av, gav; col(k, u, e, av, gav);
        d2 = fmaf(e, e, d2); wu = fmaf(u, e, wu); wga = fmaf(u, gav, wga);
    }
    d2 = wave_sum(d2); wu = wave_sum(wu); wga = wave_sum(wga);
    const float dist = sqrtf(d2);
    const float cu = dist > 1e-15f ? -dp / dist : 0.f;          // Gu = cu u
    const float sht = sh - st;
    // Gw^ of one column, complete
    auto gwhat = [&](int k, float e, float av, float gav) {
        float v = gw ? fmaf(kap, av, gw[k]) : 0.f;
        v -= fmaf(so, gav, wga * xo[k]);
        v -= cu * fmaf(sht, e, wu * (h[k] - t[k]));
        return v;
    };
    float gww = 0.f;
    for (int k = lane; k < D; k += KGE_WAVE) {
        float u, e, av, gav; col(k, u, e, av, gav);
        gww = fmaf(gwhat(k, e, av, gav), u, gww);
    }
    gww = wave_sum(gww);
    float *GO = a.neg_head ? a.GT : a.GH, *GC = a.neg_head ? a.GH : a.GT;      // own / corrupted side's output
    if (GO) GO += i * (int64_t)D;
    if (GC) GC += i * (int64_t)D;
    float *GR = a.GR ? a.GR + i * (int64_t)(2 * D) : nullptr;
    const float *gnd = a.GNd ? a.GNd + ((i / a.nd_chunk) * a.nd_Np + i % a.nd_chunk) * (int64_t)D : nullptr;
    const bool reg = a.reg_coef > 0.f && a.reg_norm > 0;
    for (int k = lane; k < D; k += KGE_WAVE) {
        float u, e, av, gav; col(k, u, e, av, gav);
        const float gup = cu * fmaf(-wu, u, e);                 // Gu through a projection
        if (GO) GO[k] = fmaf(-wga, u, gav) + sa * gup;
        if (GC) {
            float v = -sa * gup;
            if (gnd) v += gnd[k];            // neg_deg_sample: the in-batch negative row joins the corrupted side
            GC[k] = v;
        }
        if (GR) {
            float g_d = fmaf(sa, gav, cu * e);
            float g_w = wn > 0.f ? fmaf(-gww, u, gwhat(k, e, av, gav)) / wn : 0.f;
            if (reg) { g_d += reg_grad(dv[k], a.reg_coef, a.reg_norm); g_w += reg_grad(wv[k], a.reg_coef, a.reg_norm); }
            GR[k] = g_d; GR[D + k] = g_w;
        }
    }
}

inline int waves_to_blocks(int64_t waves) { return (int)((waves + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK); }

}  // namespace

int launch_transh_edge_fwd(const TranshEdgeArgs &a, hipStream_t s) {
    const bool negjob = (a.beta || a.Bn) && a.n_neg > 0;
    TranshEdgeArgs b = a;
    if (!negjob) b.n_neg = 0;
    const int64_t waves = (int64_t)b.B + b.n_neg;
    if (waves == 0) return KGE_OK;
    hipLaunchKernelGGL(transh_edge_fwd_kernel, dim3(waves_to_blocks(waves)), dim3(KGE_BLOCK), 0, s, b);
    return check_launch();
}

int launch_transh_score(const TranshNegArgs &a, hipStream_t s) {
    const int64_t n = (int64_t)a.C * a.chunk * a.N;
    if (n == 0) return KGE_OK;
    hipLaunchKernelGGL(transh_score_kernel, dim3((unsigned)((n + KGE_BLOCK - 1) / KGE_BLOCK)), dim3(KGE_BLOCK), 0, s, a);
    return check_launch();
}

int launch_transh_coef(const TranshNegArgs &a, hipStream_t s) {
    static_assert(TH_CT * TH_CR == KGE_BLOCK, "column-sum workgroup shape");
    const int nb_rows = waves_to_blocks((int64_t)a.C * a.chunk), tct = (a.N + TH_CT - 1) / TH_CT;
    const int nb = nb_rows + a.C * tct;
    if (nb == 0) return KGE_OK;
    hipLaunchKernelGGL(transh_coef_kernel, dim3(nb), dim3(KGE_BLOCK), 0, s, a, nb_rows, tct);
    return check_launch();
}

// neg_deg_sample: the edges read GN rows that the candidate jobs complete - those run first, in a launch of their own
int launch_transh_edge_bwd(const TranshBwdArgs &a, hipStream_t s) {
    TranshBwdArgs b = a;
    if (!b.GN || !b.cs) b.n_neg = 0;
    if (b.GNd && b.n_neg > 0) {
        TranshBwdArgs n = b;
        n.B = 0;
        hipLaunchKernelGGL(transh_edge_bwd_kernel, dim3(waves_to_blocks(n.n_neg)), dim3(KGE_BLOCK), 0, s, n);
        if (int rc = check_launch()) return rc;
        b.n_neg = 0;
    }
    const int64_t waves = (int64_t)b.B + b.n_neg;
    if (waves == 0) return KGE_OK;
    hipLaunchKernelGGL(transh_edge_bwd_kernel, dim3(waves_to_blocks(waves)), dim3(KGE_BLOCK), 0, s, b);
    return check_launch();
}
