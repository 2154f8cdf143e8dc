// kge_rank_rel.hip - relation ranking (kge_rank_rel_eval): every test triple (h, r, t) against ALL n_rel relations as the candidates,
//     rank_i = 1 + #{j : j not in list_i, s(h_i, j, t_i) >= s(h_i, r_i, t_i)},   list_i = {r_i} (+ the known relations of the pair).
// The reference has no counterpart (its EvalSampler corrupts entities only, dataloader/sampler.py:514-597); the protocol is stated
// in include/kge_hip.h.  For a fixed pair (h, t) the score of every model is a function of the relation row c_j alone:
//     TransE_l1 / l2   q = t - h                                   s_j = gamma - |q - c_j|_1 / _2
//     DistMult         q = h o t                                   s_j = q . c_j
//     ComplEx          q = [h_re t_re + h_im t_im | h_re t_im - h_im t_re]          s_j = q . c_j
//     SimplE           q = 1/2 [h_i o t_j | h_j o t_i]             s_j = clamp(q . c_j, +-20)      (score_fun.py:562-569)
//     RESCAL           q = vec(h t^T), d_e^2 wide                  s_j = q . vec(M_j)
//     TransR           u = h - t                                   s_j = gamma - |u P_j + c_j|_1
//     RotatE           -                                           s_j = gamma - sum_k |h_k e^{i theta_jk} - t_k|
//     QuatE            q = conj(h) (x) t, per column of the quarters  s_j = q . c^_j,  c^_j = the row normalised per quaternion
// i.e. for six models the form the entity-ranking kernels already evaluate with the relation table in the place of the entity
// table (kge_rank_gemm.hip, kge_neg_pair.hip / kge_neg_bcast.hip + kge_eval.hip; sequence in kge_api.hip).  This file holds what
// they lack: rel_query_kernel (the per-pair query rows), rel_rotate_score_kernel (RotatE over relation phases) and rel_neg_rows_kernel
// (TransR: the training forward kge_transr.hip with the roles exchanged - the relations are its "positives", Q_j = -c_j, the batch's
// u rows its shared "negatives" - leaves a [n_rel, rows] block that rank_count_kernel<true> counts transposed).
#include "kge_common.hpp"

using namespace kge;


// ---- query rows: one wavefront per test triple ----------------------------------------------------------------------------------------
struct RelQueryArgs {
    const float *ent; const int64_t *h, *t;      // this batch's head / tail ids
    int rows, d_e;
    float *Q;                                     // [rows, d_e] (RESCAL: [rows, d_e * d_e])
    float *qsq;                                   // [rows] |q|^2 or null
};

template <int MODEL, int V>
__global__ __launch_bounds__(KGE_BLOCK) void rel_query_kernel(RelQueryArgs a) {
    const int i = (int)blockIdx.x * KGE_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);
    if (i >= a.rows) return;
    const int lane = threadIdx.x & 63, D = a.d_e;
    const float *h = a.ent + a.h[i] * (int64_t)D, *t = a.ent + a.t[i] * (int64_t)D;
    if constexpr (MODEL == KGE_RESCAL) {
        // q[r * D + b] = h[r] t[b]: M_j is [D, D] row-major and s_j = h . (M_j t)  (score_fun.py:387-394)
        float *q = a.Q + (int64_t)i * D * D;
        const int nb = D / V;
        for (int p = lane; p < D * nb; p += KGE_WAVE) {
            const int r = p / nb, b = (p - r * nb) * V;
            const float hv = h[r];
            const Pack<V> tv = ld<V>(t + b);
            Pack<V> o;
#pragma unroll
            for (int e = 0; e < V; ++e) o.v[e] = hv * tv.v[e];
            st<V>(q + (int64_t)r * D + b, o);
        }
    } else if constexpr (MODEL == KGE_QUATE) {
        // q = conj(h) (x) t per column of the four quarters: <h (x) r^, t> = <conj(h) (x) t, r^>
        float *q = a.Q + (int64_t)i * D;
        const int qd = D / 4;
        for (int off = lane * V; off < qd; off += KGE_WAVE * V) {
            Pack<V> hq[4], tq[4], o[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) { hq[c] = ld<V>(h + c * qd + off); tq[c] = ld<V>(t + c * qd + off); }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const Quat g = quat_mul(quat_conj(Quat{hq[0].v[e], hq[1].v[e], hq[2].v[e], hq[3].v[e]}),
                                        Quat{tq[0].v[e], tq[1].v[e], tq[2].v[e], tq[3].v[e]});
                o[0].v[e] = g.a; o[1].v[e] = g.b; o[2].v[e] = g.c; o[3].v[e] = g.d;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) st<V>(q + c * qd + off, o[c]);
        }
    } else if constexpr (MODEL == KGE_COMPLEX || MODEL == KGE_SIMPLE) {
        float *q = a.Q + (int64_t)i * D;
        const int hd = D / 2;
        for (int off = lane * V; off < hd; off += KGE_WAVE * V) {
            const Pack<V> h0 = ld<V>(h + off), h1 = ld<V>(h + hd + off), t0 = ld<V>(t + off), t1 = ld<V>(t + hd + off);
            Pack<V> o0, o1;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if constexpr (MODEL == KGE_COMPLEX) {
                    o0.v[e] = fmaf(h1.v[e], t1.v[e], h0.v[e] * t0.v[e]);
                    o1.v[e] = fmaf(-h1.v[e], t0.v[e], h0.v[e] * t1.v[e]);
                } else {                           // (h_i, h_j) = (h0, h1), (t_i, t_j) = (t0, t1); row j = [rel | rel_inv]
                    o0.v[e] = 0.5f * h0.v[e] * t1.v[e];
                    o1.v[e] = 0.5f * t0.v[e] * h1.v[e];
                }
            }
            st<V>(q + off, o0);
            st<V>(q + hd + off, o1);
        }
    } else {
        float *q = a.Q + (int64_t)i * D;
        float s = 0.f;
        for (int off = lane * V; off < D; off += KGE_WAVE * V) {
            const Pack<V> hv = ld<V>(h + off), tv = ld<V>(t + off);
            Pack<V> o;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if constexpr (MODEL == KGE_DISTMULT) o.v[e] = hv.v[e] * tv.v[e];
                else if constexpr (MODEL == KGE_TRANSR) o.v[e] = hv.v[e] - tv.v[e];
                else o.v[e] = tv.v[e] - hv.v[e];
                s += o.v[e] * o.v[e];
            }
            st<V>(q + off, o);
        }
        if (a.qsq) {                               // (wavefront-uniform)
            s = wave_sum(s);
            if (lane == 0) a.qsq[i] = s;
        }
    }
}

template <int MODEL>
static int launch_rel_query_m(const RelQueryArgs &a, hipStream_t s) {
    const dim3 g((unsigned)((a.rows + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK)), b(KGE_BLOCK);
    const bool halves = MODEL == KGE_COMPLEX || MODEL == KGE_SIMPLE;
    const bool vec = MODEL == KGE_QUATE ? quate_vec(a.d_e) : halves ? (a.d_e / 2) % 4 == 0 : a.d_e % 4 == 0;
    if (vec) hipLaunchKernelGGL((rel_query_kernel<MODEL, 4>), g, b, 0, s, a);
    else hipLaunchKernelGGL((rel_query_kernel<MODEL, 1>), g, b, 0, s, a);
    return check_launch();
}

int launch_rel_query(int model, const float *ent, const int64_t *h, const int64_t *t, int rows, int d_e, float *Q, float *qsq,
                     hipStream_t s) {
    if (rows <= 0) return KGE_OK;
    RelQueryArgs a{ent, h, t, rows, d_e, Q, qsq};
    switch (model) {
        case KGE_TRANSE_L1: case KGE_TRANSE_L2: return launch_rel_query_m<KGE_TRANSE_L2>(a, s);
        case KGE_DISTMULT: return launch_rel_query_m<KGE_DISTMULT>(a, s);
        case KGE_COMPLEX: return launch_rel_query_m<KGE_COMPLEX>(a, s);
        case KGE_SIMPLE: return launch_rel_query_m<KGE_SIMPLE>(a, s);
        case KGE_RESCAL: return launch_rel_query_m<KGE_RESCAL>(a, s);
        case KGE_TRANSR: return launch_rel_query_m<KGE_TRANSR>(a, s);
        case KGE_QUATE: return launch_rel_query_m<KGE_QUATE>(a, s);
    }
    return KGE_ERR_ARG;
}

// ---- RotatE: s[i, j] = gamma - sum_k |h_ik e^{i theta_jk} - t_ik|,  theta_jk = rel[j, k] / rot_div  (score_fun.py:460-472) --------------
// A VALU-bound pairwise reduction like neg_fwd_pair_kernel<KGE_ROTATE>, with the rotation on the COLUMN side: workgroup = 32 rows x
// 64 relations, k in slabs of 32.  Per slab the tile's cos / sin are computed ONCE (8 sincosf per thread) and kept in LDS, and
// the 32 rows' (h_re, h_im, t_re, t_im) quadruples are staged beside them.  Lane = relation: a wavefront owns 8 rows, reads its
// relation's (cos, sin) of a column once (row stride 33 dwords: the 32 lanes of a half hit 32 banks) and the rows' quadruples as
// one 16-byte broadcast each - 8 modulus terms per two LDS reads of its own.  Padding (k beyond d_e / 2) is staged as zero rows:
// |0 e - 0| = 0.
#define RR_BM 32
#define RR_BN 64
#define RR_BK 32
#define RR_LD (RR_BK + 1)
#define RR_RPW (RR_BM / KGE_WAVES_PER_BLOCK)      // rows per wavefront

struct RelRotArgs {
    const float *ent, *rel; const int64_t *h, *t;
    int rows, K; int64_t n_rel;                   // K = d_e / 2 = d_r
    float gamma, rot_div;
    float *S;                                     // [rows, n_rel]
    int nbn;                                      // relation tiles
};

__global__ __launch_bounds__(KGE_BLOCK) void rel_rotate_score_kernel(RelRotArgs a) {
    __shared__ float cs[RR_BN][RR_LD], sn[RR_BN][RR_LD];
    __shared__ __attribute__((aligned(16))) float4 rw[RR_BM][RR_BK];
    __shared__ int64_t hoff[RR_BM], toff[RR_BM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bm = (int)blockIdx.x / a.nbn, bn = (int)blockIdx.x % a.nbn;
    const int i0 = bm * RR_BM, K = a.K;
    const int64_t j0 = (int64_t)bn * RR_BN;
    if (tid < RR_BM) {                            // (rows beyond the batch re-read its last row and are not written)
        const int i = min(i0 + tid, a.rows - 1);
        hoff[tid] = a.h[i] * (int64_t)(2 * K);
        toff[tid] = a.t[i] * (int64_t)(2 * K);
    }
    __syncthreads();
    float acc[RR_RPW];
#pragma unroll
    for (int r = 0; r < RR_RPW; ++r) acc[r] = 0.f;
    const int kk = tid & (RR_BK - 1);
    for (int k0 = 0; k0 < K; k0 += RR_BK) {
        const bool kok = k0 + kk < K;
        const int k = min(k0 + kk, K - 1);
        // the tile's phases: thread -> column kk of relations (tid >> 5) + 8 e
#pragma unroll
        for (int e = 0; e < RR_BN / 8; ++e) {
            const int jl = (tid >> 5) + 8 * e;
            const int64_t j = min(j0 + jl, a.n_rel - 1);
            float sv, cv;
            sincosf(a.rel[j * K + k] / a.rot_div, &sv, &cv);
            cs[jl][kk] = cv;
            sn[jl][kk] = sv;
        }
        // the rows' quadruples: thread -> column kk of rows (tid >> 5) + 8 e
#pragma unroll
        for (int e = 0; e < RR_BM / 8; ++e) {
            const int il = (tid >> 5) + 8 * e;
            const float *hp = a.ent + hoff[il], *tp = a.ent + toff[il];
            float4 v = make_float4(hp[k], hp[K + k], tp[k], tp[K + k]);
            if (!kok) v = make_float4(0.f, 0.f, 0.f, 0.f);
            rw[il][kk] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < RR_BK; ++c) {
            const float cv = cs[lane][c], sv = sn[lane][c];
#pragma unroll
            for (int r = 0; r < RR_RPW; ++r) {
                const float4 v = rw[wave * RR_RPW + r][c];
                const float re = fmaf(-v.y, sv, v.x * cv) - v.z;
                const float im = fmaf(v.x, sv, v.y * cv) - v.w;
                acc[r] += sqrtf(fmaf(re, re, im * im));
            }
        }
        __syncthreads();
    }
    const int64_t j = j0 + lane;
    if (j < a.n_rel) {
#pragma unroll
        for (int r = 0; r < RR_RPW; ++r) {
            const int i = i0 + wave * RR_RPW + r;
            if (i < a.rows) a.S[(int64_t)i * a.n_rel + j] = a.gamma - acc[r];
        }
    }
}

int launch_rel_rotate_score(const float *ent, const float *rel, const int64_t *h, const int64_t *t, int rows, int64_t n_rel, int d_e,
                            float gamma, float rot_div, float *S, hipStream_t s) {
    if (rows <= 0 || n_rel <= 0) return KGE_OK;
    RelRotArgs a{};
    a.ent = ent; a.rel = rel; a.h = h; a.t = t; a.rows = rows; a.K = d_e / 2; a.n_rel = n_rel; a.gamma = gamma; a.rot_div = rot_div;
    a.S = S;
    a.nbn = (int)((n_rel + RR_BN - 1) / RR_BN);
    const int64_t nb = (int64_t)((rows + RR_BM - 1) / RR_BM) * a.nbn;
    if (nb > 0x7fffffff) return KGE_ERR_ARG;
    hipLaunchKernelGGL(rel_rotate_score_kernel, dim3((unsigned)nb), dim3(KGE_BLOCK), 0, s, a);
    return check_launch();
}

// ---- TransR ---------------------------------------------------------------------------------------------------------------------------
// out = -rel (the "q" rows of the exchanged forward: score = gamma - |u P_j - out_j|_1) and ids[k] = k for k < n_ids (the
// forward walks its positives' relations and its negatives through id lists)
__global__ __launch_bounds__(KGE_BLOCK) void rel_neg_rows_kernel(const float *__restrict__ rel, int64_t n, float *__restrict__ out,
                                                                 int64_t *__restrict__ ids, int64_t n_ids) {
    const int64_t k = (int64_t)blockIdx.x * KGE_BLOCK + threadIdx.x;
    if (k < n) out[k] = -rel[k];
    if (k < n_ids) ids[k] = k;
}

int launch_rel_neg_rows(const float *rel, int64_t n_rel, int d_r, float *out, int64_t *ids, int64_t n_ids, hipStream_t s) {
    const int64_t n = n_rel * d_r, m = n > n_ids ? n : n_ids;
    if (m <= 0) return KGE_OK;
    hipLaunchKernelGGL(rel_neg_rows_kernel, dim3((unsigned)((m + KGE_BLOCK - 1) / KGE_BLOCK)), dim3(KGE_BLOCK), 0, s, rel, n, out, ids, n_ids);
    return check_launch();
}

// ---- QuatE ----------------------------------------------------------------------------------------------------------------------------
// out = the relation table normalised per quaternion (quat_unit: the arithmetic of the edge kernels), the candidate table of the
// (query row, relation row) product.  One thread per quaternion.
__global__ __launch_bounds__(KGE_BLOCK) void rel_unit_rows_kernel(const float *__restrict__ rel, int64_t n_rel, int qd,
                                                                  float *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * KGE_BLOCK + threadIdx.x;
    if (k >= n_rel * qd) return;
    const int64_t o = (k / qd) * (4 * (int64_t)qd) + k % qd;
    float n;
    const Quat u = quat_unit(Quat{rel[o], rel[o + qd], rel[o + 2 * (int64_t)qd], rel[o + 3 * (int64_t)qd]}, n);
    out[o] = u.a; out[o + qd] = u.b; out[o + 2 * (int64_t)qd] = u.c; out[o + 3 * (int64_t)qd] = u.d;
}

int launch_rel_unit_rows(const float *rel, int64_t n_rel, int d_r, float *out, hipStream_t s) {
    const int qd = d_r / 4;
    const int64_t n = n_rel * qd;
    if (n <= 0) return KGE_OK;
    if ((n + KGE_BLOCK - 1) / KGE_BLOCK > 0x7fffffff) return KGE_ERR_ARG;
    hipLaunchKernelGGL(rel_unit_rows_kernel, dim3((unsigned)((n + KGE_BLOCK - 1) / KGE_BLOCK)), dim3(KGE_BLOCK), 0, s, rel, n_rel, qd, out);
    return check_launch();
}
