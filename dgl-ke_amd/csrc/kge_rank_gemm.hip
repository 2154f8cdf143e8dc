// kge_rank_gemm.hip - ranking evaluation of the matrix-form models (KEModel.forward_test, models/general_models.py:436-485;
// candidates = every entity, dataloader/sampler.py:514-597) as ONE LDS-tiled fp32-MFMA GEMM per batch of test triples whose
// epilogue keeps a single BIT per (test triple, candidate): score >= the true triple's score.
//
// Round 6.  The evaluation used the training step's forward tiles (kge_neg_gemm.hip: one wavefront per 16 x 16 tile, operands
// straight from L2 in fragment layout - built for a 200 x 200 x 400 product that is latency) on a 1024 x 14 951 x 400 product
// and wrote the [rows, candidates] score block for a counting kernel: 241 us per batch = 51 TFLOP/s = 32 % of the fp32-MFMA
// peak, 92 % of a validation's device time (tools/eval_timing.py).  A product of this size is a throughput problem:
//   * workgroup tile 128 test rows x 128 candidates, k in stages of 32 through LDS: the main loop of kge_tile_gemm.hpp, which
//     topk_select_kernel (kge_topk.hip) runs too;
//   * epilogue: the score exactly as the forward tiles form it (tile_score: TransE_l2 from the product and the precomputed norms;
//     SimplE: clamp), compared with the row's positive score, four ballots per 16 x 64 strip -> one 64-bit
//     word per row and wavefront: 1.9 MB of mask per batch instead of 61 MB of scores written and read back;
//   * rank_mask_kernel: rank = 1 + popcount(row) - bits at the row's filtered columns - the SAME comparison result serves both
//     terms, so the true triple's own column (always in the filter list) cancels whatever its rounding.
// The pairwise models (TransE_l1, RotatE) and TransR keep the score block + rank_count_kernel (kge_eval.hip).
#include "kge_tile_gemm.hpp"

using namespace kge;

struct RankGemmArgs {
    const float *A; int rows;                     // [rows, D] pos-side vectors of this batch (dense)
    const float *nbase; const int64_t *nidx;      // candidate j: nbase + (nidx ? nidx[j] : j) * D
    int64_t N; int D;
    int l2; float gamma, clampv;
    const float *asq, *bsq, *P;                   // [rows], [N] squared norms (TransE_l2); [rows] positive scores
    unsigned long long *mask; int64_t words;      // out [rows, words] bits: score >= P
};

__global__ __launch_bounds__(256) void rank_gemm_kernel(RankGemmArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][(TILE_BM + TILE_BN) * TILE_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbn = (int)((a.N + TILE_BN - 1) / TILE_BN);
    // consecutive workgroups walk the candidates of one row block: the 128 pos-side rows stay in L2 while the table streams
    const int bm = (int)blockIdx.x / nbn, bn = (int)blockIdx.x % nbn;
    f32x4 acc[4][4];
    tile_gemm_128x128(
        lds, a.D, wave, [&](int i) { return a.A + (int64_t)min(bm * TILE_BM + i, a.rows - 1) * a.D; },
        [&](int j) { return row_ptr(a.nbase, a.nidx, min((int64_t)bn * TILE_BN + j, a.N - 1), a.D); }, acc);
    // ---- epilogue: one bit per (row, candidate); acc[i][j][r] = (row 64 wr + 16 i + 4 q + r, candidate 64 wc + 16 j + m) ------------
    const int wr = wave >> 1, wc = wave & 1;
    const int m = lane & 15, q = lane >> 4;
    const int64_t j0 = (int64_t)bn * TILE_BN + wc * 64;
    float bs[4];
    bool jok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t col = j0 + 16 * j + m;
        jok[j] = col < a.N;
        bs[j] = (a.l2 && jok[j]) ? a.bsq[col] : 0.f;
    }
    const int myrow = bm * TILE_BM + wr * 64 + lane;                 // the row whose word this lane writes
    unsigned long long word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned long long bal[4][4];                               // [r][j]: bit 16 q' + m' = (row 16 i + 4 q' + r, column 16 j + m')
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = min(bm * TILE_BM + wr * 64 + 16 * i + 4 * q + r, a.rows - 1);
            const float p = a.P[row];
            const float as = a.l2 ? a.asq[row] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = tile_score(acc[i][j][r], a.l2, a.gamma, as, bs[j], a.clampv);
                bal[r][j] = __ballot(jok[j] && x >= p);
            }
        }
        if ((lane >> 4) == i) {                                     // lanes 16 i .. 16 i + 15 own rows 16 i + (lane & 15) of the strip
            const int qq = (lane & 15) >> 2, rr = lane & 3;
            unsigned long long w = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r == rr) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) w |= ((bal[r][j] >> (16 * qq)) & 0xffffull) << (16 * j);
                }
            word = w;
        }
    }
    if (myrow < a.rows) a.mask[(int64_t)myrow * a.words + (j0 >> 6)] = word;     // (columns beyond N: zero bits)
}

// TransH (include/kge_hip.h): the same tile with its 128 pos-side rows holding the pairs (a, w^) of 64 test rows, interleaved by
// 16-row strips (transh_tile_query, kge_tile_gemm.hpp) so that a lane holds p = a . n and q = w^ . n of one (row, candidate) pair;
// the epilogue scores with transh_score and keeps the same bits in the same mask layout (rank_mask_kernel counts them)
#define RANK_TH_BM (TILE_BM / 2)
struct RankTranshArgs {
    const float *A, *W; int rows;                 // [rows, D] x 2: the pairs of this batch (dense)
    const float *nbase; const int64_t *nidx;
    int64_t N; int D;
    float gamma;
    const float *alpha, *cw, *beta, *P;           // [rows] |a|^2, w^ . a; [N] |n|^2; [rows] positive scores
    unsigned long long *mask; int64_t words;
};

__global__ __launch_bounds__(256) void rank_gemm_transh_kernel(RankTranshArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][(TILE_BM + TILE_BN) * TILE_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbn = (int)((a.N + TILE_BN - 1) / TILE_BN);
    const int bm = (int)blockIdx.x / nbn, bn = (int)blockIdx.x % nbn;
    f32x4 acc[4][4];
    tile_gemm_128x128(
        lds, a.D, wave,
        [&](int R) { return (transh_tile_is_w(R) ? a.W : a.A) + (int64_t)min(bm * RANK_TH_BM + transh_tile_query(R), a.rows - 1) * a.D; },
        [&](int j) { return row_ptr(a.nbase, a.nidx, min((int64_t)bn * TILE_BN + j, a.N - 1), a.D); }, acc);
    // ---- epilogue: p = acc[i][j][r], q = acc[i + 2][j][r] of (row 32 wr + 16 i + 4 q + r, candidate 64 wc + 16 j + m), i < 2 ----------
    const int wr = wave >> 1, wc = wave & 1;
    const int m = lane & 15, q = lane >> 4;
    const int64_t j0 = (int64_t)bn * TILE_BN + wc * 64;
    float bs[4];
    bool jok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t col = j0 + 16 * j + m;
        jok[j] = col < a.N;
        bs[j] = jok[j] ? a.beta[col] : 0.f;
    }
    const int myrow = bm * RANK_TH_BM + wr * 32 + lane;              // lanes 0 .. 31: the row whose word this lane writes
    unsigned long long word = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        unsigned long long bal[4][4];                               // [r][j]: bit 16 q' + m' = (row 16 i + 4 q' + r, column 16 j + m')
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = min(bm * RANK_TH_BM + wr * 32 + 16 * i + 4 * q + r, a.rows - 1);
            const float p = a.P[row], as = a.alpha[row], cw = a.cw[row];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = transh_score(acc[i][j][r], acc[i + 2][j][r], a.gamma, as, bs[j], cw);
                bal[r][j] = __ballot(jok[j] && x >= p);
            }
        }
        if ((lane >> 4) == i) {                                     // lanes 16 i .. 16 i + 15 own rows 16 i + (lane & 15) of the strip
            const int qq = (lane & 15) >> 2, rr = lane & 3;
            unsigned long long w = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r == rr) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) w |= ((bal[r][j] >> (16 * qq)) & 0xffffull) << (16 * j);
                }
            word = w;
        }
    }
    if (lane < 32 && myrow < a.rows) a.mask[(int64_t)myrow * a.words + (j0 >> 6)] = word;
}

// TransD (include/kge_hip.h): the same tile on the pairs (a, rho).  The candidate operand is the FIRST D columns of a table row 2 D
// wide - row_b points at the table row itself, the table is never copied - and the epilogue takes three scalars per row and two per
// candidate (transd_score).  A kernel of its own rather than a trait shared with rank_gemm_transh_kernel: the shared body compiled
// TransH's instance to a different instruction order than it had on its own
struct RankTransdArgs {
    const float *A, *W; int rows;                 // [rows, D] x 2: the pairs (a, rho) of this batch (dense)
    const float *nbase; const int64_t *nidx;      // rows 2 D wide
    int64_t N; int D;
    float gamma;
    const float *alpha, *sig, *u, *beta, *cj, *P; // [rows] |a|^2, |rho|^2, a . rho; [N] |n|^2, m . n; [rows] positive scores
    unsigned long long *mask; int64_t words;
};

__global__ __launch_bounds__(256) void rank_gemm_transd_kernel(RankTransdArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][(TILE_BM + TILE_BN) * TILE_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbn = (int)((a.N + TILE_BN - 1) / TILE_BN);
    const int bm = (int)blockIdx.x / nbn, bn = (int)blockIdx.x % nbn;
    f32x4 acc[4][4];
    tile_gemm_128x128(
        lds, a.D, wave,
        [&](int R) { return (transh_tile_is_w(R) ? a.W : a.A) + (int64_t)min(bm * RANK_TH_BM + transh_tile_query(R), a.rows - 1) * a.D; },
        [&](int j) { return row_ptr(a.nbase, a.nidx, min((int64_t)bn * TILE_BN + j, a.N - 1), 2 * a.D); }, acc);
    // ---- epilogue: p = acc[i][j][r], q = acc[i + 2][j][r] of (row 32 wr + 16 i + 4 q + r, candidate 64 wc + 16 j + m), i < 2 ----------
    const int wr = wave >> 1, wc = wave & 1;
    const int m = lane & 15, q = lane >> 4;
    const int64_t j0 = (int64_t)bn * TILE_BN + wc * 64;
    float bs[4], cj[4];
    bool jok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t col = j0 + 16 * j + m;
        jok[j] = col < a.N;
        bs[j] = jok[j] ? a.beta[col] : 0.f;
        cj[j] = jok[j] ? a.cj[col] : 0.f;
    }
    const int myrow = bm * RANK_TH_BM + wr * 32 + lane;              // lanes 0 .. 31: the row whose word this lane writes
    unsigned long long word = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        unsigned long long bal[4][4];                               // [r][j]: bit 16 q' + m' = (row 16 i + 4 q' + r, column 16 j + m')
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = min(bm * RANK_TH_BM + wr * 32 + 16 * i + 4 * q + r, a.rows - 1);
            const float p = a.P[row], as = a.alpha[row], sg = a.sig[row], u = a.u[row];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = transd_score(acc[i][j][r], acc[i + 2][j][r], a.gamma, as, sg, u, bs[j], cj[j]);
                bal[r][j] = __ballot(jok[j] && x >= p);
            }
        }
        if ((lane >> 4) == i) {                                     // lanes 16 i .. 16 i + 15 own rows 16 i + (lane & 15) of the strip
            const int qq = (lane & 15) >> 2, rr = lane & 3;
            unsigned long long w = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r == rr) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) w |= ((bal[r][j] >> (16 * qq)) & 0xffffull) << (16 * j);
                }
            word = w;
        }
    }
    if (lane < 32 && myrow < a.rows) a.mask[(int64_t)myrow * a.words + (j0 >> 6)] = word;
}

// rank_i = 1 + #{j : bit(i, j)} - #{j in filt_i : bit(i, j)};  filt_i = filt_ids[filt_ptr[2 (e0 + i)] .. filt_ptr[2 (e0 + i) + 1])
__global__ __launch_bounds__(KGE_BLOCK) void rank_mask_kernel(const unsigned long long *__restrict__ mask, int64_t words, int64_t N,
                                                             int rows, const int64_t *__restrict__ filt_ptr,
                                                             const int64_t *__restrict__ filt_ids, int64_t e0,
                                                             int32_t *__restrict__ ranks) {
    const int i = (int)blockIdx.x * KGE_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);      // one wavefront per test triple
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long *row = mask + (int64_t)i * words;
    int cnt = 0;
    for (int64_t w = lane; w < words; w += 64) cnt += __popcll(row[w]);
    if (filt_ptr) {
        const int64_t f0 = filt_ptr[2 * (e0 + i)], f1 = filt_ptr[2 * (e0 + i) + 1];
        for (int64_t k = f0 + lane; k < f1; k += 64) {
            const int64_t col = filt_ids[k];
            if (col >= 0 && col < N) cnt -= (int)((row[col >> 6] >> (col & 63)) & 1ull);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) ranks[e0 + i] = 1 + cnt;
}

bool rank_gemm_supported(int model, int d_e) {
    return (model == KGE_TRANSE_L2 || model == KGE_DISTMULT || model == KGE_COMPLEX || model == KGE_SIMPLE || model == KGE_RESCAL ||
            model == KGE_QUATE) &&
           d_e >= 4 && d_e % 4 == 0;
}
size_t rank_gemm_mask_bytes(int rows, int64_t N) { return (size_t)rows * (size_t)((N + 127) / 128 * 2) * 8; }

// A, asq (TransE_l2), P: this batch's pos-side vectors / norms / positive scores (edge_fwd); bsq: the candidates' norms
int launch_rank_gemm(int model, const float *A, int rows, const float *nbase, const int64_t *nidx, int64_t N, int D, float gamma,
                     float clampv, const float *asq, const float *bsq, const float *P, void *mask, const int64_t *filt_ptr,
                     const int64_t *filt_ids, int64_t e0, int32_t *ranks, hipStream_t s) {
    if (rows <= 0) return KGE_OK;
    RankGemmArgs a{};
    a.A = A; a.rows = rows; a.nbase = nbase; a.nidx = nidx; a.N = N; a.D = D;
    a.l2 = model == KGE_TRANSE_L2 ? 1 : 0; a.gamma = gamma; a.clampv = clampv;
    a.asq = asq; a.bsq = bsq; a.P = P;
    a.mask = reinterpret_cast<unsigned long long *>(mask);
    a.words = (N + 127) / 128 * 2;                                // whole 128-candidate tiles: every word of a row is written
    const int64_t nb = (int64_t)((rows + TILE_BM - 1) / TILE_BM) * ((N + TILE_BN - 1) / TILE_BN);
    hipLaunchKernelGGL(rank_gemm_kernel, dim3((unsigned)nb), dim3(256), 0, s, a);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(rank_mask_kernel, dim3((unsigned)((rows + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK)), dim3(KGE_BLOCK), 0, s,
                       a.mask, a.words, N, rows, filt_ptr, filt_ids, e0, ranks);
    return check_launch();
}

// TransH: A, W, alpha, cw, P: this batch's pairs, their statistics and positive scores (transh_edge_fwd); beta: the candidates' |n|^2
int launch_rank_gemm_transh(const float *A, const float *W, int rows, const float *nbase, const int64_t *nidx, int64_t N, int D, float gamma,
                            const float *alpha, const float *cw, const float *beta, const float *P, void *mask, const int64_t *filt_ptr,
                            const int64_t *filt_ids, int64_t e0, int32_t *ranks, hipStream_t s) {
    if (rows <= 0) return KGE_OK;
    RankTranshArgs a{};
    a.A = A; a.W = W; a.rows = rows; a.nbase = nbase; a.nidx = nidx; a.N = N; a.D = D; a.gamma = gamma;
    a.alpha = alpha; a.cw = cw; a.beta = beta; a.P = P;
    a.mask = reinterpret_cast<unsigned long long *>(mask);
    a.words = (N + 127) / 128 * 2;
    const int64_t nb = (int64_t)((rows + RANK_TH_BM - 1) / RANK_TH_BM) * ((N + TILE_BN - 1) / TILE_BN);
    hipLaunchKernelGGL(rank_gemm_transh_kernel, dim3((unsigned)nb), dim3(256), 0, s, a);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(rank_mask_kernel, dim3((unsigned)((rows + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK)), dim3(KGE_BLOCK), 0, s,
                       a.mask, a.words, N, rows, filt_ptr, filt_ids, e0, ranks);
    return check_launch();
}

// TransD: A, R, alpha, sig, u, P: this batch's pairs, their statistics and positive scores (transd_edge_fwd); beta, cj: the candidates'
int launch_rank_gemm_transd(const float *A, const float *R, int rows, const float *nbase, const int64_t *nidx, int64_t N, int D, float gamma,
                            const float *alpha, const float *sig, const float *u, const float *beta, const float *cj, const float *P,
                            void *mask, const int64_t *filt_ptr, const int64_t *filt_ids, int64_t e0, int32_t *ranks, hipStream_t s) {
    if (rows <= 0) return KGE_OK;
    RankTransdArgs a{};
    a.A = A; a.W = R; a.rows = rows; a.nbase = nbase; a.nidx = nidx; a.N = N; a.D = D; a.gamma = gamma;
    a.alpha = alpha; a.sig = sig; a.u = u; a.beta = beta; a.cj = cj; a.P = P;
    a.mask = reinterpret_cast<unsigned long long *>(mask);
    a.words = (N + 127) / 128 * 2;
    const int64_t nb = (int64_t)((rows + RANK_TH_BM - 1) / RANK_TH_BM) * ((N + TILE_BN - 1) / TILE_BN);
    hipLaunchKernelGGL(rank_gemm_transd_kernel, dim3((unsigned)nb), dim3(256), 0, s, a);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(rank_mask_kernel, dim3((unsigned)((rows + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK)), dim3(KGE_BLOCK), 0, s,
                       a.mask, a.words, N, rows, filt_ptr, filt_ids, e0, ranks);
    return check_launch();
}
