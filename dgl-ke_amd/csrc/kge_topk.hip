// kge_topk.hip - inference: top-K triples of a trained model and top-K similar embedding pairs (the reference's ScoreInfer /
// EmbSimInfer, models/infer.py:52-344) without a score block in memory.
//
//   * topk_select_kernel: workgroup = 128 query rows x one SEGMENT of the candidate list, walked in 128-candidate tiles in
//     increasing index order.  A tile's scores come from the main loop rank_gemm_kernel runs (k stages of 32 through LDS, 16x16x4
//     fp32 MFMA, kge_tile_gemm.hpp) for the matrix forms, or from a VALU loop over the same staging for the pairwise forms
//     (TransE_l1, RotatE, l1 and any D that is not a multiple of 4).  The tile goes to LDS; each wavefront then walks its 32
//     rows: one compare against the row's running K-th best and one ballot per score.  Survivors are merged into the row's
//     list (in the workspace, sorted) by rank counting in a per-wavefront LDS queue.  Entries are 64-bit composites
//     (order-preserving score key << 32 | ~candidate index): "composite <= threshold -> reject" is the score test AND tie
//     rule 2 (equal scores: the lower position first), and NaN (key 0) ranks below every number.
//     The filtered form (template argument TopkSelArgsF; link prediction with known-edge exclusion) looks the survivors of that
//     compare up in the row's sorted list of entity ids and drops the listed ones before the merge: a listed candidate
//     never enters a row's list or becomes its threshold.  The unfiltered instances are the code they were without it.
//   * topk_merge_kernel: bitonic sort of up to 2048 (score, ordinal) entries in LDS, fan-in 2048 / K - 1 lists per pass; a
//     tree of passes reduces the segments of a row, then the rows of a group, together with the group's running result
//     (carried across row batches by the caller).
//   * the K selected scores of the l2 forms are recomputed in the direct difference form (topk_l2_fix_kernel): the
//     |a|^2 + |b|^2 - 2 a.b form loses ~1e-3 to cancellation at the top of an l2 list.
// Workspace: O(rows x (D + segments x K)) + O(N) candidate norms, whatever |H| |R| |T| is.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <type_traits>
#include "kge_tile_gemm.hpp"
#include "kge_models.hpp"
#include "kge_own_fwd.hpp"

using namespace kge;

#define TK_MCAP 2048                              // entries of one merge workgroup

// accumulator kinds (template) and epilogues (runtime)
enum { ACC_MFMA = 0, ACC_DOT = 1, ACC_SQ = 2, ACC_L1 = 3, ACC_ROT = 4, ACC_PRE = 5, ACC_TH = 6, ACC_THV = 7, ACC_TD = 8, ACC_TDV = 9 };
// ACC_PRE (PairRE, include/kge_hip.h): query row i is the pair (a_i, w_i) - abase holds the rows' a block followed by their w block,
// [rows, D] each - and bn the candidates' norms |x_j|_2: the tile accumulates |a_ik - w_ik x_jk / |x_j||
// ACC_TH / ACC_THV (TransH, include/kge_hip.h): query row i is the pair (a_i, w^_i) - abase holds the rows' a block, their w^ block
// ([rows, D] each) and then c_i = w^_i . a_i [rows]; an = |a|^2, bn = |n|^2.  The tile accumulates p = a . n and q = w^ . n and
// scores with transh_score.  ACC_TH: the shared MFMA tile twice per candidate tile, 64 queries each with the two operands
// interleaved by strips (transh_tile_query, kge_tile_gemm.hpp); ACC_THV: the VALU tile with a second accumulator (D < 32)
// ACC_TD / ACC_TDV (TransD, include/kge_hip.h): the same two tiles as ACC_TH / ACC_THV on the pair (a_i, rho_i), D = k floats each -
// abase holds the rows' a block, their rho block ([rows, D] each), then sigma_i = |rho_i|^2 [rows] and u_i = a_i . rho_i [rows];
// an = |a|^2; bn = [beta | c], N floats each.  Candidate j is the FIRST D columns of its table row, which is 2 D wide
// (the kernel's TD); the score is transd_score
enum { EPI_RAW = 0, EPI_L2G = 1, EPI_COS = 2, EPI_JAC = 3, EPI_GMINUS = 4, EPI_GSQRT = 5 };

struct TopkSelArgs {
    const float *abase; const int64_t *aidx; int rows;   // query row i: abase + (aidx ? aidx[i] : i) * D
    const float *nbase; const int64_t *nidx;             // candidate j: nbase + (nidx ? nidx[j] : j) * D
    int64_t N; int D, epi, S, K;
    float gamma;
    const float *an, *bn;                                // [rows], [N]: |a|^2, |b|^2 (L2G, JAC) or |a|, |b| (COS)
    unsigned long long *part;                            // out [rows, S, K] composites, sorted, 0 = empty
};
// the filtered form: candidates whose ENTITY id is in filt_ids[filt_ptr[2i] .. filt_ptr[2i+1]) (ascending, unique) never enter row i's list
struct TopkSelArgsF : TopkSelArgs {
    const int64_t *filt_ptr, *filt_ids;
};

__device__ __forceinline__ uint32_t fkey(float f) {
    if (f != f) return 0u;                               // NaN: below every number
    const uint32_t u = f == 0.f ? 0u : __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float keyf(uint32_t k) {
    if (k == 0u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned long long comp_of(float s, int64_t j) {
    return ((unsigned long long)fkey(s) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)j);
}
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int64_t lane_bcast(int64_t v, int x) {                 // lane x's v (x wave-uniform)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), x);
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float epilogue(const TopkSelArgs &a, float x, int64_t row, int64_t col) {
    switch (a.epi) {
    case EPI_L2G: return l2_score(x, a.gamma, a.an[row], a.bn[col]);
    case EPI_COS: return x / (a.an[row] * a.bn[col]);
    case EPI_JAC: return x / (a.an[row] + a.bn[col] - x);
    case EPI_GMINUS: return a.gamma - x;
    case EPI_GSQRT: return a.gamma - sqrtf(x);
    default: return x;
    }
}

template <int ACC, class Args = TopkSelArgs>
__global__ __launch_bounds__(256) void topk_select_kernel(Args a) {
    constexpr bool FILT = !std::is_same<Args, TopkSelArgs>::value;
    __shared__ __attribute__((aligned(16))) float lds[2][(TILE_BM + TILE_BN) * TILE_LD];
    __shared__ unsigned long long rthr[TILE_BM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = (int)blockIdx.x / a.S, seg = (int)blockIdx.x % a.S;
    const int64_t nbn = (a.N + TILE_BN - 1) / TILE_BN, tps = (nbn + a.S - 1) / a.S;
    const int64_t tile0 = (int64_t)seg * tps, tile1 = min(nbn, tile0 + tps);
    const int r0 = rb * TILE_BM, D = a.D, K = a.K;
    constexpr bool TD = ACC == ACC_TD || ACC == ACC_TDV;                        // TransD: candidate rows 2 D wide, their first half enters
    float *sc = &lds[0][0];                                                    // [128][128] score tile (after the main loop)
    unsigned long long *un = reinterpret_cast<unsigned long long *>(&lds[0][0] + TILE_BM * TILE_BN) + wave * 256;
    for (int e = tid; e < TILE_BM * K; e += 256) {
        const int lr = e / K;
        if (r0 + lr < a.rows) a.part[((int64_t)(r0 + lr) * a.S + seg) * K + e % K] = 0ull;
    }
    if (tid < TILE_BM) rthr[tid] = 0ull;
    const int64_t *frng = nullptr;                                             // [128][2]: the rows' list ranges (filtered form)
    if constexpr (FILT) {
        __shared__ int64_t frng_lds[TILE_BM * 2];
        if (tid < TILE_BM * 2) frng_lds[tid] = a.filt_ptr[2 * (int64_t)min(r0 + (tid >> 1), a.rows - 1) + (tid & 1)];
        frng = frng_lds;
    }
    __syncthreads();
    for (int64_t bn = tile0; bn < tile1; ++bn) {
        if constexpr (ACC == ACC_MFMA) {
            // ---- the shared 128 x 128 MFMA tile (kge_tile_gemm.hpp), D % 4 == 0 ------------------------------------------------
            f32x4 acc[4][4];
            tile_gemm_128x128(
                lds, D, wave, [=](int i) { return row_ptr(a.abase, a.aidx, min(r0 + i, a.rows - 1), D); },
                [=](int j) { return row_ptr(a.nbase, a.nidx, min(bn * TILE_BN + j, a.N - 1), D); }, acc);
            const int wr = wave >> 1, wc = wave & 1;
            const int m = lane & 15, q = lane >> 4;
            // tile -> LDS: acc[i][j][r] = (row 64 wr + 16 i + 4 q + r, column 64 wc + 16 j + m)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = wr * 64 + 16 * i + 4 * q + r;
                    const int64_t grow = min(r0 + row, a.rows - 1);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int col = wc * 64 + 16 * j + m;
                        const int64_t gcol = min(bn * TILE_BN + col, a.N - 1);
                        sc[row * TILE_BN + col] = epilogue(a, acc[i][j][r], grow, gcol);
                    }
                }
        } else if constexpr (ACC == ACC_TH || ACC == ACC_TD) {
            const float *wb = a.abase + (int64_t)a.rows * D, *cb = wb + (int64_t)a.rows * D;     // (TransD: cb = sigma, u behind it)
            const int wr = wave >> 1, wc = wave & 1;
            const int m = lane & 15, q = lane >> 4;
            float sv[2][2][4][4];                                               // [half][strip][j][r]: lds is the tile's until both halves are done
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 acc[4][4];
                tile_gemm_128x128(
                    lds, D, wave,
                    [=](int R) {
                        const int64_t row = min(r0 + 64 * half + transh_tile_query(R), a.rows - 1);
                        return (transh_tile_is_w(R) ? wb : a.abase) + row * D;
                    },
                    [=](int j) { return row_ptr(a.nbase, a.nidx, min(bn * TILE_BN + j, a.N - 1), TD ? 2 * D : D); }, acc);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t grow = min(r0 + 64 * half + 32 * wr + 16 * i + 4 * q + r, a.rows - 1);
                        const float as = a.an[grow], cw = cb[grow];
                        [[maybe_unused]] float uu = 0.f;
                        if constexpr (TD) uu = cb[a.rows + grow];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int64_t gcol = min(bn * TILE_BN + wc * 64 + 16 * j + m, a.N - 1);
                            if constexpr (TD)
                                sv[half][i][j][r] = transd_score(acc[i][j][r], acc[i + 2][j][r], a.gamma, as, cw, uu, a.bn[gcol], a.bn[a.N + gcol]);
                            else sv[half][i][j][r] = transh_score(acc[i][j][r], acc[i + 2][j][r], a.gamma, as, a.bn[gcol], cw);
                        }
                    }
            }
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            sc[(64 * half + 32 * wr + 16 * i + 4 * q + r) * TILE_BN + wc * 64 + 16 * j + m] = sv[half][i][j][r];
        } else {
            // ---- VALU tile: thread (tx, ty) owns rows ty + 16 i, columns tx + 16 j; scalar staging (any D) ------------------
            const int tx = tid & 15, ty = tid >> 4;
            const int hd = D / 2;
            const int nst = ACC == ACC_ROT ? (hd + 15) / 16 : (D + TILE_BK - 1) / TILE_BK;
            float acc[8][8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
            constexpr bool PV = ACC == ACC_THV || ACC == ACC_TDV;                  // TransH / TransD: q = w^ . n next to p = a . n
            [[maybe_unused]] float acc2[PV ? 8 : 1][8];
            if constexpr (PV) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc2[i][j] = 0.f;
            }
            for (int s = 0; s < nst; ++s) {
                float g[32];
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int f = tid + 256 * i, row = f >> 5, c = f & 31;
                    const float *p = row < TILE_BM ? row_ptr(a.abase, a.aidx, min(r0 + row, a.rows - 1), D)
                                                 : row_ptr(a.nbase, a.nidx, min(bn * TILE_BN + row - TILE_BM, a.N - 1), TD ? 2 * D : D);
                    int col; bool ok;
                    if constexpr (ACC == ACC_ROT) { const int k = s * 16 + (c & 15); ok = k < hd; col = (c < 16 ? 0 : hd) + min(k, hd - 1); }
                    else { const int k = s * TILE_BK + c; ok = k < D; col = min(k, D - 1); }
                    const float v = p[col];
                    g[i] = ok ? v : 0.f;
                }
                [[maybe_unused]] float gw[16];
                if constexpr (ACC == ACC_PRE) {
                    // the candidate half of the slab normalised (x / |x|, 0 where |x| == 0)
#pragma unroll
                    for (int i = 16; i < 32; ++i) {
                        const float nj = a.bn[min(bn * TILE_BN + ((tid + 256 * i) >> 5) - TILE_BM, a.N - 1)];
                        g[i] = nj > 0.f ? g[i] / nj : 0.f;
                    }
                }
                if constexpr (ACC == ACC_PRE || PV) {
                    // the rows' w slab for the second buffer
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int f = tid + 256 * i, row = f >> 5, k = s * TILE_BK + (f & 31);
                        const float v = a.abase[((int64_t)a.rows + min(r0 + row, a.rows - 1)) * D + min(k, D - 1)];
                        gw[i] = k < D ? v : 0.f;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int f = tid + 256 * i;
                    lds[0][(f >> 5) * TILE_LD + (f & 31)] = g[i];
                }
                if constexpr (ACC == ACC_PRE || PV) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int f = tid + 256 * i;
                        lds[1][(f >> 5) * TILE_LD + (f & 31)] = gw[i];
                    }
                }
                __syncthreads();
                if constexpr (ACC == ACC_ROT) {
                    for (int k = 0; k < 16; ++k) {
                        float are[8], aim[8], bre[8], bim[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) { are[i] = lds[0][(ty + 16 * i) * TILE_LD + k]; aim[i] = lds[0][(ty + 16 * i) * TILE_LD + 16 + k]; }
#pragma unroll
                        for (int j = 0; j < 8; ++j) { bre[j] = lds[0][(TILE_BM + tx + 16 * j) * TILE_LD + k]; bim[j] = lds[0][(TILE_BM + tx + 16 * j) * TILE_LD + 16 + k]; }
#pragma unroll
                        for (int i = 0; i < 8; ++i)
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                const float dr = are[i] - bre[j], di = aim[i] - bim[j];
                                acc[i][j] += sqrtf(fmaf(dr, dr, di * di));
                            }
                    }
                } else {
                    for (int k = 0; k < TILE_BK; ++k) {
                        float av[8], bv[8];
                        [[maybe_unused]] float wv[8];
                        if constexpr (ACC == ACC_PRE || PV) {
#pragma unroll
                            for (int i = 0; i < 8; ++i) wv[i] = lds[1][(ty + 16 * i) * TILE_LD + k];
                        }
#pragma unroll
                        for (int i = 0; i < 8; ++i) av[i] = lds[0][(ty + 16 * i) * TILE_LD + k];
#pragma unroll
                        for (int j = 0; j < 8; ++j) bv[j] = lds[0][(TILE_BM + tx + 16 * j) * TILE_LD + k];
#pragma unroll
                        for (int i = 0; i < 8; ++i)
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                if constexpr (PV) { acc[i][j] = fmaf(av[i], bv[j], acc[i][j]); acc2[i][j] = fmaf(wv[i], bv[j], acc2[i][j]); }
                                else if constexpr (ACC == ACC_DOT) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
                                else if constexpr (ACC == ACC_SQ) { const float d = av[i] - bv[j]; acc[i][j] = fmaf(d, d, acc[i][j]); }
                                else if constexpr (ACC == ACC_PRE) acc[i][j] += fabsf(fmaf(-wv[i], bv[j], av[i]));
                                else acc[i][j] += fabsf(av[i] - bv[j]);
                            }
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = ty + 16 * i;
                const int64_t grow = min(r0 + row, a.rows - 1);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int col = tx + 16 * j;
                    if constexpr (ACC == ACC_TDV) {
                        const int64_t gcol = min(bn * TILE_BN + col, a.N - 1);
                        const float *sgb = a.abase + 2 * (int64_t)a.rows * D;
                        sc[row * TILE_BN + col] = transd_score(acc[i][j], acc2[i][j], a.gamma, a.an[grow], sgb[grow], sgb[a.rows + grow], a.bn[gcol],
                                                               a.bn[a.N + gcol]);
                    } else if constexpr (ACC == ACC_THV)
                        sc[row * TILE_BN + col] = transh_score(acc[i][j], acc2[i][j], a.gamma, a.an[grow], a.bn[min(bn * TILE_BN + col, a.N - 1)],
                                                               a.abase[2 * (int64_t)a.rows * D + grow]);
                    else sc[row * TILE_BN + col] = epilogue(a, acc[i][j], grow, min(bn * TILE_BN + col, a.N - 1));
                }
            }
        }
        __syncthreads();
        // ---- selection: wavefront w walks rows 32 w .. 32 w + 31 of the tile ------------------------------------------------
        [[maybe_unused]] int64_t id0 = 0, id1 = 0;                              // (filtered form) the entity ids of this lane's two candidates
        if constexpr (FILT) {
            const int64_t c0 = min(bn * TILE_BN + lane, a.N - 1), c1 = min(bn * TILE_BN + lane + 64, a.N - 1);
            id0 = a.nidx ? a.nidx[c0] : c0; id1 = a.nidx ? a.nidx[c1] : c1;
        }
        for (int lr = wave * 32; lr < wave * 32 + 32; ++lr) {
            if (r0 + lr >= a.rows) break;
            const unsigned long long thr = rthr[lr];
            const int64_t j0 = bn * TILE_BN + lane, j1 = j0 + 64;
            const unsigned long long c0 = j0 < a.N ? comp_of(sc[lr * TILE_BN + lane], j0) : 0ull;
            const unsigned long long c1 = j1 < a.N ? comp_of(sc[lr * TILE_BN + lane + 64], j1) : 0ull;
            bool s0 = c0 > thr, s1 = c1 > thr;
            unsigned long long b0 = __ballot(s0), b1 = __ballot(s1);
            if ((b0 | b1) == 0ull) continue;                                   // the common case
            if constexpr (FILT) {
                // only the survivors of the compare are looked up in the row's list (the range, read once per workgroup
                // into LDS, is wave-uniform: rows with an empty list skip this).  Up to 64 entries: one coalesced read,
                // then every entry broadcast to all lanes; longer lists: a binary search per surviving lane.
                const int64_t f0 = frng[2 * lr], f1 = frng[2 * lr + 1];
                if (f1 > f0) {
                    if (f1 - f0 <= 64) {
                        const int nf = (int)(f1 - f0);
                        const int64_t e = lane < nf ? a.filt_ids[f0 + lane] : -1;
                        bool k0 = false, k1 = false;
                        for (int x = 0; x < nf; ++x) {
                            const int64_t v = lane_bcast(e, x);
                            k0 |= v == id0; k1 |= v == id1;
                        }
                        s0 = s0 && !k0; s1 = s1 && !k1;
                    } else {
                        if (s0) s0 = !in_sorted(a.filt_ids, f0, f1, id0);
                        if (s1) s1 = !in_sorted(a.filt_ids, f0, f1, id1);
                    }
                    b0 = __ballot(s0); b1 = __ballot(s1);
                    if ((b0 | b1) == 0ull) continue;
                }
            }
            unsigned long long *list = a.part + ((int64_t)(r0 + lr) * a.S + seg) * K;
            for (int p = lane; p < K; p += 64) un[p] = list[p];
            const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
            const int n0 = __popcll(b0), n = K + n0 + __popcll(b1);
            if (s0) un[K + __popcll(b0 & below)] = c0;
            if (s1) un[K + n0 + __popcll(b1 & below)] = c1;
            wave_sync();
            unsigned long long v[4];
            int rk[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[i] = lane + 64 * i < n ? un[lane + 64 * i] : 0ull; rk[i] = 0; }
            for (int x = 0; x < n; ++x) {
                const unsigned long long u = un[x];
#pragma unroll
                for (int i = 0; i < 4; ++i) rk[i] += u > v[i] ? 1 : 0;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (v[i] != 0ull && rk[i] < K) {
                    list[rk[i]] = v[i];
                    if (rk[i] == K - 1) rthr[lr] = v[i];
                }
            wave_sync();
        }
        __syncthreads();
    }
}

// [rows, S, K] composites -> (score, ordinal = row_base[row] + j * stride; -1 = empty)
__global__ void topk_unpack_kernel(const unsigned long long *part, int64_t n, int SK, const int64_t *row_base, int64_t stride,
                                   float *os, int64_t *oo) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const unsigned long long c = part[e];
    if (c == 0ull) { os[e] = 0.f; oo[e] = -1; return; }
    const int64_t j = (int64_t)(0xffffffffu - (uint32_t)(c & 0xffffffffull));
    os[e] = keyf((uint32_t)(c >> 32));
    oo[e] = row_base[e / SK] + j * stride;
}

// the K selected entries of each row in the direct difference form: gamma - |a - b|_2
__global__ __launch_bounds__(KGE_BLOCK) void topk_l2_fix_kernel(const float *abase, const int64_t *aidx, const float *nbase,
                                                                const int64_t *nidx, int D, int rows, int K, const int64_t *row_base,
                                                                int64_t stride, float gamma, float *os, const int64_t *oo) {
    const int64_t e = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (e >= (int64_t)rows * K) return;
    const int64_t o = oo[e];
    if (o < 0) return;
    const int64_t row = e / K, j = (o - row_base[row]) / stride;
    const float *x = row_ptr(abase, aidx, row, D), *y = row_ptr(nbase, nidx, j, D);
    float s = 0.f;
    for (int k = threadIdx.x & 63; k < D; k += 64) { const float d = x[k] - y[k]; s = fmaf(d, d, s); }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) os[e] = gamma - sqrtf(s);
}

__device__ __forceinline__ bool beats(uint32_t ka, int64_t oa, uint32_t kb, int64_t ob) { return ka > kb || (ka == kb && oa < ob); }

// workgroup (g, c): top K of lists [c fan, min(L, (c+1) fan)) of group g (+ the group's running result when c == 0)
__global__ __launch_bounds__(256) void topk_merge_kernel(const float *is, const int64_t *io, int L, int fan, int K, int nout,
                                                         const float *xs, const int64_t *xo, float *os, int64_t *oo) {
    __shared__ uint32_t key[TK_MCAP];
    __shared__ int64_t ord[TK_MCAP];
    const int64_t g = (int64_t)blockIdx.x / nout;
    const int c = (int)blockIdx.x % nout, tid = threadIdx.x;
    const int l0 = c * fan, nl = min(L, l0 + fan) - l0;
    const int nin = nl * K, ntot = nin + ((xs && c == 0) ? K : 0);
    int P = 1;
    while (P < ntot) P <<= 1;
    const float *src_s = is + ((int64_t)g * L + l0) * K;
    const int64_t *src_o = io + ((int64_t)g * L + l0) * K;
    for (int e = tid; e < P; e += 256) {
        float s = 0.f; int64_t o = -1;
        if (e < nin) { s = src_s[e]; o = src_o[e]; }
        else if (e < ntot) { s = xs[g * K + e - nin]; o = xo[g * K + e - nin]; }
        key[e] = o < 0 ? 0u : fkey(s);
        ord[e] = o < 0 ? INT64_MAX : o;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int ij = i ^ j;
                if (ij > i) {
                    const bool best_first = (i & k) == 0;
                    const bool sw = best_first ? beats(key[ij], ord[ij], key[i], ord[i]) : beats(key[i], ord[i], key[ij], ord[ij]);
                    if (sw) {
                        const uint32_t tk = key[i]; key[i] = key[ij]; key[ij] = tk;
                        const int64_t to = ord[i]; ord[i] = ord[ij]; ord[ij] = to;
                    }
                }
            }
            __syncthreads();
        }
    for (int e = tid; e < K; e += 256) {
        const bool ok = e < P && ord[e] != INT64_MAX;
        os[((int64_t)g * nout + c) * K + e] = ok ? keyf(key[e]) : 0.f;
        oo[((int64_t)g * nout + c) * K + e] = ok ? ord[e] : -1;
    }
}

// a score vector as lists of K (ordinal = position)
__global__ void topk_vec_lists_kernel(const float *score, int64_t n, int64_t total, float *os, int64_t *oo) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    os[e] = e < n ? score[e] : 0.f;
    oo[e] = e < n ? e : -1;
}

// |x|^2 (sq) or |x| of rows base + (idx ? idx[i] : i) * D, one wavefront per row
__global__ __launch_bounds__(KGE_BLOCK) void topk_norm_kernel(const float *base, const int64_t *idx, int64_t n, int D, int sq,
                                                              float *out) {
    const int64_t i = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n) return;
    const float *x = row_ptr(base, idx, i, D);
    float s = 0.f;
    for (int k = threadIdx.x & 63; k < D; k += 64) s = fmaf(x[k], x[k], s);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) out[i] = sq ? s : sqrtf(s);
}

// pairwise similarity of (left[i], right[i]), one wavefront per pair (tensor_models.py:59-100, pw=True)
__global__ __launch_bounds__(KGE_BLOCK) void topk_sim_pair_kernel(int sim, const float *emb, int D, const int64_t *left,
                                                                  const int64_t *right, int64_t n, float *out) {
    const int64_t i = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n) return;
    const float *x = row_ptr(emb, left, i, D), *y = row_ptr(emb, right, i, D);
    float dot = 0.f, xx = 0.f, yy = 0.f, d1 = 0.f, d2 = 0.f;
    for (int k = threadIdx.x & 63; k < D; k += 64) {
        const float u = x[k], v = y[k], d = u - v;
        dot = fmaf(u, v, dot); xx = fmaf(u, u, xx); yy = fmaf(v, v, yy); d1 += fabsf(d); d2 = fmaf(d, d, d2);
    }
    dot = wave_sum(dot); xx = wave_sum(xx); yy = wave_sum(yy); d1 = wave_sum(d1); d2 = wave_sum(d2);
    if ((threadIdx.x & 63) != 0) return;
    float s;
    switch (sim) {
    case KGE_SIM_COSINE: s = dot / (sqrtf(xx) * sqrtf(yy)); break;
    case KGE_SIM_L2: s = -sqrtf(d2); break;
    case KGE_SIM_L1: s = -d1; break;
    case KGE_SIM_DOT: s = dot; break;
    default: s = dot / (xx + yy - dot); break;
    }
    out[i] = s;
}

// out[i] = 1 when (a_i, r_i, b_i) is in the known index: keys [M] ascending (a * n_rel + r), vals ascending within a key
__global__ void triples_known_kernel(const int64_t *keys, const int64_t *vals, int64_t M, int64_t n_rel, const int64_t *a,
                                     const int64_t *r, const int64_t *b, int64_t n, uint8_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t key = a[i] * n_rel + r[i];
    int64_t lo = 0, hi = M;
    while (lo < hi) {                                    // first position with keys[p] >= key
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    int64_t end = lo, top = M;
    while (end < top) {                                  // first position with keys[p] > key
        const int64_t mid = end + ((top - end) >> 1);
        if (keys[mid] <= key) end = mid + 1; else top = mid;
    }
    out[i] = in_sorted(vals, lo, end, b[i]) ? 1 : 0;
}

namespace {

inline size_t al(size_t x) { return (x + 255) / 256 * 256; }

int topk_fan(int K) { return std::max(1, TK_MCAP / K - 1); }

// segments per row block: about one workgroup per CU, few enough that a row's S lists merge in one pass, and at least
// TK_MIN_TILES tiles per segment - the first tile of a segment fills the row lists (a full merge per row); only the
// later tiles take the one-compare-one-ballot path
#define TK_MIN_TILES 4
int64_t topk_seg_cap(int rows, int K) {
    const int rb = std::max(1, (rows + TILE_BM - 1) / TILE_BM);
    return std::max<int64_t>(1, std::min<int64_t>(topk_fan(K), (256 + rb - 1) / rb));
}
int topk_segments(int rows, int64_t N, int K) {
    const int64_t nbn = (N + TILE_BN - 1) / TILE_BN;
    const int64_t s = std::max<int64_t>(1, std::min(nbn / TK_MIN_TILES, topk_seg_cap(rows, K))), tps = (nbn + s - 1) / s;
    return (int)((nbn + tps - 1) / tps);
}

struct TkWs {
    float *A, *an, *bn, *s0, *s1;
    int64_t *o0, *o1;
    unsigned long long *part;
    size_t need;
};
TkWs carve(void *ws, int rows, int64_t N, int D, int K) {
    TkWs w{};
    char *b = (char *)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = b ? b + off : nullptr; off = al(off + bytes + kge_carve_note(off, bytes)); return p; };
    if (rows > 0) {
        const size_t ent = (size_t)rows * (size_t)topk_seg_cap(rows, K) * K;
        w.A = (float *)take((size_t)rows * D * 4);
        w.an = (float *)take((size_t)rows * 4); w.bn = (float *)take((size_t)N * 4);
        w.part = (unsigned long long *)take(ent * 8);
        w.s0 = (float *)take(ent * 4); w.o0 = (int64_t *)take(ent * 8);
        w.s1 = (float *)take(ent * 4); w.o1 = (int64_t *)take(ent * 8);
    } else {                                           // a score vector of N entries
        const size_t ent = (size_t)((N + K - 1) / K) * K;
        w.s0 = (float *)take(ent * 4); w.o0 = (int64_t *)take(ent * 8);
        w.s1 = (float *)take(ent * 4); w.o1 = (int64_t *)take(ent * 8);
    }
    w.need = off;
    return w;
}

// tree of merge passes over G groups of L lists each (+ a running result per group in the first pass).  Output: out (when
// given) or whichever of the two buffers the last pass wrote.
int merge_tree(int64_t G, int64_t L, int K, const float *is, const int64_t *io, const float *xs, const int64_t *xo, float *out_s,
               int64_t *out_o, float *ta_s, int64_t *ta_o, float *tb_s, int64_t *tb_o, const float **res_s, const int64_t **res_o,
               hipStream_t st) {
    if (L == 1 && !xs && !out_s) { *res_s = is; *res_o = io; return KGE_OK; }
    float *ts[2] = {ta_s, tb_s};
    int64_t *to[2] = {ta_o, tb_o};
    int pp = 0;
    const int fan = topk_fan(K);
    while (true) {
        const int64_t nout = (L + fan - 1) / fan;
        const bool fin = nout == 1;
        float *ds = (fin && out_s) ? out_s : ts[pp];
        int64_t *dq = (fin && out_s) ? out_o : to[pp];
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)(G * nout)), dim3(256), 0, st, is, io, (int)L, fan, K, (int)nout,
                           xs, xo, ds, dq);
        if (int rc = check_launch()) return rc;
        xs = nullptr; xo = nullptr;
        is = ds; io = dq; L = nout; pp ^= 1;
        if (fin) break;
    }
    *res_s = is; *res_o = io;
    return KGE_OK;
}

}  // namespace

int kge_fail(int code, const char *msg);
static int tk_fail(const char *msg) { return kge_fail(KGE_ERR_ARG, msg); }

static int tk_check_model(const kge::ModelRow &m, int d_e, int d_r) {
    if (kge::widths_ok(m, d_e, d_r)) return KGE_OK;
    char msg[160];
    if (m.topk_msg) snprintf(msg, sizeof(msg), m.topk_msg, d_e, d_r);
    else snprintf(msg, sizeof(msg), "kge_topk_select: dims d_e=%d d_r=%d do not fit model %d", d_e, d_r, m.id);
    return tk_fail(msg);
}

extern "C" {

size_t kge_topk_workspace_bytes(int rows, int64_t n_cand, int d, int K) {
    if (rows < 0 || n_cand < 0 || d < 0 || K < 1 || K > KGE_TOPK_MAX) return 0;
    return carve(nullptr, rows, n_cand, d, K).need;
}

static int topk_select_impl(int func, int side, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel, const int64_t *h,
                            const int64_t *r, const int64_t *t, int rows, int d_e, int d_r, float gamma, float emb_init,
                            const int64_t *cand, int64_t n_cand, const int64_t *row_base, int64_t stride, int group_rows, int K,
                            float *res_score, int64_t *res_ord, void *ws, size_t ws_bytes, const int64_t *filt_ptr,
                            const int64_t *filt_ids, void *stream) {
    char msg[256];
    if (filt_ptr && !filt_ids) return tk_fail("kge_topk_select_filtered: filt_ptr given without filt_ids");
    const bool sim = func >= KGE_SIM_COSINE && func <= KGE_SIM_EXT_JACCARD;
    const kge::ModelRow *m = sim ? nullptr : kge::model_row(func);
    if (!sim && (!m || (m->closed & kge::E_TOPK))) {
        snprintf(msg, sizeof(msg), "kge_topk_select: unknown score function %d (TransR has no inference path)", func);
        return tk_fail(msg);
    }
    if (K < 1 || K > KGE_TOPK_MAX) {
        snprintf(msg, sizeof(msg), "kge_topk_select: K = %d outside 1 .. %d", K, KGE_TOPK_MAX);
        return tk_fail(msg);
    }
    if (rows < 0 || !ent || n_ent <= 0 || d_e <= 0 || n_cand < 0 || n_cand > 0x7fffffff || stride <= 0 || group_rows <= 0 ||
        (rows && (rows % group_rows || !h || !row_base || !res_score || !res_ord || !ws)) ||
        (!sim && (!rel || n_rel <= 0 || d_r <= 0 || !r || !t)))
        return tk_fail("kge_topk_select: bad argument");
    if (rows == 0 || n_cand == 0) return KGE_OK;
    const int64_t N = n_cand;
    const int D = d_e;
    // PairRE keeps two vectors per query row: the A entry is [a block | w block] (include/kge_hip.h)
    // TransH: [a block | w^ block | c] (2 D + 1 floats per row)
    // TransD: [a block | rho block | sigma | u] (2 k + 2 = d_e + 2 floats per row) and TWO scalars per candidate, [beta | c]: the bn
    // entry of a workspace sized for 2 N candidates (nothing else of the layout depends on the candidate count)
    const bool td = func == KGE_TRANSD;
    TkWs w = carve(ws, rows, m ? m->cand_factor * N : N, m ? m->topk_row_mul * D + m->topk_row_add : D, K);
    if (w.need > ws_bytes) {
        snprintf(msg, sizeof(msg), "kge_topk_select: workspace too small (%zu < %zu)", ws_bytes, w.need);
        return kge_fail(KGE_ERR_WORKSPACE, msg);
    }
    hipStream_t st = (hipStream_t)stream;
    // ---- query rows ----------------------------------------------------------------------------------------------------------
    const float *abase = w.A;
    const int64_t *aidx = nullptr;
    int acc, epi;
    const int mf = D % 4 == 0 && D >= TILE_BK;               // (the staging's clamped float4 re-reads need D >= 32)
    if (sim) {
        abase = ent; aidx = h;
        if (func == KGE_SIM_L1) { acc = ACC_L1; epi = EPI_GMINUS; }
        else if (func == KGE_SIM_L2) { acc = mf ? ACC_MFMA : ACC_SQ; epi = mf ? EPI_L2G : EPI_GSQRT; }
        else { acc = mf ? ACC_MFMA : ACC_DOT; epi = func == KGE_SIM_COSINE ? EPI_COS : func == KGE_SIM_EXT_JACCARD ? EPI_JAC : EPI_RAW; }
        gamma = 0.f;
    } else {
        if (int rc = tk_check_model(*m, d_e, d_r)) return rc;
        if (func == KGE_RESCAL) {
            RescalMatvecArgs m{};
            m.B = rows; m.D = d_e; m.rel = rel; m.ridx = r;
            // score = h . (M t) (score_fun.py:397-402): heads are scored by A = M t, tails by A = M^T h
            if (side) { m.y1 = ent; m.y1idx = t; m.r1 = w.A; }
            else { m.z1 = ent; m.z1idx = h; m.c1 = w.A; }
            if (int rc = launch_rescal_matvec(m, st)) return rc;
        } else if (m->own_fwd) {
            // the A entry: PairRE [a block | w block]; TransH [a block | w^ block | c]; TransD [a block | rho block | sigma | u] of k =
            // d_e / 2 columns.  The bn entry: the candidates' scalars, TransD's TWO per candidate [beta | c]
            const size_t blk = (size_t)rows * (td ? D / 2 : D);
            const kge::OwnOperand o{w.A, w.A + blk, w.an, w.A + 2 * blk, w.A + 2 * blk + rows, w.bn, w.bn + N, nullptr};
            const kge::OwnCands c{ent, cand, (int)N, nullptr, 0, 0, nullptr};
            if (int rc = kge::own_prepare(func, EdgeSrc{ent, h, ent, t, rel, r}, rows, rows, d_e, side, gamma, nullptr, o, &c, st))
                return rc;
        } else {
            EdgeFwdArgs ef{};
            ef.src = EdgeSrc{ent, h, ent, t, rel, r};
            ef.B = rows; ef.d_e = d_e; ef.d_r = d_r; ef.neg_head = side; ef.model = func;
            ef.gamma = gamma; ef.rot_div = (float)((double)emb_init / M_PI);
            ef.A = w.A;
            if (int rc = launch_edge_fwd(ef, st)) return rc;
        }
        if (func == KGE_TRANSE_L1) { acc = ACC_L1; epi = EPI_GMINUS; }
        else if (func == KGE_PAIRRE) { acc = ACC_PRE; epi = EPI_GMINUS; }
        else if (func == KGE_TRANSH) { acc = mf ? ACC_TH : ACC_THV; epi = EPI_RAW; }
        else if (td) { acc = D / 2 >= 32 ? ACC_TD : ACC_TDV; epi = EPI_RAW; }
        else if (func == KGE_ROTATE) { acc = ACC_ROT; epi = EPI_GMINUS; }
        else if (func == KGE_TRANSE_L2) { acc = mf ? ACC_MFMA : ACC_SQ; epi = mf ? EPI_L2G : EPI_GSQRT; }
        else { acc = mf ? ACC_MFMA : ACC_DOT; epi = EPI_RAW; }
    }
    // ---- norms -----------------------------------------------------------------------------------------------------------------
    if (epi == EPI_L2G || epi == EPI_COS || epi == EPI_JAC) {
        const int sq = epi != EPI_COS;
        hipLaunchKernelGGL(topk_norm_kernel, dim3((unsigned)((rows + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK)), dim3(KGE_BLOCK), 0,
                           st, abase, aidx, (int64_t)rows, D, sq, w.an);
        hipLaunchKernelGGL(topk_norm_kernel, dim3((unsigned)((N + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK)), dim3(KGE_BLOCK), 0,
                           st, ent, cand, N, D, sq, w.bn);
        if (int rc = check_launch()) return rc;
    }
    // ---- score + select ----------------------------------------------------------------------------------------------------------
    TopkSelArgs a{};
    a.abase = abase; a.aidx = aidx; a.rows = rows; a.nbase = ent; a.nidx = cand; a.N = N; a.D = td ? D / 2 : D; a.epi = epi;
    a.S = topk_segments(rows, N, K); a.K = K; a.gamma = gamma; a.an = w.an; a.bn = w.bn; a.part = w.part;
    const dim3 grid((unsigned)((int64_t)((rows + TILE_BM - 1) / TILE_BM) * a.S));
    if (filt_ptr) {
        TopkSelArgsF f{};
        static_cast<TopkSelArgs &>(f) = a;
        f.filt_ptr = filt_ptr; f.filt_ids = filt_ids;
        switch (acc) {
        case ACC_MFMA: hipLaunchKernelGGL((topk_select_kernel<ACC_MFMA, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        case ACC_DOT: hipLaunchKernelGGL((topk_select_kernel<ACC_DOT, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        case ACC_SQ: hipLaunchKernelGGL((topk_select_kernel<ACC_SQ, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        case ACC_L1: hipLaunchKernelGGL((topk_select_kernel<ACC_L1, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        case ACC_PRE: hipLaunchKernelGGL((topk_select_kernel<ACC_PRE, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        case ACC_TH: hipLaunchKernelGGL((topk_select_kernel<ACC_TH, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        case ACC_THV: hipLaunchKernelGGL((topk_select_kernel<ACC_THV, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        case ACC_TD: hipLaunchKernelGGL((topk_select_kernel<ACC_TD, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        case ACC_TDV: hipLaunchKernelGGL((topk_select_kernel<ACC_TDV, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        default: hipLaunchKernelGGL((topk_select_kernel<ACC_ROT, TopkSelArgsF>), grid, dim3(256), 0, st, f); break;
        }
    } else
    switch (acc) {
    case ACC_MFMA: hipLaunchKernelGGL(topk_select_kernel<ACC_MFMA>, grid, dim3(256), 0, st, a); break;
    case ACC_DOT: hipLaunchKernelGGL(topk_select_kernel<ACC_DOT>, grid, dim3(256), 0, st, a); break;
    case ACC_SQ: hipLaunchKernelGGL(topk_select_kernel<ACC_SQ>, grid, dim3(256), 0, st, a); break;
    case ACC_L1: hipLaunchKernelGGL(topk_select_kernel<ACC_L1>, grid, dim3(256), 0, st, a); break;
    case ACC_PRE: hipLaunchKernelGGL(topk_select_kernel<ACC_PRE>, grid, dim3(256), 0, st, a); break;
    case ACC_TH: hipLaunchKernelGGL(topk_select_kernel<ACC_TH>, grid, dim3(256), 0, st, a); break;
    case ACC_THV: hipLaunchKernelGGL(topk_select_kernel<ACC_THV>, grid, dim3(256), 0, st, a); break;
    case ACC_TD: hipLaunchKernelGGL(topk_select_kernel<ACC_TD>, grid, dim3(256), 0, st, a); break;
    case ACC_TDV: hipLaunchKernelGGL(topk_select_kernel<ACC_TDV>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(topk_select_kernel<ACC_ROT>, grid, dim3(256), 0, st, a); break;
    }
    if (int rc = check_launch()) return rc;
    const int64_t ne = (int64_t)rows * a.S * K;
    hipLaunchKernelGGL(topk_unpack_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, w.part, ne, a.S * K, row_base, stride,
                       w.s0, w.o0);
    if (int rc = check_launch()) return rc;
    // ---- segments of a row -> one list per row; l2 scores in the difference form; rows of a group + running result -> result
    const float *rs; const int64_t *ro;
    if (int rc = merge_tree(rows, a.S, K, w.s0, w.o0, nullptr, nullptr, nullptr, nullptr, w.s1, w.o1, w.s0, w.o0, &rs, &ro, st)) return rc;
    if (epi == EPI_L2G) {
        const int64_t nk = (int64_t)rows * K;
        hipLaunchKernelGGL(topk_l2_fix_kernel, dim3((unsigned)((nk + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK)), dim3(KGE_BLOCK), 0, st,
                           abase, aidx, ent, cand, D, rows, K, row_base, stride, gamma, const_cast<float *>(rs), ro);
        if (int rc = check_launch()) return rc;
    }
    float *ta_s = rs == w.s0 ? w.s1 : w.s0, *tb_s = rs == w.s0 ? w.s0 : w.s1;
    int64_t *ta_o = rs == w.s0 ? w.o1 : w.o0, *tb_o = rs == w.s0 ? w.o0 : w.o1;
    const float *fs; const int64_t *fo;
    return merge_tree(rows / group_rows, group_rows, K, rs, ro, res_score, res_ord, res_score, res_ord, ta_s, ta_o, tb_s, tb_o, &fs, &fo, st);
}

int kge_topk_select(int func, int side, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel, const int64_t *h,
                    const int64_t *r, const int64_t *t, int rows, int d_e, int d_r, float gamma, float emb_init, const int64_t *cand,
                    int64_t n_cand, const int64_t *row_base, int64_t stride, int group_rows, int K, float *res_score,
                    int64_t *res_ord, void *ws, size_t ws_bytes, void *stream) {
    return topk_select_impl(func, side, ent, n_ent, rel, n_rel, h, r, t, rows, d_e, d_r, gamma, emb_init, cand, n_cand, row_base,
                            stride, group_rows, K, res_score, res_ord, ws, ws_bytes, nullptr, nullptr, stream);
}

int kge_topk_select_filtered(int func, int side, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel, const int64_t *h,
                             const int64_t *r, const int64_t *t, int rows, int d_e, int d_r, float gamma, float emb_init,
                             const int64_t *cand, int64_t n_cand, const int64_t *row_base, int64_t stride, int group_rows, int K,
                             float *res_score, int64_t *res_ord, void *ws, size_t ws_bytes, const int64_t *filt_ptr,
                             const int64_t *filt_ids, void *stream) {
    return topk_select_impl(func, side, ent, n_ent, rel, n_rel, h, r, t, rows, d_e, d_r, gamma, emb_init, cand, n_cand, row_base,
                            stride, group_rows, K, res_score, res_ord, ws, ws_bytes, filt_ptr, filt_ids, stream);
}

int kge_triples_known(const int64_t *keys, const int64_t *vals, int64_t M, int64_t n_rel, const int64_t *a, const int64_t *r,
                      const int64_t *b, int64_t n, uint8_t *out, void *stream) {
    if (M < 0 || n < 0 || n_rel <= 0 || (M && (!keys || !vals)) || (n && (!a || !r || !b || !out)))
        return tk_fail("kge_triples_known: bad argument");
    if (n == 0) return KGE_OK;
    hipLaunchKernelGGL(triples_known_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keys, vals, M, n_rel,
                       a, r, b, n, out);
    return check_launch();
}

int kge_topk_vector(const float *score, int64_t n, int K, float *res_score, int64_t *res_ord, void *ws, size_t ws_bytes, void *stream) {
    char msg[256];
    if (K < 1 || K > KGE_TOPK_MAX) {
        snprintf(msg, sizeof(msg), "kge_topk_vector: K = %d outside 1 .. %d", K, KGE_TOPK_MAX);
        return tk_fail(msg);
    }
    if (n < 0 || (n && (!score || !ws)) || !res_score || !res_ord) return tk_fail("kge_topk_vector: bad argument");
    if (n == 0) return KGE_OK;
    TkWs w = carve(ws, 0, n, 0, K);
    if (w.need > ws_bytes) {
        snprintf(msg, sizeof(msg), "kge_topk_vector: workspace too small (%zu < %zu)", ws_bytes, w.need);
        return kge_fail(KGE_ERR_WORKSPACE, msg);
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t L = (n + K - 1) / K, total = L * K;
    hipLaunchKernelGGL(topk_vec_lists_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, score, n, total, w.s0, w.o0);
    if (int rc = check_launch()) return rc;
    const float *fs; const int64_t *fo;
    return merge_tree(1, L, K, w.s0, w.o0, res_score, res_ord, res_score, res_ord, w.s1, w.o1, w.s0, w.o0, &fs, &fo, st);
}

int kge_sim_pairwise(int sim, const float *emb, int64_t n_emb, int d, const int64_t *left, const int64_t *right, int64_t n, float *out,
                     void *stream) {
    if (sim < KGE_SIM_COSINE || sim > KGE_SIM_EXT_JACCARD || !emb || n_emb <= 0 || d <= 0 || n < 0 || (n && (!left || !right || !out)))
        return tk_fail("kge_sim_pairwise: bad argument");
    if (n == 0) return KGE_OK;
    hipLaunchKernelGGL(topk_sim_pair_kernel, dim3((unsigned)((n + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK)), dim3(KGE_BLOCK), 0,
                       (hipStream_t)stream, sim, emb, d, left, right, n, out);
    return check_launch();
}

}  // extern "C"
