// kge_rank_chunk.hip - chunked-candidate ranking (kge_rank_eval_chunked): E test triples in chunks of `chunk`, every chunk ranked
// against ITS OWN candidate list, in one launch per block of chunks.  The reference's counterparts: KEModel.forward_test over the
// batches of an EvalSampler with --neg_sample_size_eval / --neg_deg_sample_eval (models/general_models.py:436-485, the chunked
// negative scores with the own entities prepended and their diagonal masked :396-432; dataloader/sampler.py:459-597) and the
// per-triple candidate lists of forward_test_wikikg (models/general_models.py:487-527).
//
// Matrix-form models (TransE_l2, DistMult, ComplEx, SimplE, RESCAL): rank_chunk_gemm_kernel, an LDS-tiled fp32-MFMA product with
// the grid over (chunk, row tile, candidate tile).  The regime is the opposite of kge_rank_gemm.hip's: chunks are 8 .. 1000 rows,
// lists 500 .. 1000 ids (+ the chunk's own entities), so the tile is 16 (chunk < 48) or 64 rows x 256 candidates - a 16-row tile
// is the smallest the 16 x 16 x 4 MFMA has, and at the default chunk of 8 a 128-row tile would spend 15/16 of the matrix pipe on
// padding.  Every wavefront owns 64 candidates of all the tile's rows (4 or 16 independent accumulators); k runs in table order in
// stages of 32 through LDS with the same MFMA sequence per (row, candidate) as rank_gemm_kernel: a score does not depend on how
// the rows are grouped into chunks, tiles or blocks.  The main loop is its own and not kge_tile_gemm.hpp's: a single LDS buffer and
// an MI x 256 tile with all wavefronts across the candidates, for chunks far smaller than that loop's 128 rows.  The epilogue forms
// the score with the same tile_score as rank_gemm_kernel, compares it with the row's positive score, looks a candidate that counts
// up in the row's filter list (entity ids, binary search) and adds the tile's counts to the ranks with integer atomics: no
// [rows, candidates] block, no mask.
// The other models and KGE_FLAG_FORCE_PAIRWISE: the training kernels' chunked negative scores into a block (kge_api.hip) over
// the id list chunk_ids_kernel lays out, then chunk_count_kernel.
#include "kge_tile_gemm.hpp"

using namespace kge;

#define RC_BN 256
#define RC_BK 32                                  // (the stage loop below is written for two 16-k halves)
#define RC_LD (RC_BK + 4)                         // dwords per staged row: 4 x odd, conflict-free fragment reads

// rows of chunk c (the last chunk may be short)
__device__ __forceinline__ int chunk_rows(const ChunkCands &cc, int64_t c) {
    const int64_t left = cc.E - c * cc.chunk;
    return (int)(left < cc.chunk ? left : cc.chunk);
}
// entity id of column j of chunk c (m = chunk_rows): the chunk's own corrupted-side entities first when cc.own, then the list;
// -1 = empty slot (an entry < 0, or one outside the table: never dereferenced)
__device__ __forceinline__ int64_t chunk_cand_id(const ChunkCands &cc, int64_t c, int m, int64_t j) {
    int64_t id;
    if (cc.own && j < m) id = cc.own[c * cc.chunk + j];
    else {
        if (cc.own) j -= m;
        id = cc.cand ? cc.cand[c * cc.stride + j] : j;
    }
    return (id >= 0 && id < cc.n_ent) ? id : -1;
}

// |b|^2 of the candidate rows, one wavefront per slot: slots [0, rows) = the own entities of the block's rows (cc.own),
// slots rows + cl * n_cand + j = entry j of chunk c0 + cl's list (one list when `shared`).  Empty slots: 0.
__global__ __launch_bounds__(KGE_BLOCK) void chunk_bsq_kernel(ChunkCands cc, int64_t c0, int rows, int64_t n_list, const float *__restrict__ ent,
                                                              int D, float *__restrict__ bsq_own, float *__restrict__ bsq_c) {
    const int64_t k = (int64_t)blockIdx.x * KGE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int64_t n_own = cc.own ? rows : 0;
    if (k >= n_own + n_list) return;
    const int lane = threadIdx.x & 63;
    int64_t id;
    float *out;
    if (k < n_own) {
        id = cc.own[c0 * cc.chunk + k];
        out = bsq_own + k;
    } else {
        const int64_t q = k - n_own, cl = q / cc.n_cand, j = q - cl * cc.n_cand;
        id = cc.cand ? cc.cand[(c0 + cl) * cc.stride + j] : j;
        out = bsq_c + q;
    }
    float s = 0.f;
    if (id >= 0 && id < cc.n_ent) {
        const float *row = ent + id * (int64_t)D;
        for (int d = 4 * lane; d < D; d += 4 * KGE_WAVE) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(row + d);
            s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        }
    }
    s = wave_sum(s);
    if (lane == 0) *out = s;
}

struct RankChunkArgs {
    ChunkCands cc;
    int64_t c0; int nch;                          // this block of chunks; its rows are (c - c0) * chunk + i in A / asq / P
    const float *A, *asq, *P;                     // pos-side vectors [rows, D], |a|^2 (TransE_l2), positive scores
    const float *ent; int D;
    int l2; float gamma, clampv;
    const float *bsq_own, *bsq_c; int shared;     // chunk_bsq_kernel's outputs (TransE_l2)
    const int64_t *filt_ptr, *filt_ids;           // by triple number, entity ids
    int32_t *ranks;                               // [E], preset to 1: the tiles add their counts
    int nrt, nct;
};

// MI: 16-row strips per tile (tile = 16 MI rows x 256 candidates)
template <int MI>
__global__ __launch_bounds__(256) void rank_chunk_gemm_kernel(RankChunkArgs a) {
    constexpr int BM = 16 * MI;
    constexpr int NA = (BM * 8 + 255) / 256;      // pos-side float4 loads per thread and stage
    __shared__ __attribute__((aligned(16))) float lds[(BM + RC_BN) * RC_LD];
    __shared__ int rcnt[BM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const ChunkCands &cc = a.cc;
    // consecutive workgroups walk the candidate tiles of one row tile, then the row tiles of one chunk
    const int64_t b = blockIdx.x;
    const int ct = (int)(b % a.nct), rt = (int)((b / a.nct) % a.nrt), cl = (int)(b / ((int64_t)a.nct * a.nrt));
    const int64_t c = a.c0 + cl;
    const int m = chunk_rows(cc, c);
    const int own_m = cc.own ? m : 0;
    const int64_t ncols = own_m + cc.n_cand;
    if (rt * BM >= m || (int64_t)ct * RC_BN >= ncols) return;          // (workgroup-uniform)
    if (tid < BM) rcnt[tid] = 0;
    const int D = a.D;
    const int nst = (D + RC_BK - 1) / RC_BK;
    const int c4t = (tid & 7) * 4;
    // ---- staging: candidate float4 f = tid + 256 i: row f >> 3, piece f & 7; pos-side likewise over BM rows ----------------------
    const float *gb[8], *ga[NA];
    int lob[8], loa[NA];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = tid + 256 * i, row = f >> 3;
        const int64_t col = min((int64_t)ct * RC_BN + row, ncols - 1);
        const int64_t id = chunk_cand_id(cc, c, m, col);
        gb[i] = a.ent + (id < 0 ? 0 : id) * (int64_t)D + c4t;          // (an empty slot stages row 0 and is never counted)
        lob[i] = (BM + row) * RC_LD + c4t;
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int f = (tid + 256 * i) % (BM * 8), row = f >> 3;      // (f & 7 == tid & 7; threads beyond the tile re-read, never store)
        ga[i] = a.A + ((int64_t)cl * cc.chunk + min(rt * BM + row, m - 1)) * D + c4t;
        loa[i] = row * RC_LD + c4t;
    }
    f32x4 g[8], h[NA];
    // (D % 4 == 0: a thread's float4 of a stage is whole or beyond the row.  Only the LAST stage can reach beyond: its loads are
    //  clamped in-bounds re-reads, stored as zeros - as in rank_gemm_kernel)
    const bool tail = (D % RC_BK) != 0 && (nst - 1) * RC_BK + c4t >= D;
    auto gload = [&](int s) {
        const int off = min(s * RC_BK, D - 4 - c4t);
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = *reinterpret_cast<const f32x4 *>(gb[i] + off);
#pragma unroll
        for (int i = 0; i < NA; ++i) h[i] = *reinterpret_cast<const f32x4 *>(ga[i] + off);
    };
    auto lstore = [&](bool last) {
        const bool z = last && tail;
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4 *>(&lds[lob[i]]) = z ? (f32x4){0.f, 0.f, 0.f, 0.f} : g[i];
#pragma unroll
        for (int i = 0; i < NA; ++i)
            if (tid + 256 * i < BM * 8) *reinterpret_cast<f32x4 *>(&lds[loa[i]]) = z ? (f32x4){0.f, 0.f, 0.f, 0.f} : h[i];
    };
    // ---- compute: wavefront w owns candidates [64 w, +64) of the tile, all BM rows -------------------------------------------------
    const int mm = lane & 15, q = lane >> 4;
    const int aoff = mm * RC_LD + 4 * q, boff = (BM + wave * 64 + mm) * RC_LD + 4 * q;
    f32x4 acc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    gload(0);
    for (int s = 0; s < nst; ++s) {
        lstore(s + 1 == nst);
        __syncthreads();
        if (s + 1 < nst) gload(s + 1);                                 // in flight under this stage's MFMAs
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x4 af[MI], bf[4];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const f32x4 *>(&lds[aoff + i * 16 * RC_LD + kb * 16]);
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const f32x4 *>(&lds[boff + j * 16 * RC_LD + kb * 16]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = MFMA16(af[i][e], bf[j][e], acc[i][j]);
        }
        __syncthreads();
    }
    // ---- epilogue: acc[i][j][r] = (row 16 i + 4 q + r, candidate 64 wave + 16 j + mm) ------------------------------------------------
    int64_t cid[4];
    int64_t colj[4];
    float bs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t col = (int64_t)ct * RC_BN + wave * 64 + 16 * j + mm;
        colj[j] = col;
        cid[j] = col < ncols ? chunk_cand_id(cc, c, m, col) : -1;
        bs[j] = 0.f;
        if (a.l2 && cid[j] >= 0)
            bs[j] = col < own_m ? a.bsq_own[(int64_t)cl * cc.chunk + col] : a.bsq_c[(a.shared ? 0 : (int64_t)cl * cc.n_cand) + col - own_m];
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lrow = rt * BM + 16 * i + 4 * q + r;              // row within the chunk
            const bool rok = lrow < m;
            const int64_t brow = (int64_t)cl * cc.chunk + min(lrow, m - 1);
            const float p = a.P[brow];
            const float as = a.l2 ? a.asq[brow] : 0.f;
            int64_t f0 = 0, f1 = 0;
            if (a.filt_ptr && rok) { f0 = a.filt_ptr[2 * (c * cc.chunk + lrow)]; f1 = a.filt_ptr[2 * (c * cc.chunk + lrow) + 1]; }
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = tile_score(acc[i][j][r], a.l2, a.gamma, as, bs[j], a.clampv);
                if (cc.own && colj[j] == lrow) x = 0.f;                 // the triple's own column: mask[:, 0::(N+1)] = 0
                bool hit = rok && cid[j] >= 0 && x >= p;
                if (hit && f1 > f0) hit = !in_sorted(a.filt_ids, f0, f1, cid[j]);
                cnt += hit ? 1 : 0;
            }
            if (cnt) atomicAdd(&rcnt[16 * i + 4 * q + r], cnt);
        }
    }
    __syncthreads();
    if (tid < BM && rt * BM + tid < m) {
        const int v = rcnt[tid];
        if (v) atomicAdd(&a.ranks[c * cc.chunk + rt * BM + tid], v);
    }
}

int launch_chunk_bsq(const ChunkCands &cc, int64_t c0, int rows, int64_t n_list, const float *ent, int D, float *bsq_own, float *bsq_c,
                     hipStream_t s) {
    const int64_t n = (cc.own ? rows : 0) + n_list;
    if (n <= 0) return KGE_OK;
    hipLaunchKernelGGL(chunk_bsq_kernel, dim3((unsigned)((n + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK)), dim3(KGE_BLOCK), 0, s, cc, c0,
                       rows, n_list, ent, D, bsq_own, bsq_c);
    return check_launch();
}

// chunks [c0, c0 + nch): ranks[e] += #{counting candidates}; A / asq / P: the block's rows (edge_fwd / rescal_matvec)
int launch_rank_chunk_gemm(int model, const ChunkCands &cc, int64_t c0, int nch, const float *A, const float *asq, const float *P,
                           const float *ent, int D, float gamma, float clampv, const float *bsq_own, const float *bsq_c, int shared,
                           const int64_t *filt_ptr, const int64_t *filt_ids, int32_t *ranks, hipStream_t s) {
    if (nch <= 0) return KGE_OK;
    RankChunkArgs a{};
    a.cc = cc; a.c0 = c0; a.nch = nch; a.A = A; a.asq = asq; a.P = P; a.ent = ent; a.D = D;
    a.l2 = model == KGE_TRANSE_L2 ? 1 : 0; a.gamma = gamma; a.clampv = clampv;
    a.bsq_own = bsq_own; a.bsq_c = bsq_c; a.shared = shared;
    a.filt_ptr = filt_ptr; a.filt_ids = filt_ids; a.ranks = ranks;
    const bool wide = cc.chunk >= 48;
    const int bm = wide ? 64 : 16;
    a.nrt = (cc.chunk + bm - 1) / bm;
    a.nct = (int)(((cc.own ? cc.chunk : 0) + cc.n_cand + RC_BN - 1) / RC_BN);
    const int64_t nb = (int64_t)nch * a.nrt * a.nct;
    if (nb > 0x7fffffff) return KGE_ERR_ARG;
    if (wide) hipLaunchKernelGGL(rank_chunk_gemm_kernel<4>, dim3((unsigned)nb), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(rank_chunk_gemm_kernel<1>, dim3((unsigned)nb), dim3(256), 0, s, a);
    return check_launch();
}

// ---- the score-block route ---------------------------------------------------------------------------------------------------------
// ids[cl * ncols + j] = entity of column j of chunk cfirst + cl, for `nch` chunks of m rows each (ncols = own + list entries);
// empty slots read row 0 (scored, never counted)
__global__ __launch_bounds__(KGE_BLOCK) void chunk_ids_kernel(ChunkCands cc, int64_t cfirst, int nch, int m, int64_t ncols,
                                                              int64_t *__restrict__ ids) {
    const int64_t k = (int64_t)blockIdx.x * KGE_BLOCK + threadIdx.x;
    if (k >= (int64_t)nch * ncols) return;
    const int64_t cl = k / ncols, j = k - cl * ncols;
    const int64_t id = chunk_cand_id(cc, cfirst + cl, m, j);
    ids[k] = id < 0 ? 0 : id;
}

// one workgroup per row of a group of `m`-row chunks: rank = 1 + #{j : S[row, j] >= p, column j not empty, its entity not in filt}
// with the row's own column (cc.own) taken as 0.0f
__global__ __launch_bounds__(KGE_BLOCK) void chunk_count_kernel(ChunkCands cc, int64_t cfirst, int m, int64_t ncols,
                                                                const float *__restrict__ S, const float *__restrict__ P,
                                                                const int64_t *__restrict__ filt_ptr, const int64_t *__restrict__ filt_ids,
                                                                int32_t *__restrict__ ranks) {
    const int64_t gi = blockIdx.x;
    const int64_t cl = gi / m;
    const int li = (int)(gi - cl * m);
    const int64_t c = cfirst + cl, e = c * cc.chunk + li;
    const float p = P[gi];
    const float *row = S + gi * ncols;
    int64_t f0 = 0, f1 = 0;
    if (filt_ptr) { f0 = filt_ptr[2 * e]; f1 = filt_ptr[2 * e + 1]; }
    int cnt = 0;
    for (int64_t j = threadIdx.x; j < ncols; j += KGE_BLOCK) {
        const int64_t id = chunk_cand_id(cc, c, m, j);
        const float x = (cc.own && j == li) ? 0.f : row[j];
        bool hit = id >= 0 && x >= p;
        if (hit && f1 > f0) hit = !in_sorted(filt_ids, f0, f1, id);
        cnt += hit ? 1 : 0;
    }
    block_count_sum(cnt, [&](int tot) { ranks[e] = 1 + tot; });
}

int launch_chunk_ids(const ChunkCands &cc, int64_t cfirst, int nch, int m, int64_t ncols, int64_t *ids, hipStream_t s) {
    const int64_t n = (int64_t)nch * ncols;
    if (n <= 0) return KGE_OK;
    hipLaunchKernelGGL(chunk_ids_kernel, dim3((unsigned)((n + KGE_BLOCK - 1) / KGE_BLOCK)), dim3(KGE_BLOCK), 0, s, cc, cfirst, nch, m, ncols, ids);
    return check_launch();
}

int launch_chunk_count(const ChunkCands &cc, int64_t cfirst, int nch, int m, int64_t ncols, const float *S, const float *P,
                       const int64_t *filt_ptr, const int64_t *filt_ids, int32_t *ranks, hipStream_t s) {
    const int64_t rows = (int64_t)nch * m;
    if (rows <= 0) return KGE_OK;
    hipLaunchKernelGGL(chunk_count_kernel, dim3((unsigned)rows), dim3(KGE_BLOCK), 0, s, cc, cfirst, m, ncols, S, P, filt_ptr, filt_ids, ranks);
    return check_launch();
}
