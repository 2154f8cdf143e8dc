// kge_kvsall.hip - K-vs-all binary cross-entropy with label smoothing (kge_step_fused_known on a batch with N == 0, include/kge_hip.h;
// DESIGN.md 3.19): every entity of the table is a candidate of every positive edge, s_ij = a_i . e_j, and carries label 1 when it is
// the row's own true end or in the known-triple index's list of the row's query, else 0.  Nothing couples the elements of a row, so
// there is no forward pass: the gradient of an element exists as soon as its score does, and the loss is summed where dL/da is formed.
//   kva_prep_kernel   one wavefront per row: the row's list range [f0, f1) in the index (the wave-uniform key search of
//                     known_mask_kernel), its own true end, coef_i = w_i / B, dL/dp_i = 0
//   kva_bwd_a_kernel  128 x 128 score tiles (tile_gemm_128x128); one thread per tile row sets the tile's label bits in LDS from a
//                     cursor that walks its sorted list over the split's ascending tiles; the epilogue forms
//                     G = coef (sigma(s) - y'), adds softplus(s) - y' s to a running sum per row, and G goes through LDS as the first
//                     operand of G [128 x 128] . E_tile [128 x d]: GA = dL/da in one part per split, the row sums in lpart[split][row]
//   kva_loss_kernel   the splits' sums of a row, in split order -> the row's loss term
//   kva_bwd_e_kernel  a workgroup OWNS 64 entity rows: per row tile of the batch a 128 x 64 score tile (tile_gemm_128x64, kge_allent.hpp: no
//                     dropped half), label bits for the owned range by one bisection per tile row, G^T . A_tile into its
//                     register-resident [64, d] gradient, then the Adagrad rule on its rows - no gradient buffer
// No score, label or candidate gradient is ever stored.  Every sum has a fixed order: the results are bit-reproducible.  Matrix
// products are fp32 MFMA (16 x 16 x 4).  softplus and sigma come from ONE e = exp(-|s|): max(s, 0) + log(1 + e), and 1 / (1 + e) or
// e / (1 + e) - finite for every finite s.
#include <cmath>
#include "kge_allent.hpp"      // bce_terms, the label cursor and bits, tile_gemm_128x64

namespace {
using namespace kge;

// ---- per row: list range, own end, coefficient ------------------------------------------------------------------------------------
__global__ __launch_bounds__(KGE_BLOCK) void kva_prep_kernel(KvaArgs a) {
    const int i = (int)blockIdx.x * KGE_WAVES_PER_BLOCK + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= a.B) return;
    const int64_t M = a.m;
    const int64_t key = (a.neg_head ? a.t[i] : a.h[i]) * a.n_rel + a.r[i];
    int64_t f0 = 0, f1 = M;
    while (f0 < f1) {                                    // first position with keys[p] >= key
        const int64_t mid = f0 + ((f1 - f0) >> 1);
        if (a.keys[mid] < key) f0 = mid + 1; else f1 = mid;
    }
    f1 = f0;
    if (f0 < M && a.keys[f0] == key) {                   // first position with keys[p] > key: gallop, then bisect the last stride
        int64_t lo = f0 + 1, hi = M;
        for (int64_t step = 1; f0 + step < M; step <<= 1) {
            if (a.keys[f0 + step] > key) { hi = f0 + step; break; }
            lo = f0 + step + 1;
        }
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.keys[mid] <= key) lo = mid + 1; else hi = mid;
        }
        f1 = lo;
    }
    if ((threadIdx.x & 63) == 0) {
        a.rng[2 * i] = f0; a.rng[2 * i + 1] = f1;
        a.own[i] = a.neg_head ? a.h[i] : a.t[i];
        a.coef[i] = (a.w ? a.w[i] : 1.f) / (float)a.B;
        a.dpos[i] = 0.f;
    }
}

// ---- GA = G . E without atomics, the criterion fused in: one part per split --------------------------------------------------------
// grid (row tile, split, column group), registers as ova_bwd_a_kernel: wavefront w owns the 16 NJ columns d0 + 16 NJ w .. of all 128
// rows of GA, ga[ib][j][r] = (row 16 ib + 4 q + r, column dw + 16 j + m).  Column group 0 alone sums and writes the loss.
template <int NJ>
__global__ __launch_bounds__(KGE_BLOCK) void kva_bwd_a_kernel(KvaArgs a) {
    __shared__ __attribute__((aligned(16))) TileLds lds;
    __shared__ __attribute__((aligned(16))) uint32_t lab[TILE_BM][4];           // label bits of the current tile: bit c & 31 of word c >> 5 of a tile row
    __shared__ float sc[TILE_BM];
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
        cu = cursor_at(a, range_of(a, row), (int64_t)t0 * TILE_BN);
    }
    int dcl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) dcl[j] = min(dw + 16 * j + m, a.d - 1);
    f32x4 ga[8][NJ];
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int j = 0; j < NJ; ++j) ga[ib][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float rl[4][4];                                // [i][r]: loss sum of row 64 wr + 16 i + 4 q + r over this lane's columns
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rl[i][r] = 0.f;
    float *G = &lds[0][0];                         // [128 rows][KVA_LDG]: the G tile, first operand of the second product
    auto row_a = [&](int i) { return a.A + (int64_t)min(r0 + i, a.B - 1) * a.d; };
    for (int t = t0; t < t1; ++t) {
        const int64_t c0 = (int64_t)t * TILE_BN;
        auto row_b = [&](int j) { return a.ent + min(c0 + j, a.n_ent - 1) * (int64_t)a.d; };
        if (threadIdx.x < TILE_BM) {               // (the previous tile's bits were last read ahead of two barriers)
            unsigned long long bits[2];
            label_bits<2>(a, cu, c0, bits);
            *reinterpret_cast<uint4 *>(&lab[threadIdx.x][0]) =
                make_uint4((uint32_t)bits[0], (uint32_t)(bits[0] >> 32), (uint32_t)bits[1], (uint32_t)(bits[1] >> 32));
        }
        {
            f32x4 acc[4][4];
            tile_gemm_128x128(lds, a.d, wave, row_a, row_b, acc);      // (its first barrier also publishes sc / lab)
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) ok[j] = c0 + 64 * wc + 16 * j + m < a.n_ent;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 64 * wr + 16 * i + 4 * q + r;
                    const float c = sc[row];
                    const uint2 lw = *reinterpret_cast<const uint2 *>(&lab[row][2 * wc]);
                    float ls = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int col = 64 * wc + 16 * j + m;
                        const uint32_t word = j < 2 ? lw.x : lw.y;
                        const float y = (word >> (16 * (j & 1) + m)) & 1u ? y1 : y0;
                        const float s = acc[i][j][r];
                        float spl, sg;
                        bce_terms(s, spl, sg);
                        G[row * KVA_LDG + col] = ok[j] ? c * (sg - y) : 0.f;
                        if (first) ls += ok[j] ? fmaf(-y, s, spl) : 0.f;
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
    if (!first) return;                            // (uniform over the workgroup)
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

// ---- the splits of a row in split order: the row's loss term ----------------------------------------------------------------------
__global__ __launch_bounds__(KGE_BLOCK) void kva_loss_kernel(KvaArgs a) {
    const int i = blockIdx.x * KGE_BLOCK + threadIdx.x;
    if (i >= a.B) return;
    float v = 0.f;
    for (int s = 0; s < a.g.Sa; ++s) v += a.lpart[(int64_t)s * a.B + i];
    const float l = v * a.coef[i];
    if (a.row_pos) { a.row_pos[i] = 0.f; a.row_neg[i] = l; }
    if (a.acc) atomicAdd(&a.acc[2 * KGE_ACC_SLOTS + (i & (KGE_ACC_SLOTS - 1))], l);      // (one add per slot while B <= KGE_ACC_SLOTS)
}

// ---- owner-computes dense gradient with the Adagrad update fused -----------------------------------------------------------------
// A workgroup owns the entity rows e0 .. e0 + 64.  Per row tile of the batch: label bits of the owned range (one bisection per tile
// row), the 128 x 64 score tile, G^T staged in LDS [entity][edge], then G^T . A_tile into gn[ib][j][r] = (entity 16 ib + 4 q + r,
// column 16 NJ wave + 16 j + m): wavefront w holds the columns 16 NJ w .. of all 64 rows, NJ = ceil(d / 64) <= 8.
// No other workgroup reads these rows in this launch (each reads A and its own rows), so the update at the end races with nothing.
template <int NJ>
__global__ __launch_bounds__(KGE_BLOCK) void kva_bwd_e_kernel(KvaArgs a) {
    __shared__ __attribute__((aligned(16))) Tile64Lds lds;
    __shared__ __attribute__((aligned(16))) uint32_t lab[TILE_BM][2];           // label bits of the owned rows, per edge of the current row tile
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
    ListRange lr{0, 0, -1};                        // of this thread's row of the NEXT row tile: requested a whole product ahead
    if (threadIdx.x < TILE_BM) lr = range_of(a, (int)threadIdx.x);
    for (int rt = 0; rt < a.g.RT; ++rt) {
        const int r0 = rt * TILE_BM;
        auto row_a = [&](int i) { return a.A + (int64_t)min(r0 + i, a.B - 1) * a.d; };
        if (threadIdx.x < TILE_BM) {               // (the previous row tile's bits were last read ahead of two barriers)
            ListCursor cu = cursor_at(a, lr, e0);
            unsigned long long bits[1];
            label_bits<1>(a, cu, e0, bits);
            *reinterpret_cast<uint2 *>(&lab[threadIdx.x][0]) = make_uint2((uint32_t)bits[0], (uint32_t)(bits[0] >> 32));
            lr = range_of(a, r0 + TILE_BM + (int)threadIdx.x);
        }
        {
            f32x4 acc[2][4];
            tile_gemm_128x64(lds, a.d, wave, row_a, row_b, acc);      // (its first barrier also publishes lab)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float c[4];
                uint2 lw[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tr = 32 * wave + 16 * i + 4 * q + r;
                    c[r] = r0 + tr < a.B ? a.coef[r0 + tr] : 0.f;
                    lw[r] = *reinterpret_cast<const uint2 *>(&lab[tr][0]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = e0 + 16 * j + m < a.n_ent;
                    f32x4 g;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t word = j < 2 ? lw[r].x : lw[r].y;
                        const float y = (word >> (16 * (j & 1) + m)) & 1u ? y1 : y0;
                        float spl, sg;
                        bce_terms(acc[i][j][r], spl, sg);
                        g[r] = ok ? c[r] * (sg - y) : 0.f;
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

inline bool kva_ok(const KvaArgs &a) {
    return a.B > 0 && a.n_ent > 0 && a.d >= 4 && a.d % 4 == 0 && a.d <= 512 && a.m >= 0 && (a.m == 0 || (a.keys && a.vals));
}

}  // namespace

int launch_kva_prep(const KvaArgs &a, hipStream_t s) {
    if (!kva_ok(a)) return KGE_ERR_ARG;
    const int nb = (a.B + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK;
    hipLaunchKernelGGL(kva_prep_kernel, dim3(nb), dim3(KGE_BLOCK), 0, s, a);
    return kge::check_launch();
}

int launch_kva_bwd_a(const KvaArgs &a, hipStream_t s) {
    if (!kva_ok(a)) return KGE_ERR_ARG;
    const dim3 g(a.g.RT, a.g.Sa, a.g.nslab), b(KGE_BLOCK);
    switch (a.g.nj) {
        case 1: hipLaunchKernelGGL(kva_bwd_a_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(kva_bwd_a_kernel<2>, g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL(kva_bwd_a_kernel<3>, g, b, 0, s, a); break;
        default: hipLaunchKernelGGL(kva_bwd_a_kernel<4>, g, b, 0, s, a); break;
    }
    return kge::check_launch();
}

int launch_kva_loss(const KvaArgs &a, hipStream_t s) {
    if (!kva_ok(a)) return KGE_ERR_ARG;
    hipLaunchKernelGGL(kva_loss_kernel, dim3((a.B + KGE_BLOCK - 1) / KGE_BLOCK), dim3(KGE_BLOCK), 0, s, a);
    return kge::check_launch();
}

int launch_kva_bwd_e(const KvaArgs &a, hipStream_t s) {
    if (!kva_ok(a)) return KGE_ERR_ARG;
    const dim3 g((unsigned)((a.n_ent + KVA_EB - 1) / KVA_EB)), b(KGE_BLOCK);
    switch ((a.d + 63) / 64) {
        case 1: hipLaunchKernelGGL(kva_bwd_e_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(kva_bwd_e_kernel<2>, g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL(kva_bwd_e_kernel<3>, g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL(kva_bwd_e_kernel<4>, g, b, 0, s, a); break;
        case 5: hipLaunchKernelGGL(kva_bwd_e_kernel<5>, g, b, 0, s, a); break;
        case 6: hipLaunchKernelGGL(kva_bwd_e_kernel<6>, g, b, 0, s, a); break;
        case 7: hipLaunchKernelGGL(kva_bwd_e_kernel<7>, g, b, 0, s, a); break;
        default: hipLaunchKernelGGL(kva_bwd_e_kernel<8>, g, b, 0, s, a); break;
    }
    return kge::check_launch();
}
