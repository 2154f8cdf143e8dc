// kge_loss_body.hpp - LossGenerator.get_total_loss (negative half) + its gradient on ONE register-resident score row,
// shared by the stand-alone loss kernel (kge_rowwise.hip, loss_kernel_reg) and by the forward tiles' last arriver of the
// strict step's first launch (kge_neg_gemm.hip, round 4: no loss launch).  Same instructions in both places, so the two
// launch sequences give bit-identical gradients for the same scores.
// Reference: models/pytorch/loss.py:69-98 (get_total_loss), :10-38 (criteria), :76-80 (pairwise), :87-88 (-adv softmax).
#pragma once
#include "kge_common.hpp"
#include "kge_update_body.hpp"      // LANE(), acc_add

// LEAN: the common configuration (Logsigmoid, point-wise, positive part done by edge_fwd, no score clamp, no per-step
// outputs) - everything else is compiled out of the LEAN instances
__device__ __forceinline__ void loss_args_lean(LossArgs &a) {
    a.genre = KGE_LOSS_LOGSIGMOID; a.pos_row = 0; a.skip_pos = 1; a.clampv = 0.f; a.neg_copy = nullptr;
    a.row_pos = nullptr; a.row_neg = nullptr; a.diag_chunk = 0;
}

// Column layout of a register-resident row.  PK (N % 4 == 0, rows 16-byte aligned): a lane holds PACKS of four consecutive
// columns - pack p of lane l = columns 4 (l + 64 p) .. + 3, slot u = 4 p + k - so that a row moves as one 16-byte access per
// lane and pack and N = 200 fills ONE pack of 50 lanes (strided: four slots, the last with 8 live lanes at a full slot's price).
// Otherwise slot u = column lane + 64 u.  A pack is live or dead as a whole.
typedef float f32x2 __attribute__((ext_vector_type(2)));     // two fp32 in an even-aligned VGPR pair
template <bool PK> __device__ __forceinline__ int loss_col(int lane, int u) {
    return PK ? 4 * (lane + 64 * (u >> 2)) + (u & 3) : lane + 64 * u;
}
template <bool PK> __device__ __forceinline__ bool loss_live(int lane, int u, int N) {
    return (PK ? 4 * (lane + 64 * (u >> 2)) : lane + 64 * u) < N;
}
// first column of the request that brings slot u (PK: the pack's), clamped into the row instead of predicated: no branch
// joins in front of the waits
template <bool PK> __device__ __forceinline__ int loss_ld_col(int lane, int u, int N) {
    return PK ? 4 * min(lane + 64 * (u >> 2), (N >> 2) - 1) : min(lane + 64 * u, N - 1);
}
// x[] = the row at p (columns beyond N: unspecified - the callers select on loss_live)
template <int NPER, bool PK>
__device__ __forceinline__ void loss_row_load(const float *p, int lane, int N, float (&x)[NPER]) {
    if constexpr (PK) {
        static_assert(NPER % 4 == 0, "packs of four columns");
#pragma unroll
        for (int q = 0; q < NPER / 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(p + loss_ld_col<true>(lane, 4 * q, N));
            x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int u = 0; u < NPER; ++u) x[u] = p[loss_ld_col<false>(lane, u, N)];
    }
}
template <int NPER, bool PK>
__device__ __forceinline__ void loss_row_store(float *p, int lane, int N, const float (&x)[NPER]) {
    if constexpr (PK) {
#pragma unroll
        for (int q = 0; q < NPER / 4; ++q)
            if (loss_live<true>(lane, 4 * q, N)) {
                f32x4 v; v.x = x[4 * q]; v.y = x[4 * q + 1]; v.z = x[4 * q + 2]; v.w = x[4 * q + 3];
                *reinterpret_cast<f32x4 *>(p + loss_col<true>(lane, 4 * q)) = v;
            }
    } else {
#pragma unroll
        for (int u = 0; u < NPER; ++u) if (loss_live<false>(lane, u, N)) p[loss_col<false>(lane, u)] = x[u];
    }
}

// Softmax (KGE_LOSS_SOFTMAX, include/kge_hip.h): cross-entropy of the positive p against the negatives of its own row -
//   m = max(p, max_j n_j), e_p = exp(p - m), e_j = exp(n_j - m), Z = e_p + sum_j e_j, l = m + log Z - p,
//   dL/dn_j = (w / B) e_j / Z, dL/dp = -(w / B) (sum_j e_j) / Z.
// One row of loss_row_regs (below: its arguments, the column layout and the style of the passes); a function of its own with
// its own gradient registers, so that the instances it is compiled out of (LEAN) keep their instruction streams.
template <int NPER, bool PK>
__device__ __forceinline__ void loss_row_softmax(const LossArgs &a, int64_t i, const float (&nv)[NPER], float w, float p, int lane,
                                                 int slot2, unsigned kn, float *dn, int jd) {
    using namespace kge;
    const int N = a.N;
    const float invB = a.inv_B;
    float g[NPER];
    // m = max(p, max_j n_j): one wave_max; the masked diagonal column takes part with its score 0, a known pair with
    // KGE_KNOWN_SCORE (its exponential is 0.0f).  A DEAD slot holds score 0 too (the callers put it there): where every live
    // score lies below about -88, its __expf(0 - m) is +inf.  That is harmless only because dead slots leave the maximum and the
    // sum through SELECTS and the row through the store's predicate - never through a multiply by 0 (inf * 0 = NaN).
    constexpr int GS = PK ? 4 : 1;
    float mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < NPER; q += GS) {
        float m = nv[q];
#pragma unroll
        for (int u = q + 1; u < q + GS; ++u) m = fmaxf(m, nv[u]);
        mx = fmaxf(mx, loss_live<PK>(lane, q, N) ? m : -INFINITY);
    }
    mx = fmaxf(wave_max(mx), p);
    float z = 0.f;
#pragma unroll
    for (int q = 0; q < NPER; q += GS) {
        float zq = 0.f;
#pragma unroll
        for (int u = q; u < q + GS; ++u) { g[u] = __expf(nv[u] - mx); zq += g[u]; }
        z += loss_live<PK>(lane, q, N) ? zq : 0.f;
    }
    z = wave_sum(z);                                // sum_j e_j: one wave_sum
    const float ep = __expf(p - mx), Z = ep + z;    // Z >= 1: the largest term is exp(0)
    const float gs = w * invB * __builtin_amdgcn_rcpf(Z);      // weight, 1/B and 1/Z in ONE multiplier; one v_rcp_f32 per row
#pragma unroll
    for (int u = 0; u < NPER; ++u) {
        g[u] *= gs;
        if (a.l2_scale) { const float d = a.gamma - nv[u]; g[u] = d > 1e-15f ? g[u] * __builtin_amdgcn_rcpf(d) : 0.f; }
        if (a.clampv > 0.f && fabsf(nv[u]) >= a.clampv) g[u] = 0.f;
        if (loss_col<PK>(lane, u) == jd || ((kn >> u) & 1u)) g[u] = 0.f;
    }
    loss_row_store<NPER, PK>(dn, lane, N, g);
    if (lane == 0) {
        // dL/dp from the UNMASKED sum, as -(sum_j e_j) / Z (not 1 - e_p / Z: no cancellation when the positive dominates)
        a.dpos[i] = (a.clampv > 0.f && fabsf(p) >= a.clampv) ? 0.f : -gs * z;
        // log Z once per row.  Where the positive is the row's maximum, e_p = 1 and Z = 1 + z: log1p(z) by its series
        // below 2^-12 (the rounding of 1 + z would cost the small loss of a dominating positive its digits)
        const float lz = (ep == 1.f && z < 0x1p-12f) ? z * (1.f - 0.5f * z) : __builtin_amdgcn_logf(Z) * 0.6931471805599453f;
        const float l = ((mx - p) + lz) * w * invB;
        if (a.row_pos) { a.row_pos[i] = 0.f; a.row_neg[i] = l; }
        if (a.acc) acc_add(&a.acc[2 * KGE_ACC_SLOTS + slot2], l, a.B <= KGE_ACC_SLOTS);
    }
}

// nv[u] = score of column loss_col<PK>(lane, u) of row i (0 beyond N and in the masked diagonal column); w = edge weight,
// p = positive score (read only by the pairwise, Softmax and !skip_pos variants).  Writes dL/dn over the row (a.dneg, TransE_l2:
// pre-divided by the distance), the optional score copy, the row's loss terms and the running sums.  slot2: where this row's
// share of the total goes in the running sums (the stand-alone kernel: the row's own slot; the in-launch variant: a slot the
// edge half of the same launch does not touch).  kn: bit u set = slot u is a KNOWN pair (kge_known_neg_mask; the caller has put
// KGE_KNOWN_SCORE into nv[u]): its gradient is forced to 0.0f where the masked diagonal column's is.  0 (every caller but the
// stand-alone kernel with a mask): folded away.
// The arithmetic runs unpredicated on every slot, in passes over the slots (independent chains next to each other: a
// transcendental's result is not the next instruction's operand); dead slots are taken out by selects where they would
// enter a sum and by the stores' predicate (loss_row_softmax relies on the 0 in the dead slots and on the selects, see there).
// Per-row factors (weight, 1/B, 1/Z or 1/N) are folded into ONE multiplier.
// SM: the Softmax branch is compiled in - false in the forward tiles' in-launch loss rows, whose launcher refuses the genre: those
// kernels stay what they were.
template <int NPER, bool PK, bool SM = true>
__device__ __forceinline__ void loss_row_regs(const LossArgs &a, int64_t i, float (&nv)[NPER], float w, float p, int lane,
                                              int slot2, unsigned kn = 0u) {
    using namespace kge;
    const int N = a.N;
    float *dn = a.dneg + i * (int64_t)N;
    const int jd = a.diag_chunk > 0 ? (int)(i % a.diag_chunk) : -1;
    const float invB = a.inv_B;
    const int slot = (int)(i & (KGE_ACC_SLOTS - 1));
    float g[NPER];
    if (a.neg_copy) loss_row_store<NPER, PK>(a.neg_copy + i * (int64_t)N, lane, N, nv);
    if (a.pos_row) {   // the criterion reads p with its row: Softmax, or loss.py:76-80
        if (SM && a.genre == KGE_LOSS_SOFTMAX) { loss_row_softmax<NPER, PK>(a, i, nv, w, p, lane, slot2, kn, dn, jd); return; }
        const float sc = w / ((float)a.B * (float)N);
        float lsum = 0.f, dsum = 0.f;
#pragma unroll
        for (int u = 0; u < NPER; ++u) {
            float val, dv;
            criterion_fast(a.genre, p - nv[u], 1.f, a.margin, val, dv);
            const bool live = loss_live<PK>(lane, u, N);
            lsum += live ? val * sc : 0.f;
            const float dd = dv * sc;
            dsum += live ? dd : 0.f;
            g[u] = -dd;
        }
#pragma unroll
        for (int u = 0; u < NPER; ++u) {
            if (a.l2_scale) { const float d = a.gamma - nv[u]; g[u] = d > 1e-15f ? g[u] * __builtin_amdgcn_rcpf(d) : 0.f; }
            if (a.clampv > 0.f && fabsf(nv[u]) >= a.clampv) g[u] = 0.f;
            if (loss_col<PK>(lane, u) == jd || ((kn >> u) & 1u)) g[u] = 0.f;
        }
        loss_row_store<NPER, PK>(dn, lane, N, g);
        lsum = wave_sum(lsum);
        dsum = wave_sum(dsum);
        if (lane == 0) {
            a.dpos[i] = (a.clampv > 0.f && fabsf(p) >= a.clampv) ? 0.f : dsum;
            if (a.row_pos) { a.row_pos[i] = 0.f; a.row_neg[i] = lsum; }
            if (a.acc) acc_add(&a.acc[2 * KGE_ACC_SLOTS + slot2], lsum, a.B <= KGE_ACC_SLOTS);
        }
        return;
    }
    float plw = 0.f;
    if (!a.skip_pos) {
        const float wm = mean_edge_weight(a.w, a.B, lane, a.w_mean);     // positive part: the batch's MEAN importance (kge_common.hpp)
        if (lane == 0) {
            float pl, dpl;
            criterion(a.genre, p, 1.f, a.margin, pl, dpl);
            a.dpos[i] = (a.clampv > 0.f && fabsf(p) >= a.clampv) ? 0.f : dpl * wm * 0.5f * invB;
            plw = pl * wm * invB;
            if (a.row_pos) a.row_pos[i] = plw;
        }
    }
    const float neg_label = a.genre == KGE_LOSS_BCE ? 0.f : -1.f;
    // the criterion does not wait for the softmax: its transcendentals fill the max reduction's shadow
    float nl[NPER];
#pragma unroll
    for (int u = 0; u < NPER; ++u) criterion_fast(a.genre, nv[u], neg_label, a.margin, nl[u], g[u]);
    // sums: one partial per group of slots that are live or dead together (PK: a pack; strided: a slot), ONE select each
    constexpr int GS = PK ? 4 : 1;
    // element-wise multiplies / adds on the two PAIRS of a pack, spelled as packed fp32 (v_pk_mul / v_pk_add / v_pk_fma_f32: one
    // issue slot for two columns) instead of left to the vectoriser; the same operations in the same order as the scalar form
    constexpr int PW = PK ? 2 : 1;
    float acc = 0.f, rs;         // rs: the row's multiplier of the attention weights - 1/Z (-adv) or 1/N
    if (a.adv) {   // softmax(neg * T) over the row, detached (loss.py:87-88)
        float mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < NPER; q += GS) {
            float m = nv[q] * a.adv_temp;
#pragma unroll
            for (int u = q + 1; u < q + GS; ++u) m = fmaxf(m, nv[u] * a.adv_temp);
            mx = fmaxf(mx, loss_live<PK>(lane, q, N) ? m : -INFINITY);
        }
        mx = wave_max(mx);
        float z = 0.f;
#pragma unroll
        for (int q = 0; q < NPER; q += GS) {
            float zq = 0.f, aq = 0.f;
#pragma unroll
            for (int u = q; u < q + GS; u += PW) {
                if constexpr (PW == 2) {
                    const f32x2 sv = {nv[u], nv[u + 1]};
                    const f32x2 t = sv * a.adv_temp - mx;
                    const f32x2 ex = {__expf(t.x), __expf(t.y)};
                    f32x2 gg = {g[u], g[u + 1]};
                    gg *= ex;
                    g[u] = gg.x; g[u + 1] = gg.y;
                    zq += ex.x; zq += ex.y;
                    aq = fmaf(ex.x, nl[u], aq); aq = fmaf(ex.y, nl[u + 1], aq);
                } else {
                    const float ex = __expf(nv[u] * a.adv_temp - mx);
                    zq += ex;
                    aq = fmaf(ex, nl[u], aq);
                    g[u] *= ex;
                }
            }
            const bool live = loss_live<PK>(lane, q, N);
            z += live ? zq : 0.f;
            acc += live ? aq : 0.f;
        }
        // Z and the loss sum reduced side by side (two independent DPP chains); 1/Z: ONE v_rcp_f32 per row (1 ulp)
        z = wave_sum(z);
        acc = wave_sum(acc);
        rs = __builtin_amdgcn_rcpf(z);
    } else {
#pragma unroll
        for (int q = 0; q < NPER; q += GS) {
            float aq = 0.f;
#pragma unroll
            for (int u = q; u < q + GS; ++u) aq += nl[u];
            acc += loss_live<PK>(lane, q, N) ? aq : 0.f;
        }
        acc = wave_sum(acc);
        rs = a.inv_N;
    }
    const float ws = w * rs;
    acc = acc * ws * invB;
    const float gs = ws * 0.5f * invB;
#pragma unroll
    for (int u = 0; u < NPER; u += PW) {
        if constexpr (PW == 2) {
            f32x2 gg = {g[u], g[u + 1]};
            gg *= gs;
            if (a.l2_scale) {
                const f32x2 sv = {nv[u], nv[u + 1]};
                const f32x2 d = a.gamma - sv;
                const f32x2 r = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
                gg *= r;
                gg.x = d.x > 1e-15f ? gg.x : 0.f; gg.y = d.y > 1e-15f ? gg.y : 0.f;
            }
            g[u] = gg.x; g[u + 1] = gg.y;
        } else {
            g[u] *= gs;
            if (a.l2_scale) { const float d = a.gamma - nv[u]; g[u] = d > 1e-15f ? g[u] * __builtin_amdgcn_rcpf(d) : 0.f; }
        }
    }
#pragma unroll
    for (int u = 0; u < NPER; ++u) {
        if (a.clampv > 0.f && fabsf(nv[u]) >= a.clampv) g[u] = 0.f;
        if (loss_col<PK>(lane, u) == jd || ((kn >> u) & 1u)) g[u] = 0.f;
    }
    loss_row_store<NPER, PK>(dn, lane, N, g);
    if (lane == 0) {
        if (a.row_neg) a.row_neg[i] = acc;
        if (a.acc) {
            const bool uq = a.B <= KGE_ACC_SLOTS;
            if (!a.skip_pos) acc_add(&a.acc[0 * KGE_ACC_SLOTS + slot], plw, uq);
            acc_add(&a.acc[1 * KGE_ACC_SLOTS + slot], acc, uq);
            acc_add(&a.acc[2 * KGE_ACC_SLOTS + slot2], 0.5f * (plw + acc), uq);
        }
    }
}
