// kge_tucker.hpp - TuckER (include/kge_hip.h, KGE_TUCKER): the edge side of the two all-entity steps and of ranking.
// The core W[l][k][m] (d_r x d_e x d_e; row l d_e + k of the third table is W[l][k][:]) is shared by every edge, so the three
// contractions of a step are GEMMs over the whole batch whose first operand is a Kronecker product formed in LDS (kge_tucker.hip).
#pragma once
#include "kge_common.hpp"

#define TK_MIN_K 256                 // a split of the operand kernel reduces over at least this many (l, k) pairs
#define TK_WGS 256                   // workgroups the split counts aim at: one per CU

struct TkGeom {                      // how the launches cut the batch and the core; a function of (B, d_e, d_r) alone
    int RT;                          // 128-edge row tiles
    int nj, nslab;                   // operand kernel: 16-column blocks per wavefront (<= 4), groups of 64 nj output columns
    int So, lpo;                     // ... splits of the l range (one part of A each), l values per split (no split is empty)
    int njb, nslabb;                 // backward kernel: blocks per wavefront (<= 2), groups of 64 njb columns (one part of GR each)
    int Sb, lpb;                     // ... l ranges (one part of GX each), l values per range
    int NO;                          // owner kernel: groups of 64 core rows per l, the last one ragged when d_e % 64 != 0
};
inline int tk_lper(int d_e, int d_r, int wgs_fixed) {
    const int want = TK_WGS / wgs_fixed > 1 ? TK_WGS / wgs_fixed : 1;
    const int by_wgs = (d_r + want - 1) / want, by_k = (TK_MIN_K + d_e - 1) / d_e;
    return by_wgs > by_k ? by_wgs : by_k;
}
// max_parts > 0: the operand kernel writes at most that many parts (ranking keeps them in a fixed entry of its workspace)
inline TkGeom tk_geom(int B, int d_e, int d_r, int max_parts = 0) {
    TkGeom g{};
    g.RT = (B + 127) / 128;
    g.nj = (d_e + 63) / 64 < 4 ? (d_e + 63) / 64 : 4; g.nslab = (d_e + 64 * g.nj - 1) / (64 * g.nj);
    g.lpo = tk_lper(d_e, d_r, g.RT * g.nslab);
    if (max_parts > 0 && (d_r + max_parts - 1) / max_parts > g.lpo) g.lpo = (d_r + max_parts - 1) / max_parts;
    g.So = (d_r + g.lpo - 1) / g.lpo;
    g.njb = d_e > 64 ? 2 : 1; g.nslabb = (d_e + 64 * g.njb - 1) / (64 * g.njb);
    g.lpb = tk_lper(d_e, d_r, g.RT * g.nslabb); g.Sb = (d_r + g.lpb - 1) / g.lpb;
    g.NO = (d_e + 63) / 64;
    return g;
}

struct TkArgs {
    int B, de, dr, heads;            // heads: the head is the corrupted end (x = t, y = h)
    TkGeom g;
    const float *ent, *rel;          // the entity and relation tables as they are BEFORE any update of the step
    float *core, *core_state;        // [d_r d_e, d_e], [d_r d_e]: written by the owner kernel alone
    const int64_t *xid, *yid, *rid;  // [B] the kept end, the corrupted side's true end, the relation
    float *Ap;                       // [So, B, d_e] the operand in parts
    float *A, *P;                    // [B, d_e] a_i; [B] p_i = a_i . y_i
    const float *GAp; int ga_parts;  // [ga_parts, B, d_e] dL/da in parts (the all-entity kernels)
    const float *dP;                 // [B] dL/dp
    float *U;                        // [B, d_e] u_i = GA_i + dp_i y_i
    float *GXp, *GRp;                // [Sb, B, d_e], [nslabb, B, d_r] the backward kernel's parts
    float *GX, *GY, *GR;             // [B, d_e] x 2, [B, d_r] per-edge gradient rows for the update launch
    float reg_coef; int reg_norm;    // regulariser gradient of the relation row
    float lr, eps;
};
int launch_tk_operand(const TkArgs &a, hipStream_t s);      // Ap, then A and P
int launch_tk_u(const TkArgs &a, hipStream_t s);            // U and GY
int launch_tk_bwd(const TkArgs &a, hipStream_t s);          // GXp, GRp, then GX and GR
int launch_tk_core(const TkArgs &a, hipStream_t s);         // the dense core update
