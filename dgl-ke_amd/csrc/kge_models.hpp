// kge_models.hpp - the model table of the host side (kge_api.hip, kge_topk.hip): one row per model id with everything the entry
// points ask about a model before they launch - its name, its width rule and the texts for breaking it, the entries that are
// closed to it and why, and the constants of its workspaces.  dglke_amd/models.py keeps the same facts for the Python side;
// the semantics of each model are described in include/kge_hip.h (enum kge_model).  Host only: no kernel reads it.
#pragma once
#include <stdint.h>
#include "../../include/kge_hip.h"

namespace kge {

// entries that refuse some model outright (ModelRow::closed: one bit each)
enum Entry { E_STEP_ASYNC = 1, E_STEP_SHARDED = 2, E_STEP_GRADS = 4, E_STEP_FUSED_SAMPLING = 8, E_RANK_EVAL_SPLIT = 16,
             E_RANK_REL_EVAL = 32, E_MODULAR = 64, E_TOPK = 128 };
// d_r as the width rule wants it next to d_e: the same, twice, half, the square (RESCAL's matrix), or any width up to 1024 (TransR)
enum RelWidth { REL_SAME, REL_DOUBLE, REL_HALF, REL_SQUARE, REL_UPTO_1024 };

// the norm constraints (KGE_FLAG_ENT_NORM_* / KGE_FLAG_REL_NORM_*, kge_constrain.hip): a row is `ent` / `rel` equal slices, each projected
// by the flag's mode; rel == 0: the relation bits are refused, for the reason rel_why; bit k of rel_unit: relation slice k is normalised
// to length 1 whatever relation mode is set (TransH's w)
struct NormSlices { int ent, rel; unsigned rel_unit; const char *rel_why; };

struct ModelRow {
    int id; const char *name;
    // the width rule: d_e a positive multiple of ent_multiple (at most ent_max where set), d_r by `rel`.  bad_dims_first: widths that
    // are not positive are "bad dims" in front of the rule.  The texts take (d_e, d_r); topk_msg null: kge_topk_select's common text
    int ent_multiple, ent_max; RelWidth rel; bool bad_dims_first;
    const char *widths_msg, *topk_msg;
    unsigned closed; const char *closed_why;      // Entry bits and the parenthesised reason (E_MODULAR, E_TOPK: texts of their own)
    bool rel_ws_sized;                            // kge_rank_rel_workspace_bytes answers for it (the ids up to TransR)
    int cand_factor;                              // candidates the rank / top-K workspaces are sized for, per candidate
    int topk_row_mul, topk_row_add;               // floats per query row of the top-K `A` entry: mul * d_e + add
    bool own_fwd;                                 // an edge forward of its own: the host sequence of kge_own_fwd.hpp
    NormSlices norm;                              // the slices KGE_FLAG_ENT_NORM_* / KGE_FLAG_REL_NORM_* project
};

inline const ModelRow *model_row(int id) {
    static const unsigned LOCAL = E_STEP_ASYNC | E_STEP_SHARDED | E_STEP_GRADS | E_RANK_EVAL_SPLIT;
    static const unsigned OWN_FWD = LOCAL | E_STEP_FUSED_SAMPLING | E_RANK_REL_EVAL;
    static const char *const PHASES = "the row holds phases";
    static const char *const OWN_REL = "its relation-side tables are updated by kernels of their own";
    static const char *const ENTITY_ONLY = "strict step on local tables, single-table entity ranking and top-K";
    static const ModelRow rows[] = {
        {KGE_TRANSE_L1, "TransE_l1", 1, 0, REL_SAME, true, "TransE/DistMult needs d_r == d_e (got %d, %d)", nullptr, 0, nullptr, true, 1, 1, 0, false, {1, 1, 0, nullptr}},
        {KGE_TRANSE_L2, "TransE_l2", 1, 0, REL_SAME, true, "TransE/DistMult needs d_r == d_e (got %d, %d)", nullptr, 0, nullptr, true, 1, 1, 0, false, {1, 1, 0, nullptr}},
        {KGE_DISTMULT, "DistMult", 1, 0, REL_SAME, true, "TransE/DistMult needs d_r == d_e (got %d, %d)", nullptr, 0, nullptr, true, 1, 1, 0, false, {1, 1, 0, nullptr}},
        {KGE_COMPLEX, "ComplEx", 2, 0, REL_SAME, true, "ComplEx needs even d_e and d_r == d_e (got %d, %d)", nullptr, 0, nullptr, true, 1, 1, 0, false, {1, 1, 0, nullptr}},
        {KGE_ROTATE, "RotatE", 2, 0, REL_HALF, true, "RotatE needs d_r == d_e/2 (got d_e=%d d_r=%d)", nullptr, 0, nullptr, true, 1, 1, 0, false, {1, 0, 0, PHASES}},
        {KGE_SIMPLE, "SimplE", 2, 0, REL_SAME, true, "SimplE needs even d_e and d_r == d_e (got %d, %d)", nullptr, 0, nullptr, true, 1, 1, 0, false, {1, 1, 0, nullptr}},
        {KGE_RESCAL, "RESCAL", 1, 1024, REL_SQUARE, false, "RESCAL needs d_r == d_e*d_e and d_e <= 1024 (got d_e=%d d_r=%d)", nullptr, 0, nullptr,
         true, 1, 1, 0, false, {1, 0, 0, OWN_REL}},
        {KGE_TRANSR, "TransR", 1, 0, REL_UPTO_1024, false, "TransR needs 0 < d_r <= 1024 (got d_e=%d d_r=%d)", nullptr, E_MODULAR | E_TOPK, nullptr,
         true, 1, 1, 0, false, {1, 0, 0, OWN_REL}},
        // ids up to KGE_TRANSR only: a QuatE call takes the DistMult layout followed by the normalised relation table (include/kge_hip.h)
        {KGE_QUATE, "QuatE", 4, 0, REL_SAME, false, "QuatE needs d_e a positive multiple of 4 and d_r == d_e (got %d, %d)", nullptr, LOCAL,
         "strict step on local tables, single-table ranking", false, 1, 1, 0, false, {1, 1, 0, nullptr}},
        // no relation ranking: the score is not a product of a query row and the relation row
        {KGE_PAIRRE, "PairRE", 1, 0, REL_DOUBLE, false, "PairRE needs d_e > 0 and d_r == 2 * d_e, r = [rH | rT] (got %d, %d)", nullptr, OWN_FWD,
         ENTITY_ONLY, false, 1, 2, 0, true, {1, 2, 0, nullptr}},          // the A entry is [a block | w block]; r = [rH | rT]
        // every path is a matrix-core product: 16-byte rows
        {KGE_TRANSH, "TransH", 4, 0, REL_DOUBLE, false, "TransH needs d_e >= 4, d_e %% 4 == 0 and d_r == 2 * d_e, r = [d | w] (got %d, %d)",
         "kge_topk_select: TransH needs d_e >= 4, d_e %% 4 == 0 and d_r == 2 * d_e (got %d, %d)", OWN_FWD, ENTITY_ONLY, false,
         1, 2, 1, true, {1, 2, 2, nullptr}},          // [a block | w^ block | c]; r = [d | w], |w| = 1
        // rows [x | x_p] of two halves, every path a matrix-core product over the first: 16-byte halves.  TWO scalars per candidate,
        // [beta | c], in the entry of the candidate norms: the workspaces are the ones of 2 N candidates
        {KGE_TRANSD, "TransD", 8, 0, REL_SAME, false, "TransD needs d_e == d_r and d_e %% 8 == 0, rows [x | x_p] of two halves (got %d, %d)",
         "kge_topk_select: TransD needs d_e == d_r and d_e %% 8 == 0, rows [x | x_p] (got %d, %d)", OWN_FWD, ENTITY_ONLY, false,
         2, 1, 2, true, {2, 2, 0, nullptr}},          // [a block | rho block | sigma | u]; [e | e_p], [r | r_p]
    };
    for (const ModelRow &m : rows)
        if (m.id == id) return &m;
    return nullptr;                                   // ids 9, 11, 13 and everything outside 0 .. 14: "unknown model"
}

inline bool widths_ok(const ModelRow &m, int d_e, int d_r) {
    if (d_e < m.ent_multiple || d_e % m.ent_multiple || (m.ent_max && d_e > m.ent_max)) return false;
    switch (m.rel) {
    case REL_SAME: return d_r == d_e;
    case REL_DOUBLE: return (int64_t)d_r == 2 * (int64_t)d_e;
    case REL_HALF: return d_r == d_e / 2;
    case REL_SQUARE: return (int64_t)d_r == (int64_t)d_e * d_e;
    default: return d_r > 0 && d_r <= 1024;
    }
}

}  // namespace kge
