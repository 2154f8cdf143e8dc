// kge_constrain.hpp - the unit-ball projection of the rows a strict step has just updated (KGE_FLAG_ENT_NORM_* / KGE_FLAG_REL_NORM_*,
// include/kge_hip.h): the launch behind the update launch.  A header of its own, so that nothing the other translation units are
// compiled from changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One wavefront per plan record, the update launch's convention: ue_rec / ur_rec [bound][8] int32 hold {id_lo, id_hi, ...}; UE / UR
// are the bounds the record arrays were sized for (0: the table is not constrained), counts_dev[0..1] the actual counts of a
// device-built plan (null: the bounds are the counts).  A row is `parts` equal slices; bit k of `unit`: slice k is normalised to
// length 1 (else clipped to at most 1).
struct ConstrainArgs {
    float *ent, *rel;
    const int32_t *ue_rec, *ur_rec, *counts_dev;
    int UE, UR, d_e, d_r;
    int ent_parts, rel_parts;
    unsigned ent_unit, rel_unit;
};

// the widest slice the register-resident instances hold (floats); wider slices stream through twice
#define KGE_CONSTRAIN_REG_NARROW 256
#define KGE_CONSTRAIN_REG_WIDE 1024

int launch_constrain(const ConstrainArgs &a, hipStream_t s);
