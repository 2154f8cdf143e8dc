// kge_adam.hip - the Adam instances of the register-resident owner-computes update (kge_update_body.hpp, ADAM) and their
// launcher: the once-per-step update launch of kge_step_optim with KGE_OPT_ADAM.  A translation unit of its own, so that the
// kernels the Adagrad step launches (kge_rowwise.hip, kge_neg_gemm.hip) are compiled from exactly what they were compiled from
// before: nothing of this file is instantiated there.
#include "kge_common.hpp"
#include "kge_update_body.hpp"

// Same leading plain parameters as update_kernel_reg (kernel-argument preload): the record address is formed from
// preloaded registers, the record, the counts and the UpdateArgs fields leave in update_head's one scalar round.  The moment rows
// hang off the same record as the table row (id) and are requested with it - no round trip is added behind the list walk.
// One instance per NIT: un-sharded, in place, every source mode (P / GA / Q, per-edge GH / GT / GR + GN, nd_chunk) and the
// regulariser's norm at run time.
template <int NIT>
__global__ __launch_bounds__(KGE_BLOCK) void update_kernel_adam(const int32_t *ue_rec, const int32_t *ur_rec, const int32_t *counts_dev,
                                                                int UE, int UR, int nb_ent, int nbM, UpdateArgs a_in, AdamArgs o) {
    UpdateArgs a = a_in;
    a.ue_rec = ue_rec; a.ur_rec = ur_rec; a.counts_dev = counts_dev; a.UE = UE; a.UR = UR;
    const UpdateHead hd = update_head(a, nb_ent, (int)blockIdx.x, nbM);
    KGE_TL(((int)blockIdx.x < nbM - nb_ent) ? 7 : 4);
    update_reg_body<NIT, false, 0, true>(a, hd, o);
}

int launch_update_adam(const UpdateArgs &a, const AdamArgs &o, hipStream_t s) {
    const int nbE = (a.UE + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK, nbR = (a.UR + KGE_WAVES_PER_BLOCK - 1) / KGE_WAVES_PER_BLOCK;
    if (nbE + nbR == 0) return KGE_OK;
    const int dmax = a.model_d_e > a.d_r ? a.model_d_e : a.d_r;
    // the domain of the register-resident update; the entry refuses everything else with a message before the first launch
    if (a.model_d_e % 4 != 0 || a.d_r % 4 != 0 || dmax > 1024 || !o.ent_mom || (a.UR > 0 && !o.rel_mom)) return KGE_ERR_ARG;
    if (a.em.n != 0 || a.rm.n != 0 || a.emit_ent || a.emit_rel || a.gn_parts > 0 || (a.Q && !a.transe_fast)) return KGE_ERR_ARG;
    const int nbM = nbE + nbR;
    const dim3 g(nbM), b(KGE_BLOCK);
#define KGE_UPD_ADAM(N) hipLaunchKernelGGL((update_kernel_adam<N>), g, b, 0, s, a.ue_rec, a.ur_rec, a.counts_dev, a.UE, a.UR, nbE, nbM, a, o)
    if (dmax <= 256) KGE_UPD_ADAM(1); else if (dmax <= 512) KGE_UPD_ADAM(2); else KGE_UPD_ADAM(4);
#undef KGE_UPD_ADAM
    return kge::check_launch();
}
