/*
 * kge_hip.h - C ABI of libkge_hip.so, the MI355X (gfx950) implementation of the DGL-KE training
 * hot path: gather -> positive score -> chunked negative score -> loss -> analytic gradients ->
 * row-sparse Adagrad.
 *
 * The reference (awslabs/dgl-ke) has no FFI boundary for this path: it is Python calling torch
 * ops.  Each entry point below replaces one reference function (cited as file:line relative to
 * python/dglke/) and is what a maintainer would bind from those call sites (see INTEGRATION.md
 * for the ctypes stubs).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (a torch tensor); fp32 data, int64 ids
 *    (the reference's dtypes), int32 for the batch-plan CSR arrays this library defines;
 *  - no allocation, no host synchronisation and no global mutable state inside; every call takes
 *    an explicit stream (hipStream_t passed as void*) and only enqueues kernels on it, so calls
 *    can be captured into a hipGraph (the one object the library creates is the kge_pipe of the
 *    --async_update pipeline: a small host-side struct, explicitly created / destroyed by the caller);
 *  - return value 0 = success, negative = kge_status; kge_last_error() returns the message of
 *    the last failure on the calling thread;
 *  - embedding rows of ComplEx / RotatE are [re | im] halves (models/pytorch/score_fun.py:298-300).
 */
#ifndef KGE_HIP_H
#define KGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KGE_ABI_VERSION 8

/* score functions (models/general_models.py:248-268 model_name strings) */
enum kge_model {
    KGE_TRANSE_L1 = 0, /* score_fun.py:40  TransEScore(dist_func='l1') */
    KGE_TRANSE_L2 = 1, /* score_fun.py:40  TransEScore(dist_func='l2') */
    KGE_DISTMULT  = 2, /* score_fun.py:222 DistMultScore */
    KGE_COMPLEX   = 3, /* score_fun.py:289 ComplExScore */
    KGE_ROTATE    = 4, /* score_fun.py:451 RotatEScore */
    KGE_TRANSR    = 7, /* score_fun.py:110 TransRScore: third table of per-relation projection matrices
                          [d_e x d_r] (kge_tables.proj); fused step and ranking only (no modular autograd ops) */
    KGE_RESCAL    = 6, /* score_fun.py:378 RESCALScore: relation row = [d_e x d_e] matrix M (d_r = d_e*d_e),
                          p = h.(M t); BOTH corruption modes use the pos-side vector M x (:428-447) */
    KGE_SIMPLE    = 5, /* score_fun.py:556 SimplEScore: rows = [x_i | x_j] halves, relation = [r | r_inv];
                          scores are clamped to [-20, 20] like the reference (:568, :622, :641) */
    KGE_QUATE     = 8, /* QuatE (Zhang et al., NeurIPS 2019; not in the reference).  Rows are four quarters [a | b | c | d] of
                          q = d_e / 4 columns each: column k of an entity row is the quaternion a_k + b_k i + c_k j + d_k k.
                          d_e % 4 == 0, d_r == d_e.  The relation row is normalised per column: n_k = sqrt(ra^2 + rb^2 + rc^2 + rd^2),
                          r^_k = r_k / n_k (sqrtf and a true division), r^_k = 0 where n_k == 0.  With h = (a, b, c, d) and
                          r^ = (p, q, u, v) the Hamilton product h (x) r^ is
                            (ap - bq - cu - dv,  aq + bp + cv - du,  au - bv + cp + dq,  av + bu - cq + dp)
                          and s(h, r, t) = sum_k <(h (x) r^)_k, t_k> (4-component dot; no gamma, no clamp: gamma is ignored).
                          Pos-side vectors: A = h (x) r^ (tails corrupted), A = t (x) conj(r^) (heads corrupted), since
                          <h (x) r, t> = <h, t (x) conj(r)>; the chunked score is A . candidate.  Adjoint: ds/dt = h (x) r^,
                          ds/dh = t (x) conj(r^), g = ds/dr^ = conj(h) (x) t, ds/dr = (g - r^ <r^, g>) / n per quaternion (0 where
                          n == 0); gradients arriving through A chain the same way.  The regulariser acts on the raw rows.
                          Relation ranking of a fixed pair: s_j = <conj(h) (x) t, r^_j>.  Strict step on local tables, ranking and
                          top-K; kge_step_sharded, kge_step_grads, kge_step_async and kge_rank_eval_split refuse it. */
    KGE_PAIRRE    = 10,/* PairRE (Chao et al., ACL 2021; not in the reference).  (Id 9 is not a model: it stays "unknown model".)
                          Entity rows d_e wide, relation rows d_r == 2 * d_e wide, r = [rH | rT].  x^ = x / |x|_2 (sqrtf and a true
                          division), x^ = 0 where |x|_2 == 0, and
                            s(h, r, t) = gamma - sum_k |h^_k rH_k - t^_k rT_k|            (no clamp).
                          Chunked form, one for both corruption sides: per edge the pair (a, w) - tails corrupted a = h^ o rH,
                          w = rT; heads corrupted a = t^ o rT, w = rH - and s_ij = gamma - sum_k |a_ik - w_ik n^_jk|, n^_j the
                          normalised candidate row (every kernel forms the difference as fmaf(-w, n^, a)).  Adjoint, with
                          sigma_ijk = sign(a_ik - w_ik n^_jk), sign(0) = 0, G = dL/ds:  Ga_ik = -sum_j G sigma,
                          Gw_ik = sum_j G sigma n^_jk, Gn^_jk = sum_i G sigma w_ik; through a normalisation
                          gx = (gx^ - x^ <x^, gx^>) / |x| (0 where |x| == 0), applied per candidate-row occurrence.  The regulariser
                          acts on the raw rows.  Layouts: the per-op entries take the RAW rows like every model's (pos_side
                          [B, d_e], rel [B, 2 d_e], neg [C * N, d_e]; g_pos_side / g_rel / g_neg likewise, through the
                          normalisations) and keep (a, w), (Ga, Gw) and the candidate norms in their workspace.  Ranking: the pair
                          lives in the A and RV entries of the kge_rank_eval workspace (kge_rank_workspace_bytes is unchanged),
                          the candidate norms |x|_2 in its bsq entry, once per call; kge_rank_eval_chunked carves one more entry
                          of norms per candidate-list position (kge_rank_chunked_workspace_bytes answers for the id);
                          kge_step_workspace_bytes and kge_score_neg_workspace_bytes answer for the id (entries w, Gw and the
                          norms behind the common ones).  kge_topk_select / _filtered keep [a block | w block] in the A entry:
                            workspace = kge_topk_workspace_bytes(rows, n_cand, 2 * d_e, K)
                          (dglke_amd._lib.topk_workspace_bytes).  Strict step on local tables (kge_step_fused, kge_step_phase and
                          their _known forms), ranking, chunked ranking and top-K; kge_step_sharded, kge_step_grads,
                          kge_step_async, kge_step_fused_sampling (with a sampler job), kge_rank_eval_split and kge_rank_rel_eval
                          refuse it before any launch. */
    KGE_TRANSH    = 12,/* TransH (Wang et al., AAAI 2014; not in the reference).  (Ids 9 and 11 are not models: "unknown model".)
                          Entity rows d_e wide, d_e >= 4 and d_e % 4 == 0 (every path is a matrix-core product); relation rows
                          d_r == 2 * d_e wide, r = [d | w]: a translation and a hyperplane normal.  w^ = w / |w|_2 (sqrtf and a true
                          division), w^ = 0 where |w|_2 == 0; x_perp = x - (w^ . x) w^ and
                            s(h, r, t) = gamma - |h_perp + d - t_perp|_2                  (the norm, no clamp).
                          Only the direction of w is trained; the paper's soft constraints are not implemented; the regulariser
                          acts on the raw rows.  Chunked form, one for both corruption sides: per edge the pair (a, w^) - tails
                          corrupted a = h_perp + d, heads corrupted a = t_perp - d - and
                            s_ij = gamma - |a_i - n_j + (w^_i . n_j) w^_i|_2,
                          evaluated in its matrix form: with p = a_i . n_j, q = w^_i . n_j, alpha_i = |a_i|^2, beta_j = |n_j|^2,
                          c_i = w^_i . a_i the squared distance is alpha_i + beta_j - 2 p + 2 c_i q - q^2 (|w^_i| is 1, or w^_i = 0
                          and then q = 0), floored at 1e-30 like TransE_l2's.  Adjoint, with E_ij = -(dL/ds_ij) / (2 dist_ij):
                          P' = -2 E, Q' = 2 E (c_i - q_ij), kappa_i = sum_j 2 E_ij q_ij,
                            Ga_i = sum_j P'_ij n_j + 2 a_i sum_j E_ij + kappa_i w^_i,   Gw^_i = sum_j Q'_ij n_j + kappa_i a_i,
                            Gn_j = sum_i (P'_ij a_i + Q'_ij w^_i) + 2 n_j sum_i E_ij,
                          then through the projections and Gw = (Gw^ - (Gw^ . w^) w^) / |w| (0 where |w| == 0).  The products
                          run on the stacked operand [A ; W^] - 2 * chunk rows per chunk, a rows first - with the matrix-core
                          kernels of the DistMult form.  Layouts: the per-op entries take the RAW rows like every model's
                          (pos_side [B, d_e], rel [B, 2 d_e], neg [C * N, d_e]) and keep the stacked operand, the product blocks
                          and the row / column terms in their workspace; kge_step_workspace_bytes,
                          kge_score_neg_workspace_bytes and kge_rank_chunked_workspace_bytes answer for the id.  Ranking: a lives
                          in the A entry of the kge_rank_eval workspace, w^ in its RV entry, alpha in asq, c in the first Eb floats
                          of the TransR rows, beta in bsq (kge_rank_workspace_bytes is unchanged).  kge_topk_select / _filtered
                          keep [a block | w^ block | c] in the A entry:
                            workspace = kge_topk_workspace_bytes(rows, n_cand, 2 * d_e + 1, K)
                          (dglke_amd._lib.topk_workspace_bytes).  Strict step on local tables (kge_step_fused, kge_step_phase,
                          their _known forms, kge_step_optim), ranking, chunked ranking and top-K; kge_step_sharded,
                          kge_step_grads, kge_step_async, kge_step_fused_sampling (with a sampler job), kge_rank_eval_split and
                          kge_rank_rel_eval refuse it before any launch; kge_rank_rel_workspace_bytes answers 0. */
    KGE_TRANSD    = 14 /* TransD (Ji et al., ACL 2015; not in the reference).  (Ids 9, 11 and 13 are not models: "unknown model".)
                          Entity rows [e | e_p] and relation rows [r | r_p] are both d_e == d_r == 2 k floats wide, k % 4 == 0
                          (d_e % 8 == 0: every path is a matrix-core product over the first halves).  The relation's projection of
                          an entity is the rank-one map x_perp = x + (x_p . x) r_p  (M_rx = r_p x_p^T + I, equal widths) and
                            s(h, r, t) = gamma - |h_perp + r - t_perp|_2                  (the norm, no clamp).
                          Nothing is normalised; the paper's norm constraints are not implemented; the regulariser acts on the
                          raw rows.  With r_p = 0, or every e_p = 0, the model is TransE_l2 on the first halves.  Chunked form,
                          one for both corruption sides: per edge the pair (a, rho), rho = r_p - tails corrupted a = h_perp + r,
                          heads corrupted a = t_perp - r - per candidate row [n | m] the scalar c = m . n, and
                            s_ij = gamma - |a_i - n_j - c_j rho_i|_2,
                          evaluated in its matrix form: with p = a_i . n_j, q = rho_i . n_j, alpha_i = |a_i|^2, beta_j = |n_j|^2,
                          sigma_i = |rho_i|^2, u_i = a_i . rho_i the squared distance is
                            alpha_i + beta_j + c_j^2 sigma_i - 2 p + 2 c_j (q - u_i),     floored at 1e-30 like TransE_l2's.
                          Adjoint, with E_ij = -(dL/ds_ij) / (2 dist_ij): P' = -2 E, Q'_ij = 2 E_ij c_j,
                            Ga_i   = sum_j P'_ij n_j + 2 a_i sum_j E_ij - 2 rho_i sum_j E_ij c_j,
                            Grho_i = sum_j Q'_ij n_j + 2 rho_i sum_j E_ij c_j^2 - 2 a_i sum_j E_ij c_j,
                            Gc_j   = sum_i E_ij (2 c_j sigma_i - 2 u_i + 2 q_ij),
                            Gn_j   = sum_i (P'_ij a_i + Q'_ij rho_i) + 2 n_j sum_i E_ij + Gc_j m_j,     Gm_j = Gc_j n_j,
                          then the adjoint of a projection: Gx = Gx_perp + (Gx_perp . r_p) x_p, Gx_p = (Gx_perp . r_p) x,
                          Gr_p += (x_p . x) Gx_perp.  The products run on the stacked operand [A ; P] - 2 * chunk rows per chunk,
                          a rows first, k columns - against the candidates' FIRST halves with the matrix-core kernels of the
                          DistMult form.  Layouts: the per-op entries take the RAW rows like every model's (pos_side, rel
                          [B, d_e], neg [C * N, d_e]) and keep the stacked operand, a dense copy of the candidates' first halves,
                          the product blocks and the row / column terms in their workspace; kge_step_workspace_bytes,
                          kge_score_neg_workspace_bytes and kge_rank_chunked_workspace_bytes answer for the id.  Ranking and top-K
                          read the candidate operand from the table rows themselves (row stride d_e, k columns: no copy) and keep
                          TWO scalars per candidate, [beta | c] - 8 N bytes where TransH keeps 4 N - in the entry that holds the
                          candidate norms, so their workspaces are those of 2 * n_cand candidates:
                            kge_rank_eval:    kge_rank_workspace_bytes(Eb, 2 * n_cand, d_e)   (a in the A entry, rho in RV, alpha in
                                              asq, sigma and u in the first Eb floats of the first two TransR rows)
                            kge_topk_select / _filtered:  kge_topk_workspace_bytes(rows, 2 * n_cand, d_e + 2, K)   (the A entry is
                                              [a block | rho block | sigma | u]; dglke_amd._lib.topk_workspace_bytes).
                          KGE_FLAG_FORCE_PAIRWISE is ignored as for TransH.  Strict step on local tables (kge_step_fused,
                          kge_step_phase, their _known forms, kge_step_optim), ranking, chunked ranking and top-K;
                          kge_step_sharded, kge_step_grads, kge_step_async, kge_step_fused_sampling (with a sampler job),
                          kge_rank_eval_split and kge_rank_rel_eval refuse it before any launch; kge_rank_rel_workspace_bytes
                          answers 0. */
};

/* loss criteria (models/pytorch/loss.py:44-59) */
enum kge_loss {
    KGE_LOSS_LOGSIGMOID = 0,
    KGE_LOSS_LOGISTIC   = 1,
    KGE_LOSS_HINGE      = 2,
    KGE_LOSS_BCE        = 3,
    /* softmax cross-entropy of the positive against the negatives of its own row (not in the reference; the "1 vs. sampled"
     * loss, InfoNCE without a temperature).  Row i with positive score p_i, row scores n_ij (j < N, as the loss kernel sees
     * them) and weight w_i = edge importance of edge i (per edge) or 1:
     *   m_i = max(p_i, max_j n_ij);  e_p = exp(p_i - m_i), e_j = exp(n_ij - m_i), Z_i = e_p + sum_j e_j
     *   l_i = m_i + log Z_i - p_i;   loss = (1/B) sum_i w_i l_i   (no factor 1/2: there are no halves to average)
     *   dL/dn_ij = (w_i / B) e_j / Z_i;   dL/dp_i = -(w_i / B) (sum_j e_j) / Z_i
     * The masked diagonal column of KGE_FLAG_NEG_DEG_SAMPLE stays in Z_i with its score 0 and gets gradient 0; a known pair
     * (kge_step_fused_known) contributes exp(KGE_KNOWN_SCORE - m) = 0 and gets gradient 0; dL/dp_i is formed from the unmasked
     * sum.  Refused with adv (the softmax is the weighting) and with pairwise; margin and adv_temp are ignored.  Reported like
     * a pairwise loss: {nan, nan, loss, regularization}.  KGE_FLAG_FUSED_LOSS / KGE_FLAG_LOSS_IN_FWD fall back silently, as
     * for pairwise: the step takes the pairwise launch sequence (edge rows, scores, stand-alone loss kernel, ...). */
    KGE_LOSS_SOFTMAX    = 4
};

enum kge_status {
    KGE_OK            = 0,
    KGE_ERR_ARG       = -1, /* bad argument (shape / model / null pointer) */
    KGE_ERR_WORKSPACE = -2, /* workspace too small */
    KGE_ERR_LAUNCH    = -3  /* HIP launch error */
};

/* flags for kge_score_neg_* / kge_step_* : force the VALU pairwise kernels instead of the MFMA
 * GEMM kernels for the models that have a GEMM form (validation aid; TransE_l1 / RotatE always
 * use the pairwise kernels).  TransH ignores the flag in every entry - its score exists in the matrix form alone, so a call made
 * with the flag to cross-check runs the same kernels as one without; its backward products beyond 2048 rows of a chunk operand
 * (2 * chunk or N) run on the pairwise kernels whatever the flag says. */
#define KGE_FLAG_FORCE_PAIRWISE 1u
/* keep the generic edge-gradient kernel: TransE - instead of rebuilding the per-edge gradients inside the
 * update kernel; DistMult - instead of writing them from the epilogue of the backward GEMM's GA tiles
 * (validation aid) */
#define KGE_FLAG_NO_TRANSE_FAST 2u
/* matrix-core path: read the negative rows from a dense per-step copy instead of gathering them
 * from the entity table through neg_ids (tuning aid) */
#define KGE_FLAG_DENSE_NEG 4u
/* matrix-core path, pointwise criteria, N <= 256: no stand-alone loss kernel - the forward tiles emit the
 * factorised loss gradient u_ij + per-(row, 16-column tile) softmax partials and the backward wavefronts
 * combine them (4 launches per TransE step instead of 5; same results within rounding).  Opt-in: on MI355X
 * the work it moves into the two GEMM kernels costs what the loss launch cost
 * (profiles/r02_fused_loss_experiment.txt). */
#define KGE_FLAG_FUSED_LOSS 8u
/* TransE_l1 / RotatE: keep the two-pass pairwise backward (GA and GN evaluated separately) instead
 * of the kernel that evaluates every (positive, negative) pair once for both products (validation aid) */
#define KGE_FLAG_TWO_PASS_PAIR 16u
/* kge_step_fused / kge_step_sharded: --neg_deg_sample of the reference (general_models.py:396-402,
 * 424-432).  The corrupted-side entities of a chunk's OWN positives are prepended to the chunk's
 * negatives: every positive is scored against N' = chunk + N rows, the chunk x chunk diagonal (the
 * positive edge itself) is masked to score 0 (it stays in the loss, its gradient vanishes) and the
 * gradients of the in-batch rows join the POSITIVE trace of their entity.  kge_batch is unchanged
 * (N and the plan describe the SAMPLED negatives); kge_step_workspace_bytes accounts for N';
 * kge_step_out.neg_score is [B, N'], g_neg [C*N', d_e] (rows c*N' + chunk.. are the sampled ones).
 * Not available for RESCAL / TransR.  kge_step_grads (ABI 6): the in-batch rows' gradients are part of the positive-trace
 * message g0 of their entity, the sampled rows' of g1 - the traces the reference pushes. */
#define KGE_FLAG_NEG_DEG_SAMPLE 32u
/* kge_step_async: defer the relation-table update by one step as well (the reference's --async_update defers the
 * entity table only, general_models.py:639-647; with this flag no update at all sits between two steps' scoring) */
#define KGE_FLAG_ASYNC_REL 64u

/* strict step, TransE_l2 / DistMult on the matrix-core path: keep edge-forward and the forward GEMM as two launches
 * (5 launches per TransE_l2 step) instead of the merged first launch of round 3 whose tiles build the pos-side
 * fragments from the table rows themselves (4 launches).  Validation / A-B aid: same results within rounding. */
#define KGE_FLAG_SPLIT_FWD 128u

/* merged first launch: the edge-forward half also writes a dense copy of the negative rows and the backward GEMM reads it
 * instead of gathering the rows from the entity table through neg_ids (tuning / A-B aid: same speed, +1.6 MB of writes) */
#define KGE_FLAG_DENSE_BWD 256u

/* merged first launch: forward tiles with direct fragment loads of x, r and b (three gathered loads per k-step) instead of the
 * pos-side tile built once per workgroup in LDS (tuning / A-B aid) */
#define KGE_FLAG_FWD_DIRECT 512u

/* strict step, TransE_l2 / DistMult / ComplEx on the merged first launch, kge_step_out.tickets given: run LossGenerator INSIDE
 * that launch (3 launches per step): the forward tiles store final scores write-through, the workgroups of a 16-row strip draw
 * an arrival ticket and the last one runs the strip's loss rows.  Opt-in: measured SLOWER on MI355X (34.6 vs 30.6 us per cfg-T
 * step, profiles/r04_loss_fold.txt - the last arrivers' four wavefronts run 16 loss rows where the loss launch runs one row per
 * wavefront, and drain + ticket + re-read cost what the launch boundary costs).  DistMult / ComplEx results are bit-identical to
 * the 4-launch step, TransE_l2 equal within the rounding of |a|^2, |b|^2 (summed by the tiles instead of by edge_fwd). */
#define KGE_FLAG_LOSS_IN_FWD 1024u

/* ---- norm constraints of radius 1 on the rows a strict step has just updated (csrc/kge_constrain.hip) ----
 * The papers of the translation family state their models under them (TransE |e| = 1; TransH |e| <= 1, |w| = 1; TransR / TransD
 * |e|, |r|, |e_p|, |r_p| <= 1).  With one of these bits set, ONE more launch follows the update launch of kge_step_fused,
 * kge_step_fused_known, kge_step_fused_sampling, kge_step_optim (both optimizers) and the UPDATE group of kge_step_phase /
 * kge_step_phase_known.  It reads the plan records the update launch read (ue_rec / ur_rec, counts_dev) and projects every unique
 * entity row of the batch's union - positive ends and negatives alike - and, with a relation bit, every unique relation row:
 *   a row is split into equal slices (one for most models; PairRE's relation row [rH | rT], TransH's [d | w], TransD's [e | e_p] and
 *   [r | r_p] into two; csrc/kge_models.hpp); per slice n = sqrtf(sum x^2) in fp32, s = 1.0f / n, x <- x * s
 *     CLIP: only when n > 1 (a NaN norm leaves the slice alone);
 *     UNIT: when n > 0 and n != 1 (a zero slice stays zero).
 *   A slice that is not scaled keeps its bits.  Only row values change: Adagrad state, Adam moments and counts are untouched.
 *   TransH with either relation bit: d by the bit's mode, w always UNIT (the score does not change: the kernels normalise w anyway).
 * No workspace bytes are added; nothing depends on the host (graphs replay as before).  KGE_ERR_ARG before any launch: both bits of
 * one table; a relation bit for RotatE (the row holds phases), RESCAL or TransR (their relation-side tables are updated by kernels
 * of their own); any of the four bits in kge_step_sharded, kge_step_grads and kge_step_async.  The radius is 1. */
/* entity rows: scale a slice onto the unit sphere only when its norm exceeds 1 */
#define KGE_FLAG_ENT_NORM_CLIP 2048u
/* entity rows: scale every non-zero slice onto the unit sphere */
#define KGE_FLAG_ENT_NORM_UNIT 4096u
/* relation rows: as KGE_FLAG_ENT_NORM_CLIP (TransH: w is normalised to length 1 all the same) */
#define KGE_FLAG_REL_NORM_CLIP 8192u
/* relation rows: as KGE_FLAG_ENT_NORM_UNIT */
#define KGE_FLAG_REL_NORM_UNIT 16384u

int         kge_abi_version(void);
const char *kge_last_error(void);

/* ---- A2: ExternalEmbedding.__call__  (models/pytorch/tensor_models.py:270-302, line 292) ----
 * out[k,:] = table[idx[k],:] */
int kge_gather_rows(const float *table, int64_t n_rows, int dim, const int64_t *idx,
                    int64_t n_idx, float *out, void *stream);

/* ---- A3: score_func.edge_func  (score_fun.py:54-59, 229-235, 297-307, 460-472) ----
 * out[i] = positive score of (h[i], r[i], t[i]); h,t: [B,d_e]  r: [B,d_r] dense rows. */
int kge_score_pos(int model, const float *h, const float *r, const float *t, int64_t B, int d_e,
                  int d_r, float gamma, float emb_init, float *out, void *stream);
/* autograd of edge_func: (gh, gr, gt) = dpos[i] * d score/d (h, r, t) */
int kge_score_pos_bwd(int model, const float *h, const float *r, const float *t,
                      const float *dpos, int64_t B, int d_e, int d_r, float gamma,
                      float emb_init, float *gh, float *gr, float *gt, void *stream);

/* ---- A4/A5: score_func.create_neg(neg_head) closures (score_fun.py:91-108, 268-286, 345-376,
 * 512-554) called from KEModel.predict_neg_score (general_models.py:405, 426) ----
 * pos_side: the uncorrupted entity rows [C*chunk, d_e] (tails if neg_head else heads);
 * rel: [C*chunk, d_r]; neg: corrupt entity rows [C*N, d_e]; out: [C, chunk, N].
 * ws: scratch of at least kge_score_neg_workspace_bytes(). */
size_t kge_score_neg_workspace_bytes(int model, int C, int chunk, int N, int d_e);
int kge_score_neg_fwd(int model, int neg_head, const float *pos_side, const float *rel,
                      const float *neg, int C, int chunk, int N, int d_e, int d_r, float gamma,
                      float emb_init, float *out, void *ws, size_t ws_bytes, unsigned flags,
                      void *stream);
/* autograd of the closure: given dneg [C,chunk,N] -> g_pos_side [C*chunk,d_e], g_rel
 * [C*chunk,d_r], g_neg [C*N,d_e]. */
int kge_score_neg_bwd(int model, int neg_head, const float *pos_side, const float *rel,
                      const float *neg, const float *neg_score, const float *dneg, int C,
                      int chunk, int N, int d_e, int d_r, float gamma, float emb_init,
                      float *g_pos_side, float *g_rel, float *g_neg, void *ws, size_t ws_bytes,
                      unsigned flags, void *stream);

/* ---- A6: LossGenerator.get_total_loss (models/pytorch/loss.py:69-98) + its gradient ----
 * pos [B], neg [B,N], w = edge importance [B] or NULL.  loss3 = {pos_loss, neg_loss, loss}
 * (pairwise and KGE_LOSS_SOFTMAX: {nan, nan, loss}); dpos [B], dneg [B,N] = d loss / d score.
 * KGE_LOSS_SOFTMAX (definition at enum kge_loss): l_i = log(exp(p_i) + sum_j exp(n_ij)) - p_i, loss = (1/B) sum_i w_i l_i with
 * the per-edge weight; KGE_ERR_ARG with adv or pairwise; margin and adv_temp are ignored.
 * ws: scratch of 2 * a(4 * B) bytes, + 256 when loss3 is asked, a(x) = x rounded up to a multiple of 256 (two [B] float rows and
 * the staged loss terms, each 256-byte aligned); KGE_ERR_WORKSPACE before any launch when it is smaller. */
int kge_loss_fwd_bwd(int loss_genre, int adv, float adv_temp, int pairwise, float margin,
                     const float *pos, const float *neg, const float *w, int64_t B, int N,
                     float *loss3, float *dpos, float *dneg, void *ws, size_t ws_bytes,
                     void *stream);

/* ---- A9: ExternalEmbedding.update for ONE trace (tensor_models.py:304-362) ----
 * state[idx[k]] += mean_d(grad[k,d]^2) for all k (duplicates accumulate, :352), then
 * table[idx[k],:] += -lr*grad[k,:]/(sqrt(state[idx[k]])+eps) using the state AFTER all adds
 * (:353-361).  Lock-free (float atomics), two kernels. */
int kge_adagrad_scatter(float *table, float *state_sum, int64_t n_rows, int dim,
                        const int64_t *idx, const float *grad, int64_t n_idx, float lr, float eps,
                        void *stream);

/* ---- small ops of the drop-in route (KEModel.forward / forward_test with per-op autograd) ----
 * kge_scatter_add_rows: out[idx[k],:] += src[k,:] - autograd of the LOCAL-id gathers pos_g.ndata['emb'][head_ids]
 *   (general_models.py:384-388, 410-414), i.e. index_add; float atomics, out is accumulated into (caller zeroes).
 * kge_pnorm_pow(_bwd): x.norm(p)**p of a [n, dim] block (tensor_models.py:54, used by the regulariser
 *   general_models.py:572-576) - deterministic two-stage sum, ws = n floats - and its gradient
 *   gx = gout[0] * p * |x|^(p-1) * sign(x).
 * kge_mask_diag: x[c,i,i] = 0 in place on [C, chunk, Np] - the --neg_deg_sample mask (general_models.py:401-402).
 * kge_rank_from_scores: ranks[i] = 1 + #{j: neg[i,j] >= pos[i] and bias[i,j] != -1} (bias NULL: no filter) -
 *   the ranking of KEModel.forward_test (general_models.py:463-478). */
int kge_scatter_add_rows(float *out, int64_t n_rows, int dim, const int64_t *idx, const float *src, int64_t n_idx,
                         void *stream);
int kge_pnorm_pow(const float *x, int64_t n, int dim, int p, float *out, void *ws, size_t ws_bytes, void *stream);
int kge_pnorm_pow_bwd(const float *x, int64_t n, int dim, int p, const float *gout, float *gx, void *stream);
int kge_mask_diag(float *x, int C, int chunk, int Np, void *stream);
int kge_rank_from_scores(const float *neg, const float *pos, const float *bias, int64_t E, int64_t N, int64_t *ranks,
                         void *stream);

/* ---- fused step: KEModel.forward + loss.backward() + KEModel.update
 * (train_pytorch.py:141-152; general_models.py:529-588) for one batch ----
 *
 * The batch is the content of the reference's (pos_g, neg_g) pair (general_models.py:376-427,
 * dataloader/sampler.py:421-457) as flat id arrays, plus a "plan": the grouping of duplicate rows
 * that lets every table row be updated by exactly one wavefront, deterministically and without
 * atomics, with the reference's trace order (entity pos-unique trace, then entity negative trace,
 * then relation trace; tensor_models.py:316). */
typedef struct kge_batch {
    int32_t B;      /* positive edges                                                       */
    int32_t C;      /* neg_g.num_chunks                                                     */
    int32_t chunk;  /* neg_g.chunk_size  (C*chunk == B)                                     */
    int32_t N;      /* neg_g.neg_sample_size                                                */
    int32_t neg_head;
    int32_t U;      /* number of unique positive entities (len(pos_g.ndata['id']))          */
    int32_t UE;     /* unique entities in (pos nodes U negative nodes)                      */
    int32_t UR;     /* unique relations                                                     */
    const int64_t *h_gid;   /* [B]   global head entity id  = nid[h_local]                   */
    const int64_t *t_gid;   /* [B]   global tail entity id                                   */
    const int64_t *rel_ids; /* [B]   pos_g.edata['id']                                       */
    const int64_t *neg_ids; /* [C*N] neg_g.ndata['id'][head_nid|tail_nid]                    */
    const float   *edge_w;  /* [B] pos_g.edata['impts'] or NULL                              */
    /* plan */
    const int64_t *ue_id;       /* [UE]   global entity id of union entry u                  */
    const int32_t *ue_pos_ptr;  /* [UE+1] CSR into ue_pos_adj (empty list: not a pos node)   */
    const int32_t *ue_pos_adj;  /* [2B]   edge*2 + side (0 = head end, 1 = tail end)         */
    const int32_t *ue_neg_ptr;  /* [UE+1] CSR into ue_neg_slot                               */
    const int32_t *ue_neg_slot; /* [C*N]  positions in neg_ids holding this entity           */
    const int64_t *ur_id;       /* [UR]   unique relation id                                 */
    const int32_t *ur_ptr;      /* [UR+1] CSR into ur_edge                                   */
    const int32_t *ur_edge;     /* [B]    edges carrying this relation                       */
    /* packed records, 32-byte aligned, one per unique row: everything the update kernel needs  */
    /* to request the row and its first gradient rows in ONE dependent round                    */
    const int32_t *ue_rec;      /* [UE][8] {id_lo, id_hi, pos_begin, pos_end, neg_begin,     */
                                /*          neg_end, ue_pos_adj[pos_begin]|-1, ue_neg_slot[neg_begin]|-1} */
    const int32_t *ur_rec;      /* [UR][8] {id_lo, id_hi, edge_begin, edge_end, ur_edge[edge_begin], 0,0,0} */
    /* batches built ON THE DEVICE (kge_sample_batches): UE / UR above are upper bounds and the  */
    /* kernels read the actual counts from this device array of FOUR int32 {UE, UR, corrupt-head */
    /* flag of the step, edges of the batch's most frequent relation}; NULL for host-built plans */
    const int32_t *counts_dev;
    /* ABI 8: mean of edge_w[0..B) in fp32, computed ONCE per batch by whoever builds it (dglke_amd/plan.py).  The reference weights */
    /* every positive edge by the batch's MEAN importance (loss.py:75,82: a [B] * [B,1] broadcast); <= 0 (or edge_w NULL): the     */
    /* kernels sum the weights themselves, every row's wavefront for itself (what ABI <= 7 always did).                             */
    float edge_w_mean;
    int32_t reserved_;
} kge_batch;

typedef struct kge_hparams {
    int32_t model;       /* enum kge_model                                                   */
    int32_t d_e, d_r;    /* entity / relation row widths in floats                           */
    int32_t loss_genre;  /* enum kge_loss; KGE_LOSS_SOFTMAX: softmax cross-entropy of the    */
                         /* positive against its row, adv and pairwise must be 0             */
    int32_t adv;         /* args.neg_adversarial_sampling                                    */
    int32_t pairwise;
    int32_t reg_norm;    /* args.regularization_norm                                         */
    uint32_t flags;
    float gamma, emb_init, lr, adv_temp, margin, reg_coef, eps /* 1e-10 */;
} kge_hparams;

typedef struct kge_tables {
    float *ent;        /* [n_ent, d_e] entity_emb.emb                                        */
    float *ent_state;  /* [n_ent]      entity_emb.state_sum                                  */
    float *rel;        /* [n_rel, d_r]                                                       */
    float *rel_state;  /* [n_rel]                                                            */
    int64_t n_ent, n_rel;
    float *proj;       /* TransR only: [n_rel, d_e*d_r] projection_emb.emb (score_fun.py:114-118), else NULL */
    float *proj_state; /* TransR only: [n_rel] projection_emb.state_sum                      */
} kge_tables;

/* optional outputs of a step (any may be NULL) */
typedef struct kge_step_out {
    float *loss4;      /* {pos_loss, neg_loss, loss (without reg), regularization} of THIS   */
                       /* step (costs one extra single-block reduction kernel)              */
    float *loss_accum; /* [4][KGE_ACC_SLOTS] running sums over steps of the same four        */
                       /* quantities, spread over slots so that no per-step reduction is     */
                       /* needed; reduce with kge_reduce_loss() when the log is wanted       */
                       /* (replaces the 3-4 .item() host syncs per step of loss.py:95-97)    */
    float *pos_score;  /* [B]                                                                */
    float *neg_score;  /* [C,chunk,N] scores (copied before they are overwritten)            */
    float *g_pos_ent;  /* [UE, d_e] trace-0 gradient per union entry (0 if not a pos node)   */
    float *g_neg;      /* [C*N, d_e]  trace-1 gradient                                       */
    float *g_rel;      /* [B, d_r]    relation-trace gradient                                */
    int32_t *tickets;  /* [KGE_TICKET_INTS] hand-off words of KGE_FLAG_LOSS_IN_FWD (ABI 6): ZERO when    */
                       /* first handed over, returned to zero by every step; one array per stream of */
                       /* steps (concurrent steps must not share it).  NULL: the flag is ignored.    */
                       /* A step that finds a word outside [0, workgroups per strip) traps           */
                       /* (hipErrorLaunchFailure at the next synchronisation).                        */
} kge_step_out;

#define KGE_ACC_SLOTS 4096
#define KGE_TICKET_INTS 4096
/* out4 = per-quantity sums of the running-sum slots (divide by the number of steps for the
 * averages the reference prints, train_pytorch.py:165-167); optionally zero the slots. */
int kge_reduce_loss(float *loss_accum, float *out4, int zero_after, void *stream);

/* ---- the workspace contract: holds for EVERY (ws, ws_bytes) pair of this header, sized by its *_workspace_bytes function ----
 *  - contents on entry are arbitrary: the library never reads a workspace byte that the same call has not written before
 *    (calls that share a workspace by design - the phases of one kge_step_phase step, the steps of one kge_step_async group up
 *    to the flush, the jobs k = 0 .. last (advance > 0) of one sampler group on their tail scratch: job k's third phase reads its
 *    header and sorted keys under the first launch of job k + 1's step - count as one call);
 *  - contents on exit are unspecified;
 *  - nothing is written outside the buffers carved from [ws, ws + need), need = what the size function returns: a caller may
 *    allocate exactly that many bytes, and each carved buffer is written within its own bounds;
 *  - ws must be 256-byte aligned;
 *  - the caller-zeroed words are no workspace and must hold zeros when first handed over: kge_step_out.tickets,
 *    kge_step_out.loss_accum, the sampler `state` and the route counters.
 * ws_bytes below the size function's value returns KGE_ERR_WORKSPACE before any launch. */
size_t kge_step_workspace_bytes(const kge_hparams *hp, int B, int C, int chunk, int N, int UE,
                                int UR);
/* forward + backward + update of one batch, enqueued on `stream`. */
int kge_step_fused(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b,
                   const kge_step_out *out, void *ws, size_t ws_bytes, void *stream);

/* ---- --async_update (models/pytorch/tensor_models.py:136-175 async_update, :364-375 create/finish_async_update;
 * models/general_models.py:639-647; train_pytorch.py:120-121, 194-195; docs/source/train.rst:217-259) ----
 * The reference hands the entity gradients of step s to a helper PROCESS and starts step s+1 while they are
 * applied: the gather of step s+1 may miss the update of step s (<= 1 step of staleness), racily.  Here the
 * staleness is exact and race-free, and the "helper" is the other half of a horizontally fused launch:
 *
 *     [ forward(s) || UPDATE(s-1) ]  ->  loss(s)  ->  [ backward(s) || PREP(s+1) ]  ->  [ forward(s+1) || UPDATE(s) ] ...
 *
 *   PREP(s)   = gather + positive scores + pos-side vectors + DENSE COPIES of every row the step reads again
 *               (negative rows; h / t / r rows for the per-edge gradient kernel and the regulariser);
 *   forward / loss / backward(s) read only PREP's copies;
 *   UPDATE(s-1) = row-sparse Adagrad with the gradients of step s-1, applied to the rows as they are then, in the
 *               SAME launch as the forward matrix-core tiles of step s (different workspace half).
 * UPDATE(s-1) is launched after PREP(s) and completes before PREP(s+1): step s+1 gathers entity rows that contain
 * every update up to s-1 and not the update of s - bit-reproducible, one stream, no events.
 * By default only the ENTITY table is deferred, like the reference (general_models.py:639-647 defers entity_emb
 * only): the relation trace of step s is applied right after backward(s) and PREP(s+1) is its own launch.
 * KGE_FLAG_ASYNC_REL defers the relation trace too; then nothing touches the tables between backward(s) and
 * PREP(s+1), and - when the caller names the next batch (b_next) - PREP(s+1) shares the backward launch of step s
 * (three launches per step on the critical path).  b_next may be NULL (PREP runs at the start of the next call).
 * The PREP that ran ahead is used by the next call only if that call passes the same batch arrays (b->h_gid), the same
 * hyper-parameters and asks for no per-step outputs; the arrays of b_next must not be rebuilt in between (a sampler slot
 * is re-sampled only after kge_step_async_flush).
 * kge_step_async_flush() applies the last pending update (call it before reading the tables and at the end of a
 * captured group of steps; the step after a flush gathers fully updated rows).  Gradients, including the
 * regulariser, are those of the rows as gathered.  Not available for RESCAL / TransR.  The workspace holds two halves (kge_step_async_workspace_bytes).  kge_pipe is host-side state only. */
typedef struct kge_pipe kge_pipe;
int kge_pipe_create(kge_pipe **pipe);
int kge_pipe_destroy(kge_pipe *pipe);
size_t kge_step_async_workspace_bytes(const kge_hparams *hp, int B, int C, int chunk, int N, int UE, int UR);
int kge_step_async(kge_pipe *pipe, const kge_hparams *hp, const kge_tables *tb, const kge_batch *b,
                   const kge_batch *b_next, const kge_step_out *out, void *ws, size_t ws_bytes, void *stream);
int kge_step_async_flush(kge_pipe *pipe, void *stream);

/* ---- the strict step in four pieces (the reference's per-phase timers, train_pytorch.py:127-177: sample / forward /
 * backward / update): calling the four phase groups in this order on one stream IS kge_step_fused - same kernels,
 * same workspace; the caller puts events between them.  TransR's forward projections sit in GATHER. */
#define KGE_PHASE_GATHER   1   /* ids -> rows, positive scores, pos-side vectors, positive-loss part */
#define KGE_PHASE_FORWARD  2   /* chunked negative scores + loss */
#define KGE_PHASE_BACKWARD 4   /* gradients w.r.t. the pos-side vectors, the negative rows and the per-edge rows */
#define KGE_PHASE_UPDATE   8   /* row-sparse Adagrad on both tables */
int kge_step_phase(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out,
                   void *ws, size_t ws_bytes, int phases, void *stream);

/* ---- range-sharded training (one process per GPU) ----
 * kge_step_grads: same as kge_step_fused but instead of updating the entity table it EMITS, per
 * union entry u, the two trace gradients and their Adagrad increments so that the owner rank can
 * apply them: g0[u,:] (trace 0), gs0[u] = mean(g0^2); g1[u,:] = sum over duplicates (trace 1),
 * gs1[u] = sum_k mean(g_k^2).  The relation table is still updated locally unless rel_emit.
 * kge_step_out.g_pos_ent may be asked for next to a DENSE emit by union entry (ld_e == 0, ent_by_id == 0, no msg_rows): it then
 * holds a copy of g0; with any other emit layout the call returns KGE_ERR_ARG. */
typedef struct kge_emit {
    float *g0;  float *gs0;  /* [UE,d_e], [UE] */
    float *g1;  float *gs1;  /* [UE,d_e], [UE] */
    float *gr;  float *gsr;  /* [UR,d_r], [UR] summed relation gradient (NULL: update locally) */
    /* row strides in floats (0 = dense: d_e / 1 / d_r / 1).  With strides the six arrays can be
     * interleaved into ONE message per row - e.g. [g0 | g1 | gs0 gs1 pad pad] with ld_e = 2*d_e+4 -
     * so that a single all-to-all pushes both traces (see kge_adagrad_apply_packed). */
    int32_t ld_e;            /* stride of g0, g1, gs0, gs1 */
    int32_t ld_r;            /* stride of gr, gsr */
    int32_t *rid;            /* optional [UR*ld_r] view: relation id written as two int32 words at */
                             /* rid[u*ld_r], rid[u*ld_r+1] (lo, hi) next to the gradient, or NULL;  */
                             /* on device-built plans rows u in [unique relations, UR) get id -1    */
    int32_t ent_by_id;       /* != 0: the entity messages of union entry u are written at row       */
                             /* ue_id[u] instead of row u (batches re-addressed to cache rows by     */
                             /* kge_route_build: the message array is then laid out like the cache) */
    int32_t reserved;
    /* ABI 8 - PACKED single-trace entity messages (the push all-to-all moves one trace per row instead of two, of which one was   */
    /* almost always empty): msg_rows != NULL -> union entry u writes ONE message [g (d_e) | gs | link | . .] (ld_e = d_e + 4) at   */
    /* row msg_rows[2u] of g0 - its positive trace if it has one, else its negative trace - and, only when the row is in BOTH      */
    /* traces (msg_rows[2u+1] = p >= 0), the negative trace as a second message at position p of the same owner bucket's extra     */
    /* region (`link` = p in the first one's header, else -1).  msg_rows comes from kge_route_build (ue_msg); g1 / gs* are unused.  */
    /* Only the register-resident update kernel writes this layout: d_e and d_r (RESCAL: d_e) multiples of 4 and at most 1024      */
    /* floats.  Any other width returns KGE_ERR_ARG before anything is launched (the two-trace layouts serve every width), and so    */
    /* does msg_rows without g0, with ld_e < d_e + 4 or with msg_cap / msg_cap_extra < 1.                                            */
    const int32_t *msg_rows;
    int32_t msg_cap, msg_cap_extra;   /* bucket geometry of the packed messages: cap + cap_extra rows per owner, extra region from cap */
} kge_emit;
int kge_step_grads(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b,
                   const kge_step_out *out, const kge_emit *emit, void *ws, size_t ws_bytes,
                   void *stream);
/* owner side: for k < n: s = state[idx[k]] + gs[k]; state = s; table[idx[k],:] += -lr*g[k,:] /
 * (sqrt(s)+eps).  idx must be unique within one call (one wavefront owns one row). A row with
 * gs[k] == 0 and an all-zero gradient is left untouched. */
int kge_adagrad_apply_rows(float *table, float *state_sum, int64_t n_rows, int dim,
                           const int64_t *idx, const float *g, const float *gs, int64_t n,
                           float lr, float eps, void *stream);

/* ---- ranking evaluation: KEModel.forward_test (models/general_models.py:436-485) over the
 * batches an EvalSampler would produce (dataloader/sampler.py:514-597; test loop
 * train_pytorch.py:199-253), for E test triples at once ----
 * For triple i the corrupted side (head if neg_head else tail) is replaced by every candidate
 * (cand == NULL: all n_ent entities, column j = entity j; else the n_cand ids in cand) and
 *   ranks[i] = 1 + #{j : score(i,j) >= score(i)} - #{j in filt_i : score(i,j) >= score(i)}
 * filt_i = filt_ids[filt_ptr[2i] .. filt_ptr[2i+1]) are candidate COLUMNS whose corrupted triple
 * exists in the graph (the reference's bias == -1 mask, :463-475; unique within a list; filt_ptr
 * is [E][2] begin/end so that triples with the same (h,r) or (r,t) share one list; NULL =
 * --no_eval_filter, where the true triple's own column is a candidate like any other: it counts as in the
 * reference on every table whose scores are exact in fp32, otherwise its tile-form score and the directly formed
 * positive score may differ in the last bit and rounding decides).
 * Ties: a candidate that scores EXACTLY the positive score counts, as in the reference (`>=`, pessimistic: a
 * collapsed model ranks last, not first); -0.0 and +0.0 compare equal; SimplE compares after the clamp, so
 * candidates saturated at the positive score's +-20 tie with it (tests/test_gpu_rank_ties.py pins all three on
 * every ranking entry point below).  One pass per
 * Eb triples.  Matrix-form models (TransE_l2, DistMult, ComplEx, SimplE, RESCAL): a tiled fp32-MFMA
 * GEMM whose epilogue keeps the comparison bit of every (triple, candidate) pair, ranks from the
 * bit mask (csrc/kge_rank_gemm.hip); KGE_FLAG_FORCE_PAIRWISE, the pairwise models and TransR: the
 * training kernels' chunked negative scores as a block + a counting kernel.
 * pos_score_out (optional) receives the E true-triple scores. */
size_t kge_rank_workspace_bytes(int Eb, int64_t n_cand, int d_e);
int kge_rank_eval(int model, int neg_head, const float *ent, int64_t n_ent, const float *rel,
                  int64_t n_rel, const int64_t *h, const int64_t *r, const int64_t *t, int64_t E,
                  int d_e, int d_r, float gamma, float emb_init, const int64_t *cand, int64_t n_cand,
                  const int64_t *filt_ptr, const int64_t *filt_ids, int Eb, int32_t *ranks,
                  float *pos_score_out, void *ws, size_t ws_bytes, unsigned flags, void *stream);

/* same with the TransR projection table (proj = NULL for every other model); for TransR `cand` must be given
 * (pass the identity list for "all entities") */
int kge_rank_eval_ex(int model, int neg_head, const float *ent, int64_t n_ent, const float *rel,
                     int64_t n_rel, const float *proj, const int64_t *h, const int64_t *r, const int64_t *t,
                     int64_t E, int d_e, int d_r, float gamma, float emb_init, const int64_t *cand,
                     int64_t n_cand, const int64_t *filt_ptr, const int64_t *filt_ids, int Eb, int32_t *ranks,
                     float *pos_score_out, void *ws, size_t ws_bytes, unsigned flags, void *stream);

/* the same ranking with the candidates in a table other than the query rows: the evaluation of a range-sharded entity table
 * without assembling it.  The reference splits the TEST TRIPLES over its processes, each scoring against one table in shared
 * host memory (train.py:230-257, 330-350; train_pytorch.py:199-253); here every rank scores ALL test triples against the
 * candidates it OWNS and the counts are summed over the ranks: rank = 1 + sum_k (ranks_k - 1).
 *   h / t index the query table qent [n_qent, d_e] (a compact block of the test triples' rows), r indexes rel / proj;
 *   candidate j is cent[cand[j]] (cent = the rank's shard, [n_cent, d_e]), or cent[j] for j < n_cent when cand == NULL;
 *   filter lists hold columns of that candidate set, as in kge_rank_eval.  TransR needs proj and an explicit `cand`.
 * Output as kge_rank_eval: ranks[i] = 1 + #{unfiltered candidates scoring >= the true triple}.  Every candidate's score is
 * formed exactly as kge_rank_eval_ex forms it over the whole table, so the shards' counts add up to its ranks.  An empty
 * candidate set (n_cent == 0 or n_cand == 0: a rank that owns no rows) sets every rank to 1 without a kernel launch and
 * leaves pos_score_out unwritten.  Workspace: kge_rank_workspace_bytes(Eb, candidate count, d_e). */
int kge_rank_eval_split(int model, int neg_head, const float *qent, int64_t n_qent, const float *cent, int64_t n_cent,
                        const float *rel, int64_t n_rel, const float *proj, const int64_t *h, const int64_t *r,
                        const int64_t *t, int64_t E, int d_e, int d_r, float gamma, float emb_init, const int64_t *cand,
                        int64_t n_cand, const int64_t *filt_ptr, const int64_t *filt_ids, int Eb, int32_t *ranks,
                        float *pos_score_out, void *ws, size_t ws_bytes, unsigned flags, void *stream);

/* ---- chunked-candidate ranking (csrc/kge_rank_chunk.hip): KEModel.forward_test over the batches of an EvalSampler with
 * --neg_sample_size_eval / --neg_deg_sample_eval (models/general_models.py:396-432, 436-485; dataloader/sampler.py:459-597) and
 * the per-triple candidate lists of forward_test_wikikg (models/general_models.py:487-527), for E test triples in one call ----
 * Chunk c holds the triples [c * chunk, min(E, (c + 1) * chunk)) (the last chunk may be short) and is ranked against ITS OWN
 * candidates cand[c * cand_stride .. + n_cand): cand_stride == 0 = one list shared by all chunks, cand == NULL = all n_ent
 * entities (n_cand ignored).  An entry < 0 is an empty slot and never counts (ragged lists); repeats are separate candidates.
 * An entry >= n_ent is the caller's error: the library never reads through it (it is left out like an empty slot) and does
 * not report it - no call here synchronises; dglke_amd.eval checks its lists before the call and raises.
 *   ranks[i] = 1 + #{candidate j of i's chunk : score(i, j) >= score(i), cand_j not in filt_i}
 * filt_i = filt_ids[filt_ptr[2i] .. filt_ptr[2i+1]) holds ENTITY ids, ascending and unique within a list, rows may share lists -
 * the layout of kge_topk_select_filtered, what eval.build_filter_device returns; filt_ptr == NULL: raw ranking.
 * self_cand != 0 (--neg_deg_sample_eval): the corrupted-side entities (heads when neg_head, else tails) of a chunk's own m
 * triples are prepended, m + n_cand candidates; column i' of triple i' takes the score exactly 0.0f, as the reference's zero
 * mask leaves it (general_models.py:396-402, 417-432: mask[:, 0::(N+1)] = 0), so it counts iff 0 >= score(i').  Together with a
 * filter: KGE_ERR_ARG (the reference asserts that the two exclude each other).
 * Matrix-form models: an fp32-MFMA tile kernel over (chunk, row tile, candidate tile) whose epilogue compares, filters and
 * counts - no score block.  TransE_l1, RotatE, TransR and KGE_FLAG_FORCE_PAIRWISE: the training kernels' chunked negative scores
 * into a block of the workspace + a counting kernel.  TransR needs proj.  E == 0: KGE_OK without a launch.
 * Workspace: any size from kge_rank_chunked_workspace_bytes(model, chunk, chunk, ...) (one chunk) up; the entry walks E in blocks
 * of as many whole chunks as fit.  n_cand of the size function = the candidates per list (n_ent for cand == NULL). */
size_t kge_rank_chunked_workspace_bytes(int model, int rows, int chunk, int64_t n_cand, int self_cand, int d_e, int d_r);
int kge_rank_eval_chunked(int model, int neg_head, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel,
                          const float *proj, const int64_t *h, const int64_t *r, const int64_t *t, int64_t E,
                          int d_e, int d_r, float gamma, float emb_init, int chunk,
                          const int64_t *cand, int64_t n_cand, int64_t cand_stride, int self_cand,
                          const int64_t *filt_ptr, const int64_t *filt_ids, int32_t *ranks, float *pos_score_out,
                          void *ws, size_t ws_bytes, unsigned flags, void *stream);

/* ---- relation ranking (csrc/kge_rank_rel.hip): every test triple (h, r, t) against ALL n_rel relations ----
 * The reference has no counterpart - its evaluation corrupts entities only - so no reference line can be cited; the protocol is
 * fixed here.  For test triple i = (h, r, t)
 *   ranks[i] = 1 + #{j in [0, n_rel) : j not in list_i, s(h, j, t) >= s(h, r, t)}
 * list_i = filt_ids[filt_ptr[2i] .. filt_ptr[2i+1]) holds RELATION ids (column j = relation j), ascending and unique; rows may
 * share a list.  It is REQUIRED and always holds the triple's own relation r: the own column never counts, raw or filtered - its
 * score and the positive score are formed in two different ways, so their >= would be decided by rounding.  Raw ranking:
 * list_i = {r}; filtered ranking: {r} united with every j for which (h, j, t) is a known triple (dglke_amd.eval.build_relation_filter
 * builds both).  s is the score kge_rank_eval ranks with (SimplE clamped at +-20, RotatE's phase = row / (emb_init / pi));
 * pos_score_out (optional) receives the E true-triple scores.
 * For a fixed (h, t) the score is a function of the relation row c_j alone: TransE q = t - h, gamma - |q - c_j|; DistMult /
 * ComplEx / SimplE / RESCAL q . c_j with q = h o t, [h_re t_re + h_im t_im | h_re t_im - h_im t_re], 1/2 [h_i o t_j | h_j o t_i],
 * vec(h t^T) - the forms of kge_rank_eval's kernels with the relation table as the candidate table (TransE_l2 and the dot forms:
 * the fp32-MFMA tile kernel + bit mask; TransE_l1, widths that are no multiple of 4 and KGE_FLAG_FORCE_PAIRWISE: the pairwise
 * score block + counting kernel); RotatE: gamma - sum_k |h_k e^{i theta_jk} - t_k| by a kernel that keeps a relation tile's
 * cos / sin in LDS; TransR: gamma - |(h - t) P_j + c_j|_1 by the training forward with the relations as its positives (needs
 * proj).  RESCAL and TransR cost d_e * d_r multiply-adds per (triple, relation) - inherent to the models - and RESCAL's query
 * rows are d_e^2 wide: size Eb from the workspace you can afford.
 * One pass per Eb triples (Eb > E is taken as E); the ranks do not depend on Eb.  Workspace: kge_rank_rel_workspace_bytes(model, Eb,
 * n_rel, d_e, d_r) (0: bad arguments).  Errors before any launch: KGE_ERR_ARG for a null pointer, a bad model / width combination,
 * TransR without proj, n_rel > 0x7fffffff, Eb <= 0, a missing filter pointer; KGE_ERR_WORKSPACE for a workspace that is too small.
 * E == 0: KGE_OK without a launch.
 * KGE_QUATE: q = conj(h) (x) t and s_j = q . c^_j, c^_j the relation row normalised per quaternion; the call first writes the
 * normalised table [n_rel, d_r] into its workspace and the dot-form kernels read that.  kge_rank_rel_workspace_bytes answers for
 * the ids up to KGE_TRANSR only (0 for every other id, KGE_QUATE included); the workspace of a KGE_QUATE call is the
 * KGE_DISTMULT layout followed by that table:
 *   kge_rank_rel_workspace_bytes(KGE_DISTMULT, Eb, n_rel, d_e, d_r) + n_rel * d_r * sizeof(float) rounded up to 256 bytes
 * (dglke_amd._lib.rank_rel_workspace_bytes). */
size_t kge_rank_rel_workspace_bytes(int model, int Eb, int64_t n_rel, int d_e, int d_r);
int kge_rank_rel_eval(int model, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel, const float *proj,
                      const int64_t *h, const int64_t *r, const int64_t *t, int64_t E, int d_e, int d_r,
                      float gamma, float emb_init, const int64_t *filt_ptr, const int64_t *filt_ids, int Eb,
                      int32_t *ranks, float *pos_score_out, void *ws, size_t ws_bytes, unsigned flags, void *stream);

/* ---- peer-to-peer sharded step (xGMI direct; the Hogwild multi-GPU mode) ----
 * The reference's multi-GPU trainer keeps ONE entity table in shared host memory and lets every
 * trainer process gather from it and update it without locks (train.py:298-317 --num_proc,
 * tensor_models.py:233 share_memory, :304-362 update; relation table likewise unless
 * --rel_part).  Here the shared table is the union of the 8 GPUs' HBM: rank k owns the rows
 * [k*rows_per_shard, (k+1)*rows_per_shard) of both tables (+ Adagrad state), every rank maps all
 * peers' shards into its address space (kge_ipc_export / kge_ipc_open = hipIpc handles) and
 * kge_step_sharded runs the SAME kernels as kge_step_fused with row addresses resolved through
 * the shard map: remote rows are read and read-modify-written directly over xGMI, no collective
 * and no host work in the step.  Within a rank the update is still owner-computes and
 * deterministic; across ranks it is Hogwild, exactly like the reference's shared table.
 * The four pointer arrays are DEVICE arrays [n_shards] of bases valid in the calling process. */
typedef struct kge_shards {
    int32_t n_shards, reserved;
    int64_t ent_rows_per_shard, rel_rows_per_shard;
    float *const *ent_rows;  float *const *ent_state;
    float *const *rel_rows;  float *const *rel_state;
    int64_t n_ent, n_rel;    /* global row counts (ids in the batch are global) */
    /* ABI 8 - TransR / RESCAL on sharded ENTITY tables (the reference trains TransR on 8 GPUs with --rel_part,                    */
    /* examples/freebase/multi_gpu.sh:80-89: every trainer holds the rows of ITS relations on its own GPU,                         */
    /* general_models.py:590-637).  rel_local != NULL: the relation-side tables are LOCAL to the calling rank - [n_rel, d_r] rows   */
    /* (RESCAL: d_e x d_e matrices) + state, and for TransR the projection table [n_rel, d_e * d_r] + state                        */
    /* (score_fun.py:114-118) - and rel_rows / rel_state are ignored.  The step gathers the batch's entity rows through the shard   */
    /* map into dense copies, runs the TransR / RESCAL kernels on those, updates relation-side rows in place and entity rows        */
    /* through the shard map.  Required for KGE_TRANSR / KGE_RESCAL, optional (relation table replicated per rank) otherwise.       */
    float *rel_local, *rel_state_local;
    float *proj_local, *proj_state_local;
} kge_shards;
int kge_step_sharded(const kge_hparams *hp, const kge_shards *sh, const kge_batch *b,
                     const kge_step_out *out, void *ws, size_t ws_bytes, void *stream);
/* rows of a sharded table by global id (evaluation / checkpoint helper): out[k,:] = row idx[k] */
int kge_gather_rows_sharded(float *const *shard_rows, int n_shards, int64_t rows_per_shard, int dim,
                            const int64_t *idx, int64_t n_idx, float *out, void *stream);
/* hipIpc plumbing for the shard map.  export: handle64 = 64-byte hipIpcMemHandle_t of the
 * ALLOCATION that contains dev_ptr, *offset = dev_ptr - allocation base.  open: maps a peer's
 * allocation into this process (current device) and returns its base; close unmaps it. */
#define KGE_IPC_HANDLE_BYTES 64
int kge_ipc_export(const void *dev_ptr, void *handle64, int64_t *offset);
int kge_ipc_open(const void *handle64, void **base);
int kge_ipc_close(void *base);

/* ---- on-device sampler + plan builder (replaces the DGL EdgeSampler wrappers of
 * dataloader/sampler.py:376-419, 823-876 and the host plan of dglke_amd/plan.py) ----
 * heads/rels/tails: the training triples in HBM; perm: base edge permutation or NULL (sequential order);
 * state: device int64[4] = {(legacy) position, step number (1-based), ticket counter (0 between launches), unused}, advanced
 * by the launch itself (its last workgroup); builds n_slots
 * consecutive batches (batch k = step state[1]+k: odd steps corrupt tails, even steps heads;
 * C*N uniform negatives with replacement from a counter-based RNG keyed by (seed, step)).  Epochs consist of
 * floor(n_train / B) WHOLE batches (the trailing partial batch is dropped, dataloader/sampler.py:503-504) and
 * every epoch has its own edge order (shuffle=True): epoch 0 = perm, epoch e > 0 = perm composed with an affine
 * bijection of [0, n_train) keyed by (seed, e).  n_train >= B.
 * Limits: 2B + C*N <= 8192 (one workgroup sorts a batch in LDS: 4 keys per thread up to 4096 elements, the
 * wide instance 8 keys per thread - the reference's batch-2048 recipes are 6144). */
size_t kge_sampler_slot_bytes(int B, int C, int N);
int kge_sample_batches(const int64_t *heads, const int64_t *rels, const int64_t *tails,
                       const int64_t *perm, int64_t n_train, int64_t n_ent, int B, int C, int chunk,
                       int N, uint64_t seed, int64_t *state, void *slots, size_t slot_bytes,
                       int n_slots, void *stream);
/* ---- ABI 7 (round 5): the sampler as TAIL WORKGROUPS of the training step's own launches (csrc/kge_sampler_tail.hpp) ----
 * kge_step_fused_sampling = kge_step_fused of batch `b` whose first, backward and update launches each carry a few extra
 * 256-thread workgroups that build ONE other batch - the one kge_sample_batches would build as batch `k` of its next launch
 * (step state[1] + k: same ids from the same counter RNG / epoch permutation, same plan, bit for bit) - into `slot`, a phase per
 * launch (ids + bucketed keys | per-bucket sort + scans | relocation to the final lists and records - that last phase on the NEXT
 * step's first launch, `prev_slot`; the group's last job: on its own update launch).  Batch k is complete one launch into the
 * step that carries job k + 1 (the last one: when its step ends); nothing is launched for it.
 * The reference's counterpart: the EdgeSampler worker threads that build the next batches while a step runs
 * (dataloader/sampler.py:823-876).  `state` is NOT advanced by a job unless `advance` > 0 (the group's last job: advance by that
 * many batches, after every job of the group has read it).  `scratch`: kge_sampler_tail_scratch_bytes(), one buffer shared by
 * all jobs of a stream.  Steps whose launches cannot carry the tail (everything but the 4-launch strict step of TransE_l2 /
 * DistMult / ComplEx on local tables) return KGE_ERR_ARG: use kge_sample_batches then.  job == NULL: plain kge_step_fused. */
typedef struct kge_sampler_job {
    const int64_t *heads, *rels, *tails, *perm;   /* as kge_sample_batches */
    int64_t  n_train, n_ent;
    int      B, C, chunk, N;
    uint64_t seed;
    int64_t *state;             /* int64[8]: {position, step (1-based), ticket, -} as kge_sample_batches uses them + {epoch, mul, add, reciprocal}: the epoch constants the jobs cache (initialise word 4 to -1) */
    void    *slot;              /* output slot of THIS batch (kge_sampler_slot_bytes) */
    void    *scratch; size_t scratch_bytes;
    int      k;                 /* index of the batch within the group under construction */
    int      advance;           /* > 0: last job of the group - advance `state` by this many batches */
    int      pre_permuted;      /* != 0: heads / rels / tails are already in base-permutation order (x[perm[i]] at i): the job skips
                                 * the perm lookup - one dependent memory round less in its first phase; perm != NULL still means
                                 * "a new edge order every epoch" */
    int      reserved;
    void    *prev_slot;         /* slot of the job the PREVIOUS step carried (k - 1), whose last phase rides on this step's first launch; NULL for k = 0.
                                 * The group's last job (advance > 0) finishes under its own step's update launch. */
} kge_sampler_job;
size_t kge_sampler_tail_scratch_bytes(int B, int C, int N, int64_t n_ent);
int kge_step_fused_sampling(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out,
                            void *ws, size_t ws_bytes, const kge_sampler_job *job, void *stream);

/* host-side: point a kge_batch at slot `slot` (pure pointer arithmetic, no device access) */
int kge_batch_from_slot(void *slots, size_t slot_bytes, int slot, int B, int C, int chunk, int N,
                        int neg_head, kge_batch *out);

/* ---- the WEIGHTED sampler launch (dglke_train --subsampling_weight, --edge_importance_on_device) ----
 * kge_sample_batches with one float per training triple: `weights` [n_train], indexed like heads / rels / tails (i.e. after
 * perm).  A weighted slot is the unweighted slot - every offset byte for byte - followed by edge_w, float[B], behind `counts`
 * (kge_sampler_slot_bytes_weighted); the workgroup that loads heads[e] and tails[e] of edge i stores weights[e] to edge_w[i].
 * The weights enter neither the RNG nor the epoch permutation nor the plan: ids, lists, records, counts and the state after the
 * launch are those of kge_sample_batches from the same state.  weights == NULL: KGE_ERR_ARG; slot_bytes smaller than
 * kge_sampler_slot_bytes_weighted(): KGE_ERR_WORKSPACE; nothing is launched in either case.  `hip_stream`: the stream of the
 * launch (conventions above), the last argument as everywhere.
 * kge_batch_from_slot_weighted points kge_batch.edge_w at the slot's array and leaves edge_w_mean = 0: the kernels of every step
 * entry then sum the B weights themselves (one lane-strided pass per wavefront that needs the mean).  The sampler tail jobs
 * (kge_step_fused_sampling) carry no weights. */
size_t kge_sampler_slot_bytes_weighted(int B, int C, int N);
int kge_sample_batches_weighted(const int64_t *heads, const int64_t *rels, const int64_t *tails,
                                const int64_t *perm, const float *weights, int64_t n_train, int64_t n_ent, int B, int C,
                                int chunk, int N, uint64_t seed, int64_t *state, void *slots, size_t slot_bytes,
                                int n_slots, void *hip_stream);
int kge_batch_from_slot_weighted(void *slots, size_t slot_bytes, int slot, int B, int C, int chunk, int N,
                                 int neg_head, kge_batch *out);

/* ---- frequency ("subsampling") weights of training triples (csrc/kge_subsample.hip) ----
 * keys_hr [m_hr] / keys_tr [m_tr]: the training split's h * n_rel + r and t * n_rel + r, each sorted ascending WITH multiplicity
 * (a triple present twice counts twice).  Per triple i of heads / rels / tails [n]: n_hr, n_tr = the number of keys equal to
 * heads[i] * n_rel + rels[i] in keys_hr and to tails[i] * n_rel + rels[i] in keys_tr (upper bound - lower bound), and
 *     out[i] = scale * (1 / sqrtf((float)(n_hr + n_tr + 6)))
 * - IEEE square root and division; the + 6 is the start value 4 of both counters of RotatE's count_frequency (a pair seen n
 * times counts n + 3).  scale > 0.  n_ent * n_rel >= 2^62: KGE_ERR_ARG.  One thread per triple; no allocation, no
 * synchronisation, capturable.  `hip_stream`: the stream of the launch, the last argument as everywhere. */
int kge_subsampling_weights(const int64_t *keys_hr, int64_t m_hr, const int64_t *keys_tr, int64_t m_tr,
                            const int64_t *heads, const int64_t *rels, const int64_t *tails, int64_t n, int64_t n_ent,
                            int64_t n_rel, float scale, float *out, void *hip_stream);

/* owner side, packed messages (one row per message, `ld` floats apart):
 *   msg = [ g_0 (dim) | ... | g_{T-1} (dim) | gs_0 .. gs_{T-1} | (id_lo id_hi as int32 bits when idx == NULL) ]
 * applies the T traces of every row in order (trace t: s += gs_t; row += -lr*g_t/(sqrt(s)+eps)).
 * Row ids come from idx[k] or, when idx is NULL, from the two int32 words stored after the gs
 * values (a negative id skips the row).  Ids must be unique within one call. */
int kge_adagrad_apply_packed(float *table, float *state_sum, int64_t n_rows, int dim,
                             const int64_t *idx, const float *msg, int ld, int64_t n, int ntraces,
                             float lr, float eps, void *stream);

/* ---- TransR, per-op (drop-in) route: the projections of TransRScore.prepare / create_neg_prepare
 * (models/pytorch/score_fun.py:131-166, th.matmul in the reference) and their autograd, on DENSE gathered operands ----
 * proj: [B, d_e * d_r] gathered projection rows, row i viewed as P_i [d_e, d_r] (projection_emb(rel_id), :133, :142)
 * kge_transr_project:          out[i,:] = x[i,:] P_i                                   (:135-136, :144-145)
 * kge_transr_project_bwd:      gx[i,:] = P_i gy[i,:];  gproj[i] (+)= x[i,:] (x) gy[i,:]  (either output may be NULL)
 * kge_transr_project_neg:      Y[c,i,j,:] = neg[c,j,:] P_{c,i}   [C, chunk, N, d_r]     (:147-148: every negative of a chunk
 *                              through every positive's matrix)
 * kge_transr_project_neg_bwd:  gneg[c,j,:] = sum_i gY[c,i,j,:] P_{c,i}^T;  gproj[c,i] (+)= neg_c^T gY[c,i]
 * fp32-MFMA tile routine of kge_transr.hip (64 x 64 tiles through LDS); accumulate != 0 adds into gproj. */
int kge_transr_project(const float *proj, const float *x, int64_t B, int d_e, int d_r, float *out, void *stream);
int kge_transr_project_bwd(const float *proj, const float *x, const float *gy, int64_t B, int d_e, int d_r, float *gx,
                           float *gproj, int accumulate, void *stream);
int kge_transr_project_neg(const float *proj, const float *neg, int C, int chunk, int N, int d_e, int d_r, float *Y,
                           void *stream);
int kge_transr_project_neg_bwd(const float *proj, const float *neg, const float *gY, int C, int chunk, int N, int d_e, int d_r,
                               float *gneg, float *gproj, int accumulate, void *stream);

/* ---- device-side routing of the range-sharded step (entity table sharded by id range over the ranks,
 * pull -> compute -> push with owner-side Adagrad, KEModel.pull_model / push_gradient, models/general_models.py:650-680,
 * kvserver.py:41-51) - no host round trip, fixed-size messages, so that the collectives between these calls are plain
 * equal-split all-to-alls (dglke_amd/dist.py) ----
 * kge_route_build: the batch's sorted unique entity ids (b->ue_id, count in b->counts_dev[0] or b->UE) are cut into `world` owner
 *   buckets (owner = id / rows_per_shard) of capacity `cap`:
 *     req_ids[o*cap + p]  = p-th id requested from owner o, -1 beyond the bucket's fill;
 *     cache row of an entity = o*cap + p - the position its row will have in the concatenated replies;
 *     h_loc / t_loc / neg_loc = the batch's edge ends and negative slots as cache rows, ue_loc / ue_rec_loc = the plan's id
 *     array and packed records with cache rows as ids: kge_batch_localized() points a kge_batch at them.
 *   Entries that do not fit their bucket are counted in *overflow (must be checked by the caller at its log interval: the
 *   step treats them as row world*cap, a dump row of the cache that is never sent); one workgroup, ~3 us.
 * kge_gather_rows_req: owner side of the pull - out[k,:] = table[ids[k] - id_offset,:], entries with ids[k] < 0 (pads) or
 *   outside [id_offset, id_offset + n_rows) are skipped.
 * kge_adagrad_apply_merged: owner side of the push for nsrc sources x cap messages (layout [g_0 | .. | g_{T-1} | gs_0 ..
 *   gs_{T-1} | ..], ld floats apart); the id of message k is the int32 pair id_words[k*id_stride_words], [.. + 1] (a separate
 *   int64 array: stride 2; ids inside the messages: stride ld) minus id_offset; negative ids are pads.  Within a source the
 *   ids are ascending with the pads at the end and unique; the same row may come from several sources: the wavefront of its
 *   first source applies every occurrence in source order (trace order inside a message) - deterministic, one launch. */
/* kge_route_fill: *max_fill = max(*max_fill, the largest owner-bucket fill) over n_batches batches - b0 and, for n_batches > 1, the
 *   batches whose ue_id / counts_dev arrays lie k * stride_bytes behind b0's (consecutive slots of kge_sample_batches: stride =
 *   the slot size).  One launch per GROUP of batches; the caller reads the word before the group's steps run and grows `cap`
 *   when needed, so that no entry ever overflows its bucket (dglke_amd/dist.py DistEngine.ensure_capacity). */
/* ABI 8: max_fill is int32[2] - [1] = the largest number of entries of ONE owner bucket that are in BOTH traces of a batch (the
 *   extra-region capacity `cap2` the packed messages need; 0 when the batches carry no plan records). */
int kge_route_fill(const kge_batch *b0, int n_batches, size_t stride_bytes, int world, int64_t rows_per_shard, int32_t *max_fill,
                   void *stream);
/* ABI 8, packed entity messages: ue_msg != NULL -> also writes, per union entry u, ue_msg[2u] = its message row
 *   owner * (cap + cap2) + position (the dump row world * (cap + cap2) for an entry that does not fit) and ue_msg[2u+1] = the
 *   position of its SECOND message in the bucket's extra region (row owner * (cap + cap2) + cap + p, p = rank of u among the
 *   both-trace entries of its bucket), or -1 when u is in one trace only; both-trace entries beyond cap2 are counted in
 *   *overflow.  ue_msg NULL (cap2 ignored): two-trace messages. */
int kge_route_build(const kge_batch *b, int world, int64_t rows_per_shard, int cap, int64_t *req_ids, int64_t *h_loc,
                    int64_t *t_loc, int64_t *neg_loc, int64_t *ue_loc, int32_t *ue_rec_loc, int32_t *overflow, int cap2,
                    int32_t *ue_msg, void *stream);
/* kge_route_build for a whole GROUP of batches in one launch (round 4): batch k's plan arrays lie k * in_stride_bytes behind b0's
 * (consecutive slots of kge_sample_batches), its six outputs k * out_stride_bytes behind the pointers given (one pool per group).
 * Same results per batch as kge_route_build.  Called once per sampled group, after the bucket capacity was checked (kge_route_fill):
 * the step itself then starts with the id exchange. */
int kge_route_build_group(const kge_batch *b0, int n_batches, size_t in_stride_bytes, int world, int64_t rows_per_shard, int cap,
                          int64_t *req_ids, int64_t *h_loc, int64_t *t_loc, int64_t *neg_loc, int64_t *ue_loc, int32_t *ue_rec_loc,
                          size_t out_stride_bytes, int32_t *overflow, int cap2, int32_t *ue_msg, void *stream);
int kge_batch_localized(const kge_batch *b, const int64_t *h_loc, const int64_t *t_loc, const int64_t *neg_loc,
                        const int64_t *ue_loc, const int32_t *ue_rec_loc, kge_batch *out);
int kge_gather_rows_req(const float *table, int64_t n_rows, int dim, const int64_t *ids, int64_t id_offset, int64_t n_ids,
                        float *out, void *stream);
/* ABI 8: cap_extra > 0 = PACKED messages (see kge_emit.msg_rows): source s's bucket is cap + cap_extra message rows, message
 *   (s, pos) = [g | gs | link | . .] (ntraces must be 1, ld >= dim + 4); link >= 0 names a second message of the same row at
 *   bucket position cap + link, applied behind the first (positive trace, then negative trace: the reference's order). */
int kge_adagrad_apply_merged(float *table, float *state_sum, int64_t n_rows, int dim, int nsrc, int cap, const int32_t *id_words,
                             int64_t id_stride_words, int64_t id_offset, const float *msg, int ld, int ntraces, int cap_extra,
                             float lr, float eps, void *stream);

/* two kge_adagrad_apply_merged jobs - the entity-shard apply and the relation-replica apply of one sharded step - as ONE launch
 * (independent tables and messages; same arithmetic and order per job as two separate calls: bit-identical results) */
typedef struct kge_merge_job {
    float *table, *state_sum;
    int64_t n_rows;
    int32_t dim, nsrc, cap, ld, ntraces, cap_extra;   /* cap_extra > 0: packed messages (ABI 8; 0: [g_0 | .. | gs_0 ..] messages) */
    const int32_t *id_words; int64_t id_stride_words, id_offset;
    const float *msg;
} kge_merge_job;
int kge_adagrad_apply_merged_pair(const kge_merge_job *a, const kge_merge_job *b, float lr, float eps, void *stream);


/* ---- inference: top-K triples (the reference's ScoreInfer, models/infer.py:52-214) and top-K similar embedding pairs
 * (EmbSimInfer, :216-344) with no score block in memory (csrc/kge_topk.hip) ----
 * kge_topk_select scores `rows` query rows against a candidate list and keeps, per group of `group_rows` consecutive rows,
 * the K best (score, ordinal) pairs merged with the group's running result res_score / res_ord [rows / group_rows][K]
 * (ordinal -1 = empty slot; fill with -1 before a group's first call).  Candidate j of row i has the ordinal
 * row_base[i] + j * stride; equal scores rank by ordinal (lower first), NaN below every number.
 *   func = a model id (TransE_l1 .. RESCAL; TransR has no inference path): row i is T(h_i, r_i) scored against tails
 *          (side 0) or T(t_i, r_i) against heads (side 1), formed as in kge_rank_eval; the score forms are the reference's
 *          `infer` methods (score_fun.py), gamma as given, RotatE's phase from emb_init.
 *   func = KGE_SIM_*: row i is ent[h_i] (r, t, rel unused); tensor_models.py:59-100.
 * cand == NULL: every row of `ent` (n_cand of them).  Workspace: kge_topk_workspace_bytes(rows, n_cand, d_e, K), which is
 * O(rows x (d_e + segments x K)) + 4 n_cand bytes.  rows == 0: the workspace of kge_topk_vector over n_cand scores.
 * kge_topk_vector: the K best of n scores (ordinal = position), merged with the running result like kge_topk_select.
 * kge_sim_pairwise: out[i] = sim(emb[left[i]], emb[right[i]]). */
#define KGE_TOPK_MAX 128
enum { KGE_SIM_COSINE = 16, KGE_SIM_L2 = 17, KGE_SIM_L1 = 18, KGE_SIM_DOT = 19, KGE_SIM_EXT_JACCARD = 20 };
size_t kge_topk_workspace_bytes(int rows, int64_t n_cand, int d_e, int K);
int kge_topk_select(int func, int side, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel, const int64_t *h,
                    const int64_t *r, const int64_t *t, int rows, int d_e, int d_r, float gamma, float emb_init, const int64_t *cand,
                    int64_t n_cand, const int64_t *row_base, int64_t stride, int group_rows, int K, float *res_score,
                    int64_t *res_ord, void *ws, size_t ws_bytes, void *stream);
int kge_topk_vector(const float *score, int64_t n, int K, float *res_score, int64_t *res_ord, void *ws, size_t ws_bytes, void *stream);
/* link prediction with known-edge exclusion (the reference's link_predict with exclude_mode, models/ke_model.py:205-455, which
 * filters after the fact: the 4K best, a loop over g.edge_ids, a full argsort when that was not enough).  The filtered
 * form of the selection: a candidate j whose ENTITY id (cand[j], or j when cand == NULL) is in row i's list
 * filt_ids[filt_ptr[2i] .. filt_ptr[2i+1]) - ascending and unique within the list, rows may share lists, an empty range
 * filters nothing (the layout of the rank evaluation's lists) - never enters the selection: a group with fewer than K
 * unlisted candidates leaves ordinal -1 in the remaining slots.  Any candidate list (unsorted, repeated ids: every position
 * of a listed id is left out).  filt_ptr == NULL: exactly the unfiltered entry point; same workspace, same errors, and
 * filt_ids == NULL with a filt_ptr is an argument error. */
int kge_topk_select_filtered(int func, int side, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel, const int64_t *h,
                             const int64_t *r, const int64_t *t, int rows, int d_e, int d_r, float gamma, float emb_init,
                             const int64_t *cand, int64_t n_cand, const int64_t *row_base, int64_t stride, int group_rows, int K,
                             float *res_score, int64_t *res_ord, void *ws, size_t ws_bytes, const int64_t *filt_ptr,
                             const int64_t *filt_ids, void *stream);
/* out[i] = 1 when the triple (a_i, r_i, b_i) is in the known index, else 0 (ke_model.py:349-377, 'mask', and the per-triple
 * g.edge_ids of triplet_wise): keys [M] ascending with keys = a * n_rel + r, vals [M] ascending within a key; a two-level
 * binary search (the key, then the value inside the key's range), since key * n_entities + value need not fit int64. */
int kge_triples_known(const int64_t *keys, const int64_t *vals, int64_t M, int64_t n_rel, const int64_t *a, const int64_t *r,
                      const int64_t *b, int64_t n, uint8_t *out, void *stream);
int kge_sim_pairwise(int sim, const float *emb, int64_t n_emb, int d, const int64_t *left, const int64_t *right, int64_t n, float *out,
                     void *stream);

/* ---- known triples left out of the TRAINING negatives (dglke_train --exclude_positive; the reference sampler's `exclude_positive`,
 * dataloader/sampler.py:377, 396, 418, which its CLI hard-wires to False, train.py:125-158) ----
 * kge_known: a set K of known triples as the two sorted (key, entity) indexes the evaluation side already builds
 * (dglke_amd.eval.sort_known_device): unique pairs, ascending by key, then entity.  Tail side: key = h * n_rel + r, values = tails
 * (used by the steps that corrupt tails); head side: key = t * n_rel + r, values = heads.  m_* == 0 (pointers may be NULL): an
 * empty side, nothing is known.  Ids int64, n_entities * n_rel < 2^62.
 * Row i of a batch is the positive (h_i, r_i, t_i) of chunk c, column j holds n = neg_ids[c * N + j]; the pair (i, j) is KNOWN when
 * the corrupted triple - (n, r_i, t_i) / (h_i, r_i, n) - is in K (n equal to the row's own corrupted entity is the simplest
 * case).  A known pair behaves in LossGenerator exactly as a negative whose score is minus infinity: loss term 0 in all four
 * genres, pointwise and pairwise; gradient exactly 0.0f; self-adversarial weight 0 and no share in the softmax normaliser; the
 * denominators 1 / N and 1 / B do not change.  It is implemented as the large finite score KGE_KNOWN_SCORE, so a row whose N
 * columns are all known needs no special case (its softmax is uniform over zeros): loss 0, zero gradients, no NaN / Inf.
 * kge_step_out.neg_score holds KGE_KNOWN_SCORE exactly at the known pairs.  Positive scores, the positive loss part, the
 * regulariser, the plan and the sampler are untouched.
 * kge_known_neg_mask: ONE launch (csrc/kge_known.hip) that writes one bit per pair, mask[B][ceil(N / 32)] (bit j & 31 of word
 * j >> 5 of row i), kge_known_mask_bytes(B, N) bytes.  The corrupted side is kge_batch.counts_dev[2] on device-built plans,
 * kge_batch.neg_head otherwise.
 * kge_step_fused_known / kge_step_phase_known: kge_step_fused_sampling (job may be NULL: kge_step_fused) / kge_step_phase with the
 * mask launch in front of the loss launch (phase group FORWARD) and the stand-alone loss kernel reading the mask.  The mask buffer
 * is the caller's (one per stream of steps); kge_step_workspace_bytes does not change.  known == NULL: exactly the old entries
 * (mask is ignored).  KGE_ERR_ARG before any launch: KGE_FLAG_FUSED_LOSS / KGE_FLAG_LOSS_IN_FWD (their loss does not run in the
 * stand-alone kernel), KGE_FLAG_NEG_DEG_SAMPLE, a null or too small mask, n_rel <= 0, a side with m > 0 and no arrays.  Gradient
 * emission, sharded tables and the async pipeline have no entry with a known index.  The sampler job rides on the same three
 * launches as in kge_step_fused_sampling (the mask and loss launches carry nothing), with the same limits. */
#define KGE_KNOWN_SCORE (-1.0e6f)
typedef struct kge_known {
    const int64_t *keys_tail, *vals_tail; int64_t m_tail;   /* key = h * n_rel + r -> known tails */
    const int64_t *keys_head, *vals_head; int64_t m_head;   /* key = t * n_rel + r -> known heads */
    int64_t n_rel;
} kge_known;
size_t kge_known_mask_bytes(int B, int N);
int kge_known_neg_mask(const kge_batch *b, const kge_known *known, uint32_t *mask, size_t mask_bytes, void *stream);
int kge_step_fused_known(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out, void *ws,
                         size_t ws_bytes, const kge_sampler_job *job, const kge_known *known, uint32_t *mask, size_t mask_bytes,
                         void *stream);
int kge_step_phase_known(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out, void *ws,
                         size_t ws_bytes, int phases, const kge_known *known, uint32_t *mask, size_t mask_bytes, void *stream);

/* ---- the optimizer as an argument of the strict step: --optimizer Adam (csrc/kge_adam.hip) ----
 * kge_step_optim is the strict single-table step (kge_step_fused / kge_step_phase, with or without a known-triple index) whose
 * update launch is chosen by `opt->kind`:
 *  KGE_OPT_ADAGRAD  the existing step: bit for bit the tables and state of kge_step_fused / kge_step_fused_known (all four phase
 *                   bits) or of kge_step_phase / kge_step_phase_known; beta1, beta2, eps and the moment pointers are ignored.
 *  KGE_OPT_ADAM     lazy (row-sparse) Adam with a PER-ROW step count, the rule of DGL's sparse Adam.  G = the sum of a table row's
 *                   gradient traces in the step, formed exactly as the Adagrad step forms them (positive trace, then negative
 *                   trace, regulariser terms where the Adagrad step adds them; a relation row: its relation trace).  For a row x
 *                   touched by the step:
 *                       c  = min(c + 1, 2^24)                 per-row count of updates; a float holds it exactly
 *                       m  = beta1 m + (1 - beta1) G
 *                       v  = beta2 v + (1 - beta2) G*G
 *                       x -= lr (m / (1 - beta1^c)) / (sqrt(v / (1 - beta2^c)) + eps)
 *                   One update per row per step: a row in both entity traces is updated once with the sum (the Adagrad step
 *                   applies its two traces one after the other).  Rows the step does not touch keep value, moments and count bit
 *                   for bit.  A touched row with G == 0 still counts, decays its moments and moves by its momentum; with
 *                   m = v = 0 too it stays exactly where it is (0 / (0 + eps) = 0).  lr is kge_hparams.lr; kge_hparams.eps is
 *                   not read.  The count is per row, not a global step number: nothing in a step depends on a host-side value,
 *                   so a captured graph of many steps replays like any other.
 * Storage: kge_tables.ent_state [n_ent] and rel_state [n_rel] hold the counts c (zero at start); ent_mom [n_ent, 2, d_e] and
 * rel_mom [n_rel, 2, d_r] hold each row's m, then its v, contiguous, zero at start - three times the table memory.
 * `phases`: as in kge_step_phase; all four bits = the whole strict step in one call.  `known` may be NULL (mask is then ignored),
 * else as in kge_step_fused_known.  The workspace is that of kge_step_workspace_bytes - Adam needs no more.  TransE_l1 under Adam
 * sums its backward's GN partials in the stand-alone reduction launch (the Adagrad step folds them into its update).
 * KGE_ERR_ARG before any launch, the message naming this entry and the reason: RESCAL / TransR (their relation-side tables are
 * updated by kernels of their own), null moments, a beta outside [0, 1), eps <= 0, a row width that is no multiple of 4 or
 * beyond 1024 floats (the domain of the register-resident update), an unknown kind, a bad phase mask.
 * `hip_stream`: the stream of the launches, the last argument as everywhere.  The sharded step, kge_step_grads, kge_step_async and
 * the sampler-tail step have no Adam form. */
#define KGE_OPT_ADAGRAD 0
#define KGE_OPT_ADAM 1
typedef struct kge_optim {
    int32_t kind;               /* KGE_OPT_ADAGRAD 0, KGE_OPT_ADAM 1 */
    float beta1, beta2, eps;    /* 0.9, 0.999, 1e-8 */
    float *ent_mom, *rel_mom;   /* [n_ent, 2, d_e], [n_rel, 2, d_r] */
} kge_optim;
int kge_step_optim(const kge_hparams *hp, const kge_optim *opt, const kge_tables *tb, const kge_batch *b, const kge_step_out *out,
                   void *ws, size_t ws_bytes, int phases, const kge_known *known, uint32_t *mask, size_t mask_bytes,
                   void *hip_stream);

/* ---- test support: not part of the stable boundary ----
 * kge_debug_carve: while set (per calling thread), every buffer that an entry point or a *_workspace_bytes function carves from a
 * workspace is recorded as trace[2k] = offset from the base that carve started at, trace[2k + 1] = bytes (HOST memory, room for
 * cap_pairs pairs; further buffers are counted, not recorded), and `gap` extra bytes are left behind every buffer before the
 * 256-byte round-up.  The size functions and the entries share the allocators, so they agree with the gap as without it.  The
 * call resets the count; (NULL, 0, 0) switches the setting off: the layout is then exactly the documented one.
 * kge_debug_carve_count: buffers carved by this thread since its last kge_debug_carve call.
 * kge_debug_epoch_order (csrc/kge_debug.hip): the device sampler's epoch order - edge i of epoch e is perm[(i * mul + add) mod n_train],
 * (mul, add) hashed from (seed, e) - evaluated by the sampler kernels' own inline functions for n (epoch[k], pos[k]) pairs, without
 * any triple, so that graphs of 2^32 triples and more can be tested: out[5k .. 5k + 4] = {the index by the sampler launch's
 * remainder, the index by the tail jobs' cached reciprocal, mul, add, floor((2^64 - 1) / n_train)} (the last three as 64-bit
 * patterns).  shuffled == 0: a sampler without a base permutation (every epoch the identity).  epoch, pos, out: device memory;
 * every pos[k] must be in [0, n_train) - the caller's responsibility.  KGE_ERR_ARG: n_train <= 0, n < 0, a null pointer. */
int kge_debug_carve(int64_t *trace, int cap_pairs, size_t gap);
int kge_debug_carve_count(void);
int kge_debug_epoch_order(int64_t n_train, uint64_t seed, int shuffled, const int64_t *epoch, const int64_t *pos, int64_t n,
                          int64_t *out /* [n][5]: index, index_fast, mul, add, rinv */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_H */
