// kge_api.hip - the C ABI of libkge_hip.so (include/kge_hip.h): argument checking, workspace
// carving and the kernel sequence of each entry point.  No allocation, no synchronisation: every
// function only enqueues kernels on the caller's stream.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <algorithm>
#include "kge_common.hpp"
#include "kge_constrain.hpp"
#include "kge_models.hpp"
#include "kge_own_fwd.hpp"
#include "kge_sampler_common.hpp"

namespace {

using kge::clamp_of; using kge::fill_gemm; using kge::fill_pair;
using kge::OwnBlock; using kge::OwnBufs; using kge::OwnBwd; using kge::OwnCands; using kge::OwnOperand;

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define KGE_TRY(expr)                                                                  \
    do {                                                                               \
        const int rc_ = (expr);                                                        \
        if (rc_ != KGE_OK) return fail(rc_, "%s failed (%d) at %s:%d", #expr, rc_, __FILE__, __LINE__); \
    } while (0)

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// kge_debug_carve (test support): where to record the carved buffers of this thread's calls, and the gap behind each
thread_local struct { int64_t *trace; int cap, count; size_t gap; bool on; } g_carve = {nullptr, 0, 0, 0, false};

// bump allocator over the caller's workspace.  Each workspace has ONE carve function (carve_neg, carve_step, carve_rank): the
// entry point carves its buffers with it, the *_workspace_bytes function runs it on a measuring Carver and returns the offset
struct Carver {
    uintptr_t base; size_t size, off;
    Carver(void *p, size_t n) : base((uintptr_t)p), size(n), off(0) {}
    Carver() : Carver(nullptr, SIZE_MAX) {}            // measuring: the pointers it hands out are never used
    void *bytes(size_t n) {
        const size_t o = off;
        off = align_up(off + n + kge_carve_note(o, n));
        return (void *)(base + o);
    }
    float *f(size_t n_floats) { return (float *)bytes(n_floats * sizeof(float)); }
    int64_t *i64(size_t n) { return (int64_t *)bytes(n * sizeof(int64_t)); }
    bool ok() const { return off <= size; }
};

int check_model(int model, int d_e, int d_r) {
    const kge::ModelRow *m = kge::model_row(model);
    if (!m) return fail(KGE_ERR_ARG, "unknown model %d", model);
    if (m->bad_dims_first && (d_e <= 0 || d_r <= 0)) return fail(KGE_ERR_ARG, "bad dims d_e=%d d_r=%d", d_e, d_r);
    if (!kge::widths_ok(*m, d_e, d_r)) return fail(KGE_ERR_ARG, m->widths_msg, d_e, d_r);
    return KGE_OK;
}

// the entry `who` is closed to the model (kge_models.hpp): every other id passes
int closed(kge::Entry e, int model, const char *who) {
    const kge::ModelRow *m = kge::model_row(model);
    if (!m || !(m->closed & e)) return KGE_OK;
    if (e == kge::E_MODULAR) return fail(KGE_ERR_ARG, "%s has no modular score ops: use kge_step_fused / kge_rank_eval_ex", m->name);
    return fail(KGE_ERR_ARG, "%s: not available for %s (%s)", who, m->name, m->closed_why);
}

inline float rot_div_of(float emb_init) { return (float)((double)emb_init / M_PI); }

bool use_mfma(int model, int d_e, int N, unsigned flags) {
    return !(flags & KGE_FLAG_FORCE_PAIRWISE) && neg_mfma_supported(model, d_e, N);
}

int check_loss(int genre, int adv, int pairwise) {
    if (genre < KGE_LOSS_LOGSIGMOID || genre > KGE_LOSS_SOFTMAX) return fail(KGE_ERR_ARG, "unknown loss genre %d", genre);
    if (genre == KGE_LOSS_SOFTMAX && adv) return fail(KGE_ERR_ARG, "Softmax loss cannot be adversarial sampled: the softmax is the weighting");
    if (genre == KGE_LOSS_SOFTMAX && pairwise) return fail(KGE_ERR_ARG, "Softmax loss cannot be applied to pairwise loss function");
    if (pairwise && adv) return fail(KGE_ERR_ARG, "loss cannot be pairwise and adversarial sampled");
    if (pairwise && genre != KGE_LOSS_LOGISTIC && genre != KGE_LOSS_HINGE)
        return fail(KGE_ERR_ARG, "this loss cannot be applied to pairwise loss function");
    return KGE_OK;
}

// ---- the norm constraints (KGE_FLAG_ENT_NORM_* / KGE_FLAG_REL_NORM_*, include/kge_hip.h) ----
enum : unsigned { NORM_ENT = KGE_FLAG_ENT_NORM_CLIP | KGE_FLAG_ENT_NORM_UNIT, NORM_REL = KGE_FLAG_REL_NORM_CLIP | KGE_FLAG_REL_NORM_UNIT };

const char *norm_flag_name(unsigned fl) {
    return (fl & KGE_FLAG_ENT_NORM_CLIP) ? "KGE_FLAG_ENT_NORM_CLIP" : (fl & KGE_FLAG_ENT_NORM_UNIT) ? "KGE_FLAG_ENT_NORM_UNIT" :
           (fl & KGE_FLAG_REL_NORM_CLIP) ? "KGE_FLAG_REL_NORM_CLIP" : "KGE_FLAG_REL_NORM_UNIT";
}

// the entries that have no launch behind their update to carry the projection (sharded tables, gradient emission, the stale pipeline)
int norm_closed(const kge_hparams *hp, const char *who) {
    if (!hp || !(hp->flags & (NORM_ENT | NORM_REL))) return KGE_OK;
    return fail(KGE_ERR_ARG, "%s: %s is not available here (the norm constraints run behind the update launch of the strict step on "
                             "local tables)", who, norm_flag_name(hp->flags));
}

// the strict step: one mode per table, and a relation row that has slices (kge_models.hpp); the model id has been checked
int check_norm(const kge_hparams *hp, const char *who) {
    const unsigned fl = hp->flags;
    if (!(fl & (NORM_ENT | NORM_REL))) return KGE_OK;
    if ((fl & NORM_ENT) == NORM_ENT)
        return fail(KGE_ERR_ARG, "%s: KGE_FLAG_ENT_NORM_CLIP and KGE_FLAG_ENT_NORM_UNIT are two modes of one table: set one", who);
    if ((fl & NORM_REL) == NORM_REL)
        return fail(KGE_ERR_ARG, "%s: KGE_FLAG_REL_NORM_CLIP and KGE_FLAG_REL_NORM_UNIT are two modes of one table: set one", who);
    const kge::ModelRow *m = kge::model_row(hp->model);
    if ((fl & NORM_REL) && m->norm.rel == 0)
        return fail(KGE_ERR_ARG, "%s: %s is not available for %s (%s)", who, norm_flag_name(fl & NORM_REL), m->name, m->norm.rel_why);
    return KGE_OK;
}

// no per-step output asked: the plain training step
bool plain_out(const kge_step_out *out) {
    return !out || (!out->loss4 && !out->pos_score && !out->neg_score && !out->g_pos_ent && !out->g_neg && !out->g_rel);
}

// the criterion and its operands; everything else (row terms, running sums, score transforms) is the caller's
void fill_loss(LossArgs &a, const LossParams &lp, int B, int N, const float *pos, const float *neg, const float *w, float *dpos, float *dneg) {
    a = LossArgs{};
    a.B = B; a.N = N; a.genre = lp.genre; a.adv = lp.adv; a.pos_row = lp.pos_row; a.adv_temp = lp.adv_temp; a.margin = lp.margin;
    a.pos = pos; a.neg = neg; a.w = w; a.dpos = dpos; a.dneg = dneg;
}
// the fields EdgeFwdArgs and EdgeBwdArgs share; inputs beyond them, outputs and the regulariser are the caller's
template <class Args>
void fill_edge(Args &e, const EdgeSrc &src, int model, int B, int d_e, int d_r, int neg_head, float gamma, float rot_div) {
    e = Args{};
    e.src = src; e.B = B; e.d_e = d_e; e.d_r = d_r; e.neg_head = neg_head; e.model = model; e.gamma = gamma; e.rot_div = rot_div;
}
void fill_edge_bwd(EdgeBwdArgs &e, const EdgeSrc &src, int model, int B, int d_e, int d_r, int neg_head, float gamma, float rot_div,
                   const float *dpos, const float *GA) {
    fill_edge(e, src, model, B, d_e, d_r, neg_head, gamma, rot_div);
    e.dpos = dpos; e.GA = GA;
}

// SimplE, modular backward: no gradient through a saturated clamp
__global__ void clamp_mask_kernel(const float *dneg, const float *score, float c, float *W, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    W[k] = fabsf(score[k]) >= c ? 0.f : dneg[k];
}

__global__ void l2_scale_kernel(const float *dneg, const float *score, float gamma, float *W, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float d = gamma - score[k];
    W[k] = d > 1e-15f ? dneg[k] / d : 0.f;
}

}  // namespace

int kge_fail(int code, const char *msg) { return fail(code, "%s", msg); }

size_t kge_carve_note(size_t off, size_t bytes) {
    if (!g_carve.on) return 0;
    if (g_carve.trace && g_carve.count < g_carve.cap) {
        g_carve.trace[2 * g_carve.count] = (int64_t)off;
        g_carve.trace[2 * g_carve.count + 1] = (int64_t)bytes;
    }
    g_carve.count++;
    return g_carve.gap;
}

extern "C" {

int kge_abi_version(void) { return KGE_ABI_VERSION; }
const char *kge_last_error(void) { return g_err; }

// test support: trace + guard gaps of every buffer this thread carves from now on (include/kge_hip.h)
int kge_debug_carve(int64_t *trace, int cap_pairs, size_t gap) {
    if (cap_pairs < 0 || (cap_pairs > 0 && !trace)) return fail(KGE_ERR_ARG, "kge_debug_carve: bad argument");
    g_carve.trace = cap_pairs ? trace : nullptr; g_carve.cap = cap_pairs; g_carve.count = 0; g_carve.gap = gap;
    g_carve.on = cap_pairs > 0 || gap > 0;
    return KGE_OK;
}
int kge_debug_carve_count(void) { return g_carve.count; }

int kge_gather_rows(const float *table, int64_t n_rows, int dim, const int64_t *idx, int64_t n_idx,
                    float *out, void *stream) {
    if (!table || (!out && n_idx) || (!idx && n_idx) || dim <= 0 || n_rows < 0 || n_idx < 0)
        return fail(KGE_ERR_ARG, "kge_gather_rows: bad argument");
    KGE_TRY(launch_gather_rows(table, dim, idx, n_idx, out, (hipStream_t)stream));
    return KGE_OK;
}

int kge_score_pos(int model, const float *h, const float *r, const float *t, int64_t B, int d_e,
                  int d_r, float gamma, float emb_init, float *out, void *stream) {
    if (int rc = check_model(model, d_e, d_r)) return rc;
    if (!h || !r || !t || !out || B < 0) return fail(KGE_ERR_ARG, "kge_score_pos: bad argument");
    if (int rc = closed(kge::E_MODULAR, model, "kge_score_pos")) return rc;
    if (model == KGE_RESCAL) {                       // p = h . (M t), one pass over M per edge
        RescalMatvecArgs m{};
        m.B = (int)B; m.D = d_e; m.rel = r; m.y1 = t; m.pd = h; m.p = out;
        KGE_TRY(launch_rescal_matvec(m, (hipStream_t)stream));
        return KGE_OK;
    }
    if (kge::model_row(model)->own_fwd) {
        KGE_TRY(kge::own_prepare(model, EdgeSrc{h, nullptr, t, nullptr, r, nullptr}, (int)B, 0, d_e, 0, gamma, out, OwnOperand{}, nullptr, (hipStream_t)stream));
        return KGE_OK;
    }
    EdgeFwdArgs a;
    fill_edge(a, EdgeSrc{h, nullptr, t, nullptr, r, nullptr}, model, (int)B, d_e, d_r, 0, gamma, rot_div_of(emb_init));
    a.pos_score = out;
    KGE_TRY(launch_edge_fwd(a, (hipStream_t)stream));
    return KGE_OK;
}

int kge_score_pos_bwd(int model, const float *h, const float *r, const float *t, const float *dpos,
                      int64_t B, int d_e, int d_r, float gamma, float emb_init, float *gh, float *gr,
                      float *gt, void *stream) {
    if (int rc = check_model(model, d_e, d_r)) return rc;
    if (!h || !r || !t || !dpos || B < 0) return fail(KGE_ERR_ARG, "kge_score_pos_bwd: bad argument");
    if (int rc = closed(kge::E_MODULAR, model, "kge_score_pos_bwd")) return rc;
    if (model == KGE_RESCAL) {                       // gh = dp M t, gt = dp M^T h, gr = dp h t^T
        if (!gh || !gt || !gr) return fail(KGE_ERR_ARG, "kge_score_pos_bwd: RESCAL needs all three outputs");
        hipStream_t s = (hipStream_t)stream;
        RescalMatvecArgs m{};
        m.B = (int)B; m.D = d_e; m.rel = r; m.y1 = t; m.r1 = gh; m.z1 = h; m.c1 = gt;
        KGE_TRY(launch_rescal_matvec(m, s));
        KGE_TRY(launch_rescal_axpy(dpos, gh, nullptr, (int)B, d_e, gh, s));
        KGE_TRY(launch_rescal_axpy(dpos, gt, nullptr, (int)B, d_e, gt, s));
        RescalOuterArgs o{};
        o.B = (int)B; o.D = d_e; o.c = dpos; o.u = h; o.v = t; o.G = gr;
        KGE_TRY(launch_rescal_outer(o, s));
        return KGE_OK;
    }
    if (kge::model_row(model)->own_fwd) {             // the positive edges alone: no block behind them
        OwnBwd x{}; x.dpos = dpos; x.GH = gh; x.GT = gt; x.GR = gr;
        KGE_TRY(kge::own_backward(model, OwnBlock{1, (int)B, 0, d_e, gamma, OwnOperand{}, nullptr, nullptr, nullptr}, nullptr,
                                  EdgeSrc{h, nullptr, t, nullptr, r, nullptr}, 0, nullptr, nullptr, x, (hipStream_t)stream));
        return KGE_OK;
    }
    EdgeBwdArgs a;
    fill_edge_bwd(a, EdgeSrc{h, nullptr, t, nullptr, r, nullptr}, model, (int)B, d_e, d_r, 0, gamma, rot_div_of(emb_init), dpos, nullptr);
    a.clamp_pos = 1; a.GH = gh; a.GT = gt; a.GR = gr;
    KGE_TRY(launch_edge_bwd(a, (hipStream_t)stream));
    return KGE_OK;
}

// the workspace of the modular negative-score entry points (forward and backward share it)
struct NegBufs { float *A, *asq, *bsq, *W, *GA, *GNp; OwnBufs own; };
static size_t carve_neg(Carver &cv, NegBufs &w, int model, int C, int chunk, int N, int d_e) {
    const size_t B = (size_t)C * chunk;
    w.A = cv.f(B * d_e);                              // pos-side vectors
    w.asq = cv.f(B); w.bsq = cv.f((size_t)C * N);     // |a|^2, |b|^2 (TransE_l2, matrix-core forward)
    w.W = cv.f(B * (size_t)N);                        // L2-scaled / clamp-masked dneg
    w.GA = cv.f(B * d_e);
    w.GNp = neg_bwd_lc_supported(model, d_e) ? cv.f(neg_bwd_lc_partial_floats(model, C, chunk, N, d_e)) : nullptr;
    kge::own_carve(model, cv, w.own, w.A, w.asq, w.bsq, w.GA, B, (size_t)C * N, (size_t)N, (size_t)d_e);      // (nothing for the other models)
    return cv.off;
}

size_t kge_score_neg_workspace_bytes(int model, int C, int chunk, int N, int d_e) {
    Carver cv; NegBufs w; return carve_neg(cv, w, model, C, chunk, N, d_e);
}

// pos-side vectors A = T(pos_side, rel) for the modular negative-score entry points
static int neg_prepare(int model, int neg_head, const float *pos_side, const float *rel, const float *neg, int C, int chunk, int N,
                       int d_e, int d_r, float gamma, float emb_init, bool l2g, const NegBufs &w, hipStream_t s) {
    const int B = C * chunk;
    if (model == KGE_RESCAL) {
        RescalMatvecArgs m{};
        m.B = B; m.D = d_e; m.rel = rel; m.y1 = pos_side; m.r1 = w.A;
        KGE_TRY(launch_rescal_matvec(m, s));
        return KGE_OK;
    }
    if (kge::model_row(model)->own_fwd) {      // the operand of every edge and the scalars of every candidate row, one launch
        const OwnCands c{neg, nullptr, C * N, nullptr, 0, 0, nullptr};
        KGE_TRY(kge::own_prepare(model, EdgeSrc{pos_side, nullptr, pos_side, nullptr, rel, nullptr}, B, chunk, d_e, neg_head, gamma, nullptr, w.own.o, &c, s));
        return KGE_OK;
    }
    EdgeFwdArgs a;
    fill_edge(a, EdgeSrc{pos_side, nullptr, pos_side, nullptr, rel, nullptr}, model, B, d_e, d_r, neg_head, gamma, rot_div_of(emb_init));
    a.A = w.A;
    if (l2g) { a.asq = w.asq; a.nbase = neg; a.nidx = nullptr; a.n_neg = C * N; a.bsq = w.bsq; }
    KGE_TRY(launch_edge_fwd(a, s));
    return KGE_OK;
}

int kge_score_neg_fwd(int model, int neg_head, const float *pos_side, const float *rel, const float *neg, int C, int chunk, int N,
                      int d_e, int d_r, float gamma, float emb_init, float *out, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    if (int rc = check_model(model, d_e, d_r)) return rc;
    if (!pos_side || !rel || !neg || !out || !ws || C < 0 || chunk <= 0 || N <= 0)
        return fail(KGE_ERR_ARG, "kge_score_neg_fwd: bad argument");
    if (int rc = closed(kge::E_MODULAR, model, "kge_score_neg_fwd")) return rc;
    if (C == 0) return KGE_OK;
    hipStream_t s = (hipStream_t)stream;
    Carver cv(ws, ws_bytes); NegBufs w;
    if (carve_neg(cv, w, model, C, chunk, N, d_e) > ws_bytes) return fail(KGE_ERR_WORKSPACE, "workspace too small");
    const bool mf = use_mfma(model, d_e, N, flags);
    if (int rc = neg_prepare(model, neg_head, pos_side, rel, neg, C, chunk, N, d_e, d_r, gamma, emb_init, mf && model == KGE_TRANSE_L2, w, s)) return rc;
    if (kge::model_row(model)->own_fwd) {
        KGE_TRY(kge::own_scores(model, OwnBlock{C, chunk, N, d_e, gamma, w.own.o, neg, nullptr, w.own.PQ}, out, s));
    } else if (mf) {
        GemmArgs g; fill_gemm(g, model, C, chunk, N, d_e, gamma, w.A, neg, nullptr);
        g.S = out; g.asq = w.asq; g.bsq = w.bsq;
        KGE_TRY(launch_neg_fwd_gemm(g, s));
    } else {
        NegArgs na; fill_pair(na, model, C, chunk, N, d_e, gamma, w.A, neg, nullptr);
        na.S = out;
        KGE_TRY(launch_neg_fwd_pair(na, s));
    }
    return KGE_OK;
}

int kge_score_neg_bwd(int model, int neg_head, const float *pos_side, const float *rel, const float *neg, const float *neg_score,
                      const float *dneg, int C, int chunk, int N, int d_e, int d_r, float gamma, float emb_init, float *g_pos_side,
                      float *g_rel, float *g_neg, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    if (int rc = check_model(model, d_e, d_r)) return rc;
    if (!pos_side || !rel || !neg || !dneg || !g_pos_side || !g_rel || !g_neg || !ws || C < 0 || chunk <= 0 || N <= 0)
        return fail(KGE_ERR_ARG, "kge_score_neg_bwd: bad argument");
    if (int rc = closed(kge::E_MODULAR, model, "kge_score_neg_bwd")) return rc;
    if ((model == KGE_TRANSE_L2 || model == KGE_SIMPLE) && !neg_score)
        return fail(KGE_ERR_ARG, "kge_score_neg_bwd: TransE_l2 / SimplE need the forward scores");
    if (C == 0) return KGE_OK;
    hipStream_t s = (hipStream_t)stream;
    const int B = C * chunk;
    Carver cv(ws, ws_bytes); NegBufs w;
    const size_t need = carve_neg(cv, w, model, C, chunk, N, d_e);
    if (need > ws_bytes) return fail(KGE_ERR_WORKSPACE, "workspace too small: need %zu bytes", need);
    if (int rc = neg_prepare(model, neg_head, pos_side, rel, neg, C, chunk, N, d_e, d_r, gamma, emb_init, false, w, s)) return rc;
    if (kge::model_row(model)->own_fwd) {
        OwnBwd x{}; x.GR = g_rel; x.products = true;
        (neg_head ? x.GT : x.GH) = g_pos_side;
        KGE_TRY(kge::own_backward(model, OwnBlock{C, chunk, N, d_e, gamma, w.own.o, neg, nullptr, w.own.PQ}, &w.own,
                                  EdgeSrc{pos_side, nullptr, pos_side, nullptr, rel, nullptr}, neg_head, dneg, g_neg, x, s));
        return KGE_OK;
    }
    const float *Wuse = dneg;
    if (model == KGE_TRANSE_L2 || model == KGE_SIMPLE) {
        const int64_t n = (int64_t)B * N;
        const dim3 grid((unsigned)((n + 255) / 256));
        if (model == KGE_TRANSE_L2) hipLaunchKernelGGL(l2_scale_kernel, grid, dim3(256), 0, s, dneg, neg_score, gamma, w.W, n);
        else hipLaunchKernelGGL(clamp_mask_kernel, grid, dim3(256), 0, s, dneg, neg_score, KGE_SIMPLE_CLAMP, w.W, n);
        Wuse = w.W;
    }
    bool gemm = use_mfma(model, d_e, N, flags);
    if (gemm) {
        GemmArgs g; fill_gemm(g, model, C, chunk, N, d_e, gamma, w.A, neg, nullptr);
        g.W = Wuse; g.GA = w.GA; g.GN = g_neg;
        // KGE_ERR_ARG: chunk or N above the rows a backward tile's workgroup indexes (GB_MAXK, kge_neg_gemm.hip) - nothing was
        // launched, the pair kernels take any size (the reference accepts any chunk_size / neg_sample_size)
        const int rc = launch_neg_bwd_gemm(g, s);
        if (rc == KGE_ERR_ARG) gemm = false;
        else if (rc != KGE_OK) return fail(rc, "launch_neg_bwd_gemm failed (%d)", rc);
    }
    if (!gemm) {
        NegArgs na; fill_pair(na, model, C, chunk, N, d_e, gamma, w.A, neg, nullptr);
        na.W = Wuse; na.GA = w.GA; na.GN = g_neg;
        na.GNp = (flags & KGE_FLAG_TWO_PASS_PAIR) ? nullptr : w.GNp;      // null: the two-pass kernels
        KGE_TRY(launch_neg_bwd_pair(na, s));
    }
    if (model == KGE_RESCAL) {                       // a = M x:  dL/dx = M^T GA,  dL/dM = GA x^T
        RescalMatvecArgs m{};
        m.B = B; m.D = d_e; m.rel = rel; m.z1 = w.GA; m.c1 = g_pos_side;
        KGE_TRY(launch_rescal_matvec(m, s));
        RescalOuterArgs o{};
        o.B = B; o.D = d_e; o.u = w.GA; o.v = pos_side; o.G = g_rel;
        KGE_TRY(launch_rescal_outer(o, s));
        return KGE_OK;
    }
    EdgeBwdArgs e;
    fill_edge_bwd(e, EdgeSrc{pos_side, nullptr, pos_side, nullptr, rel, nullptr}, model, B, d_e, d_r, neg_head, gamma,
                  rot_div_of(emb_init), nullptr, w.GA);
    e.GH = neg_head ? nullptr : g_pos_side;
    e.GT = neg_head ? g_pos_side : nullptr;
    e.GR = g_rel;
    KGE_TRY(launch_edge_bwd(e, s));
    return KGE_OK;
}

int kge_loss_fwd_bwd(int loss_genre, int adv, float adv_temp, int pairwise, float margin, const float *pos, const float *neg,
                     const float *w, int64_t B, int N, float *loss3, float *dpos, float *dneg, void *ws, size_t ws_bytes, void *stream) {
    if (int rc = check_loss(loss_genre, adv, pairwise)) return rc;
    if (!pos || !neg || !dpos || !dneg || !ws || B <= 0 || N <= 0)
        return fail(KGE_ERR_ARG, "kge_loss_fwd_bwd: bad argument");
    Carver cv(ws, ws_bytes);
    float *row_pos = cv.f(B), *row_neg = cv.f(B);
    // finalize writes 4 floats {pos, neg, loss, reg}; loss3 has room for 3 -> stage in ws (carved before the first launch: a
    // workspace too small for it is refused with nothing enqueued)
    float *l4 = loss3 ? cv.f(4) : nullptr;
    if (!cv.ok()) return fail(KGE_ERR_WORKSPACE, "workspace too small (%zu < %zu)", ws_bytes, cv.off);
    LossArgs a;
    fill_loss(a, LossParams{loss_genre, adv, loss_pos_row(loss_genre, pairwise), adv_temp, margin}, (int)B, N, pos, neg, w, dpos, dneg);
    a.row_pos = row_pos; a.row_neg = row_neg;
    KGE_TRY(launch_loss(a, (hipStream_t)stream));
    if (loss3) {
        FinalizeArgs f{};
        f.B = (int)B; f.UE = 0; f.UR = 0; f.pos_row = loss_pos_row(loss_genre, pairwise);
        f.row_pos = row_pos; f.row_neg = row_neg; f.loss4 = l4;
        KGE_TRY(launch_finalize(f, (hipStream_t)stream));
        if (hipMemcpyAsync(loss3, l4, 3 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
            return fail(KGE_ERR_LAUNCH, "hipMemcpyAsync failed");
    }
    return KGE_OK;
}

int kge_reduce_loss(float *loss_accum, float *out4, int zero_after, void *stream) {
    if (!loss_accum || !out4) return fail(KGE_ERR_ARG, "kge_reduce_loss: null argument");
    KGE_TRY(launch_reduce_acc(loss_accum, out4, zero_after, (hipStream_t)stream));
    return KGE_OK;
}

int kge_adagrad_scatter(float *table, float *state_sum, int64_t n_rows, int dim, const int64_t *idx,
                        const float *grad, int64_t n_idx, float lr, float eps, void *stream) {
    if (!table || !state_sum || (!idx && n_idx) || (!grad && n_idx) || dim <= 0 || n_rows < 0)
        return fail(KGE_ERR_ARG, "kge_adagrad_scatter: bad argument");
    KGE_TRY(launch_adagrad_scatter(table, state_sum, dim, idx, grad, n_idx, lr, eps, (hipStream_t)stream));
    return KGE_OK;
}

int kge_scatter_add_rows(float *out, int64_t n_rows, int dim, const int64_t *idx, const float *src, int64_t n_idx, void *stream) {
    if ((n_idx && (!out || !idx || !src)) || dim <= 0 || n_rows < 0 || n_idx < 0) return fail(KGE_ERR_ARG, "kge_scatter_add_rows: bad argument");
    KGE_TRY(launch_scatter_add_rows(out, dim, idx, src, n_idx, (hipStream_t)stream));
    return KGE_OK;
}

int kge_pnorm_pow(const float *x, int64_t n, int dim, int p, float *out, void *ws, size_t ws_bytes, void *stream) {
    if (!out || (n && !x) || n < 0 || dim <= 0 || p <= 0 || !ws) return fail(KGE_ERR_ARG, "kge_pnorm_pow: bad argument");
    if (ws_bytes < (size_t)(n > 0 ? n : 1) * sizeof(float))
        return fail(KGE_ERR_WORKSPACE, "kge_pnorm_pow: workspace too small (%zu < n floats = %zu)", ws_bytes, (size_t)(n > 0 ? n : 1) * sizeof(float));
    KGE_TRY(launch_pnorm(x, n, dim, p, (float *)ws, out, (hipStream_t)stream));
    return KGE_OK;
}

int kge_pnorm_pow_bwd(const float *x, int64_t n, int dim, int p, const float *gout, float *gx, void *stream) {
    if ((n && (!x || !gx)) || !gout || n < 0 || dim <= 0 || p <= 0) return fail(KGE_ERR_ARG, "kge_pnorm_pow_bwd: bad argument");
    KGE_TRY(launch_pnorm_bwd(x, n * (int64_t)dim, p, gout, gx, (hipStream_t)stream));
    return KGE_OK;
}

int kge_mask_diag(float *x, int C, int chunk, int Np, void *stream) {
    if (!x || C < 0 || chunk < 0 || Np <= 0) return fail(KGE_ERR_ARG, "kge_mask_diag: bad argument");
    KGE_TRY(launch_mask_diag(x, C, chunk, Np, (hipStream_t)stream));
    return KGE_OK;
}

int kge_rank_from_scores(const float *neg, const float *pos, const float *bias, int64_t E, int64_t N, int64_t *ranks, void *stream) {
    if ((E && (!neg || !pos || !ranks)) || E < 0 || N < 0 || N >= (1 << 24)) return fail(KGE_ERR_ARG, "kge_rank_from_scores: bad argument");
    KGE_TRY(launch_rank_mask(neg, pos, bias, E, N, ranks, (hipStream_t)stream));
    return KGE_OK;
}

int kge_adagrad_apply_packed(float *table, float *state_sum, int64_t n_rows, int dim,
                             const int64_t *idx, const float *msg, int ld, int64_t n, int ntraces,
                             float lr, float eps, void *stream) {
    if (!table || !state_sum || (n && !msg) || dim <= 0 || n_rows < 0 || ntraces < 1 ||
        ld < ntraces * dim + ntraces + (idx ? 0 : 2))
        return fail(KGE_ERR_ARG, "kge_adagrad_apply_packed: bad argument");
    KGE_TRY(launch_adagrad_apply_packed(table, state_sum, dim, idx, msg, ld, n, ntraces, lr, eps, (hipStream_t)stream));
    return KGE_OK;
}

int kge_adagrad_apply_rows(float *table, float *state_sum, int64_t n_rows, int dim,
                           const int64_t *idx, const float *g, const float *gs, int64_t n, float lr,
                           float eps, void *stream) {
    if (!table || !state_sum || (n && (!idx || !g || !gs)) || dim <= 0 || n_rows < 0)
        return fail(KGE_ERR_ARG, "kge_adagrad_apply_rows: bad argument");
    KGE_TRY(launch_adagrad_apply_rows(table, state_sum, dim, idx, g, gs, n, lr, eps, (hipStream_t)stream));
    return KGE_OK;
}

// ------------------------------------------------------------------------------------------
// fused step
// ------------------------------------------------------------------------------------------
// phases of one step.  The strict step runs all three back to back on one stream; the --async_update pipeline
// (kge_step_async) runs PREP(s) | SCORE(s) on the caller's stream and UPDATE(s-1) on its side stream in between.
enum { PH_PREP = 1, PH_FWD = 2, PH_BWD = 16, PH_SCORE = 18, PH_UPD_ENT = 4, PH_UPD_REL = 8, PH_UPDATE = 12, PH_ALL = 31,
       PH_STRICT = 32 };   // PH_STRICT: the phases belong to a strict step issued in pieces (kge_step_phase): table reads stay
                           // table reads (no dense copies), exactly the kernels of PH_ALL

// what a call of the step driver (run_step) does beyond the plain strict step; each entry point sets only what it uses
struct StepCall {
    const kge_emit *emit = nullptr;          // gradient emission instead of the entity update (kge_step_grads)
    const kge_shards *sh = nullptr;          // peer-to-peer sharded tables (kge_step_sharded)
    int phases = PH_ALL;
    UpdateArgs *build_update = nullptr;      // PH_UPD_*: fill the launch arguments instead of launching
    const UpdateArgs *co_update = nullptr;   // PH_FWD: another step's update to run alongside the forward
    EdgeFwdArgs *build_prep = nullptr;       // PH_PREP: fill the launch arguments instead of launching
    const EdgeFwdArgs *co_prep = nullptr;    // PH_BWD: the NEXT step's PREP to run alongside the backward
    const SmpTail *tail = nullptr;           // the sampler job this step's launches carry as tail workgroups
    const kge_known *known = nullptr;        // known triples left out of the negatives (kge_step_*_known): PH_FWD builds the pair mask
    uint32_t *known_mask = nullptr;          // ... into this buffer of the caller's, and the stand-alone loss kernel reads it
    size_t known_mask_bytes = 0;
    const AdamArgs *adam = nullptr;          // the update launch is the Adam form (kge_step_optim, KGE_OPT_ADAM)
    const char *who = "kge_step_fused";      // the entry, as the refusals of the norm-constraint flags name it
};

static StepCall phase_call(int phases, const char *who = nullptr) {
    StepCall c; c.phases = phases;
    if (who) c.who = who;
    return c;
}

// every buffer of one step's workspace.  carve_step is the only description of the layout: kge_step_workspace_bytes measures
// with it, the step carves with it.  The layout depends on (hp, B, C, chunk, N, UE, UR, copies) alone - not on the outputs asked,
// emission, sharding or the phase mask - so the phase calls of one step agree on every pointer.
struct StepBufs {
    float *A, *Bn, *asq, *bsq, *P, *dP, *S, *PM, *PS, *PL, *GA, *GN, *GH, *GT, *GR;
    float *RV, *RC1, *RC2, *Rgs, *Rstd, *Rreg, *Rpp;                                // RESCAL
    float *Xd; int64_t *iota, *ndids;                                               // RESCAL / TransR
    float *HP, *TP, *Q, *SG, *DQ, *TR1, *TR2, *GP, *gs0, *gs1, *k0, *k1, *TGNp, *gs1p; signed char *Z;   // TransR
    float *row_pos, *row_neg, *reg_ent, *reg_rel, *GNp, *Hc, *Tc, *Rc;
    OwnBufs own;                                                                    // PairRE, TransH, TransD (kge_own_fwd.hpp)
};

// Ns: the SAMPLED negatives per chunk (kge_batch.N).  copies: room for PREP's dense h / t / r rows (the async pipeline)
static size_t carve_step(Carver &cv, StepBufs &w, const kge_hparams *hp, int B_, int C, int chunk, int Ns, int UE, int UR, bool copies) {
    w = StepBufs{};
    const bool nd = (hp->flags & KGE_FLAG_NEG_DEG_SAMPLE) != 0;
    const int N = nd ? chunk + Ns : Ns;                   // neg_deg_sample: the chunk's own positives join its negatives
    const size_t B = B_, d_e = hp->d_e, d_r = hp->d_r, CN = (size_t)C * N, tj16 = (N + 15) / 16;
    const bool rescal = hp->model == KGE_RESCAL, transr = hp->model == KGE_TRANSR;
    w.A = cv.f(B * d_e); w.Bn = cv.f(CN * d_e);           // pos-side vectors; dense negative rows (pairwise kernels, dense-negative modes)
    w.asq = cv.f(B); w.bsq = cv.f(CN);
    w.P = cv.f(B); w.dP = cv.f(B);                        // positive score, dL/dp
    w.S = cv.f(B * (size_t)N);                            // scores, then dL/dn in place
    w.PM = cv.f(B * tj16); w.PS = cv.f(B * tj16); w.PL = cv.f(B * tj16);   // per-(row, 16-column tile) partials: max / sum-exp / loss
    // the shared-pair backward of RotatE / TransE_l1 leaves GA in up to 8 parts (neg_bwd_lc_splits; 1 for every other model)
    w.GA = cv.f(B * d_e * (size_t)(!(hp->flags & KGE_FLAG_TWO_PASS_PAIR) ? neg_bwd_lc_splits(hp->model, C, chunk, N, hp->d_e) : 1));
    w.GN = cv.f(CN * d_e);
    w.GH = cv.f(B * d_e); w.GT = cv.f(B * d_e);           // GH doubles as the P rows of the TransE fast path
    if (rescal) {      // V = M t, parts of M^T h and M^T GA per row block (no [B, d_r] buffer) + update scratch
        w.RV = cv.f(B * d_e); w.RC1 = cv.f(B * d_e * RESCAL_RBN); w.RC2 = cv.f(B * d_e * RESCAL_RBN);
        w.Rgs = cv.f(B * RESCAL_RB); w.Rstd = cv.f(UR);
        w.Rreg = cv.f((size_t)UR * (RESCAL_RB > RESCAL_RBN ? RESCAL_RB : RESCAL_RBN)); w.Rpp = cv.f(B * RESCAL_RBN);
    } else w.GR = cv.f(B * d_r);
    if (transr || rescal) {      // sharded entity tables: dense [h | t | negative] rows + identity ids
        w.Xd = cv.f((2 * B + CN) * d_e); w.iota = cv.i64(2 * B + CN);
    }
    if (transr && nd) w.ndids = cv.i64(CN);               // neg_deg_sample: the combined [own | sampled] id list
    if (transr) {      // projections, q, signs, dq; P s, P dq; sign bytes; per-edge projection gradients
        w.HP = cv.f(B * d_r); w.TP = cv.f(B * d_r); w.Q = cv.f(B * d_r); w.SG = cv.f(B * d_r); w.DQ = cv.f(B * d_r);
        w.TR1 = cv.f(B * d_e); w.TR2 = cv.f(B * d_e);
        w.Z = (signed char *)cv.f((B * N * d_r + 3) / 4);
        w.GP = cv.f(B * d_e * d_r);
        w.gs0 = cv.f(B); w.gs1 = cv.f(B); w.k0 = cv.f(UR); w.k1 = cv.f(UR);
        w.TGNp = cv.f((size_t)TRANSR_GN_GROUPS_WIDE * CN * d_e);
        w.gs1p = cv.f(B * ((d_e + 63) / 64) * ((d_r + 63) / 64));   // sum of squares per 64 x 64 tile of the projection gradients
    }
    w.row_pos = cv.f(B); w.row_neg = cv.f(B); w.reg_ent = cv.f(UE); w.reg_rel = cv.f(UR);
    if (neg_bwd_lc_supported(hp->model, hp->d_e))         // TransE_l1 / RotatE: GN partials of the shared-pair backward
        w.GNp = cv.f(neg_bwd_lc_partial_floats(hp->model, C, chunk, N, hp->d_e));
    if (copies) { w.Hc = cv.f(B * d_e); w.Tc = cv.f(B * d_e); w.Rc = cv.f(B * d_r); }
    kge::own_carve(hp->model, cv, w.own, w.A, w.asq, w.bsq, w.GA, B, CN, (size_t)N, d_e);
    return cv.off;
}

size_t kge_step_workspace_bytes(const kge_hparams *hp, int B, int C, int chunk, int N, int UE, int UR) {
    Carver cv; StepBufs w; return carve_step(cv, w, hp, B, C, chunk, N, UE, UR, false);
}

// ---- known triples left out of the negatives (kge_known.hip) ----
size_t kge_known_mask_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return (size_t)B * (size_t)((N + 31) / 32) * sizeof(uint32_t);
}

static int check_known(const kge_known *k, const uint32_t *mask, size_t mask_bytes, int B, int N) {
    if (k->n_rel <= 0 || k->m_tail < 0 || k->m_head < 0 || (k->m_tail > 0 && (!k->keys_tail || !k->vals_tail)) ||
        (k->m_head > 0 && (!k->keys_head || !k->vals_head)))
        return fail(KGE_ERR_ARG, "kge_known: n_rel > 0 and both sorted sides (keys, vals, m >= 0) are required");
    if (!mask || mask_bytes < kge_known_mask_bytes(B, N))
        return fail(KGE_ERR_ARG, "kge_known: the mask buffer is missing or smaller than kge_known_mask_bytes(B, N) (%zu < %zu)", mask_bytes,
                    kge_known_mask_bytes(B, N));
    return KGE_OK;
}

static KnownMaskArgs known_args(const kge_batch *b, const kge_known *k, uint32_t *mask) {
    KnownMaskArgs a{};
    a.B = b->B; a.chunk = b->chunk; a.N = b->N; a.neg_head = b->neg_head;
    a.h = b->h_gid; a.r = b->rel_ids; a.t = b->t_gid; a.neg = b->neg_ids; a.counts_dev = b->counts_dev;
    a.keys[0] = k->keys_tail; a.vals[0] = k->vals_tail; a.m[0] = k->m_tail;
    a.keys[1] = k->keys_head; a.vals[1] = k->vals_head; a.m[1] = k->m_head;
    a.n_rel = k->n_rel; a.mask = mask;
    return a;
}

int kge_known_neg_mask(const kge_batch *b, const kge_known *known, uint32_t *mask, size_t mask_bytes, void *stream) {
    if (!b || !known) return fail(KGE_ERR_ARG, "kge_known_neg_mask: null argument");
    if (b->B <= 0 || b->C <= 0 || b->chunk <= 0 || b->N <= 0 || (int64_t)b->C * b->chunk != b->B)
        return fail(KGE_ERR_ARG, "kge_known_neg_mask: need C*chunk == B (B=%d C=%d chunk=%d)", b->B, b->C, b->chunk);
    if (!b->h_gid || !b->t_gid || !b->rel_ids || !b->neg_ids) return fail(KGE_ERR_ARG, "kge_known_neg_mask: null batch pointer");
    if (int rc = check_known(known, mask, mask_bytes, b->B, b->N)) return rc;
    KGE_TRY(launch_known_mask(known_args(b, known, mask), (hipStream_t)stream));
    return KGE_OK;
}

// every path decision of one step call, from its inputs alone
struct StepPlan {
    int N, CN;                 // negative rows per chunk / per batch as the scoring, loss and gradient kernels see them
    bool nd, reg, pos_row, is_l2, transr, rescal, own, rescal_rel, sh_dense, pipelined, want4;   // own: an edge forward of its own (kge_own_fwd.hpp)
    bool gemm, fused_loss, transe_fast, qfuse, need_cp, dense_neg, l2g, merged_fwd, merged_pair, fold_loss, dense_bwd;
    bool ew_bwd, lc, fuse_gnred, fold_upd; int ga_parts, fold_nrw;
};

static StepPlan plan_step(const kge_hparams *hp, const kge_batch *b, const kge_step_out *out, const StepCall &c) {
    StepPlan p{};
    const unsigned fl = hp->flags; const kge_shards *sh = c.sh;
    const int model = hp->model, d_e = hp->d_e, d_r = hp->d_r, C = b->C, chunk = b->chunk, phases = c.phases;
    // neg_deg_sample: the scoring / loss / gradient kernels see N = chunk + (sampled negatives) rows per chunk; the
    // plan of the batch keeps indexing the sampled ones (b->N)
    p.nd = (fl & KGE_FLAG_NEG_DEG_SAMPLE) != 0;
    const int N = p.N = p.nd ? chunk + b->N : b->N; p.CN = C * N;
    p.reg = hp->reg_coef > 0.f && hp->reg_norm > 0; p.pos_row = loss_pos_row(hp->loss_genre, hp->pairwise) != 0; p.want4 = out && out->loss4;
    p.is_l2 = model == KGE_TRANSE_L2; p.transr = model == KGE_TRANSR; p.rescal = model == KGE_RESCAL;
    p.own = kge::model_row(model)->own_fwd;
    p.rescal_rel = p.rescal && d_e % 4 == 0;         // RESCAL's passes over M per unique relation (16-byte accesses)
    p.sh_dense = sh && (p.transr || p.rescal);       // the two families run on a dense block of the batch's entity rows (Step::setup)
    p.pipelined = phases != PH_ALL && !(phases & PH_STRICT);      // the async pipeline (kge_step_async)
    p.gemm = use_mfma(model, d_e, N, fl);            // matrix-core negative scoring
    // KGE_FLAG_FUSED_LOSS (matrix-core path, pointwise criteria): no loss kernel - the forward tiles emit the factorised gradient
    // (kge_neg_gemm.hip).  4 launches per step instead of 5, 1.6 MB less traffic, but measured 41.7 vs 41.1 us per step at cfg-T
    // (profiles/r02_fused_loss_experiment.txt), so it is opt-in.  (RESCAL has no edge_fwd: its positive-loss part lives in the loss kernel)
    p.fused_loss = p.gemm && !p.pos_row && !p.nd && !p.rescal && model != KGE_QUATE && (fl & KGE_FLAG_FUSED_LOSS) &&
                   neg_gemm_fused_loss_supported(chunk, N);
    const bool transe = model == KGE_TRANSE_L1 || p.is_l2;
    // TransE fast path: edge_fwd leaves P rows, the update rebuilds the per-edge gradients from them (no edge_bwd launch)
    p.transe_fast = transe && !p.pos_row && !p.nd && d_e % 4 == 0 && d_r % 4 == 0 && (d_e > d_r ? d_e : d_r) <= 1024 && !(fl & KGE_FLAG_NO_TRANSE_FAST);
    // ... behind the matrix-core backward: its GA epilogue also writes Q = GA +/- P (into the GT buffer, unused on this path)
    // and the update reads one gradient row per list entry (GemmArgs::Q)
    p.qfuse = p.transe_fast && p.gemm;
    // async pipeline: dense copies of the h / t / r rows as PREP gathered them, for the kernels that read them again after
    // the previous step's update has started (edge_bwd)
    p.need_cp = p.pipelined && (!p.transe_fast || p.reg || (out && out->g_rel));
    // the scoring kernels read the dense copy Bn of the negative rows.  Sharded tables: they re-read the rows many times - never
    // from the (remote, uncached) table.  Async pipeline: everything after PREP must read the rows as PREP gathered them (the
    // previous step's update is changing the tables meanwhile)
    p.dense_neg = !p.gemm || sh || p.pipelined || p.nd || (fl & KGE_FLAG_DENSE_NEG);
    p.l2g = p.gemm && p.is_l2;                       // GEMM form of the L2 distance needs |a|^2, |b|^2
    // PREP and the forward of a strict step can share ONE launch: not in the async pipeline (its forward shares a launch with
    // the previous update already), only when this call runs both and launches both itself
    const bool one_fwd = !p.pipelined && !p.pos_row && (phases & (PH_PREP | PH_FWD)) == (PH_PREP | PH_FWD) && !c.build_prep &&
                         !c.co_update && !(fl & KGE_FLAG_SPLIT_FWD);
    // edge-forward and the forward GEMM in one launch (kge_neg_gemm.hip, neg_fwd_edge_kernel): the tiles build their pos-side
    // fragments from the table rows themselves and emit raw products, the loss kernel applies the TransE_l2 distance transform.
    // 4 launches per TransE_l2 step instead of 5.  Not for the dense-negative modes (sharded / neg_deg_sample) and the fused-loss variant.
    p.merged_fwd = p.gemm && !p.dense_neg && !p.fused_loss && one_fwd && neg_fwd_gemm_with_edge_supported(model, d_e, d_r) &&
                   !(model == KGE_COMPLEX && (fl & KGE_FLAG_FWD_DIRECT));
    // ... and the pairwise family's TransE_l1: its forward tasks build the uniform rows x +/- r themselves and gather the negative
    // rows through neg_ids; the edge half writes the dense copies (A, Bn) the backward kernels read
    p.merged_pair = !p.gemm && !p.nd && !sh && !p.rescal && !p.transr && one_fwd && neg_fwd_bcast_with_edge_supported(model, d_e, d_r);
    // KGE_FLAG_LOSS_IN_FWD: ... and LossGenerator too - the forward tiles store final scores and the workgroup of a 16-row
    // strip that arrives last runs the strip's loss rows (kge_neg_gemm.hip, neg_fwd_loss_edge_kernel): 3 launches per TransE_l2 /
    // DistMult / ComplEx step.  Needs the caller's ticket words (kge_step_out.tickets); pointwise criteria; |a|^2 and |b|^2 of the
    // TransE_l2 distance are then computed by the tiles, not by the edge half.  Opt-in: slower than the loss launch on MI355X
    // (profiles/r04_loss_fold.txt).
    p.fold_loss = p.merged_fwd && out && out->tickets && (fl & KGE_FLAG_LOSS_IN_FWD) && !(fl & KGE_FLAG_FWD_DIRECT) &&
                  neg_fwd_loss_fold_supported(model, C, chunk, N, d_e, d_r);
    // KGE_FLAG_DENSE_BWD: the merged launch's edge half also writes the dense copy of the negative rows and the backward GEMM
    // reads that (no id round).  Measured equal to gathering through neg_ids (profiles/r03_merged_fwd.txt) at +1.6 MB of writes: opt-in
    p.dense_bwd = p.merged_fwd && (fl & KGE_FLAG_DENSE_BWD);
    // DistMult / ComplEx / SimplE, strict step on local tables: the GA tiles of the backward GEMM write the per-edge gradient rows
    // in their epilogue (GemmArgs::ew_*) - no edge_bwd launch (5 -> 4 launches per step)
    p.ew_bwd = p.gemm && ((model == KGE_DISTMULT && d_e % 4 == 0) || ((model == KGE_COMPLEX || model == KGE_SIMPLE) && d_e % 8 == 0)) &&
               !p.pipelined && !c.co_prep && !p.nd && !sh && !p.fused_loss && !p.qfuse && d_r == d_e &&
               !(fl & KGE_FLAG_NO_TRANSE_FAST);      // (the flag that keeps TransE on edge_bwd keeps DistMult there too)
    p.ga_parts = 1;
    if (p.gemm || p.transr) return p;
    // ---- the pairwise kernels' backward (they always read the dense copy Bn: no gathered negatives) ----
    // shared-pair kernel (one pair evaluation feeds GA and GN, GN in per-row-group partials); else the two-pass kernels
    p.lc = neg_bwd_lc_supported(model, d_e) && !(fl & KGE_FLAG_TWO_PASS_PAIR);
    const int parts = (fl & KGE_FLAG_TWO_PASS_PAIR) ? 1 : neg_bwd_lc_splits(model, C, chunk, N, d_e);
    // shared-pair backward followed by edge_bwd: the sum of its GN partials shares the edge_bwd launch (same inputs' producer,
    // independent jobs).  Not with neg_deg_sample (edge_bwd reads GN) and not on the TransE fast path (no edge_bwd).  On
    // peer-to-peer sharded tables too - edge_bwd resolves its rows through the shard map, the reduction is local
    p.fuse_gnred = p.lc && !p.nd && !p.transe_fast && !p.rescal && d_e % 4 == 0 && N % 4 == 0 &&
                   (model == KGE_ROTATE || model == KGE_TRANSE_L1) && !(fl & KGE_FLAG_SPLIT_FWD);
    // TransE_l1 (fast path: no edge_bwd launch to share): the update kernel sums the GN partials and GA parts itself - the
    // stand-alone reduction launch (5.2 us + a boundary) leaves the strict step.  One-call strict step on local tables, no
    // gradient outputs (they read the summed buffers).
    p.fold_nrw = neg_bwd_lc_nrw(model, C, chunk, d_e);
    // (Adam: the stand-alone reduction launch - the Adam instances read summed GN / GA rows, there is no folded Adam instance)
    p.fold_upd = !c.adam && phases == PH_ALL && p.lc && p.transe_fast && model == KGE_TRANSE_L1 && !p.nd && !sh && !c.emit && !c.build_update &&
                 !c.co_update && !c.co_prep && !(out && (out->g_neg || out->g_rel || out->g_pos_ent)) && d_e % 4 == 0 && d_e <= 512 &&
                 N % 4 == 0 && p.fold_nrw <= 6 && parts <= 4 && !(fl & KGE_FLAG_SPLIT_FWD) && (!p.reg || hp->reg_norm == 3);
    // GA in parts only where the shared-pair kernel runs: its stand-alone partial reduction adds them up in place, the
    // edge_bwd launch that carries the reduction (fuse_gnred) adds them while it reads the row
    if (parts > 1 && p.lc && N % 4 == 0 && !p.rescal) p.ga_parts = parts;
    return p;
}

// one call of the step driver: the caller's arguments, the plan, the buffers and the argument blocks the phases share
struct Step {
    const kge_hparams *hp; const kge_tables *tb; const kge_batch *b; const kge_step_out *out; const StepCall &c; hipStream_t s;
    StepPlan p; StepBufs w;
    kge::ShardMap em, rm; EdgeSrc src;
    kge_tables tbd; kge_batch bd;                  // sh_dense: the dense block as tables / batch ...
    const kge_tables *tbx; const kge_batch *bx;    // ... what the TransR / RESCAL kernels read
    float *P, *GN, *GR, *acc;                      // workspace buffers or the caller's outputs
    LossParams lp; float rot_div;
    TransRArgs tr; EdgeFwdArgs ef; GemmArgs g; NegArgs na;
    int setup(void *ws, size_t ws_bytes), phase_prep(), prep_transr(), prep_rescal(), phase_fwd(), fwd_gemm(), phase_bwd(), bwd_neg_gemm();
    int bwd_transr(), bwd_rescal(), phase_update(); void fill_score(), fill_step_loss(LossArgs &la);
    OwnBlock own_block() const { return OwnBlock{b->C, b->chunk, p.N, hp->d_e, hp->gamma, w.own.o, w.Bn, nullptr, w.own.PQ}; }
};

// argument checks, then the plan, the workspace and the argument blocks every phase shares
int Step::setup(void *ws, size_t ws_bytes) {
    const kge_shards *sh = c.sh;
    if (!hp || !tb || !b || !ws) return fail(KGE_ERR_ARG, "kge_step: null argument");
    // (ABI 8: rel_local = relation-side tables local to this rank, relation partitioning)
    if (sh && (sh->n_shards < 1 || sh->ent_rows_per_shard <= 0 || !sh->ent_rows || !sh->ent_state || (sh->rel_local && !sh->rel_state_local) ||
               (!sh->rel_local && (sh->rel_rows_per_shard <= 0 || !sh->rel_rows || !sh->rel_state))))
        return fail(KGE_ERR_ARG, "kge_step_sharded: bad shard map");
    if (int rc = check_model(hp->model, hp->d_e, hp->d_r)) return rc;
    if (int rc = check_norm(hp, c.who)) return rc;
    // the relation-matrix models in the gradient-emitting step: only with the relation side applied IN PLACE (emit->gr NULL, the
    // all-to-all engine under relation partitioning).  Their kernels run against the row cache like every model's, the relation
    // matrices / projection rows of the batch belong to this rank and are updated here, only entity messages leave
    if (hp->model == KGE_RESCAL && ((c.emit && c.emit->gr) || (sh && !sh->rel_local)))
        return fail(KGE_ERR_ARG, "RESCAL: the gradient-emitting step needs the relation trace in place (emit.gr NULL: relation partitioning); "
                                 "on sharded tables it needs kge_shards.rel_local (ABI 8)");
    if (b->B <= 0 || b->C <= 0 || b->chunk <= 0 || b->N <= 0 || (int64_t)b->C * b->chunk != b->B)
        return fail(KGE_ERR_ARG, "kge_step: need C*chunk == B (B=%d C=%d chunk=%d)", b->B, b->C, b->chunk);
    if (int rc = check_loss(hp->loss_genre, hp->adv, hp->pairwise)) return rc;
    if ((!sh && (!tb->ent || !tb->ent_state || !tb->rel || !tb->rel_state)) || !b->h_gid || !b->t_gid || !b->rel_ids || !b->neg_ids ||
        !b->ue_id || !b->ue_pos_ptr || !b->ue_pos_adj || !b->ue_neg_ptr || !b->ue_neg_slot || !b->ur_id || !b->ur_ptr || !b->ur_edge ||
        !b->ue_rec || !b->ur_rec)
        return fail(KGE_ERR_ARG, "kge_step: null table / batch pointer");
    // neg_deg_sample in the gradient-emitting step: the in-batch rows' gradients join the row's positive-trace message g0 through
    // edge_bwd, the sampled rows' the negative-trace message g1 through the update's slot remap, exactly as in the fused step.
    // TransR and RESCAL too - the reference's concat-and-mask sits in front of head_neg_prepare / tail_neg_prepare,
    // general_models.py:396-402, 417-432: model-agnostic.  Not on sharded tables / in the gradient-emitting step.
    if ((hp->flags & KGE_FLAG_NEG_DEG_SAMPLE) && (hp->model == KGE_RESCAL || hp->model == KGE_TRANSR) && (sh || c.emit))
        return fail(KGE_ERR_ARG, "neg_deg_sample for RESCAL / TransR: single-table step only");
    if (sh) {
        em = kge::ShardMap{sh->ent_rows, sh->ent_state, sh->ent_rows_per_shard, sh->n_shards};
        if (!sh->rel_local) rm = kge::ShardMap{sh->rel_rows, sh->rel_state, sh->rel_rows_per_shard, sh->n_shards};
    }
    p = plan_step(hp, b, out, c);
    Carver cv(ws, ws_bytes);
    const size_t need = carve_step(cv, w, hp, b->B, b->C, b->chunk, b->N, b->UE, b->UR, p.pipelined);
    // ---- TransR / RESCAL on peer-to-peer sharded ENTITY tables (ABI 8; the reference trains TransR on 8 GPUs with
    // --rel_part, examples/freebase/multi_gpu.sh:80-89).  Their kernels address `table + id * width`; here the batch's entity rows
    // are first gathered through the shard map into ONE dense block [h rows | t rows | negative rows] and the kernels run on that
    // block with identity index arrays - no kernel of the two families changes.  The relation-side tables (relation rows /
    // matrices, TransR's projection table) are local to the rank (kge_shards.rel_local: relation partitioning); the entity update
    // goes through the shard map by global id like every other model's.
    tbx = tb; bx = b;
    if (p.sh_dense) {
        tbd = *tb; bd = *b;
        tbd.ent = w.Xd; tbd.ent_state = nullptr; tbd.n_ent = 2 * b->B + b->C * b->N;
        tbd.rel = sh->rel_local; tbd.rel_state = sh->rel_state_local; tbd.n_rel = sh->n_rel;
        tbd.proj = sh->proj_local; tbd.proj_state = sh->proj_state_local;
        bd.h_gid = w.iota; bd.t_gid = w.iota + b->B; bd.neg_ids = w.iota + 2 * b->B;
        tbx = &tbd; bx = &bd;
    }
    if (p.transr) {
        if (c.emit && c.emit->gr) return fail(KGE_ERR_ARG, "TransR: the gradient-emitting step needs the relation trace in place (emit.gr NULL: relation partitioning)");
        if (sh && !sh->rel_local) return fail(KGE_ERR_ARG, "TransR on sharded tables needs kge_shards.rel_local / proj_local (ABI 8)");
        if (!tbx->proj || !tbx->proj_state) return fail(KGE_ERR_ARG, "TransR needs kge_tables.proj / proj_state");
    }
    if (c.emit && c.emit->msg_rows) {
        // packed single-trace messages are written by the register-resident update kernel alone (launch_update sends every other
        // width to the generic update_kernel, which knows the two-trace layouts only) - refused here, before the first launch
        const int dr_u = p.rescal ? hp->d_e : hp->d_r;
        if (hp->d_e % 4 != 0 || dr_u % 4 != 0 || (hp->d_e > dr_u ? hp->d_e : dr_u) > 1024)
            return fail(KGE_ERR_ARG, "kge_step_grads: packed messages (emit.msg_rows) need row widths that are multiples of 4 and at most "
                                     "1024 floats (d_e=%d d_r=%d); use the two-trace messages", hp->d_e, hp->d_r);
        if (!c.emit->g0 || c.emit->ld_e < hp->d_e + 4 || c.emit->msg_cap < 1 || c.emit->msg_cap_extra < 1)
            return fail(KGE_ERR_ARG, "kge_step_grads: packed messages need g0, ld_e >= d_e + 4 and the bucket geometry");
    }
    if (c.emit && out && out->g_pos_ent && (c.emit->ld_e > 0 || c.emit->ent_by_id))
        return fail(KGE_ERR_ARG, "g_pos_ent output cannot be combined with a strided emit or with messages addressed by row id");
    if (need > ws_bytes) return fail(KGE_ERR_WORKSPACE, "kge_step: workspace too small (%zu < %zu)", ws_bytes, need);
    if (c.known) {
        // the known pairs are taken out by the STAND-ALONE loss kernel: every step form whose loss runs elsewhere is refused, and so is
        // neg_deg_sample (its in-batch columns are positives of the chunk by construction: the two do not combine)
        if (hp->flags & (KGE_FLAG_FUSED_LOSS | KGE_FLAG_LOSS_IN_FWD))
            return fail(KGE_ERR_ARG, "known-triple exclusion: KGE_FLAG_FUSED_LOSS / KGE_FLAG_LOSS_IN_FWD run the loss outside the stand-alone kernel");
        if (p.nd) return fail(KGE_ERR_ARG, "known-triple exclusion: not available with KGE_FLAG_NEG_DEG_SAMPLE");
        if (sh || c.emit || p.pipelined)
            return fail(KGE_ERR_ARG, "known-triple exclusion: strict single-table step only (no gradient emission, sharding or async pipeline)");
        if (int rc = check_known(c.known, c.known_mask, c.known_mask_bytes, b->B, b->N)) return rc;
    }
    if (p.pipelined && (sh || c.emit || p.transr || p.rescal))
        return fail(KGE_ERR_ARG, "kge_step_async: not available for RESCAL / TransR and the sharded / gradient-emitting steps");
    // a batch of the NEXT group is built by tail workgroups of this step's first, backward and update launches
    // (kge_sampler_tail.hpp) - the one-call strict step of the matrix-core family in its 4-launch form
    if (c.tail && !(p.merged_fwd && !p.fold_loss && p.gemm && c.phases == PH_ALL && !c.co_prep && !c.co_update && !c.build_update &&
                    !c.build_prep && !p.transr && !p.rescal && hp->d_e % 4 == 0 && hp->d_r % 4 == 0 &&
                    (hp->d_e > hp->d_r ? hp->d_e : hp->d_r) <= 1024))
        return fail(KGE_ERR_ARG, "kge_step_fused_sampling: this step's launches cannot carry the sampler (matrix-core models, strict "
                                 "4-launch step on local tables only)");
    P = (out && out->pos_score) ? out->pos_score : w.P; GN = (out && out->g_neg) ? out->g_neg : w.GN;
    GR = (out && out->g_rel && !p.transe_fast) ? out->g_rel : w.GR;
    acc = out ? out->loss_accum : nullptr;
    lp = LossParams{hp->loss_genre, hp->adv, p.pos_row ? 1 : 0, hp->adv_temp, hp->margin}; rot_div = rot_div_of(hp->emb_init);
    src = EdgeSrc{tb->ent, b->h_gid, tb->ent, b->t_gid, tb->rel, b->rel_ids, em, rm};
    if (p.transr) {
        tr.HP = w.HP; tr.TP = w.TP; tr.Q = w.Q; tr.SG = w.SG; tr.DQ = w.DQ; tr.Z = w.Z; tr.GP = w.GP;
        tr.gs0 = w.gs0; tr.gs1 = w.gs1; tr.k0 = w.k0; tr.k1 = w.k1; tr.GNp = w.TGNp; tr.gs1p = w.gs1p;
        tr.nG = transr_gn_groups(hp->d_e, hp->d_r, b->chunk, p.N);
        tr.B = b->B; tr.C = b->C; tr.chunk = b->chunk; tr.N = p.N; tr.De = hp->d_e; tr.Dr = hp->d_r; tr.neg_head = b->neg_head;
        tr.UR = b->UR; tr.reg_norm = hp->reg_norm; tr.gamma = hp->gamma; tr.lr = hp->lr; tr.eps = hp->eps; tr.reg_coef = p.reg ? hp->reg_coef : 0.f;
        tr.ent = tbx->ent; tr.h_gid = bx->h_gid; tr.t_gid = bx->t_gid; tr.neg_ids = bx->neg_ids; tr.rel_ids = b->rel_ids;
        tr.rel = tbx->rel; tr.proj = tbx->proj; tr.proj_state = tbx->proj_state; tr.P = P; tr.S = w.S; tr.GN = GN; tr.GR = GR; tr.dpos = w.dP;
        tr.ur_id = b->ur_id; tr.ur_ptr = b->ur_ptr; tr.ur_edge = b->ur_edge; tr.counts_dev = b->counts_dev;
        // neg_deg_sample: the kernels address the negatives through ONE id list - the combined [own | sampled] ids per chunk
        // (N = chunk + sampled; the update adds the sampled rows' regulariser)
        if (p.nd) { tr.neg_ids = w.ndids; tr.nd_chunk = b->chunk; }
    }
    return KGE_OK;
}

// ---- PREP: gather + positive score + pos-side vectors (+ positive-loss part, + P rows for TransE) ----
// TransR: hp = h P, tp = t P in one pass over every edge's projection matrix; then p, sign(u), q; then the
// batched projection of the chunk's negatives with the L1 epilogue (scores + sign bytes)
int Step::prep_transr() {
    if (p.nd) KGE_TRY(launch_nd_ids(b->neg_head ? b->h_gid : b->t_gid, b->neg_ids, b->C, b->chunk, b->N, w.ndids, s));
    RescalMatvecArgs m{};
    m.B = b->B; m.D = hp->d_e; m.Dc = hp->d_r; m.rel = tbx->proj; m.ridx = b->rel_ids;
    m.z1 = tbx->ent; m.z1idx = bx->h_gid; m.c1 = tr.HP;
    m.z2 = tbx->ent; m.z2idx = bx->t_gid; m.c2 = tr.TP;
    KGE_TRY(launch_rescal_matvec(m, s));
    KGE_TRY(launch_transr_pos(tr, s));
    KGE_TRY(launch_transr_fwd(tr, s));
    return KGE_OK;
}

// RESCAL: V = M t (always: p = h.V), A = M x with x = h in tail mode (then a second product of the same pass)
int Step::prep_rescal() {
    const int B = b->B, d_e = hp->d_e;
    if (!p.rescal_rel) {               // d_e not a multiple of 4: one pass over M per EDGE
        RescalMatvecArgs m{};
        m.B = B; m.D = d_e; m.rel = tbx->rel; m.ridx = b->rel_ids;
        m.y1 = tbx->ent; m.y1idx = bx->t_gid; m.r1 = b->neg_head ? w.A : w.RV;
        if (!b->neg_head) { m.y2 = tbx->ent; m.y2idx = bx->h_gid; m.r2 = w.A; }
        m.pd = tbx->ent; m.pdidx = bx->h_gid; m.p = P;
        KGE_TRY(launch_rescal_matvec(m, s));
    } else {      // one pass over M per UNIQUE relation of the batch; the row blocks' parts of p are added by a one-thread-per-edge launch
        RescalRelFwdArgs m{};
        m.B = B; m.D = d_e; m.UR = b->UR; m.rel = tbx->rel; m.ent = tbx->ent; m.hidx = bx->h_gid; m.tidx = bx->t_gid;
        m.ur_id = b->ur_id; m.ur_ptr = b->ur_ptr; m.ur_edge = b->ur_edge; m.counts_dev = b->counts_dev;
        m.V = b->neg_head ? w.A : w.RV; m.W = b->neg_head ? nullptr : w.A; m.ppart = w.Rpp; m.P = P;
        if (p.reg) {      // the regulariser's products ride on this pass (they live in the front of RC1, which the update's pass over
            //               the matrices overwrites only AFTER the traced rows' mean squares were taken from them)
            m.PV = w.RC1; m.PW = w.RC1 + (size_t)B * d_e; m.rho = w.RC1 + 2 * (size_t)B * d_e;
            m.reg_coef = hp->reg_coef; m.reg_norm = hp->reg_norm;
        }
        KGE_TRY(launch_rescal_rel_fwd(m, s));
    }
    if (p.dense_neg) {                 // pairwise fallback kernels read a dense copy of the negative rows
        EdgeFwdArgs nb{};
        nb.B = 0; nb.d_e = d_e; nb.d_r = d_e; nb.model = KGE_DISTMULT; nb.nbase = tbx->ent; nb.nidx = bx->neg_ids; nb.n_neg = p.CN; nb.Bn = w.Bn;
        if (p.nd) { nb.nd_own = b->neg_head ? b->h_gid : b->t_gid; nb.nd_chunk = b->chunk; nb.nd_Ns = b->N; }
        KGE_TRY(launch_edge_fwd(nb, s));
    }
    return KGE_OK;
}

int Step::phase_prep() {
    if (p.sh_dense) KGE_TRY(launch_gather3_sharded(em, hp->d_e, b->h_gid, b->t_gid, b->neg_ids, b->B, b->C * b->N, w.Xd, w.iota, s));
    // (ef is filled for every family: the merged launches of the forward carry it)
    fill_edge(ef, src, hp->model, b->B, hp->d_e, hp->d_r, b->neg_head, hp->gamma, rot_div);
    ef.pos_score = P; ef.A = w.A; ef.P = p.transe_fast ? w.GH : nullptr;      // TransE fast path: P rows reuse the GH buffer
    // ids of the rows the scoring kernels treat as negatives.  neg_deg_sample: [the chunk's own corrupted-side entities |
    // the sampled ids] per chunk - edge_fwd resolves that on the fly and writes the dense copy Bn every later kernel reads
    ef.nbase = tb->ent; ef.nidx = b->neg_ids; ef.n_neg = p.CN;
    if (p.nd) { ef.nd_own = b->neg_head ? b->h_gid : b->t_gid; ef.nd_chunk = b->chunk; ef.nd_Ns = b->N; }
    ef.Bn = (p.dense_neg || p.dense_bwd) ? w.Bn : nullptr;
    if (p.need_cp) { ef.Hc = w.Hc; ef.Tc = w.Tc; ef.Rc = w.Rc; }
    ef.asq = (p.l2g && !p.fold_loss) ? w.asq : nullptr; ef.bsq = (p.l2g && !p.fold_loss) ? w.bsq : nullptr;
    ef.do_pos_loss = p.pos_row ? 0 : 1; ef.lp = lp; ef.w = b->edge_w; ef.w_mean = b->edge_w_mean;
    ef.dpos = w.dP; ef.row_pos = p.want4 ? w.row_pos : nullptr; ef.acc = acc;
    if (p.transr) return prep_transr();
    if (p.rescal) return prep_rescal();
    if (p.own) {       // own edge forward: P, the operand, the dense negative rows and their scalars; the loss kernel takes the positive part
        const OwnCands cn{ef.nbase, ef.nidx, ef.n_neg, ef.nd_own, ef.nd_chunk, ef.nd_Ns, w.Bn};
        KGE_TRY(kge::own_prepare(hp->model, src, b->B, b->chunk, hp->d_e, b->neg_head, hp->gamma, P, w.own.o, &cn, s));
        return KGE_OK;
    }
    if (c.build_prep) { *c.build_prep = ef; return KGE_OK; }
    if (!p.merged_fwd && !p.merged_pair) KGE_TRY(launch_edge_fwd(ef, s));     // merged: launched together with the forward tiles
    return KGE_OK;
}

// the argument blocks of the negative scoring kernels, as the forward AND the backward of this step use them
void Step::fill_score() {
    if (p.transr) return;
    if (p.gemm) {
        fill_gemm(g, hp->model, b->C, b->chunk, p.N, hp->d_e, hp->gamma, w.A, p.dense_neg ? w.Bn : tb->ent, p.dense_neg ? nullptr : b->neg_ids);
        g.S = w.S; g.adv_temp = hp->adv_temp; g.asq = w.asq; g.bsq = w.bsq;
        g.lp = lp; g.w = b->edge_w;
        if (p.fused_loss) { g.PM = w.PM; g.PS = w.PS; g.PL = w.PL; g.Sraw = out ? out->neg_score : nullptr; }
    } else {
        fill_pair(na, hp->model, b->C, b->chunk, p.N, hp->d_e, hp->gamma, w.A, w.Bn, nullptr);
        na.S = w.S;
    }
}

// the step's criterion: in place over the scores S, dL/dp into dP
void Step::fill_step_loss(LossArgs &la) {
    fill_loss(la, lp, b->B, p.N, P, w.S, b->edge_w, w.dP, w.S);
    la.w_mean = b->edge_w_mean; la.acc = acc; la.row_neg = p.want4 ? w.row_neg : nullptr;
    la.l2_scale = p.is_l2 ? 1 : 0; la.gamma = hp->gamma; la.clampv = clamp_of(hp->model);
    la.neg_copy = out ? out->neg_score : nullptr;
}

// ---- FWD: chunked negative scores, then the criterion ----
int Step::fwd_gemm() {
    bool fused_launch = false;
    if (c.co_update) {                  // async pipeline: forward GEMM(s) + update(s-1) in ONE launch
        const int rc = launch_neg_fwd_gemm_with_update(g, *c.co_update, s);
        if (rc == KGE_OK) fused_launch = true;
        else if (rc != KGE_ERR_ARG) return fail(rc, "launch_neg_fwd_gemm_with_update failed (%d)", rc);
        else KGE_TRY(launch_update(*c.co_update, s));      // no fused instantiation: one after the other
    }
    if (!p.merged_fwd) {
        if (!fused_launch) KGE_TRY(launch_neg_fwd_gemm(g, s));
        return KGE_OK;
    }
    g.xbase = tb->ent; g.xidx = b->neg_head ? b->t_gid : b->h_gid; g.rbase = tb->rel; g.ridx = b->rel_ids;
    g.asign = b->neg_head ? -1.f : 1.f; g.lds_off = (hp->flags & KGE_FLAG_FWD_DIRECT) ? 1 : 0;
    if (p.fold_loss) {
        LossArgs la; fill_step_loss(la); la.skip_pos = 1;          // (pointwise; row_pos: written by the edge half)
        KGE_TRY(launch_neg_fwd_gemm_with_edge_loss(g, ef, la, out->tickets, s));
    } else KGE_TRY(launch_neg_fwd_gemm_with_edge(g, ef, s, c.tail));
    return KGE_OK;
}

int Step::phase_fwd() {
    if (p.transr) {                               // scores already in S (PREP)
    } else if (p.gemm) {
        if (int rc = fwd_gemm()) return rc;
    } else {
        if (c.co_update) KGE_TRY(launch_update(*c.co_update, s));
        if (p.merged_pair) {
            NegArgs nf = na;                // the forward gathers the negatives from the table (Bn is written by this launch)
            nf.nbase = tb->ent; nf.nidx = b->neg_ids;
            nf.xbase = tb->ent; nf.xidx = b->neg_head ? b->t_gid : b->h_gid; nf.rbase = tb->rel; nf.ridx = b->rel_ids;
            nf.asign = b->neg_head ? -1.f : 1.f;
            KGE_TRY(launch_neg_fwd_bcast_with_edge(nf, ef, s));
        } else if (p.own) {
            KGE_TRY(kge::own_scores(hp->model, own_block(), w.S, s));
        } else KGE_TRY(launch_neg_fwd_pair(na, s));
    }
    if (p.fused_loss || p.fold_loss) return KGE_OK;  // no stand-alone loss kernel: the backward GEMM / the forward tiles run it
    if (c.known) KGE_TRY(launch_known_mask(known_args(b, c.known, c.known_mask), s));      // one extra launch ahead of the loss
    LossArgs la; fill_step_loss(la);
    la.row_pos = p.want4 ? w.row_pos : nullptr;
    if (p.merged_fwd && p.is_l2) { la.l2_raw = 1; la.l2_chunk = b->chunk; la.asq = w.asq; la.bsq = w.bsq; }
    la.skip_pos = (p.pos_row || p.rescal || p.transr || p.own) ? 0 : 1; la.diag_chunk = p.nd ? b->chunk : 0;  // RESCAL / TransR / own edge forward: no edge_fwd -> positive part here
    KGE_TRY(launch_loss(la, s, c.known ? c.known_mask : nullptr));
    return KGE_OK;
}

// ---- BWD: gradients w.r.t. the pos-side vectors and the negative rows, then the per-edge head / tail / relation rows ----
int Step::bwd_neg_gemm() {
    g.W = w.S; g.w = b->edge_w; g.lp = lp;      // fused loss: S holds u_ij and PM/PS/PL (fill_score) the partials
    if (p.dense_bwd) { g.nbase = w.Bn; g.nidx = nullptr; }
    g.GA = w.GA; g.GN = GN;
    if (p.qfuse) {                                // TransE: the update reads Q = GA +/- P, GA itself only on request (g_rel output)
        g.Q = w.GT; g.QP = w.GH; g.qc = b->neg_head ? 1.f : -1.f;
        if (!(out && out->g_rel)) g.GA = nullptr;
    }
    g.reg_coef = (p.reg && !p.nd) ? hp->reg_coef : 0.f; g.reg_norm = hp->reg_norm;   // nd: the update adds it (sampled rows only)
    g.row_neg = (p.fused_loss && p.want4) ? w.row_neg : nullptr;
    g.acc = p.fused_loss ? acc : nullptr;
    if (p.ew_bwd) {
        g.ew_ent = src.hbase; g.ew_rel = src.rbase; g.ew_h = src.hidx; g.ew_t = src.tidx; g.ew_r = src.ridx;
        g.ew_dpos = w.dP; g.ew_GH = w.GH; g.ew_GT = w.GT; g.ew_GR = GR;
        g.ew_reg_coef = p.reg ? hp->reg_coef : 0.f; g.ew_reg_norm = hp->reg_norm; g.ew_neg_head = b->neg_head;
        if (!(out && out->g_rel)) g.GA = nullptr;         // nobody reads GA itself then
    }
    if (c.co_prep) {                      // async pipeline: backward GEMM(s) + PREP(s+1) in ONE launch
        const int rc = launch_neg_bwd_gemm_with_prep(g, *c.co_prep, s);
        if (rc == KGE_OK) return KGE_OK;
        if (rc != KGE_ERR_ARG) return fail(rc, "launch_neg_bwd_gemm_with_prep failed (%d)", rc);
    }
    KGE_TRY(launch_neg_bwd_gemm(g, s, c.tail));
    if (c.co_prep) KGE_TRY(launch_edge_fwd(*c.co_prep, s));  // no fused instantiation: one after the other
    return KGE_OK;
}

// TransR: dq, GN, per-edge projection gradients, relation-vector gradients; then the entity gradients through the projections:
// GH = P (-dp s) (+ P dq, tail mode), GT = P (+dp s) (+ P dq, head mode)
int Step::bwd_transr() {
    const int B = b->B, d_e = hp->d_e;
    KGE_TRY(launch_transr_bwd(tr, s));
    RescalMatvecArgs m{};
    m.B = B; m.D = d_e; m.Dc = hp->d_r; m.rel = tbx->proj; m.ridx = b->rel_ids;
    m.y1 = tr.SG; m.r1 = w.TR1; m.y2 = tr.DQ; m.r2 = w.TR2;
    KGE_TRY(launch_rescal_matvec(m, s));
    KGE_TRY(launch_rescal_axpy(w.dP, w.TR1, b->neg_head ? nullptr : w.TR2, B, d_e, w.GH, s, -1.f));
    KGE_TRY(launch_rescal_axpy(w.dP, w.TR1, b->neg_head ? w.TR2 : nullptr, B, d_e, w.GT, s, 1.f));
    // neg_deg_sample: the in-batch negative rows are slices of the positive trace - their gradient joins GH (head mode) / GT
    if (p.nd) KGE_TRY(launch_nd_fold(GN, b->neg_head ? w.GH : w.GT, B, b->chunk, p.N, d_e, s));
    // projection table first: the entity update changes the h / t rows its rank-1 trace reads
    KGE_TRY(launch_transr_proj_update(tr, s));
    return KGE_OK;
}

// RESCAL: M^T h and M^T GA come out of the relation update's own pass over M (one per unique relation, row-block parts);
// GH = dp M t (+ M^T GA, tail mode), GT = dp M^T h (+ M^T GA, head mode) are combined after it;  the relation
// gradient stays factored.  (d_e not a multiple of 4: a pass over M per edge for the two products, then the update's own)
int Step::bwd_rescal() {
    const int B = b->B, d_e = hp->d_e;
    const float *Vr = b->neg_head ? w.A : w.RV;           // M t
    float *Gnd = b->neg_head ? w.GH : w.GT;               // neg_deg_sample: the in-batch negative rows' gradient joins this side
    if (!p.rescal_rel) {
        RescalMatvecArgs m{};
        m.B = B; m.D = d_e; m.rel = tbx->rel; m.ridx = b->rel_ids;
        m.z1 = tbx->ent; m.z1idx = bx->h_gid; m.c1 = w.RC1;
        m.z2 = w.GA; m.c2 = w.RC2;
        KGE_TRY(launch_rescal_matvec(m, s));
        KGE_TRY(launch_rescal_axpy(w.dP, Vr, b->neg_head ? nullptr : w.RC2, B, d_e, w.GH, s));
        KGE_TRY(launch_rescal_axpy(w.dP, w.RC1, b->neg_head ? w.RC2 : nullptr, B, d_e, w.GT, s));
        if (p.nd) KGE_TRY(launch_nd_fold(GN, Gnd, B, b->chunk, p.N, d_e, s));
    }
    if (out && out->g_rel) {        // test / debugging output: materialise dp h t^T + GA x^T + regulariser
        RescalOuterArgs o{};
        o.B = B; o.D = d_e; o.c = w.dP; o.u = tbx->ent; o.uidx = bx->h_gid; o.v = tbx->ent; o.vidx = bx->t_gid;
        o.G = out->g_rel;
        KGE_TRY(launch_rescal_outer(o, s));
        o.c = nullptr; o.u = w.GA; o.uidx = nullptr; o.vidx = b->neg_head ? bx->t_gid : bx->h_gid; o.accumulate = 1;
        if (p.reg) { o.rel = tbx->rel; o.ridx = b->rel_ids; o.reg_coef = hp->reg_coef; o.reg_norm = hp->reg_norm; }
        KGE_TRY(launch_rescal_outer(o, s));
    }
    // relation matrices first: the entity update changes the h / t rows this kernel reads
    RescalUpdateArgs ru{};
    ru.B = B; ru.D = d_e; ru.UE = b->UE; ru.UR = b->UR; ru.neg_head = b->neg_head; ru.reg_norm = hp->reg_norm;
    ru.rel_ids = b->rel_ids; ru.gs = w.Rgs; ru.inv_std = w.Rstd; ru.reg_part = (p.want4 || (p.reg && acc)) ? w.Rreg : nullptr;
    ru.lr = hp->lr; ru.eps = hp->eps; ru.reg_coef = p.reg ? hp->reg_coef : 0.f;
    ru.rel = tbx->rel; ru.rel_state = tbx->rel_state; ru.ent = tbx->ent; ru.hidx = bx->h_gid; ru.tidx = bx->t_gid;
    ru.dpos = w.dP; ru.GA = w.GA; ru.ur_id = b->ur_id; ru.ur_ptr = b->ur_ptr; ru.ur_edge = b->ur_edge;
    ru.counts_dev = b->counts_dev; ru.reg_rel = p.want4 ? w.reg_rel : nullptr; ru.acc = acc;
    if (p.rescal_rel) { ru.c1p = w.RC1; ru.c2p = w.RC2; }
    if (p.rescal_rel && p.reg) { ru.PV = w.RC1; ru.PW = w.RC1 + (size_t)B * d_e; ru.rho = w.RC1 + 2 * (size_t)B * d_e; }
    KGE_TRY(launch_rescal_update_rel(ru, s));
    if (p.rescal_rel) {
        RescalCombineArgs cb{};
        cb.B = B; cb.D = d_e; cb.neg_head = b->neg_head; cb.dpos = w.dP; cb.V = Vr; cb.c1p = w.RC1; cb.c2p = w.RC2; cb.GH = w.GH; cb.GT = w.GT;
        KGE_TRY(launch_rescal_combine(cb, s));
        if (p.nd) KGE_TRY(launch_nd_fold(GN, Gnd, B, b->chunk, p.N, d_e, s));
    }
    return KGE_OK;
}

int Step::phase_bwd() {
    if (p.transr) return bwd_transr();
    if (p.own) {       // nd: the update adds the sampled rows' regulariser, and the in-batch rows' gradient joins the positive trace
        const OwnBwd x{w.dP, p.reg ? hp->reg_coef : 0.f, hp->reg_norm, (p.reg && !p.nd) ? hp->reg_coef : 0.f, p.nd, w.GH, w.GT, GR, false};
        KGE_TRY(kge::own_backward(hp->model, own_block(), &w.own, src, b->neg_head, w.S, GN, x, s));
        return KGE_OK;
    }
    if (p.gemm) {
        if (int rc = bwd_neg_gemm()) return rc;
    } else {
        na.W = w.S; na.GA = w.GA; na.GN = GN;
        na.reg_coef = (p.reg && !p.nd) ? hp->reg_coef : 0.f; na.reg_norm = hp->reg_norm;
        na.GNp = p.lc ? w.GNp : nullptr;
        na.defer_reduce = (p.fuse_gnred || p.fold_upd) ? 1 : 0;       // the partials are summed by edge_bwd's launch / by the update
        na.ga_parts = p.ga_parts; na.ga_stride = (int64_t)b->B * hp->d_e;
        KGE_TRY(launch_neg_bwd_pair(na, s));
        if (c.co_prep) KGE_TRY(launch_edge_fwd(*c.co_prep, s));
    }
    if (p.rescal) return bwd_rescal();
    // per-edge gradients of head / tail / relation rows (TransE rebuilds them in the update, ew_bwd: written by the GA tiles).
    if (p.ew_bwd || (p.transe_fast && !(out && out->g_rel))) return KGE_OK;
    // Rows as the gradient kernels of THIS step see them: the tables, or PREP's dense copies (async pipeline)
    const EdgeSrc src_bwd = p.need_cp ? EdgeSrc{w.Hc, nullptr, w.Tc, nullptr, w.Rc, nullptr, kge::ShardMap{}, kge::ShardMap{}} : src;
    EdgeBwdArgs eb;
    fill_edge_bwd(eb, src_bwd, hp->model, b->B, hp->d_e, hp->d_r, b->neg_head, hp->gamma, rot_div, w.dP, w.GA);
    eb.reg_coef = p.reg ? hp->reg_coef : 0.f; eb.reg_norm = hp->reg_norm;
    if (p.transe_fast) {
        // the per-edge relation gradient is not materialised on the fast path; rebuild it for the
        // caller with the generic kernel BEFORE the tables change (test / debugging output only)
        eb.GR = out->g_rel;
    } else {
        eb.GH = w.GH; eb.GT = w.GT; eb.GR = GR;
        eb.ga_parts = p.fuse_gnred ? na.ga_parts : 1; eb.ga_stride = na.ga_stride;
        if (p.nd) { eb.GNd = GN; eb.nd_chunk = b->chunk; eb.nd_Np = p.N; }   // in-batch negative rows -> positive trace
    }
    if (!p.fuse_gnred) KGE_TRY(launch_edge_bwd(eb, s));
    else if (const int rc = launch_edge_bwd_with_gn_reduce(eb, na, p.fold_nrw, s)) return fail(rc, "launch_edge_bwd_with_gn_reduce failed (%d)", rc);
    return KGE_OK;
}

// ---- UPDATE: owner-computes Adagrad on both tables (or gradient emission for sharded training), then the loss reduction ----
int Step::phase_update() {
    const kge_shards *sh = c.sh; const kge_emit *emit = c.emit;
    const int d_e = hp->d_e, d_r = hp->d_r, phases = c.phases;
    UpdateArgs ua{};
    ua.model_d_e = d_e; ua.d_r = p.rescal ? d_e : d_r; ua.reg_norm = hp->reg_norm;
    ua.UE = (phases & PH_UPD_ENT) ? b->UE : 0;            // the async pipeline applies the two tables' traces separately
    ua.UR = (p.rescal || !(phases & PH_UPD_REL)) ? 0 : b->UR;
    ua.lr = hp->lr; ua.eps = hp->eps; ua.reg_coef = p.reg ? hp->reg_coef : 0.f;
    ua.ent = tb->ent; ua.ent_state = tb->ent_state; ua.rel = tb->rel; ua.rel_state = tb->rel_state; ua.em = em; ua.rm = rm;
    if (sh && sh->rel_local) { ua.rel = sh->rel_local; ua.rel_state = sh->rel_state_local; }    // (rm.n == 0: rank-local relation table)
    ua.ue_id = b->ue_id; ua.ue_pos_ptr = b->ue_pos_ptr; ua.ue_pos_adj = b->ue_pos_adj; ua.ue_neg_ptr = b->ue_neg_ptr; ua.ue_neg_slot = b->ue_neg_slot;
    ua.ur_id = b->ur_id; ua.ur_ptr = b->ur_ptr; ua.ur_edge = b->ur_edge; ua.ue_rec = b->ue_rec; ua.ur_rec = b->ur_rec; ua.counts_dev = b->counts_dev;
    ua.GH = w.GH; ua.GT = w.GT; ua.GN = GN; ua.GR = GR;
    ua.transe_fast = p.transe_fast ? 1 : 0; ua.neg_head = b->neg_head; ua.P = w.GH; ua.GA = w.GA;
    ua.Q = p.qfuse ? w.GT : nullptr; ua.acc = acc;
    ua.reg_ent = p.want4 ? w.reg_ent : nullptr; ua.reg_rel = p.want4 ? w.reg_rel : nullptr;
    ua.ld_e = d_e; ua.ld_r = d_r; ua.ld_gs_e = 1; ua.ld_gs_r = 1;
    if (p.nd) { ua.nd_chunk = b->chunk; ua.nd_Ns = b->N; ua.nd_Np = p.N; }
    if (p.fold_upd) {                  // TransE_l1: this kernel sums the backward's GN partials / GA parts (plan_step)
        ua.GNp = w.GNp; ua.gn_parts = p.fold_nrw; ua.gn_stride = (int64_t)p.CN * d_e;
        ua.gn_reg_coef = p.reg ? hp->reg_coef : 0.f; ua.gn_reg_norm = hp->reg_norm;
        ua.ga_parts = p.ga_parts; ua.ga_stride = (int64_t)b->B * d_e;
    }
    if (p.pipelined && p.reg) {
        // the regulariser of the positive-trace rows is part of the gradient the reference computes in forward, from the
        // rows as gathered: evaluate it on PREP's copies.  (The relation trace is only deferred with KGE_FLAG_ASYNC_REL;
        // otherwise it lands before anything else touches the relation table and the current row IS the gathered row.)
        ua.Hs = w.Hc; ua.Ts = w.Tc;
        if (p.nd) ua.Ns = w.Bn;        // the update adds the regulariser of the sampled negative rows in this mode
        ua.Rs = ((hp->flags & KGE_FLAG_ASYNC_REL) && p.transe_fast) ? w.Rc : nullptr;
    }
    if (emit) {
        ua.g0 = emit->g0; ua.gs0 = emit->gs0; ua.g1 = emit->g1; ua.gs1 = emit->gs1;
        ua.gr = emit->gr; ua.gsr = emit->gsr; ua.rid = emit->rid;
        ua.emit_ent = 1; ua.emit_rel = emit->gr ? 1 : 0; ua.emit_by_id = emit->ent_by_id ? 1 : 0;
        if (emit->msg_rows) {                     // packed single-trace entity messages (ABI 8; checked in Step::setup)
            ua.msg_rows = emit->msg_rows; ua.msg_cap = emit->msg_cap; ua.msg_capT = emit->msg_cap + emit->msg_cap_extra;
            ua.g1 = nullptr; ua.gs0 = nullptr; ua.gs1 = nullptr;
        }
        if (emit->ld_e > 0) { ua.ld_e = emit->ld_e; ua.ld_gs_e = emit->ld_e; }
        if (emit->ld_r > 0) { ua.ld_r = emit->ld_r; ua.ld_gs_r = emit->ld_r; }
    }
    // g_pos_ent next to a dense emit by union entry (the only emit it combines with, Step::setup): the kernel has one trace-0
    // pointer - it writes the message array g0, which is the same [UE, d_e] block, and the output is a copy of it
    const bool copy_g0 = emit && out && out->g_pos_ent && (phases & PH_UPD_ENT);
    if (out && out->g_pos_ent && !emit) ua.g0 = out->g_pos_ent;
    if (c.build_update) { *c.build_update = ua; return KGE_OK; }
    if (c.adam) KGE_TRY(launch_update_adam(ua, *c.adam, s));
    else KGE_TRY(launch_update(ua, s, c.tail));
    if (hp->flags & (NORM_ENT | NORM_REL)) {
        // the projection of the rows this update has just written, from the same plan records (kge_constrain.hip).  A step that
        // carries a sampler job: its tail workgroups write the job's slot, the previous job's slot and the scratch
        // (kge_sampler_tail.hpp) - never the arrays of the batch this step runs on, which this launch reads
        const kge::NormSlices &ns = kge::model_row(hp->model)->norm;
        ConstrainArgs ca{};
        ca.ent = tb->ent; ca.rel = tb->rel; ca.ue_rec = b->ue_rec; ca.ur_rec = b->ur_rec; ca.counts_dev = b->counts_dev;
        ca.UE = (hp->flags & NORM_ENT) ? b->UE : 0; ca.UR = (hp->flags & NORM_REL) ? b->UR : 0;
        ca.d_e = d_e; ca.d_r = d_r; ca.ent_parts = ns.ent; ca.rel_parts = ns.rel;
        ca.ent_unit = (hp->flags & KGE_FLAG_ENT_NORM_UNIT) ? ~0u : 0u;
        ca.rel_unit = (hp->flags & KGE_FLAG_REL_NORM_UNIT) ? ~0u : ns.rel_unit;
        KGE_TRY(launch_constrain(ca, s));
    }
    if (copy_g0 && hipMemcpyAsync(out->g_pos_ent, emit->g0, (size_t)b->UE * d_e * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(KGE_ERR_LAUNCH, "hipMemcpyAsync failed");
    // deterministic reduction of this step's loss terms (only when the caller wants the per-step values; running sums are
    // accumulated by the kernels above without it)
    if (p.want4 && (phases & PH_UPD_ENT)) {
        FinalizeArgs f{};
        f.B = b->B; f.UE = b->UE; f.UR = b->UR; f.pos_row = p.pos_row ? 1 : 0;
        f.row_pos = w.row_pos; f.row_neg = w.row_neg; f.reg_ent = w.reg_ent; f.reg_rel = w.reg_rel;
        f.counts_dev = b->counts_dev; f.loss4 = out->loss4;
        KGE_TRY(launch_finalize(f, s));
    }
    return KGE_OK;
}

// the driver behind every kge_step_* entry point
static int run_step(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out, void *ws,
                    size_t ws_bytes, void *stream, const StepCall &c = StepCall{}) {
    Step x{hp, tb, b, out, c, (hipStream_t)stream};
    if (int rc = x.setup(ws, ws_bytes)) return rc;
    if (c.phases & PH_PREP) if (int rc = x.phase_prep()) return rc;
    if (c.phases & PH_SCORE) x.fill_score();
    if (c.phases & PH_FWD) if (int rc = x.phase_fwd()) return rc;
    if (c.phases & PH_BWD) if (int rc = x.phase_bwd()) return rc;
    if (c.phases & PH_UPDATE) if (int rc = x.phase_update()) return rc;
    return KGE_OK;
}

int kge_step_fused(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b,
                   const kge_step_out *out, void *ws, size_t ws_bytes, void *stream) {
    return run_step(hp, tb, b, out, ws, ws_bytes, stream);
}

// ---- the strict step that also BUILDS a batch of the next group (sampler tail workgroups, kge_sampler_tail.hpp) ----
size_t kge_sampler_tail_scratch_bytes(int B, int C, int N, int64_t n_ent) {
    if (B <= 0 || C <= 0 || N <= 0) return 0;
    return (size_t)tail_scratch(B, C * N, n_ent > ((int64_t)1 << (32 - SP_CODE_BITS))).total;
}

// the strict step with a known-triple index: kge_step_fused (job NULL) / kge_step_fused_sampling + the pair mask in front of the loss
static int step_sampling(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out, void *ws,
                         size_t ws_bytes, const kge_sampler_job *job, StepCall c, void *stream) {
    if (!job) return run_step(hp, tb, b, out, ws, ws_bytes, stream, c);
    if (hp) if (int rc = closed(kge::E_STEP_FUSED_SAMPLING, hp->model, "kge_step_fused_sampling")) return rc;
    if (!job->heads || !job->rels || !job->tails || !job->state || !job->slot || !job->scratch || job->n_train <= 0 || job->n_ent <= 0 ||
        job->B <= 0 || job->C <= 0 || job->chunk <= 0 || job->N <= 0 || job->C * job->chunk != job->B || job->k < 0 || job->advance < 0)
        return fail(KGE_ERR_ARG, "kge_step_fused_sampling: bad sampler job");
    if (job->n_train < job->B) return fail(KGE_ERR_ARG, "kge_step_fused_sampling: fewer training triples than one batch (n_train < batch)");
    if (2 * job->B + job->C * job->N > SP_MAXE || job->B > SP_MAXE / 2 || job->n_ent >= ((int64_t)1 << 51))
        return fail(KGE_ERR_ARG, "kge_step_fused_sampling: 2 * batch + chunks * neg <= 4096 (larger batches: build the plan on the host)");
    if (job->scratch_bytes < kge_sampler_tail_scratch_bytes(job->B, job->C, job->N, job->n_ent))
        return fail(KGE_ERR_WORKSPACE, "kge_step_fused_sampling: scratch too small (kge_sampler_tail_scratch_bytes)");
    c.who = "kge_step_fused_sampling";
    SmpTail t{};
    t.a.H = job->heads; t.a.R = job->rels; t.a.T = job->tails; t.a.perm = job->perm; t.a.n_train = job->n_train; t.a.n_ent = job->n_ent;
    t.a.B = job->B; t.a.C = job->C; t.a.chunk = job->chunk; t.a.N = job->N; t.a.seed = job->seed; t.a.state = job->state;
    t.a.slots = (char *)job->slot; t.a.slot_bytes = 0; t.a.preperm = job->pre_permuted ? 1 : 0; t.slot3 = (char *)job->prev_slot;
    t.scratch = (char *)job->scratch; t.k = job->k; t.advance = job->advance; t.phase = 1;
    c.tail = &t;
    return run_step(hp, tb, b, out, ws, ws_bytes, stream, c);
}

int kge_step_fused_sampling(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out, void *ws,
                            size_t ws_bytes, const kge_sampler_job *job, void *stream) {
    return step_sampling(hp, tb, b, out, ws, ws_bytes, job, StepCall{}, stream);
}

int kge_step_fused_known(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out, void *ws,
                         size_t ws_bytes, const kge_sampler_job *job, const kge_known *known, uint32_t *mask, size_t mask_bytes,
                         void *stream) {
    StepCall c; c.who = "kge_step_fused_known";
    if (known) { c.known = known; c.known_mask = mask; c.known_mask_bytes = mask_bytes; }
    return step_sampling(hp, tb, b, out, ws, ws_bytes, job, c, stream);
}

// ------------------------------------------------------------------------------------------
// --async_update: the update of step s-1 overlaps the scoring of step s (two HIP streams)
// ------------------------------------------------------------------------------------------
struct kge_pipe {
    bool pending;        // a step has been scored but its (entity) update is not enqueued yet
    int parity;          // workspace half of the NEXT step
    int upd_phases;      // what the pending update covers (entity trace, or entity + relation with KGE_FLAG_ASYNC_REL)
    kge_hparams hp; kge_tables tb; kge_batch b; kge_step_out out; bool has_out;
    void *ws; size_t ws_bytes;     // workspace half of the pending step
    bool prepped;        // PREP of the next step already ran (inside the previous call's backward launch) ...
    const void *prep_key;          // ... for the batch whose h_gid array is this,
    kge_hparams prep_hp;           // ... with these hyper-parameters (it is reused only by a call that asks for the same plain step)
};

int kge_pipe_create(kge_pipe **pipe) {
    if (!pipe) return fail(KGE_ERR_ARG, "kge_pipe_create: null argument");
    kge_pipe *p = new (std::nothrow) kge_pipe();
    if (!p) return fail(KGE_ERR_LAUNCH, "kge_pipe_create: out of host memory");
    *pipe = p;
    return KGE_OK;
}

int kge_pipe_destroy(kge_pipe *p) {
    delete p;
    return KGE_OK;
}

size_t kge_step_async_workspace_bytes(const kge_hparams *hp, int B, int C, int chunk, int N, int UE, int UR) {
    // two halves (the update of step s-1 reads its gradients while step s fills the other half), each with room for the dense h / t / r copies
    Carver cv; StepBufs w; return 2 * carve_step(cv, w, hp, B, C, chunk, N, UE, UR, true);
}

int kge_step_async(kge_pipe *p, const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_batch *b_next,
                   const kge_step_out *out, void *ws, size_t ws_bytes, void *stream) {
    if (!p || !hp || !tb || !b || !ws) return fail(KGE_ERR_ARG, "kge_step_async: null argument");
    if (int rc = closed(kge::E_STEP_ASYNC, hp->model, "kge_step_async")) return rc;
    if (int rc = norm_closed(hp, "kge_step_async")) return rc;
    const size_t half = (ws_bytes / 2) & ~(size_t)255;
    void *wsp = (char *)ws + (size_t)p->parity * half;
    void *wsn = (char *)ws + (size_t)(p->parity ^ 1) * half;
    const bool defer_rel = (hp->flags & KGE_FLAG_ASYNC_REL) != 0;
    // PREP(s): gathers the rows (update s-2 has landed: stream order) and makes the dense copies the rest of the step
    // reads - unless the previous call already ran it inside its backward launch
    // (a PREP that ran ahead was built for a plain step - no per-step outputs - with the previous call's hyper-parameters: it
    //  serves this call only if this call wants exactly that; otherwise PREP runs again)
    const bool reuse = p->prepped && p->prep_key == (const void *)b->h_gid && plain_out(out) &&
                       memcmp(&p->prep_hp, hp, sizeof(kge_hparams)) == 0;
    if (!reuse)
        if (int rc = run_step(hp, tb, b, out, wsp, half, stream, phase_call(PH_PREP))) return rc;
    p->prepped = false;
    // launch A: forward(s) || UPDATE(s-1)
    UpdateArgs co{};
    StepCall c = phase_call(PH_FWD);
    if (p->pending) {
        p->pending = false;
        const kge_step_out *po = p->has_out ? &p->out : nullptr;
        StepCall u = phase_call(p->upd_phases);
        if (!(po && po->loss4)) u.build_update = &co;     // (per-step loss wanted: the reduction kernel follows the update - keep them together)
        if (int rc = run_step(&p->hp, &p->tb, &p->b, po, p->ws, p->ws_bytes, stream, u)) return rc;
        c.co_update = u.build_update;
    }
    if (int rc = run_step(hp, tb, b, out, wsp, half, stream, c)) return rc;
    // launch C: backward(s) || PREP(s+1).  Only when nothing touches the tables between this backward and the next PREP
    // (relation trace deferred too), for the plain step (no per-step outputs)
    EdgeFwdArgs ef{};
    const bool have_prep = b_next && defer_rel && plain_out(out);
    if (have_prep) {
        c = phase_call(PH_PREP); c.build_prep = &ef;
        if (int rc = run_step(hp, tb, b_next, out, wsn, half, stream, c)) return rc;
    }
    c = phase_call(PH_BWD); c.co_prep = have_prep ? &ef : nullptr;
    if (int rc = run_step(hp, tb, b, out, wsp, half, stream, c)) return rc;
    if (have_prep) { p->prepped = true; p->prep_key = (const void *)b_next->h_gid; p->prep_hp = *hp; }
    // the reference defers the ENTITY table only (general_models.py:639-647: create_async_update on entity_emb;
    // relation_emb.update stays in the training loop): relation trace now
    if (!defer_rel)
        if (int rc = run_step(hp, tb, b, out, wsp, half, stream, phase_call(PH_UPD_REL))) return rc;
    p->upd_phases = defer_rel ? PH_UPDATE : PH_UPD_ENT;
    p->hp = *hp; p->tb = *tb; p->b = *b; p->has_out = out != nullptr;
    if (out) p->out = *out;
    p->ws = wsp; p->ws_bytes = half;
    p->pending = true;
    p->parity ^= 1;
    return KGE_OK;
}

int kge_step_async_flush(kge_pipe *p, void *stream) {
    if (!p) return fail(KGE_ERR_ARG, "kge_step_async_flush: null argument");
    if (p->pending) {
        p->pending = false;
        if (int rc = run_step(&p->hp, &p->tb, &p->b, p->has_out ? &p->out : nullptr, p->ws, p->ws_bytes, stream, phase_call(p->upd_phases))) return rc;
    }
    p->prepped = false;         // a PREP that ran ahead gathered rows without this update: it must not be reused
    return KGE_OK;
}

int kge_step_phase(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out,
                   void *ws, size_t ws_bytes, int phases, void *stream) {
    // the strict step, one phase group at a time (same kernels, same order: calling the four groups in sequence IS
    // kge_step_fused); exists so that the caller can put events between the groups (the reference's per-phase timers)
    if (phases <= 0 || phases > (KGE_PHASE_GATHER | KGE_PHASE_FORWARD | KGE_PHASE_BACKWARD | KGE_PHASE_UPDATE))
        return fail(KGE_ERR_ARG, "kge_step_phase: bad phase mask %d", phases);
    int ph = 0;
    if (phases & KGE_PHASE_GATHER) ph |= PH_PREP;
    if (phases & KGE_PHASE_FORWARD) ph |= PH_FWD;
    if (phases & KGE_PHASE_BACKWARD) ph |= PH_BWD;
    if (phases & KGE_PHASE_UPDATE) ph |= PH_UPDATE;
    return run_step(hp, tb, b, out, ws, ws_bytes, stream, phase_call(ph | PH_STRICT, "kge_step_phase"));
}

int kge_step_phase_known(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out, void *ws,
                         size_t ws_bytes, int phases, const kge_known *known, uint32_t *mask, size_t mask_bytes, void *stream) {
    if (!known) return kge_step_phase(hp, tb, b, out, ws, ws_bytes, phases, stream);
    if (phases <= 0 || phases > (KGE_PHASE_GATHER | KGE_PHASE_FORWARD | KGE_PHASE_BACKWARD | KGE_PHASE_UPDATE))
        return fail(KGE_ERR_ARG, "kge_step_phase_known: bad phase mask %d", phases);
    int ph = 0;
    if (phases & KGE_PHASE_GATHER) ph |= PH_PREP;
    if (phases & KGE_PHASE_FORWARD) ph |= PH_FWD;
    if (phases & KGE_PHASE_BACKWARD) ph |= PH_BWD;
    if (phases & KGE_PHASE_UPDATE) ph |= PH_UPDATE;
    StepCall c = phase_call(ph | PH_STRICT, "kge_step_phase_known");
    c.known = known; c.known_mask = mask; c.known_mask_bytes = mask_bytes;
    return run_step(hp, tb, b, out, ws, ws_bytes, stream, c);
}

// the strict step with the optimizer as an argument: KGE_OPT_ADAGRAD is the existing step, KGE_OPT_ADAM swaps the update launch
// for its Adam form (kge_adam.hip) - everything in front of the update is the same launches on the same arguments
int kge_step_optim(const kge_hparams *hp, const kge_optim *opt, const kge_tables *tb, const kge_batch *b, const kge_step_out *out,
                   void *ws, size_t ws_bytes, int phases, const kge_known *known, uint32_t *mask, size_t mask_bytes, void *hip_stream) {
    const int all = KGE_PHASE_GATHER | KGE_PHASE_FORWARD | KGE_PHASE_BACKWARD | KGE_PHASE_UPDATE;
    if (!hp || !opt || !tb || !b || !ws) return fail(KGE_ERR_ARG, "kge_step_optim: null argument");
    if (phases <= 0 || phases > all) return fail(KGE_ERR_ARG, "kge_step_optim: bad phase mask %d", phases);
    if (opt->kind != KGE_OPT_ADAGRAD && opt->kind != KGE_OPT_ADAM)
        return fail(KGE_ERR_ARG, "kge_step_optim: unknown optimizer kind %d (KGE_OPT_ADAGRAD, KGE_OPT_ADAM)", opt->kind);
    if (opt->kind == KGE_OPT_ADAGRAD) {
        if (phases != all) return kge_step_phase_known(hp, tb, b, out, ws, ws_bytes, phases, known, mask, mask_bytes, hip_stream);
        return kge_step_fused_known(hp, tb, b, out, ws, ws_bytes, nullptr, known, mask, mask_bytes, hip_stream);
    }
    if (hp->model == KGE_RESCAL || hp->model == KGE_TRANSR)
        return fail(KGE_ERR_ARG, "kge_step_optim: Adam is not available for RESCAL / TransR (their relation-side tables are updated by "
                                 "kernels of their own)");
    if (!opt->ent_mom || !opt->rel_mom)
        return fail(KGE_ERR_ARG, "kge_step_optim: Adam needs the moment tables ent_mom [n_ent, 2, d_e] and rel_mom [n_rel, 2, d_r]");
    if (!(opt->beta1 >= 0.f && opt->beta1 < 1.f) || !(opt->beta2 >= 0.f && opt->beta2 < 1.f))
        return fail(KGE_ERR_ARG, "kge_step_optim: Adam needs beta1 and beta2 in [0, 1) (got %g, %g)", (double)opt->beta1, (double)opt->beta2);
    if (!(opt->eps > 0.f)) return fail(KGE_ERR_ARG, "kge_step_optim: Adam needs eps > 0 (got %g)", (double)opt->eps);
    if (hp->d_e <= 0 || hp->d_r <= 0 || hp->d_e % 4 != 0 || hp->d_r % 4 != 0 || hp->d_e > 1024 || hp->d_r > 1024)
        return fail(KGE_ERR_ARG, "kge_step_optim: Adam runs in the register-resident update - row widths must be multiples of 4 and at "
                                 "most 1024 floats (d_e=%d d_r=%d)", hp->d_e, hp->d_r);
    AdamArgs o{};
    o.ent_mom = opt->ent_mom; o.rel_mom = opt->rel_mom; o.beta1 = opt->beta1; o.beta2 = opt->beta2; o.eps = opt->eps;
    o.omb1 = (float)(1.0 - (double)opt->beta1); o.omb2 = (float)(1.0 - (double)opt->beta2);
    o.lb1 = (float)std::log((double)opt->beta1); o.lb2 = (float)std::log((double)opt->beta2);      // (beta 0: -inf, expm1 gives -1)
    int ph = PH_ALL;
    if (phases != all) {
        ph = PH_STRICT;
        if (phases & KGE_PHASE_GATHER) ph |= PH_PREP;
        if (phases & KGE_PHASE_FORWARD) ph |= PH_FWD;
        if (phases & KGE_PHASE_BACKWARD) ph |= PH_BWD;
        if (phases & KGE_PHASE_UPDATE) ph |= PH_UPDATE;
    }
    StepCall c = phase_call(ph, "kge_step_optim");
    c.adam = &o;
    if (known) { c.known = known; c.known_mask = mask; c.known_mask_bytes = mask_bytes; }
    return run_step(hp, tb, b, out, ws, ws_bytes, hip_stream, c);
}

int kge_step_grads(const kge_hparams *hp, const kge_tables *tb, const kge_batch *b, const kge_step_out *out, const kge_emit *emit,
                   void *ws, size_t ws_bytes, void *stream) {
    if (hp) if (int rc = closed(kge::E_STEP_GRADS, hp->model, "kge_step_grads")) return rc;
    if (int rc = norm_closed(hp, "kge_step_grads")) return rc;
    if (!emit || !emit->g0 || (!emit->msg_rows && (!emit->gs0 || !emit->g1 || !emit->gs1)))
        return fail(KGE_ERR_ARG, "kge_step_grads: emit buffers g0/gs0/g1/gs1 are required (packed messages: g0 + msg_rows)");
    if ((emit->gr == nullptr) != (emit->gsr == nullptr))
        return fail(KGE_ERR_ARG, "kge_step_grads: gr and gsr must be given together");
    StepCall c; c.emit = emit;
    return run_step(hp, tb, b, out, ws, ws_bytes, stream, c);
}

// TransR's rows of a batch of test triples: projected head / tail, q = x P - r, sign(hp + r - tp); n floats each
struct TransRRows { float *THP, *TTP, *TQ, *TSG; };
static void carve_transr_rows(Carver &cv, TransRRows &w, size_t n) {
    w.THP = cv.f(n); w.TTP = cv.f(n); w.TQ = cv.f(n); w.TSG = cv.f(n);
}

// what every ranking entry needs of a batch of `rows` test triples (h, r, t: the batch's ids) before it scores candidates: the positive
// scores P and the pos-side vectors A (+ their squared norms asq when given).  A == null: positive scores only (relation ranking).
// TransR: only the projections hp, tp - launch_transr_pos, which the caller runs with its own candidates, makes P and q from them.
static int rank_pos_side(int model, int neg_head, const float *ent, const float *rel, const float *proj, const int64_t *h,
                         const int64_t *r, const int64_t *t, int rows, int d_e, int d_r, float gamma, float rot_div, float *P,
                         float *A, float *asq, float *RV, const TransRRows &w, hipStream_t s, int th_chunk = 0) {
    if (model == KGE_TRANSR) {
        RescalMatvecArgs m{};
        m.B = rows; m.D = d_e; m.Dc = d_r; m.rel = proj; m.ridx = r;
        m.z1 = ent; m.z1idx = h; m.c1 = w.THP; m.z2 = ent; m.z2idx = t; m.c2 = w.TTP;
        KGE_TRY(launch_rescal_matvec(m, s));
    } else if (model == KGE_RESCAL) {
        RescalMatvecArgs m{};
        m.B = rows; m.D = d_e; m.rel = rel; m.ridx = r;
        m.y1 = ent; m.y1idx = t; m.pd = ent; m.pdidx = h; m.p = P;
        if (A) {
            m.r1 = neg_head ? A : RV;                   // V = M t
            if (!neg_head) { m.y2 = ent; m.y2idx = h; m.r2 = A; }
        }
        KGE_TRY(launch_rescal_matvec(m, s));
    } else if (kge::model_row(model)->own_fwd) {
        // th_chunk == 0 (kge_rank_eval): a in the A entry, the second vector (w, w^, rho) in the RV entry; else A is the stacked operand
        // of chunks of th_chunk rows (PairRE: the pair always lives in A and RV).  |a|^2 in asq; the rows' other scalars (TransH: w^ . a;
        // TransD: |rho|^2, a . rho) in the first `rows` floats of the THP and TTP entries (TransR's, free here)
        KGE_TRY(kge::own_prepare(model, EdgeSrc{ent, h, ent, t, rel, r}, rows, th_chunk, d_e, neg_head, gamma, P,
                                 OwnOperand{A, RV, asq, w.THP, w.TTP, nullptr, nullptr, nullptr}, nullptr, s));
    } else {
        EdgeFwdArgs ef;
        fill_edge(ef, EdgeSrc{ent, h, ent, t, rel, r}, model, rows, d_e, d_r, neg_head, gamma, rot_div);
        ef.pos_score = P; ef.A = A; ef.asq = asq;
        KGE_TRY(launch_edge_fwd(ef, s));
    }
    return KGE_OK;
}

struct RankBufs : TransRRows { float *A, *asq, *P, *bsq, *S, *RV; };
static size_t carve_rank(Carver &cv, RankBufs &w, int Eb, int64_t N, int d_e) {
    w.A = cv.f((size_t)Eb * d_e); w.asq = cv.f(Eb); w.P = cv.f(Eb); w.bsq = cv.f((size_t)N);
    w.S = (float *)cv.bytes(std::max((size_t)Eb * (size_t)N * sizeof(float), rank_gemm_mask_bytes(Eb, N)));   // scores / the comparison mask
    w.RV = cv.f((size_t)Eb * d_e);                      // V = M t (RESCAL)
    carve_transr_rows(cv, w, (size_t)Eb * 1024);        // (d_r <= 1024)
    return cv.off;
}

size_t kge_rank_workspace_bytes(int Eb, int64_t n_cand, int d_e) {
    Carver cv; RankBufs w; return carve_rank(cv, w, Eb, n_cand, d_e);
}

int kge_rank_eval(int model, int neg_head, const float *ent, int64_t n_ent, const float *rel,
                  int64_t n_rel, const int64_t *h, const int64_t *r, const int64_t *t, int64_t E,
                  int d_e, int d_r, float gamma, float emb_init, const int64_t *cand, int64_t n_cand,
                  const int64_t *filt_ptr, const int64_t *filt_ids, int Eb, int32_t *ranks,
                  float *pos_score_out, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    return kge_rank_eval_ex(model, neg_head, ent, n_ent, rel, n_rel, nullptr, h, r, t, E, d_e, d_r, gamma, emb_init, cand,
                            n_cand, filt_ptr, filt_ids, Eb, ranks, pos_score_out, ws, ws_bytes, flags, stream);
}

// the ranking loop of kge_rank_eval_ex / kge_rank_eval_split: h / t index the query table qent (positive rows, pos-side vectors),
// candidate j is row cent + (cand ? cand[j] : j) * d_e.  Arguments checked by the callers; N = the candidate count, > 0.
static int rank_eval_impl(int model, int neg_head, const float *qent, const float *cent, const float *rel, const float *proj,
                          const int64_t *h, const int64_t *r, const int64_t *t, int64_t E, int d_e, int d_r, float gamma, float emb_init,
                          const int64_t *cand, int64_t N, const int64_t *filt_ptr, const int64_t *filt_ids, int Eb, int32_t *ranks,
                          float *pos_score_out, void *ws, size_t ws_bytes, unsigned flags, hipStream_t s) {
    // (TransD keeps TWO scalars per candidate, [beta | c], in the bsq entry: the workspace of 2 N candidates, include/kge_hip.h)
    const bool td = model == KGE_TRANSD;
    Carver cv(ws, ws_bytes); RankBufs w;
    const size_t need = carve_rank(cv, w, Eb, kge::model_row(model)->cand_factor * N, d_e);
    if (need > ws_bytes) return fail(KGE_ERR_WORKSPACE, "kge_rank_eval: workspace too small (%zu < %zu)", ws_bytes, need);
    float *A = w.A, *asq = w.asq, *bsq = w.bsq, *S = w.S;
    const bool gemm = use_mfma(model, d_e, (int)N, flags);
    const bool l2g = gemm && model == KGE_TRANSE_L2;
    const float rot_div = rot_div_of(emb_init);
    if (l2g) {       // |b|^2 of every candidate row, once
        EdgeFwdArgs nb{};
        nb.B = 0; nb.d_e = d_e; nb.d_r = d_r; nb.model = model; nb.nbase = cent; nb.nidx = cand; nb.n_neg = (int)N;
        nb.bsq = bsq;
        KGE_TRY(launch_edge_fwd(nb, s));
    }
    // the scalars of every candidate row, once: PairRE |x|, TransH |n|^2, TransD |n|^2 and m . n (the bsq entry)
    const OwnOperand cands{nullptr, nullptr, nullptr, nullptr, nullptr, bsq, bsq + N, nullptr};
    if (kge::model_row(model)->own_fwd) KGE_TRY(kge::own_cand_rows(model, cent, cand, N, d_e, cands, s));
    const bool th = model == KGE_TRANSH;
    for (int64_t e0 = 0; e0 < E; e0 += Eb) {
        const int rows = (int)((E - e0) < Eb ? (E - e0) : Eb);
        float *P = pos_score_out ? pos_score_out + e0 : w.P;
        KGE_TRY(rank_pos_side(model, neg_head, qent, rel, proj, h + e0, r + e0, t + e0, rows, d_e, d_r, gamma, rot_div, P, A,
                              (l2g || th || td) ? asq : nullptr, w.RV, w, s));
        if (td) {       // the candidate operand is the table row's first half: the table is not copied
            KGE_TRY(launch_rank_gemm_transd(A, w.RV, rows, cent, cand, N, d_e / 2, gamma, asq, w.THP, w.TTP, bsq, bsq + N, P, S, filt_ptr, filt_ids,
                                            e0, ranks, s));
            continue;
        }
        if (th) {
            KGE_TRY(launch_rank_gemm_transh(A, w.RV, rows, cent, cand, N, d_e, gamma, asq, w.THP, bsq, P, S, filt_ptr, filt_ids, e0, ranks, s));
            continue;
        }
        if (model == KGE_TRANSR) {
            // the training kernels with one chunk = this batch of test triples and the candidates as negatives
            TransRArgs tr{};
            tr.B = rows; tr.C = 1; tr.chunk = rows; tr.N = (int)N; tr.De = d_e; tr.Dr = d_r; tr.neg_head = neg_head;
            tr.gamma = gamma; tr.ent = qent; tr.cent = cent; tr.h_gid = h + e0; tr.t_gid = t + e0; tr.neg_ids = cand; tr.rel_ids = r + e0;
            tr.rel = rel; tr.proj = const_cast<float *>(proj);
            tr.HP = w.THP; tr.TP = w.TTP; tr.Q = w.TQ; tr.SG = w.TSG; tr.P = P; tr.S = S; tr.Z = nullptr;
            KGE_TRY(launch_transr_pos(tr, s));
            KGE_TRY(launch_transr_fwd(tr, s));
        } else if (gemm && rank_gemm_supported(model, d_e)) {
            // one tiled GEMM per batch whose epilogue keeps the comparison bits; ranks from the mask (kge_rank_gemm.hip)
            KGE_TRY(launch_rank_gemm(model, A, rows, cent, cand, N, d_e, gamma, clamp_of(model), asq, bsq, P, S, filt_ptr, filt_ids, e0,
                                     ranks, s));
            continue;
        } else if (gemm) {
            GemmArgs g; fill_gemm(g, model, 1, rows, (int)N, d_e, gamma, A, cent, cand);
            g.S = S; g.asq = asq; g.bsq = bsq;
            KGE_TRY(launch_neg_fwd_gemm(g, s));
        } else if (model == KGE_PAIRRE) {
            KGE_TRY(kge::own_scores(model, OwnBlock{1, rows, (int)N, d_e, gamma, OwnOperand{A, w.RV, nullptr, nullptr, nullptr, bsq}, cent, cand, nullptr}, S, s));
        } else {
            NegArgs na; fill_pair(na, model, 1, rows, (int)N, d_e, gamma, A, cent, cand);
            na.S = S;
            KGE_TRY(launch_neg_fwd_pair(na, s));
        }
        KGE_TRY(launch_rank_count(S, P, rows, N, filt_ptr, filt_ids, e0, ranks, s));
    }
    return KGE_OK;
}

// what kge_rank_eval_ex and kge_rank_eval_split ask of the arguments they share
static int check_rank_args(const char *who, const float *qent, const float *rel, int64_t n_rel, const int64_t *h, const int64_t *r,
                           const int64_t *t, int64_t E, const int64_t *filt_ptr, const int64_t *filt_ids, int Eb, const int32_t *ranks,
                           const void *ws) {
    if (!qent || !rel || n_rel <= 0 || E < 0 || (E && (!h || !r || !t || !ranks)) || !ws || Eb <= 0)
        return fail(KGE_ERR_ARG, "%s: bad argument", who);
    if ((filt_ptr == nullptr) != (filt_ids == nullptr)) return fail(KGE_ERR_ARG, "%s: filt_ptr and filt_ids must be given together", who);
    return KGE_OK;
}

int kge_rank_eval_ex(int model, int neg_head, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel, const float *proj,
                     const int64_t *h, const int64_t *r, const int64_t *t, int64_t E, int d_e, int d_r, float gamma, float emb_init,
                     const int64_t *cand, int64_t n_cand, const int64_t *filt_ptr, const int64_t *filt_ids, int Eb, int32_t *ranks,
                     float *pos_score_out, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    if (int rc = check_model(model, d_e, d_r)) return rc;
    if (model == KGE_TRANSR && (!proj || !cand))
        return fail(KGE_ERR_ARG, "kge_rank_eval_ex: TransR needs the projection table and an explicit candidate list");
    if (n_ent <= 0) return fail(KGE_ERR_ARG, "kge_rank_eval: bad argument");
    if (int rc = check_rank_args("kge_rank_eval", ent, rel, n_rel, h, r, t, E, filt_ptr, filt_ids, Eb, ranks, ws)) return rc;
    const int64_t N = cand ? n_cand : n_ent;
    if (N <= 0 || N > 0x7fffffff) return fail(KGE_ERR_ARG, "kge_rank_eval: bad candidate count %lld", (long long)N);
    if (E == 0) return KGE_OK;
    return rank_eval_impl(model, neg_head, ent, ent, rel, proj, h, r, t, E, d_e, d_r, gamma, emb_init, cand, N, filt_ptr, filt_ids,
                          Eb, ranks, pos_score_out, ws, ws_bytes, flags, (hipStream_t)stream);
}

int kge_rank_eval_split(int model, int neg_head, const float *qent, int64_t n_qent, const float *cent, int64_t n_cent, const float *rel,
                        int64_t n_rel, const float *proj, const int64_t *h, const int64_t *r, const int64_t *t, int64_t E, int d_e, int d_r,
                        float gamma, float emb_init, const int64_t *cand, int64_t n_cand, const int64_t *filt_ptr, const int64_t *filt_ids,
                        int Eb, int32_t *ranks, float *pos_score_out, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    if (int rc = check_model(model, d_e, d_r)) return rc;
    if (int rc = closed(kge::E_RANK_EVAL_SPLIT, model, "kge_rank_eval_split")) return rc;
    if (model == KGE_TRANSR && !proj)
        return fail(KGE_ERR_ARG, "kge_rank_eval_split: TransR needs the projection table");
    if (n_qent <= 0 || n_cent < 0) return fail(KGE_ERR_ARG, "kge_rank_eval_split: bad argument");
    if (int rc = check_rank_args("kge_rank_eval_split", qent, rel, n_rel, h, r, t, E, filt_ptr, filt_ids, Eb, ranks, ws)) return rc;
    const int64_t N = cand ? n_cand : n_cent;
    if (N < 0 || N > 0x7fffffff) return fail(KGE_ERR_ARG, "kge_rank_eval_split: bad candidate count %lld", (long long)N);
    if (N > 0 && !cent) return fail(KGE_ERR_ARG, "kge_rank_eval_split: candidates without a candidate table");
    if (E == 0) return KGE_OK;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {                     // a rank that owns no candidate: every count is 0 (pos_score_out is not written)
        return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ranks), 1, (size_t)E, s) == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
    }
    if (model == KGE_TRANSR && !cand)
        return fail(KGE_ERR_ARG, "kge_rank_eval_split: TransR needs an explicit candidate list");
    return rank_eval_impl(model, neg_head, qent, cent, rel, proj, h, r, t, E, d_e, d_r, gamma, emb_init, cand, N, filt_ptr, filt_ids,
                          Eb, ranks, pos_score_out, ws, ws_bytes, flags, s);
}

// ---- chunked-candidate ranking (kge_rank_chunk.hip) ----
// one block of whole chunks: pos-side vectors / norms / positive scores of its rows, the candidates' norms (TransE_l2), and - for the
// score-block route only, but the layout does not depend on the flags - the id list and the score block
struct ChunkBufs : TransRRows { float *A, *asq, *P, *RV, *bsq_own, *bsq_c, *S, *Pnrm, *TPQ, *TNh; int64_t *ids; size_t arow; };
static size_t carve_chunked(Carver &cv, ChunkBufs &w, int model, int64_t rows, int chunk, int64_t n_cand, int self_cand, int d_e, int d_r) {
    const size_t nch = (size_t)((rows + chunk - 1) / chunk), R = nch * (size_t)chunk;
    const size_t ncols = (size_t)n_cand + (self_cand ? (size_t)chunk : 0);
    const bool th = model == KGE_TRANSH, td = model == KGE_TRANSD;       // (TransD: the stacked (a, rho) is 2 R rows of d_e / 2)
    w.arow = (th ? 2 : 1) * (size_t)d_e;                                        // floats per test row of the A entry (TransH: the stacked operand (a, w^))
    w.A = cv.f(R * w.arow); w.asq = cv.f(R); w.P = cv.f(R);
    w.RV = cv.f(model == KGE_RESCAL || model == KGE_PAIRRE ? R * d_e : 0);      // V = M t (RESCAL); w of the pair (PairRE)
    carve_transr_rows(cv, w, model == KGE_TRANSR ? R * (size_t)d_r : (th || td) ? R : 0);   // (TransH: w^ . a in the first entry; TransD: |rho|^2, a . rho)
    w.bsq_own = cv.f(R); w.bsq_c = cv.f(nch * (size_t)n_cand);
    w.ids = cv.i64(nch * ncols);
    w.S = cv.f(R * ncols);
    w.Pnrm = (model == KGE_PAIRRE || th) ? cv.f(nch * ncols) : nullptr;       // PairRE: |x| per position of the id lists; TransH: |x|^2
    w.TPQ = (th || td) ? cv.f(2 * R * ncols) : nullptr;                // TransH / TransD: the raw products p | q
    if (td) w.Pnrm = cv.f(2 * nch * ncols);                            // TransD: [beta | c] per position of the id lists
    w.TNh = td ? cv.f(nch * ncols * (size_t)(d_e / 2)) : nullptr;      // TransD: the listed rows' first halves, dense (the products' operand)
    return cv.off;
}

size_t kge_rank_chunked_workspace_bytes(int model, int rows, int chunk, int64_t n_cand, int self_cand, int d_e, int d_r) {
    if (rows <= 0 || chunk <= 0 || n_cand < 0 || d_e <= 0 || d_r <= 0) return 0;
    Carver cv; ChunkBufs w; return carve_chunked(cv, w, model, rows, chunk, n_cand, self_cand, d_e, d_r);
}

int kge_rank_eval_chunked(int model, int neg_head, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel,
                          const float *proj, const int64_t *h, const int64_t *r, const int64_t *t, int64_t E,
                          int d_e, int d_r, float gamma, float emb_init, int chunk,
                          const int64_t *cand, int64_t n_cand, int64_t cand_stride, int self_cand,
                          const int64_t *filt_ptr, const int64_t *filt_ids, int32_t *ranks, float *pos_score_out,
                          void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    if (int rc = check_model(model, d_e, d_r)) return rc;
    if (chunk <= 0) return fail(KGE_ERR_ARG, "kge_rank_eval_chunked: chunk must be positive (got %d)", chunk);
    if (self_cand && filt_ptr)
        return fail(KGE_ERR_ARG, "kge_rank_eval_chunked: self_cand and a filter exclude each other "
                                 "(if negative sampling based on degree, we can't filter positive edges)");
    if ((filt_ptr == nullptr) != (filt_ids == nullptr))
        return fail(KGE_ERR_ARG, "kge_rank_eval_chunked: filt_ptr and filt_ids must be given together");
    if (model == KGE_TRANSR && !proj) return fail(KGE_ERR_ARG, "kge_rank_eval_chunked: TransR needs the projection table");
    if (!ent || !rel || n_ent <= 0 || n_rel <= 0 || E < 0 || (E && (!h || !r || !t || !ranks)) || !ws)
        return fail(KGE_ERR_ARG, "kge_rank_eval_chunked: bad argument");
    const int64_t NC = cand ? n_cand : n_ent;
    if (NC <= 0 || cand_stride < 0 || (int64_t)chunk * (NC + (self_cand ? chunk : 0)) > 0x7fffffff)
        return fail(KGE_ERR_ARG, "kge_rank_eval_chunked: bad candidate count %lld / stride %lld", (long long)NC, (long long)cand_stride);
    if (E == 0) return KGE_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nch_all = (E + chunk - 1) / chunk;
    const int64_t ncols_full = NC + (self_cand ? chunk : 0);
    // the largest block of whole chunks that fits the workspace (and the 32-bit element counts of the training kernels)
    auto need_of = [&](int64_t nch) { Carver cv; ChunkBufs w; return carve_chunked(cv, w, model, nch * chunk, chunk, NC, self_cand, d_e, d_r); };
    if (need_of(1) > ws_bytes)
        return fail(KGE_ERR_WORKSPACE, "kge_rank_eval_chunked: workspace too small for one chunk (%zu < %zu)", ws_bytes, need_of(1));
    int64_t lo = 1, hi = std::min(nch_all, std::max<int64_t>(1, (int64_t)(1 << 30) / ((int64_t)chunk * ncols_full)));
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (need_of(mid) <= ws_bytes) lo = mid; else hi = mid - 1;
    }
    const int64_t nchb = lo;
    Carver cv(ws, ws_bytes); ChunkBufs w;
    carve_chunked(cv, w, model, nchb * chunk, chunk, NC, self_cand, d_e, d_r);
    const bool gemm = model != KGE_TRANSR && use_mfma(model, d_e, (int)NC, flags) && rank_gemm_supported(model, d_e);
    const bool l2g = gemm && model == KGE_TRANSE_L2;
    const bool shared = !cand || cand_stride == 0;
    const float rot_div = rot_div_of(emb_init);
    ChunkCands cc{};
    cc.cand = cand; cc.n_cand = NC; cc.stride = cand_stride; cc.own = self_cand ? (neg_head ? h : t) : nullptr;
    cc.n_ent = n_ent; cc.E = E; cc.chunk = chunk;
    if (l2g && shared) {             // |b|^2 of the one list, once
        ChunkCands c1 = cc; c1.own = nullptr;
        KGE_TRY(launch_chunk_bsq(c1, 0, 0, NC, ent, d_e, w.bsq_own, w.bsq_c, s));
    }
    for (int64_t c0 = 0; c0 < nch_all; c0 += nchb) {
        const int nch = (int)std::min(nchb, nch_all - c0);
        const int64_t e0 = c0 * chunk;
        const int rows = (int)std::min<int64_t>((int64_t)nch * chunk, E - e0);
        float *P = pos_score_out ? pos_score_out + e0 : w.P;
        KGE_TRY(rank_pos_side(model, neg_head, ent, rel, proj, h + e0, r + e0, t + e0, rows, d_e, d_r, gamma, rot_div, P, w.A,
                              (l2g || kge::model_row(model)->own_fwd) ? w.asq : nullptr, w.RV, w, s, chunk));
        if (gemm) {
            if (l2g && (!shared || self_cand)) {
                ChunkCands c1 = cc; if (shared) c1.cand = nullptr;
                KGE_TRY(launch_chunk_bsq(c1, c0, rows, shared ? 0 : (int64_t)nch * NC, ent, d_e, w.bsq_own, w.bsq_c, s));
            }
            if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ranks + e0), 1, (size_t)rows, s) != hipSuccess)
                return fail(KGE_ERR_LAUNCH, "kge_rank_eval_chunked: memset failed");
            KGE_TRY(launch_rank_chunk_gemm(model, cc, c0, nch, w.A, w.asq, P, ent, d_e, gamma, clamp_of(model), w.bsq_own, w.bsq_c,
                                           shared ? 1 : 0, filt_ptr, filt_ids, ranks, s));
            continue;
        }
        // score-block route: the whole chunks of the block in one call of the training kernels, a short last chunk in its own
        const int nfull = rows / chunk, rem = rows % chunk;
        for (int gidx = 0; gidx < 2; ++gidx) {
            const int C = gidx == 0 ? nfull : (rem ? 1 : 0), m = gidx == 0 ? chunk : rem;
            if (C == 0) continue;
            const int64_t row_off = gidx == 0 ? 0 : (int64_t)nfull * chunk;
            const int64_t cfirst = c0 + (gidx == 0 ? 0 : nfull);
            const int64_t ncols = NC + (self_cand ? m : 0);
            int64_t *ids = w.ids + (gidx == 0 ? 0 : (int64_t)nfull * ncols_full);
            float *S = w.S + row_off * ncols_full;
            KGE_TRY(launch_chunk_ids(cc, cfirst, C, m, ncols, ids, s));
            if (model == KGE_TRANSR) {
                TransRArgs tr{};
                tr.B = C * m; tr.C = C; tr.chunk = m; tr.N = (int)ncols; tr.De = d_e; tr.Dr = d_r; tr.neg_head = neg_head;
                tr.gamma = gamma; tr.ent = ent; tr.cent = ent; tr.h_gid = h + e0 + row_off; tr.t_gid = t + e0 + row_off;
                tr.neg_ids = ids; tr.rel_ids = r + e0 + row_off; tr.rel = rel; tr.proj = const_cast<float *>(proj);
                tr.HP = w.THP + row_off * d_r; tr.TP = w.TTP + row_off * d_r; tr.Q = w.TQ + row_off * d_r; tr.SG = w.TSG + row_off * d_r;
                tr.P = P + row_off; tr.S = S; tr.Z = nullptr;
                KGE_TRY(launch_transr_pos(tr, s));
                KGE_TRY(launch_transr_fwd(tr, s));
            } else if (kge::model_row(model)->own_fwd) {
                // the candidate scalars (TransD: [beta | c] and the first halves) per position of the lists; the stacked operand and
                // the product block: two rows per test row
                const int64_t poff = gidx == 0 ? 0 : (int64_t)nfull * ncols_full;
                const OwnOperand o{w.A + row_off * w.arow, w.RV + row_off * d_e, w.asq + row_off, w.THP + row_off, w.TTP + row_off,
                                   w.Pnrm + poff, w.TNh ? w.Pnrm + nchb * ncols_full + poff : nullptr, w.TNh ? w.TNh + poff * (d_e / 2) : nullptr};
                KGE_TRY(kge::own_cand_rows(model, ent, ids, (int64_t)C * ncols, d_e, o, s));
                KGE_TRY(kge::own_scores(model, OwnBlock{C, m, (int)ncols, d_e, gamma, o, ent, ids, w.TPQ ? w.TPQ + 2 * row_off * ncols_full : nullptr}, S, s));
            } else {
                NegArgs na; fill_pair(na, model, C, m, (int)ncols, d_e, gamma, w.A + row_off * d_e, ent, ids);
                na.S = S;
                KGE_TRY(launch_neg_fwd_pair(na, s));
            }
            KGE_TRY(launch_chunk_count(cc, cfirst, C, m, ncols, S, P + row_off, filt_ptr, filt_ids, ranks, s));
        }
    }
    return KGE_OK;
}

// ---- relation ranking (kge_rank_rel.hip) ----
// one batch of Eb test triples: query rows / their norms / positive scores, the relation rows' norms (TransE_l2), the score block or
// comparison mask, and TransR's projected rows, negated relation rows and identity ids.  The layout does not depend on the flags.
struct RelBufs : TransRRows { float *Q, *qsq, *P, *csq, *S, *RQ, *RN; int64_t *ids; };
static size_t carve_rank_rel(Carver &cv, RelBufs &w, int model, int Eb, int64_t n_rel, int d_e, int d_r) {
    const size_t qw = model == KGE_ROTATE ? 0 : model == KGE_RESCAL ? (size_t)d_e * d_e : (size_t)d_e;
    w.Q = cv.f((size_t)Eb * qw); w.qsq = cv.f(Eb); w.P = cv.f(Eb); w.csq = cv.f((size_t)n_rel);
    w.S = (float *)cv.bytes(std::max((size_t)Eb * (size_t)n_rel * sizeof(float), rank_gemm_mask_bytes(Eb, n_rel)));
    carve_transr_rows(cv, w, model == KGE_TRANSR ? (size_t)Eb * d_r : 0);
    w.RQ = cv.f(model == KGE_TRANSR ? (size_t)n_rel * d_r : 0);
    w.ids = cv.i64(model == KGE_TRANSR ? std::max((size_t)n_rel, (size_t)Eb) : 0);
    w.RN = model == KGE_QUATE ? cv.f((size_t)n_rel * d_r) : nullptr;       // QuatE: the relation table normalised per quaternion
    return cv.off;
}

size_t kge_rank_rel_workspace_bytes(int model, int Eb, int64_t n_rel, int d_e, int d_r) {
    if (Eb <= 0 || n_rel <= 0 || n_rel > 0x7fffffff || check_model(model, d_e, d_r) != KGE_OK) return 0;
    if (!kge::model_row(model)->rel_ws_sized) return 0;
    Carver cv; RelBufs w; return carve_rank_rel(cv, w, model, Eb, n_rel, d_e, d_r);
}

int kge_rank_rel_eval(int model, const float *ent, int64_t n_ent, const float *rel, int64_t n_rel, const float *proj,
                      const int64_t *h, const int64_t *r, const int64_t *t, int64_t E, int d_e, int d_r,
                      float gamma, float emb_init, const int64_t *filt_ptr, const int64_t *filt_ids, int Eb,
                      int32_t *ranks, float *pos_score_out, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    if (int rc = check_model(model, d_e, d_r)) return rc;
    if (int rc = closed(kge::E_RANK_REL_EVAL, model, "kge_rank_rel_eval")) return rc;
    if (model == KGE_TRANSR && !proj) return fail(KGE_ERR_ARG, "kge_rank_rel_eval: TransR needs the projection table");
    if (!ent || !rel || n_ent <= 0 || n_rel <= 0 || E < 0 || (E && (!h || !r || !t || !ranks)) || !ws)
        return fail(KGE_ERR_ARG, "kge_rank_rel_eval: bad argument (a null pointer or a count that is not positive)");
    if (n_rel > 0x7fffffff) return fail(KGE_ERR_ARG, "kge_rank_rel_eval: bad relation count %lld", (long long)n_rel);
    if (Eb <= 0) return fail(KGE_ERR_ARG, "kge_rank_rel_eval: Eb must be positive (got %d)", Eb);
    if (!filt_ptr || !filt_ids)
        return fail(KGE_ERR_ARG, "kge_rank_rel_eval: filt_ptr and filt_ids are required (every list holds the triple's own relation)");
    if (E == 0) return KGE_OK;
    if (Eb > E) Eb = (int)E;
    hipStream_t s = (hipStream_t)stream;
    Carver cv(ws, ws_bytes); RelBufs w;
    const size_t need = carve_rank_rel(cv, w, model, Eb, n_rel, d_e, d_r);
    if (need > ws_bytes) return fail(KGE_ERR_WORKSPACE, "kge_rank_rel_eval: workspace too small (%zu < %zu)", ws_bytes, need);
    const float rot_div = rot_div_of(emb_init);
    // the width and the form of the (query row, relation row) product
    const int D = model == KGE_RESCAL ? d_e * d_e : d_e;
    const int form = model == KGE_TRANSE_L1 ? KGE_TRANSE_L1 : model == KGE_TRANSE_L2 ? KGE_TRANSE_L2 : KGE_DISTMULT;
    const bool matrix = model != KGE_TRANSE_L1 && model != KGE_ROTATE && model != KGE_TRANSR;
    const bool gemm = matrix && !(flags & KGE_FLAG_FORCE_PAIRWISE) && rank_gemm_supported(form, D);
    const bool l2g = gemm && model == KGE_TRANSE_L2;
    if (l2g) {       // |c|^2 of every relation row, once
        EdgeFwdArgs nb{};
        nb.B = 0; nb.d_e = d_e; nb.d_r = d_r; nb.model = model; nb.nbase = rel; nb.nidx = nullptr; nb.n_neg = (int)n_rel;
        nb.bsq = w.csq;
        KGE_TRY(launch_edge_fwd(nb, s));
    }
    if (model == KGE_TRANSR) KGE_TRY(launch_rel_neg_rows(rel, n_rel, d_r, w.RQ, w.ids, std::max<int64_t>(n_rel, Eb), s));
    // QuatE: s_j = <conj(h) (x) t, r^_j> - the product runs against the normalised rows
    const float *relc = rel;
    if (model == KGE_QUATE) { KGE_TRY(launch_rel_unit_rows(rel, n_rel, d_r, w.RN, s)); relc = w.RN; }
    for (int64_t e0 = 0; e0 < E; e0 += Eb) {
        const int rows = (int)((E - e0) < Eb ? (E - e0) : Eb);
        float *P = pos_score_out ? pos_score_out + e0 : w.P;
        // positive scores: the forward of the true triples, as kge_rank_eval forms them (no pos-side vectors: the query rows follow)
        KGE_TRY(rank_pos_side(model, 0, ent, rel, proj, h + e0, r + e0, t + e0, rows, d_e, d_r, gamma, rot_div, P, nullptr, nullptr,
                              nullptr, w, s));
        if (model == KGE_TRANSR) {
            TransRArgs tp{};
            tp.B = rows; tp.C = 1; tp.chunk = rows; tp.De = d_e; tp.Dr = d_r; tp.gamma = gamma; tp.ent = ent;
            tp.h_gid = h + e0; tp.t_gid = t + e0; tp.rel_ids = r + e0; tp.rel = rel; tp.proj = const_cast<float *>(proj);
            tp.HP = w.THP; tp.TP = w.TTP; tp.Q = w.TQ; tp.SG = w.TSG; tp.P = P;
            KGE_TRY(launch_transr_pos(tp, s));
        }
        if (model == KGE_ROTATE) {
            KGE_TRY(launch_rel_rotate_score(ent, rel, h + e0, t + e0, rows, n_rel, d_e, gamma, rot_div, w.S, s));
            KGE_TRY(launch_rank_count(w.S, P, rows, n_rel, filt_ptr, filt_ids, e0, ranks, s));
            continue;
        }
        KGE_TRY(launch_rel_query(model, ent, h + e0, t + e0, rows, d_e, w.Q, l2g ? w.qsq : nullptr, s));
        if (model == KGE_TRANSR) {
            // the training forward with the roles exchanged: "positive" j = relation j (matrix P_j, q row -c_j), the batch's u rows
            // are the one chunk's shared "negatives": S[j, i] = gamma - |u_i P_j + c_j|_1
            TransRArgs tr{};
            tr.B = (int)n_rel; tr.C = 1; tr.chunk = (int)n_rel; tr.N = rows; tr.De = d_e; tr.Dr = d_r; tr.gamma = gamma;
            tr.ent = w.Q; tr.cent = w.Q; tr.neg_ids = w.ids; tr.rel_ids = w.ids; tr.rel = rel; tr.proj = const_cast<float *>(proj);
            tr.Q = w.RQ; tr.S = w.S; tr.Z = nullptr;
            KGE_TRY(launch_transr_fwd(tr, s));
            KGE_TRY(launch_rank_count(w.S, P, rows, n_rel, filt_ptr, filt_ids, e0, ranks, s, true));
        } else if (gemm) {
            KGE_TRY(launch_rank_gemm(form, w.Q, rows, relc, nullptr, n_rel, D, gamma, clamp_of(model), w.qsq, w.csq, P, w.S, filt_ptr,
                                     filt_ids, e0, ranks, s));
        } else {
            NegArgs na; fill_pair(na, form, 1, rows, (int)n_rel, D, gamma, w.Q, relc, nullptr);
            na.clampv = clamp_of(model);
            na.S = w.S;
            KGE_TRY(launch_neg_fwd_pair(na, s));
            KGE_TRY(launch_rank_count(w.S, P, rows, n_rel, filt_ptr, filt_ids, e0, ranks, s));
        }
    }
    return KGE_OK;
}

int kge_step_sharded(const kge_hparams *hp, const kge_shards *sh, const kge_batch *b,
                     const kge_step_out *out, void *ws, size_t ws_bytes, void *stream) {
    if (!sh) return fail(KGE_ERR_ARG, "kge_step_sharded: null shard map");
    if (hp) if (int rc = closed(kge::E_STEP_SHARDED, hp->model, "kge_step_sharded")) return rc;
    if (int rc = norm_closed(hp, "kge_step_sharded")) return rc;
    // (RESCAL's relation "row" is a d_e x d_e matrix streamed by its own kernels: only the entity width is bounded)
    if (hp && (hp->d_e % 4 || hp->d_e > 1024 || (hp->model != KGE_RESCAL && (hp->d_r % 4 || hp->d_r > 1024))))
        return fail(KGE_ERR_ARG, "kge_step_sharded: row widths must be multiples of 4 and <= 1024 floats");
    kge_tables tb{};
    tb.n_ent = sh->n_ent; tb.n_rel = sh->n_rel;
    if (sh->rel_local) {              // ABI 8: relation-side tables local to this rank (relation ids resolve to them directly)
        tb.rel = sh->rel_local; tb.rel_state = sh->rel_state_local;
        tb.proj = sh->proj_local; tb.proj_state = sh->proj_state_local;
    }
    StepCall c; c.sh = sh;
    return run_step(hp, &tb, b, out, ws, ws_bytes, stream, c);
}

int kge_gather_rows_sharded(float *const *shard_rows, int n_shards, int64_t rows_per_shard, int dim,
                            const int64_t *idx, int64_t n_idx, float *out, void *stream) {
    if (!shard_rows || n_shards < 1 || rows_per_shard <= 0 || dim <= 0 || n_idx < 0 || (n_idx && (!idx || !out)))
        return fail(KGE_ERR_ARG, "kge_gather_rows_sharded: bad argument");
    KGE_TRY(launch_gather_rows_sharded(shard_rows, n_shards, rows_per_shard, dim, idx, n_idx, out, (hipStream_t)stream));
    return KGE_OK;
}

int kge_ipc_export(const void *dev_ptr, void *handle64, int64_t *offset) {
    static_assert(sizeof(hipIpcMemHandle_t) == KGE_IPC_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
    if (!dev_ptr || !handle64 || !offset) return fail(KGE_ERR_ARG, "kge_ipc_export: null argument");
    hipDeviceptr_t base = nullptr; size_t size = 0;
    hipError_t e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)dev_ptr);
    if (e != hipSuccess) return fail(KGE_ERR_LAUNCH, "hipMemGetAddressRange: %s", hipGetErrorString(e));
    hipIpcMemHandle_t h;
    e = hipIpcGetMemHandle(&h, base);
    if (e != hipSuccess) return fail(KGE_ERR_LAUNCH, "hipIpcGetMemHandle: %s", hipGetErrorString(e));
    memcpy(handle64, &h, sizeof(h));
    *offset = (int64_t)((const char *)dev_ptr - (const char *)base);
    return KGE_OK;
}

int kge_ipc_open(const void *handle64, void **base) {
    if (!handle64 || !base) return fail(KGE_ERR_ARG, "kge_ipc_open: null argument");
    hipIpcMemHandle_t h;
    memcpy(&h, handle64, sizeof(h));
    hipError_t e = hipIpcOpenMemHandle(base, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return fail(KGE_ERR_LAUNCH, "hipIpcOpenMemHandle: %s", hipGetErrorString(e));
    return KGE_OK;
}

int kge_ipc_close(void *base) {
    if (!base) return KGE_OK;
    hipError_t e = hipIpcCloseMemHandle(base);
    if (e != hipSuccess) return fail(KGE_ERR_LAUNCH, "hipIpcCloseMemHandle: %s", hipGetErrorString(e));
    return KGE_OK;
}

}  // extern "C"
