// kge_own_fwd.hpp - the host drivers of the models with an edge forward of their own (ModelRow::own_fwd: PairRE, TransH, TransD;
// kernels in kge_pairre.hip, kge_transh.hip, kge_transd.hip).  Their host sequence is the same four operations wherever it runs -
// the strict step, the modular score entries, single-table and chunked ranking, the query rows of top-K:
//
//   own_carve     the buffers of one block of B edges against CN candidate rows, N per chunk
//   own_prepare   the edge forward of B edges (+ the candidate-row jobs of the same launch)
//   own_scores    the chunked scores of a block into S
//   own_backward  dL/dS -> the candidates' gradient rows, then the per-edge head / tail / relation rows
//
// Each is written once per model and has ONE dispatch point, the switch of its own_* function.  The functions only enqueue kernels
// and return the launchers' codes; which kernel INSTANCE ranks or selects (launch_rank_gemm_transh / _transd, the ACC_* kinds of
// top-K) stays with those entries.  Host only.
#pragma once
#include "kge_common.hpp"

namespace kge {

inline float clamp_of(int model) { return model == KGE_SIMPLE ? KGE_SIMPLE_CLAMP : 0.f; }

inline void fill_gemm(GemmArgs &g, int model, int C, int chunk, int N, int d_e, float gamma, const float *A, const float *nbase, const int64_t *nidx) {
    g = GemmArgs{};
    g.model = model; g.C = C; g.chunk = chunk; g.N = N; g.D = d_e; g.gamma = gamma;
    g.A = A; g.nbase = nbase; g.nidx = nidx; g.B = C * chunk; g.clampv = clamp_of(model);
}
inline void fill_pair(NegArgs &na, int model, int C, int chunk, int N, int d_e, float gamma, const float *A, const float *nbase, const int64_t *nidx) {
    na = NegArgs{};
    na.model = model; na.C = C; na.chunk = chunk; na.N = N; na.d_e = d_e; na.gamma = gamma;
    na.A = A; na.nbase = nbase; na.nidx = nidx; na.clampv = clamp_of(model);
}

// where the per-edge operand of a block and the scalars of its rows and candidates live.  Each model uses the entries it has:
//                                     PairRE           TransH                      TransD (k = d_e / 2)
struct OwnOperand {
    float *A;                       // a [B, d_e]       stacked (a, w^) [2 B, d_e]  stacked (a, rho) [2 B, k]
    float *W;                       // w [B, d_e]       w^, rho when the operand is NOT stacked (own_prepare, chunk == 0): a alone in A
    float *alpha;                   // -                |a|^2 [B]                   |a|^2 [B]
    float *r1, *r2;                 // -                w^ . a [B], -               |rho|^2 [B], a . rho [B]
    float *beta;                    // |n| [n]          |n|^2 [n]                   |n|^2 [n]       of the n candidate rows
    float *cj, *Nh;                 // -                -                           m . n [n], the rows' dense first halves [n, k]
};
// the candidate rows a prepare launch reads next to its edges: base + (idx ? idx[j] : j) * d_e, or the neg_deg_sample id scheme
// (EdgeFwdArgs); Bn: their dense copy or null
struct OwnCands { const float *nbase; const int64_t *nidx; int n_neg; const int64_t *nd_own; int nd_chunk, nd_Ns; float *Bn; };
// one chunked scoring block: C chunks of `chunk` rows against N candidate rows each, and (TransH, TransD) its raw products p | q
struct OwnBlock { int C, chunk, N, d_e; float gamma; OwnOperand o; const float *nbase; const int64_t *nidx; float *PQ; };
// the buffers of a block in the strict step and the modular entries: the operand, the products and the terms of the backward
struct OwnBufs {
    OwnOperand o; float *PQ;
    float *PQc, *rs, *k1, *rc2, *cs, *gc;     // P' | Q'; row terms (k1: TransH's kappa, TransD's rc); column terms
    float *GA, *GW, *GNp;                     // Ga (PairRE) / the stacked Ga | Gw^, Ga | Grho; Gw (PairRE); TransD's Gn products [CN, k]
};
// what the backward does beyond the negative rows' gradients; everything may stay zero (the modular entries)
struct OwnBwd {
    const float *dpos;                        // [B] dL/dp: the positive edge's part
    float reg_coef; int reg_norm;             // regulariser of the relation row (reg_norm also: of the candidate rows)
    float n_reg_coef;                         // regulariser of the candidate rows
    bool nd;                                  // neg_deg_sample: the in-batch negative rows' gradient joins the positive trace
    float *GH, *GT, *GR;                      // which of them receive the per-edge gradients
    bool products;                            // PQ is not there yet (no forward ran on these buffers): run the products first
};

// A, asq, bsq, GA: the entries every model has ([B, d_e], [B], [CN], [B, d_e]); PairRE's a and Ga and the stacked models' |a|^2 and
// |n|^2 live there.  The Carver sequence is the layout of include/kge_hip.h
template <class CV>
void own_carve(int model, CV &cv, OwnBufs &t, float *A, float *asq, float *bsq, float *GA, size_t B, size_t CN, size_t N, size_t d_e) {
    t = OwnBufs{};
    const size_t k = d_e / 2;
    switch (model) {
    case KGE_PAIRRE:
        t.o.A = A; t.GA = GA;
        t.o.W = cv.f(B * d_e); t.GW = cv.f(B * d_e); t.o.beta = cv.f(CN);       // w, Gw, candidate norms
        break;
    case KGE_TRANSH:
        t.o.alpha = asq; t.o.beta = bsq;
        t.o.A = cv.f(2 * B * d_e); t.o.r1 = cv.f(B);            // (a, w^) stacked; w^ . a (|a|^2, |n|^2: the asq / bsq entries)
        t.PQ = cv.f(2 * B * N); t.PQc = cv.f(2 * B * N);        // raw p | q; P' | Q'
        t.rs = cv.f(B); t.k1 = cv.f(B); t.cs = cv.f(CN);        // row and column terms of the backward
        t.GA = cv.f(2 * B * d_e);                               // Ga | Gw^ products
        break;
    case KGE_TRANSD:
        t.o.alpha = asq; t.o.beta = bsq;
        t.o.A = cv.f(2 * B * k); t.o.r1 = cv.f(B); t.o.r2 = cv.f(B);    // (a, rho) stacked; |rho|^2, a . rho (|a|^2, |n|^2: the asq / bsq entries)
        t.o.cj = cv.f(CN); t.o.Nh = cv.f(CN * k);                       // m . n and the dense first half of every candidate row
        t.PQ = cv.f(2 * B * N); t.PQc = cv.f(2 * B * N);                // raw p | q; P' | Q'
        t.rs = cv.f(B); t.k1 = cv.f(B); t.rc2 = cv.f(B);                // row sums of the backward
        t.cs = cv.f(CN); t.gc = cv.f(CN);                               // its column sums
        t.GA = cv.f(2 * B * k); t.GNp = cv.f(CN * k);                   // Ga | Grho and Gn products
        break;
    }
}

// chunk: the rows per chunk of the stacked operand; 0: two blocks, a in o.A and the second vector in o.W (PairRE: always).
// B == 0: the candidate-row jobs alone
inline int own_prepare(int model, const EdgeSrc &src, int B, int chunk, int d_e, int neg_head, float gamma, float *P, const OwnOperand &o,
                       const OwnCands *c, hipStream_t s) {
    static const OwnCands none{};
    if (!c) c = &none;
    switch (model) {
    case KGE_PAIRRE: {
        PairreEdgeArgs e{};
        e.src = src; e.B = B; e.d_e = d_e; e.neg_head = neg_head; e.gamma = gamma; e.pos_score = P; e.A = o.A; e.W = o.W;
        e.nbase = c->nbase; e.nidx = c->nidx; e.n_neg = c->n_neg; e.nd_own = c->nd_own; e.nd_chunk = c->nd_chunk; e.nd_Ns = c->nd_Ns;
        e.Bn = c->Bn; e.nrm = o.beta;
        return launch_pairre_edge_fwd(e, s);
    }
    case KGE_TRANSH: {
        TranshEdgeArgs e{};
        e.src = src; e.B = B; e.chunk = chunk ? chunk : B; e.d_e = d_e; e.neg_head = neg_head; e.gamma = gamma; e.pos_score = P;
        e.AW = o.A; e.W = chunk ? nullptr : o.W; e.alpha = o.alpha; e.cw = o.r1;
        e.nbase = c->nbase; e.nidx = c->nidx; e.n_neg = c->n_neg; e.nd_own = c->nd_own; e.nd_chunk = c->nd_chunk; e.nd_Ns = c->nd_Ns;
        e.Bn = c->Bn; e.beta = o.beta;
        return launch_transh_edge_fwd(e, s);
    }
    case KGE_TRANSD: {
        TransdEdgeArgs e{};
        e.src = src; e.B = B; e.chunk = chunk ? chunk : B; e.d_e = d_e; e.neg_head = neg_head; e.gamma = gamma; e.pos_score = P;
        e.AP = o.A; e.W = chunk ? nullptr : o.W; e.alpha = o.alpha; e.sig = o.r1; e.u = o.r2;
        e.nbase = c->nbase; e.nidx = c->nidx; e.n_neg = c->n_neg; e.nd_own = c->nd_own; e.nd_chunk = c->nd_chunk; e.nd_Ns = c->nd_Ns;
        e.Bn = c->Bn; e.Nh = o.Nh; e.beta = o.beta; e.cj = o.cj;
        return launch_transd_edge_fwd(e, s);
    }
    }
    return KGE_ERR_ARG;
}

// the scalars (and TransD: the dense first halves) of n candidate rows base + (idx ? idx[j] : j) * d_e into o.beta, o.cj, o.Nh
inline int own_cand_rows(int model, const float *base, const int64_t *idx, int64_t n, int d_e, const OwnOperand &o, hipStream_t s) {
    const OwnCands c{base, idx, (int)n, nullptr, 0, 0, nullptr};
    return own_prepare(model, EdgeSrc{}, 0, 0, d_e, 0, 0.f, nullptr, OwnOperand{nullptr, nullptr, nullptr, nullptr, nullptr, o.beta, o.cj, o.Nh}, &c, s);
}

inline void own_fill_neg(PairreNegArgs &n, const OwnBlock &k) {
    n = PairreNegArgs{};
    n.C = k.C; n.chunk = k.chunk; n.N = k.N; n.d_e = k.d_e; n.gamma = k.gamma; n.A = k.o.A; n.W = k.o.W; n.nbase = k.nbase; n.nidx = k.nidx;
    n.nrm = k.o.beta;
}
inline void own_fill_neg(TranshNegArgs &n, const OwnBlock &k) {
    n = TranshNegArgs{};
    n.C = k.C; n.chunk = k.chunk; n.N = k.N; n.d_e = k.d_e; n.gamma = k.gamma; n.alpha = k.o.alpha; n.cw = k.o.r1; n.beta = k.o.beta; n.PQ = k.PQ;
}
inline void own_fill_neg(TransdNegArgs &n, const OwnBlock &k) {
    n = TransdNegArgs{};
    n.C = k.C; n.chunk = k.chunk; n.N = k.N; n.gamma = k.gamma; n.alpha = k.o.alpha; n.sig = k.o.r1; n.u = k.o.r2; n.beta = k.o.beta;
    n.cj = k.o.cj; n.PQ = k.PQ;
}
// TransH, TransD: the DistMult form of the tiles of kge_neg_gemm.hip over the stacked operand (2 chunk rows per chunk).  TransH:
// [A ; W^] against the candidate rows; TransD: [A ; P] (k columns) against the candidates' dense first halves
inline void own_fill_gemm(int model, GemmArgs &g, const OwnBlock &k) {
    if (model == KGE_TRANSH) fill_gemm(g, KGE_DISTMULT, k.C, 2 * k.chunk, k.N, k.d_e, k.gamma, k.o.A, k.nbase, k.nidx);
    else fill_gemm(g, KGE_DISTMULT, k.C, 2 * k.chunk, k.N, k.d_e / 2, k.gamma, k.o.A, k.o.Nh, nullptr);
}
// p | q = the stacked operand . candidates^T on the forward tiles
inline int own_products(int model, const OwnBlock &k, hipStream_t s) {
    GemmArgs g; own_fill_gemm(model, g, k);
    g.S = k.PQ;
    return launch_neg_fwd_gemm(g, s);
}

inline int own_scores(int model, const OwnBlock &k, float *S, hipStream_t s) {
    switch (model) {
    case KGE_PAIRRE: {
        PairreNegArgs n; own_fill_neg(n, k);
        n.S = S;
        return launch_pairre_neg_fwd(n, s);
    }
    case KGE_TRANSH: {
        if (int rc = own_products(model, k, s)) return rc;
        TranshNegArgs n; own_fill_neg(n, k);
        n.S = S;
        return launch_transh_score(n, s);
    }
    case KGE_TRANSD: {
        if (int rc = own_products(model, k, s)) return rc;
        TransdNegArgs n; own_fill_neg(n, k);
        n.S = S;
        return launch_transd_score(n, s);
    }
    }
    return KGE_ERR_ARG;
}

// TransH, TransD: the coefficient blocks are in t.PQc -> the products t.GA (stacked) and GN (TransH: the candidates' gradient rows;
// TransD: t.GNp, their first halves' part) on the backward tiles in their DistMult form with K = 2 chunk; beyond the rows a tile's workgroup indexes (GB_MAXK) the pairwise kernels, which take any size
inline int own_bwd_products(int model, const OwnBlock &k, const OwnBufs &t, float *GN, hipStream_t s) {
    GemmArgs g; own_fill_gemm(model, g, k);
    g.W = t.PQc; g.GA = t.GA; g.GN = GN;
    if ((2 * k.chunk > k.N ? 2 * k.chunk : k.N) <= KGE_NEG_BWD_GEMM_MAXK) return launch_neg_bwd_gemm(g, s);
    // decided here: any error of the launcher stays an error.  Both sides are tested by the s7 shapes of tests/new_model_shape_cases.py,
    // TransH and TransD: s7a (2 chunk = 2064) and s7b (N = 2049) come here, s7c (2 chunk = 2048) is the last shape on the tiles
    NegArgs na; fill_pair(na, KGE_DISTMULT, g.C, g.chunk, g.N, g.D, g.gamma, g.A, g.nbase, g.nidx);
    na.W = t.PQc; na.GA = t.GA; na.GN = GN;
    return launch_neg_bwd_pair(na, s);
}

// G = dL/dS of the block k whose buffers are *bufs (B = k.C * k.chunk edges from src) -> GN [C*N, d_e] and the rows x asks for.
// bufs == null: the positive edges alone (x.dpos) - no negative backward, nothing of a block enters the edge backward
inline int own_backward(int model, const OwnBlock &k, const OwnBufs *bufs, const EdgeSrc &src, int neg_head, const float *G, float *GN,
                        const OwnBwd &x, hipStream_t s) {
    static const OwnBufs none{};
    const OwnBufs &t = bufs ? *bufs : none;
    const int B = k.C * k.chunk;
    switch (model) {
    case KGE_PAIRRE: {
        PairreNegArgs n; own_fill_neg(n, k);
        n.G = G; n.GA = t.GA; n.GW = t.GW; n.GN = GN; n.reg_coef = x.n_reg_coef; n.reg_norm = x.reg_norm;
        if (bufs) if (int rc = launch_pairre_neg_bwd(n, s)) return rc;
        PairreBwdArgs e{};
        e.src = src; e.B = B; e.d_e = k.d_e; e.neg_head = neg_head; e.dpos = x.dpos; e.GA = t.GA; e.GW = t.GW;
        e.reg_coef = x.reg_coef; e.reg_norm = x.reg_norm; e.GH = x.GH; e.GT = x.GT; e.GR = x.GR;
        if (x.nd) { e.GNd = GN; e.nd_chunk = k.chunk; e.nd_Np = k.N; }       // in-batch negative rows -> positive trace
        return launch_pairre_edge_bwd(e, s);
    }
    case KGE_TRANSH: {
        if (x.products) if (int rc = own_products(model, k, s)) return rc;
        TranshNegArgs n; own_fill_neg(n, k);
        n.G = G; n.PQc = t.PQc; n.rs = t.rs; n.kap = t.k1; n.cs = t.cs;
        if (bufs) if (int rc = launch_transh_coef(n, s)) return rc;
        if (bufs) if (int rc = own_bwd_products(model, k, t, GN, s)) return rc;
        TranshBwdArgs e{};
        e.src = src; e.B = B; e.chunk = k.chunk; e.d_e = k.d_e; e.neg_head = neg_head; e.dpos = x.dpos;
        e.GAW = t.GA; e.rs = t.rs; e.kap = t.k1;
        e.reg_coef = x.reg_coef; e.reg_norm = x.reg_norm; e.GH = x.GH; e.GT = x.GT; e.GR = x.GR;
        e.nbase = k.nbase; e.n_neg = k.C * k.N; e.cs = t.cs; e.GN = GN; e.n_reg_coef = x.n_reg_coef;
        if (x.nd) { e.GNd = GN; e.nd_chunk = k.chunk; e.nd_Np = k.N; }
        return launch_transh_edge_bwd(e, s);
    }
    case KGE_TRANSD: {
        if (x.products) if (int rc = own_products(model, k, s)) return rc;
        TransdNegArgs n; own_fill_neg(n, k);
        n.G = G; n.PQc = t.PQc; n.rs = t.rs; n.rc = t.k1; n.rc2 = t.rc2; n.cs = t.cs; n.gc = t.gc;
        if (bufs) if (int rc = launch_transd_coef(n, s)) return rc;
        if (bufs) if (int rc = own_bwd_products(model, k, t, t.GNp, s)) return rc;      // k columns: the edge backward assembles GN from them
        TransdBwdArgs e{};
        e.src = src; e.B = B; e.chunk = k.chunk; e.d_e = k.d_e; e.neg_head = neg_head; e.dpos = x.dpos;
        e.GAP = t.GA; e.rs = t.rs; e.rc = t.k1; e.rc2 = t.rc2;
        e.reg_coef = x.reg_coef; e.reg_norm = x.reg_norm; e.GH = x.GH; e.GT = x.GT; e.GR = x.GR;
        e.nbase = k.nbase; e.n_neg = k.C * k.N; e.cs = t.cs; e.gc = t.gc; e.GNp = t.GNp; e.GN = GN; e.n_reg_coef = x.n_reg_coef;
        if (x.nd) { e.GNd = GN; e.nd_chunk = k.chunk; e.nd_Np = k.N; }
        return launch_transd_edge_bwd(e, s);
    }
    }
    return KGE_ERR_ARG;
}

}  // namespace kge
