"""Case table and input builders of the per-op ("modular") C-ABI tests (test infrastructure; a plain module, not a conftest).

The per-op entry points (kge_score_pos / _bwd, kge_score_neg_fwd / _bwd, kge_pnorm_pow / _bwd, kge_mask_diag, kge_gather_rows,
kge_scatter_add_rows, kge_adagrad_scatter, kge_adagrad_apply_rows, kge_rank_from_scores) are what INTEGRATION.md offers to a
reference maintainer and what the drop-in KEModel is built from; they do not run the fused step's code.  The cases below are
shared by
  tests/test_modular_op_inputs.py   (CPU): every case through the oracle in float32 and float64 - the inputs exercise what they
                                    claim and the reference alone stays inside every cap;
  tests/test_gpu_modular_ops.py     (GPU): every op against a float64 statement of the same operation on the same float32 inputs.

References.  numpy: oracle/kge_oracle.py, evaluated chunk by chunk (oracle_neg) so that a pairwise [rows, N, D] float64 block
stays near 128 MB.  torch float64 (torch_neg; on the device in the GPU file, on the CPU in the cross-check of the CPU file): the
same formulas, for the shapes where numpy is too slow.

Exclusions (conditions, not measurements - asserted by both files, ROW_CAP of loss_option_cases.py):
  TransE_l1   sign(a - b) where |a - b| < L1_TAU * max(1, |a| / 0.09) in float64: the float32 pos-side vector fl(x +- r) may sit
              on the other side of b; the gradient rows such an element feeds are excluded (l1_ambiguous);
  SimplE      a float64 score within 1e-4 of the clamp at +-20: the clamp's gradient mask may differ (clamp_edge).
"""
import os
import zlib

import numpy as np

from loss_option_cases import ROW_CAP, SHAPES as RECIPE_SHAPES
from oracle import kge_oracle as O

FORCE_PAIRWISE, TWO_PASS_PAIR = 1, 16                 # include/kge_hip.h KGE_FLAG_*
GB_MAXK = 2048                                        # kge_neg_gemm.hip: rows of a chunk operand a backward GEMM workgroup indexes
SCORE_RTOL = SCORE_ATOL = 1e-4                        # the suite's score tolerance (BASELINE north star)
GRAD_RTOL = 3e-4                                      # of the largest component of the compared array (test_gpu_parity.grad_tol)
L1_TAU = 4e-9
CLAMP = O.SIMPLE_CLAMP
CLAMP_BAND = 1e-4
MODELS = ("TransE_l1", "TransE_l2", "DistMult", "ComplEx", "RotatE", "SimplE", "RESCAL")
MATRIX_MODELS = ("TransE_l2", "DistMult", "ComplEx", "SimplE", "RESCAL")
PAIR_MODELS = ("TransE_l1", "RotatE")
N_ENT_FB15K = 14951


def rel_width(model, d_e):
    return d_e // 2 if model == "RotatE" else (d_e * d_e if model == "RESCAL" else d_e)


def width_ok(model, d_e):
    return d_e % 2 == 0 or model in ("TransE_l1", "TransE_l2", "DistMult", "RESCAL")


def bcast_ok(model, d_e):
    """kge_neg_bcast.hip neg_bcast_supported"""
    return (d_e // 2) % 8 == 0 if model == "RotatE" else d_e % 16 == 0


def kernel_path(model, chunk, N, d_e, flags):
    """the kernel instances kge_score_neg_fwd / _bwd reach for a case (kge_api.hip use_mfma, kge_neg_pair.hip launch_neg_*_pair,
    kge_neg_bcast.hip launch_neg_bwd_bcast) - named in every case id"""
    gemm = model in MATRIX_MODELS and d_e % 4 == 0 and not (flags & FORCE_PAIRWISE)
    pair = "bcast" if bcast_ok(model, d_e) else "pair32"
    if pair == "bcast" and model in PAIR_MODELS:
        shared = N % 4 == 0 and not (flags & TWO_PASS_PAIR)
        bwd_pair = "lc_shared" if shared else "bcast_two_pass"
    else:
        bwd_pair = pair
    if gemm:
        return "fwd_gemm+" + ("bwd_gemm" if max(chunk, N) <= GB_MAXK else "bwd_%s_beyond_maxk" % bwd_pair)
    return "fwd_%s+bwd_%s" % (pair, bwd_pair)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def simple_clamp_scale(d_e, sigma=15.0):
    """table scale for which SimplE's raw score 0.5 * sum_k a_k b_k (a = product of two U(-s, s), b ~ U(-s, s)) has standard
    deviation `sigma`: 0.5 * sqrt(d_e / 27) * s^3"""
    return float((sigma / (0.5 * np.sqrt(d_e / 27.0))) ** (1.0 / 3.0))


# --------------------------------------------------------------------------------------------------------------------------
# (a) score_neg
# --------------------------------------------------------------------------------------------------------------------------
def neg_case(model, C, chunk, N, d_e, flags=0, scale=1.0, gamma=12.0, kind="plain", fwd_only=False, tag=""):
    c = dict(model=model, C=C, chunk=chunk, N=N, d_e=d_e, d_r=rel_width(model, d_e), flags=flags, scale=scale, gamma=gamma,
             emb_init=scale, kind=kind, fwd_only=fwd_only)
    path = kernel_path(model, chunk, N, d_e, flags)
    c["path"] = path.split("+")[0] if fwd_only else path
    c["id"] = "%s%s-C%d-c%d-N%d-D%d-f%d-%s" % (model, "-" + (tag or kind) if (tag or kind != "plain") else "", C, chunk, N, d_e, flags, c["path"])
    return c


def _flag_set(model):
    return (0, FORCE_PAIRWISE) if model in MATRIX_MODELS else (0, TWO_PASS_PAIR)


def _neg_cases():
    out = []

    def add(model, shape, flags=None, **kw):
        if not width_ok(model, shape[3]) or (model == "RESCAL" and shape[3] > 1024):
            return
        for f in (_flag_set(model) if flags is None else flags):
            out.append(neg_case(model, *shape, flags=f, **kw))

    # ---- the recipes' shapes (tests/test_gpu_parity.py SHAPES: chunk = N = neg_sample_size, D = the recipes' row width)
    for m in ("TransE_l2", "DistMult", "TransE_l1"):
        add(m, (5, 200, 200, 400), scale=0.125, gamma=48.0, tag="recipe")
    for m in ("ComplEx", "RotatE"):
        add(m, (4, 256, 256, 400), scale=0.125, gamma=48.0, tag="recipe")
    add("SimplE", (4, 128, 128, 400), tag="recipe")
    add("RESCAL", (4, 64, 64, 64), tag="recipe")
    add("RESCAL", (4, 64, 64, 100), tag="recipe")
    # ---- ragged and degenerate sizes; widths that change the instance (30 / 18: no 16-byte rows -> generic 32 x 32 pair kernel
    #      for the matrix models too; 36: ragged k stage of the MFMA tiles; 4: one k step)
    for m in MODELS:
        for shape in ((3, 37, 44, 48), (1, 129, 260, 112), (3, 1, 7, 32), (2, 9, 1, 32), (2, 5, 6, 4), (2, 20, 24, 36), (2, 20, 24, 30),
                      (2, 20, 24, 18), (1, 8, 12, 2048)):
            add(m, shape)
    # ---- TransE_l1 / RotatE: d_e 40 / 24 / 20 have no bcast kernel ((d_e / 2) % 8 for RotatE, d_e % 16 for TransE_l1); 16 has, and
    #      with it the shared-pair backward (neg_bwd_lc_supported: d_e % 4 for RotatE, d_e % 2 for TransE_l1) unless N % 4 != 0
    for shape in ((2, 20, 24, 40), (2, 20, 24, 16), (2, 20, 22, 16), (2, 20, 24, 20)):
        add("TransE_l1", shape)
    for shape in ((2, 20, 24, 24), (2, 20, 24, 16), (2, 20, 22, 16), (2, 20, 24, 20)):
        add("RotatE", shape)
    # ---- the backward GEMM's row limit: both sides of it, the gradients must match on both
    for m in ("TransE_l2", "DistMult"):
        for shape in ((1, 8, GB_MAXK, 64), (1, 8, GB_MAXK + 1, 64), (1, GB_MAXK + 1, 8, 64)):
            add(m, shape, flags=(0,), tag="maxk")
    # ---- the evaluation shape (infer / forward_test: one chunk of test triples against every entity), forward only
    for m in ("TransE_l2", "DistMult", "ComplEx", "RotatE"):
        add(m, (1, 64, N_ENT_FB15K, 400), flags=(0,), scale=0.125, gamma=48.0, fwd_only=True, tag="eval")
    for m in ("TransE_l2", "DistMult", "ComplEx"):
        add(m, (1, 1000, N_ENT_FB15K, 400), flags=(0,), scale=0.125, gamma=48.0, fwd_only=True, tag="eval")
    # ---- SimplE with a share of the scores in the clamp; TransE_l2 with one negative row equal to its pos-side vector
    add("SimplE", (4, 128, 128, 400), scale=simple_clamp_scale(400), kind="clamp")
    add("SimplE", (3, 37, 44, 48), scale=simple_clamp_scale(48), kind="clamp")
    add("SimplE", (2, 20, 24, 30), scale=simple_clamp_scale(30), kind="clamp")
    add("TransE_l2", (3, 37, 44, 48), kind="coincident")
    return out


NEG_CASES = _neg_cases()
COINCIDENT = (1, 5, 7)          # (chunk index, positive row, negative row) of the planted pair of a 'coincident' case


def neg_inputs(c, neg_head):
    """float32 x [B, d_e] (the uncorrupted entity), r [B, d_r], nb [C * N, d_e], W [C, chunk, N] (a random signed dL/dn)"""
    rng = np.random.RandomState(_seed("neg", c["model"], c["C"], c["chunk"], c["N"], c["d_e"], c["kind"], bool(neg_head)))
    s, B = c["scale"], c["C"] * c["chunk"]
    inp = dict(x=rng.uniform(-s, s, (B, c["d_e"])).astype(np.float32), r=rng.uniform(-s, s, (B, c["d_r"])).astype(np.float32),
               nb=rng.uniform(-s, s, (c["C"] * c["N"], c["d_e"])).astype(np.float32),
               W=rng.uniform(-1, 1, (c["C"], c["chunk"], c["N"])).astype(np.float32))
    if c["kind"] == "coincident":       # relation 0: a = x exactly, in every precision
        ci, i, j = COINCIDENT
        inp["r"][ci * c["chunk"] + i] = 0.0
        inp["nb"][ci * c["N"] + j] = inp["x"][ci * c["chunk"] + i]
    return inp


def _blocks(c, elems):
    """(chunk index, first row, end row) blocks with rows * N * d_e <= elems"""
    blk = max(1, min(c["chunk"], elems // max(1, c["N"] * c["d_e"])))
    return [(ci, i0, min(c["chunk"], i0 + blk)) for ci in range(c["C"]) for i0 in range(0, c["chunk"], blk)]


def oracle_neg(c, neg_head, inp, dtype=np.float64, grads=True, elems=1 << 24):
    """the oracle's pos_side -> score_neg -> score_neg_bwd -> pos_side_bwd in `dtype`, block by block.
    Returns dict(score [C, chunk, N], gx [B, d_e], gr [B, d_r], gn [C * N, d_e])."""
    model, C, chunk, N = c["model"], c["C"], c["chunk"], c["N"]
    x, r, nb, W = (inp[k].astype(dtype) for k in ("x", "r", "nb", "W"))
    gamma = dtype(c["gamma"])
    a = O.pos_side(model, neg_head, x, r, c["emb_init"])
    S = np.empty((C, chunk, N), dtype)
    ga, gn = np.zeros_like(a), np.zeros_like(nb)
    for ci, i0, i1 in _blocks(c, elems if model in PAIR_MODELS else 1 << 62):
        rows, cols = slice(ci * chunk + i0, ci * chunk + i1), slice(ci * N, (ci + 1) * N)
        S[ci, i0:i1] = O.score_neg(model, a[rows], nb[cols], 1, i1 - i0, N, gamma)[0]
        if grads:
            g_a, g_b = O.score_neg_bwd(model, a[rows], nb[cols], W[ci, i0:i1][None], 1, i1 - i0, N, gamma)
            ga[rows] = g_a
            gn[cols] += g_b
    out = dict(score=S)
    if grads:
        gx, gr = O.pos_side_bwd(model, neg_head, x, r, ga, c["emb_init"])
        out.update(gx=gx.astype(dtype), gr=gr.astype(dtype), gn=gn)
    return out


def _t_halves(x):
    d = x.shape[-1] // 2
    return x[..., :d], x[..., d:]


def _t_pos_side(th, model, neg_head, x, r, emb_init):
    if model in ("TransE_l1", "TransE_l2"):
        return x - r if neg_head else x + r
    if model == "DistMult":
        return x * r
    if model == "RESCAL":
        return th.einsum("bij,bj->bi", r.reshape(r.shape[0], x.shape[-1], -1), x)
    xi, xj = _t_halves(x)
    if model == "SimplE":
        rel, rinv = _t_halves(r)
        return th.cat([rel * xj, rinv * xi], -1) if neg_head else th.cat([rinv * xj, xi * rel], -1)
    if model == "ComplEx":
        rr, ir = _t_halves(r)
    else:
        ph = r / (emb_init / np.pi)
        rr, ir = th.cos(ph), th.sin(ph)
    if neg_head:
        return th.cat([xi * rr + xj * ir, -xi * ir + xj * rr], -1)
    return th.cat([xi * rr - xj * ir, xi * ir + xj * rr], -1)


def _t_score(th, model, a, bn, gamma):
    if model in ("DistMult", "ComplEx", "RESCAL"):
        return a @ bn.T
    if model == "SimplE":
        return th.clamp(0.5 * (a @ bn.T), -CLAMP, CLAMP)
    d = a[:, None, :] - bn[None, :, :]
    if model == "TransE_l1":
        return gamma - d.abs().sum(-1)
    if model == "TransE_l2":                # batched_l2_dist's clamp (score_fun.py:26-34), on the exact squared distance
        return gamma - th.sqrt(th.clamp((d * d).sum(-1), min=1e-30))
    re, im = _t_halves(d)
    return gamma - th.sqrt(re * re + im * im).sum(-1)


def torch_neg(c, neg_head, inp, device="cpu", grads=True, elems=1 << 26):
    """the same operation in torch float64 with autograd, block by block; numpy results shaped like oracle_neg's"""
    import torch as th
    model, C, chunk, N = c["model"], c["C"], c["chunk"], c["N"]
    x, r, nb = (th.tensor(inp[k], dtype=th.float64, device=device, requires_grad=grads) for k in ("x", "r", "nb"))
    W = th.tensor(inp["W"], dtype=th.float64, device=device)
    S = th.empty((C, chunk, N), dtype=th.float64, device=device)
    for ci, i0, i1 in _blocks(c, elems if model in PAIR_MODELS + ("TransE_l2",) else 1 << 62):
        rows = slice(ci * chunk + i0, ci * chunk + i1)
        with th.set_grad_enabled(grads):
            s = _t_score(th, model, _t_pos_side(th, model, neg_head, x[rows], r[rows], c["emb_init"]), nb[ci * N:(ci + 1) * N], c["gamma"])
            S[ci, i0:i1] = s.detach()
            if grads:
                (s * W[ci, i0:i1]).sum().backward()
    out = dict(score=S.cpu().numpy())
    if grads:
        out.update(gx=x.grad.cpu().numpy(), gr=r.grad.cpu().numpy(), gn=nb.grad.cpu().numpy())
    return out


def l1_ambiguous(c, neg_head, inp, elems=1 << 24):
    """TransE_l1: (negative slots, edges) fed by an element with |a - b| < L1_TAU * max(1, |a| / 0.09), from the float64 operands
    (half an ulp of the float32 pos-side vector: 3.7e-9 at |a| ~ 0.09, growing with |a|)"""
    a = O.pos_side(c["model"], neg_head, inp["x"].astype(np.float64), inp["r"].astype(np.float64), c["emb_init"])
    nb = inp["nb"].astype(np.float64)
    chunk, N = c["chunk"], c["N"]
    slots, edges = set(), set()
    for ci, i0, i1 in _blocks(c, elems):
        ar = a[ci * chunk + i0:ci * chunk + i1]
        tau = L1_TAU * np.maximum(1.0, np.abs(ar) / 0.09)
        amb = (np.abs(ar[:, None, :] - nb[None, ci * N:(ci + 1) * N, :]) < tau[:, None, :]).any(-1)
        ii, jj = np.nonzero(amb)
        edges.update((ci * chunk + i0 + ii).tolist())
        slots.update((ci * N + jj).tolist())
    return sorted(slots), sorted(edges)


def clamp_stats(c, score64_raw):
    """SimplE: (share of pairs in the clamp, negative slots, edges fed by a float64 raw score within CLAMP_BAND of +-20)"""
    C, chunk, N = c["C"], c["chunk"], c["N"]
    raw = np.abs(score64_raw.reshape(C, chunk, N))
    ci, ii, jj = np.nonzero(np.abs(raw - CLAMP) < CLAMP_BAND)
    return float((raw > CLAMP).mean()), sorted(set((ci * N + jj).tolist())), sorted(set((ci * chunk + ii).tolist()))


def simple_raw(c, neg_head, inp):
    """float64 un-clamped SimplE scores [C, chunk, N]"""
    a = O.pos_side("SimplE", neg_head, inp["x"].astype(np.float64), inp["r"].astype(np.float64))
    return 0.5 * np.einsum("cik,cjk->cij", a.reshape(c["C"], c["chunk"], -1), inp["nb"].astype(np.float64).reshape(c["C"], c["N"], -1))


def neg_exclusions(c, neg_head, inp):
    """(negative slots, edges) excluded from the gradient comparison of a case, from the float64 reference alone"""
    if c["fwd_only"]:
        return [], []
    if c["model"] == "TransE_l1":
        return l1_ambiguous(c, neg_head, inp)
    if c["model"] == "SimplE":
        return clamp_stats(c, simple_raw(c, neg_head, inp))[1:]
    return [], []


def check_row_cap(rows, total, what):
    assert len(rows) <= ROW_CAP * total, "%s: %d of %d rows excluded (cap %g)" % (what, len(rows), total, ROW_CAP)


def check_neg_caps(c, slots, edges, tag):
    check_row_cap(slots, c["C"] * c["N"], tag + " g_neg")
    check_row_cap(edges, c["C"] * c["chunk"], tag + " g_pos_side / g_rel")


def masked(got, want, rows):
    got = np.array(got, dtype=np.float64, copy=True)
    if len(rows):
        got[rows] = np.asarray(want, dtype=np.float64)[rows]
    return got


def score_bound(ref):
    return SCORE_ATOL + SCORE_RTOL * np.abs(ref)


def grad_bound(ref):
    """3e-4 of the largest component + 3e-4 relative, as _close(got, ref, 3e-4, grad_tol(ref)) applies it"""
    ref = np.asarray(ref, np.float64)
    return GRAD_RTOL * max(float(np.abs(ref).max()) if ref.size else 0.0, 1e-12) + GRAD_RTOL * np.abs(ref)


def worst(got, ref, bound):
    """(largest |got - ref| / bound - <= 1 passes -, the error there, the bound there)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, "shape %s vs %s" % (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0, 0.0, 0.0
    if not np.isfinite(got).all():
        return float("inf"), float("inf"), 0.0
    err = np.abs(got - ref)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    k = int(np.argmax(ratio))
    return float(ratio.flat[k]), float(err.flat[k]), float(bound.flat[k])


def coincident_rows(c):
    """(negative slot, edge) of the planted pair"""
    ci, i, j = COINCIDENT
    return ci * c["N"] + j, ci * c["chunk"] + i


def neg_errors(c, got, ref, slots, edges, ref32=None):
    """{quantity: (largest |got - ref| / bound, largest |got - ref|)} of one score_neg result against the float64 reference, the
    excluded rows replaced.  ref32 (a 'coincident' case: the float32 oracle's result): the planted pair's score and the two
    gradient rows it feeds are allowed max(suite bound, 3 x the float32 oracle's own error) - the reference's float32
    |a|^2 + |b|^2 - 2 a.b loses the pair's distance to cancellation (tests/test_modular_op_inputs.py measures that it does)."""
    res = {}
    sb = score_bound(ref["score"])
    bounds = {k: np.broadcast_to(grad_bound(ref[k]), ref[k].shape).copy() for k in ("gx", "gr", "gn") if k in ref}
    if c["kind"] == "coincident":
        ci, i, j = COINCIDENT
        slot, edge = coincident_rows(c)
        sb[ci, i, j] = np.inf if ref32 is None else max(sb[ci, i, j], 3.0 * abs(float(ref32["score"][ci, i, j]) - ref["score"][ci, i, j]))
        for k, row in (("gx", edge), ("gr", edge), ("gn", slot)):
            e32 = np.inf if ref32 is None else 3.0 * np.abs(ref32[k][row].astype(np.float64) - ref[k][row]).max()
            bounds[k][row] = np.maximum(bounds[k][row], e32)
    res["score"] = worst(got["score"], ref["score"], sb)
    if not c["fwd_only"]:
        for k, rows in (("gx", edges), ("gr", edges), ("gn", slots)):
            res[k] = worst(masked(got[k], ref[k], rows), ref[k], bounds[k])
    return res


def neg_fuzz_case(seed):
    """one random small score_neg configuration (its own seeded generator)"""
    rng = np.random.RandomState(52000 + seed)
    model = MODELS[seed % 7]
    d_e = int(rng.choice([4, 8, 12, 16, 18, 20, 24, 32, 36, 48, 64, 80, 96, 130]))
    if model == "RESCAL":
        d_e = min(d_e, 64)
    if not width_ok(model, d_e):
        d_e += 1
    C, chunk = int(rng.randint(1, 5)), int(rng.choice([1, 3, 4, 8, 16, 17, 32, 33, 70]))
    N = int(rng.choice([1, 2, 5, 8, 16, 20, 36, 64, 65, 130]))
    flags = int(rng.choice(_flag_set(model)))
    c = neg_case(model, C, chunk, N, d_e, flags=flags, scale=float(rng.choice([0.25, 1.0])), gamma=float(rng.choice([6.0, 12.0])), tag="fuzz%d" % seed)
    return c


FUZZ_N = int(os.environ.get("KGE_MODULAR_FUZZ_N", "24"))      # KGE_MODULAR_FUZZ_N=500 for a longer hunt


# --------------------------------------------------------------------------------------------------------------------------
# (b) score_pos
# --------------------------------------------------------------------------------------------------------------------------
POS_B = (1, 37, 1000, 4101)
_POS_WIDTHS = (400, 48, 112, 4, 36, 30, 18, 2048, 40, 24, 16)


def pos_cases():
    out = []
    for m in MODELS:
        for d_e in ((4, 18, 30, 36, 48, 64, 100, 112) if m == "RESCAL" else _POS_WIDTHS):
            if not width_ok(m, d_e):
                continue
            Bs = tuple(b for b in POS_B if m != "RESCAL" or b * d_e * d_e <= 4101 * 64 * 64)
            out.append(dict(id="%s-D%d" % (m, d_e), model=m, d_e=d_e, d_r=rel_width(m, d_e), Bs=Bs, scale=1.0, gamma=12.0, emb_init=1.0,
                            kind="plain"))
    for d_e in (400, 48, 30):        # SimplE inputs that cross the positive clamp
        s = simple_clamp_scale(d_e)
        out.append(dict(id="SimplE-clamp-D%d" % d_e, model="SimplE", d_e=d_e, d_r=d_e, Bs=POS_B, scale=s, gamma=12.0, emb_init=s, kind="clamp"))
    return out


POS_CASES = pos_cases()


def pos_inputs(c, B):
    rng = np.random.RandomState(_seed("pos", c["id"], B))
    s = c["scale"]
    return dict(h=rng.uniform(-s, s, (B, c["d_e"])).astype(np.float32), r=rng.uniform(-s, s, (B, c["d_r"])).astype(np.float32),
                t=rng.uniform(-s, s, (B, c["d_e"])).astype(np.float32), dp=rng.uniform(-1, 1, B).astype(np.float32))


def oracle_pos(c, inp, dtype=np.float64):
    h, r, t, dp = (inp[k].astype(dtype) for k in ("h", "r", "t", "dp"))
    gamma = dtype(c["gamma"])
    s = O.score_pos(c["model"], h, r, t, gamma, c["emb_init"])
    gh, gr, gt = O.score_pos_bwd(c["model"], h, r, t, dp, gamma, c["emb_init"])
    return dict(score=s, gh=gh, gr=gr, gt=gt)


def pos_exclusions(c, inp):
    """edges excluded from the gradient comparison: TransE_l1 sign ambiguity of h + r - t, SimplE scores at the clamp's edge"""
    h, r, t = (inp[k].astype(np.float64) for k in ("h", "r", "t"))
    if c["model"] == "TransE_l1":
        tau = L1_TAU * np.maximum(1.0, np.abs(h + r) / 0.09)
        return np.nonzero((np.abs(h + r - t) < tau).any(-1))[0].tolist()
    if c["model"] == "SimplE":
        return np.nonzero(np.abs(np.abs(simple_pos_raw(inp)) - CLAMP) < CLAMP_BAND)[0].tolist()
    return []


def simple_pos_raw(inp):
    h, r, t = (inp[k].astype(np.float64) for k in ("h", "r", "t"))
    d = h.shape[1] // 2
    return 0.5 * (h[:, :d] * r[:, :d] * t[:, d:] + t[:, :d] * r[:, d:] * h[:, d:]).sum(-1)


# --------------------------------------------------------------------------------------------------------------------------
# (c) - (g): the small ops
# --------------------------------------------------------------------------------------------------------------------------
PNORM_SHAPES = [(n, dim) for n in (1, 3000) for dim in (1, 30, 400, 800)] + [(None, 777)]        # (None, dim): a 1-D input


def pnorm_input(n, dim, zeros=False):
    rng = np.random.RandomState(_seed("pnorm", n, dim, zeros))
    x = rng.uniform(-1, 1, (dim,) if n is None else (n, dim)).astype(np.float32)
    if zeros:
        x[rng.rand(*x.shape) < 0.3] = 0.0
        x.flat[0] = 0.0
    return x


def pnorm_ref(x, p, gout=1.0):
    x64 = x.astype(np.float64)
    return O.reg_value([x64], 1.0, p), O.reg_grad(x64, gout, p)


# C, chunk, Np: C * chunk no multiple of 256; chunk < Np, == Np, > Np (the kernel's `i < Np` guard)
MASK_SHAPES = [(3, 37, 81), (5, 200, 400), (3, 37, 37), (2, 129, 129), (3, 44, 37), (1, 300, 7), (7, 1, 1), (1, 1, 5)]


def mask_diag_ref(x, C, chunk, Np):
    y = x.reshape(C, chunk, Np).copy()
    i = np.arange(min(chunk, Np))
    y[:, i, i] = 0.0
    return y


GATHER_CASES = [("distinct", 3000, 3000, 400), ("distinct", 3000, 3000, 30), ("hub", 5, 4096, 400), ("hub", 5, 4096, 30)]


def gather_input(kind, rows, n_idx, dim):
    rng = np.random.RandomState(_seed("gather", kind, rows, n_idx, dim))
    block = rng.uniform(-1, 1, (rows, dim)).astype(np.float32)
    idx = rng.permutation(rows)[:n_idx] if kind == "distinct" else rng.randint(0, rows, n_idx)
    g = rng.uniform(-1, 1, (n_idx, dim)).astype(np.float32)
    return block, idx.astype(np.int64), g


def scatter_add_ref(rows, idx, g):
    """float64 index_add and its per-element bound count * 2^-24 * sum |terms| (the worst case of any summation order)"""
    ref, mag, cnt = np.zeros((rows, g.shape[1])), np.zeros((rows, g.shape[1])), np.zeros(rows)
    np.add.at(ref, idx, g.astype(np.float64))
    np.add.at(mag, idx, np.abs(g.astype(np.float64)))
    np.add.at(cnt, idx, 1.0)
    return ref, cnt[:, None] * 2.0 ** -24 * mag


ADAGRAD_DIMS = (400, 30)
ADAGRAD_ROWS = 3000


def adagrad_input(dim, dup):
    """table [4000, dim], state [4000], 3000 (idx, grad) rows; dup: indices drawn with replacement plus a hub of 5 rows"""
    rng = np.random.RandomState(_seed("adagrad", dim, dup))
    n_tab = 4000
    table = rng.uniform(-0.1, 0.1, (n_tab, dim)).astype(np.float32)
    state = (rng.rand(n_tab) * 1e-3).astype(np.float32)
    if dup:
        idx = rng.randint(0, n_tab, ADAGRAD_ROWS)
        hub =rng.rand(ADAGRAD_ROWS) < 0.2
        idx[hub] = rng.randint(0, 5, int(hub.sum()))
    else:
        idx = rng.permutation(n_tab)[:ADAGRAD_ROWS]
    grad = (rng.randn(ADAGRAD_ROWS, dim) * 0.01).astype(np.float32)
    return table, state, idx.astype(np.int64), grad


RANK_SHAPES = [(E, N) for E in (1, 1000) for N in (1, 63, 64, 65, N_ENT_FB15K)]


def rank_input(E, N, with_bias):
    """scores on a coarse grid (exact ties with the positive are common), row 0: every candidate beats the positive, last row: none"""
    rng = np.random.RandomState(_seed("rank", E, N, with_bias))
    neg = (rng.randint(-40, 40, (E, N)) / 8.0).astype(np.float32)
    pos = (rng.randint(-40, 40, E) / 8.0).astype(np.float32)
    pos[0] = -5.0                           # the grid's lowest value: every candidate beats or ties it
    neg[0, ::7] = pos[0]                    # ... and some tie exactly
    if E > 1:
        pos[-1] = 6.0
        neg[1, :] = pos[1]                  # a row of nothing but ties: `>=` counts every one
    bias = None
    if with_bias:
        bias = np.where(rng.rand(E, N) < 0.3, -1.0, 0.0).astype(np.float32)
    return neg, pos, bias


def rank_ref(neg, pos, bias):
    keep = np.ones(neg.shape, bool) if bias is None else bias != -1.0
    return 1 + ((neg >= pos[:, None]) & keep).sum(1).astype(np.int64)


# --------------------------------------------------------------------------------------------------------------------------
# (h) the drop-in model at the recipes' shapes (tables and batches of tests/loss_option_cases.py, the recipes' regularisers)
# --------------------------------------------------------------------------------------------------------------------------
DROPIN = [("cfgT", 1e-9), ("cfgD", 2e-6), ("complex", 2e-6), ("rotate", 1e-7), ("l1", 1e-7), ("simple", 2e-6)]
assert all(k in RECIPE_SHAPES for k, _ in DROPIN)


def dropin_l1_tau(ent64, rel64):
    """tests/test_gpu_parity.py::_l1_ambiguous takes one tau: L1_TAU scaled with the largest pos-side magnitude |x +- r| the tables allow"""
    return L1_TAU * max(1.0, float(np.abs(ent64).max() + np.abs(rel64).max()) / 0.09)
