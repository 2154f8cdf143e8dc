"""The per-op ("modular") C-ABI entry points against float64 at the recipes' shapes and at the sizes where their kernels change
instance (cases and references: tests/modular_op_cases.py; their inputs are guarded on the CPU by tests/test_modular_op_inputs.py).

Every op is called through dglke_amd.ops and compared with a float64 statement of the same operation evaluated from the same
float32 inputs: the oracle (numpy), or - for the pairwise [chunk, N, D] blocks - the same formulas in torch float64 on the
device (cross-checked against the oracle on the CPU).  Tolerances are the suite's: scores 1e-4 abs + 1e-4 rel, gradients 3e-4 of
the largest component of the compared array; the small ops are bit-exact or carry the bound derived at their test.

Exclusions are conditions on the float64 operands, capped at 2 % of the rows of every compared array (asserted): TransE_l1
elements whose sign(a - b) float32 cannot resolve, SimplE pairs at the clamp's edge.  The planted coincident pair of TransE_l2
is allowed 3 x the float32 oracle's own error (the reference's float32 distance of that pair is cancellation noise).

modular_op_errors.txt, written next to the suite's other reports, records per op and case the largest error next to its bound.
"""
import time

import numpy as np
import pytest
import torch

import loss_option_cases as L
import modular_op_cases as M
from oracle import kge_oracle as O
from test_gpu_loss_options import _report_dir
from test_gpu_parity import DEV, _close, _l1_ambiguous, _masked, grad_tol, make_args

pytestmark = pytest.mark.gpu

ERRORS = {}          # (op, case) -> {quantity: (err / bound, err, bound)}, note
T0 = time.time()


def _record(op, case, note="", **q):
    rec = ERRORS.setdefault((op, case), dict(q={}, note=""))
    for k, v in q.items():
        if k not in rec["q"] or v[0] >= rec["q"][k][0]:
            rec["q"][k] = v
    rec["note"] = note or rec["note"]
    try:
        import os
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "modular_op_errors.txt"), "w") as f:
            f.write("per-op C-ABI entry points against float64: largest |error| / bound per op, case and quantity (<= 1 passes), that error, "
                    "its bound\n(wall time of this file up to the last record: %.0f s)\n" % (time.time() - T0))
            for (o, c) in sorted(ERRORS):
                r = ERRORS[(o, c)]
                f.write("%-12s %s  %s\n" % (o, c, r["note"]))
                for k in sorted(r["q"]):
                    f.write("    %-10s err/bound %8.4f   err %.3e   bound %.3e\n" % ((k,) + tuple(r["q"][k])))
    except OSError:
        pass


def _dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_() if grad else t


def _poison(*shapes):
    """outputs are torch.empty blocks: hand the allocator NaN-filled blocks of their sizes first, so that an element a kernel
    leaves unwritten is not a stale correct value of the previous run"""
    blocks = [torch.full(s, float("nan"), device=DEV) for s in shapes]
    torch.cuda.synchronize()
    del blocks


def _check(errs, tag):
    for k, (ratio, err, bound) in errs.items():
        assert ratio <= 1.0, "%s %s: %.2f bounds off (error %.3e, bound %.3e)" % (tag, k, ratio, err, bound)


# --------------------------------------------------------------------------------------------------------------------------
# (a) score_neg forward and backward
# --------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _neg_reference(c, neg_head):
    """inputs, float64 reference and exclusions of a case; shared by the flag variants of one shape (the last few are kept)"""
    key = (c["model"], c["C"], c["chunk"], c["N"], c["d_e"], c["kind"], c["scale"], c["gamma"], neg_head)
    if key not in _REF:
        while len(_REF) >= 4:
            _REF.pop(next(iter(_REF)))
        inp = M.neg_inputs(c, neg_head)
        ref = M.torch_neg(c, neg_head, inp, DEV, grads=not c["fwd_only"])
        _REF[key] = (inp, ref, M.neg_exclusions(c, neg_head, inp))
    return _REF[key]


def _run_neg(c, inp, neg_head, W=None):
    from dglke_amd import ops
    C, chunk, N = c["C"], c["chunk"], c["N"]
    x, r, nb = _dev(inp["x"], True), _dev(inp["r"], True), _dev(inp["nb"], True)
    _poison((C, chunk, N))
    with torch.set_grad_enabled(not c["fwd_only"]):
        s = ops.score_neg(c["model"], neg_head, x, r, nb, C, chunk, N, c["gamma"], emb_init=c["emb_init"], flags=c["flags"])
    got = dict(score=s.detach().cpu().numpy())
    if not c["fwd_only"]:
        _poison(tuple(x.shape), tuple(r.shape), tuple(nb.shape))
        (s * _dev(inp["W"] if W is None else W)).sum().backward()
        got.update(gx=x.grad.cpu().numpy(), gr=r.grad.cpu().numpy(), gn=nb.grad.cpu().numpy())
    return got


def run_neg_case(c, op="score_neg"):
    for neg_head in (False, True):
        tag = "%s neg_head=%d" % (c["id"], neg_head)
        inp, ref, (slots, edges) = _neg_reference(c, neg_head)
        M.check_neg_caps(c, slots, edges, tag)
        got = _run_neg(c, inp, neg_head)
        assert all(np.isfinite(v).all() for v in got.values()), tag + ": non-finite output"
        ref32, note = None, ""
        if c["kind"] == "coincident":
            ref32 = M.oracle_neg(c, neg_head, inp, np.float32)
            ci, i, j = M.COINCIDENT
            note = "planted pair: |score error| kernel %.3e, float32 oracle %.3e (bound 3 x)" % (
                abs(float(got["score"][ci, i, j]) - ref["score"][ci, i, j]), abs(float(ref32["score"][ci, i, j]) - ref["score"][ci, i, j]))
        if c["kind"] == "clamp":
            raw = M.simple_raw(c, neg_head, inp)
            hit = np.abs(raw) > M.CLAMP + M.CLAMP_BAND
            assert 0.01 <= hit.mean() <= 0.5, tag
            assert np.array_equal(got["score"][hit], (np.sign(raw[hit]) * M.CLAMP).astype(np.float32)), tag + ": a clamped score is not exactly +-20"
            only = _run_neg(c, inp, neg_head, W=inp["W"] * hit)           # dL/dn on clamped pairs alone: no gradient anywhere
            assert not (only["gx"].any() or only["gr"].any() or only["gn"].any()), tag + ": a clamped pair carries gradient"
            note = "%.1f %% of the pairs clamped, %d rows at the clamp's edge excluded" % (100 * hit.mean(), len(slots) + len(edges))
        if c["model"] == "TransE_l1" and not c["fwd_only"]:
            note = "%d + %d sign-ambiguous rows excluded" % (len(slots), len(edges))
        errs = M.neg_errors(c, got, ref, slots, edges, ref32=ref32)
        _record(op, tag, note, **errs)
        _check(errs, tag)


@pytest.mark.parametrize("c", M.NEG_CASES, ids=lambda c: c["id"])
def test_score_neg_matches_float64(c):
    """kge_score_neg_fwd / kge_score_neg_bwd, both neg_head modes, a random signed dL/dn: scores, pos-side rows, relation rows
    and negative rows.  The case id ends in the kernel instances the case reaches (modular_op_cases.kernel_path): the stand-alone
    forward / backward GEMM, the bcast kernels (shared-pair `lc` or two-pass backward), the generic 32 x 32 pair kernels, and
    the pair kernels behind the backward GEMM's row limit."""
    run_neg_case(c)


@pytest.mark.parametrize("seed", range(M.FUZZ_N))
def test_score_neg_random_shapes_match_float64(seed):
    """fuzz over model x (C, chunk, N, d_e) x neg_head x flags"""
    run_neg_case(M.neg_fuzz_case(seed), op="neg_fuzz")


def test_score_neg_refuses_a_rescal_width_it_cannot_serve():
    """RESCAL rows wider than 1024 (the d_e = 2048 case of the other models): refused with its message, not computed wrongly"""
    from dglke_amd import _lib, ops
    x, r = torch.zeros(1, 2048, device=DEV), torch.zeros(1, 2048 * 2048, device=DEV)
    with pytest.raises(_lib.KgeError, match="RESCAL needs d_r == d_e\\*d_e and d_e <= 1024"):
        ops.score_neg("RESCAL", False, x, r, torch.zeros(3, 2048, device=DEV), 1, 1, 3, 12.0)
    with pytest.raises(_lib.KgeError, match="RESCAL needs d_r == d_e\\*d_e and d_e <= 1024"):
        ops.score_pos("RESCAL", x, r, x, 12.0)


# --------------------------------------------------------------------------------------------------------------------------
# (b) score_pos forward and backward
# --------------------------------------------------------------------------------------------------------------------------
def run_pos_case(c, Bs=None):
    """the body of test_score_pos_matches_float64 at the case's batch sizes (or `Bs`); -> every output, by batch size"""
    from dglke_amd import ops
    res = {}
    for B in Bs or c["Bs"]:
        tag = "%s B=%d" % (c["id"], B)
        inp = M.pos_inputs(c, B)
        ref = M.oracle_pos(c, inp)
        edges = M.pos_exclusions(c, inp)
        M.check_row_cap(edges, B, tag)
        h, r, t = _dev(inp["h"], True), _dev(inp["r"], True), _dev(inp["t"], True)
        _poison((B,))
        s = ops.score_pos(c["model"], h, r, t, c["gamma"], emb_init=c["emb_init"])
        _poison(tuple(h.shape), tuple(r.shape), tuple(t.shape))
        (s * _dev(inp["dp"])).sum().backward()
        got = dict(score=s.detach().cpu().numpy(), gh=h.grad.cpu().numpy(), gr=r.grad.cpu().numpy(), gt=t.grad.cpu().numpy())
        note = ""
        if c["kind"] == "clamp":
            raw = M.simple_pos_raw(inp)
            hit = np.abs(raw) > M.CLAMP + M.CLAMP_BAND
            assert np.array_equal(got["score"][hit], (np.sign(raw[hit]) * M.CLAMP).astype(np.float32)), tag + ": a clamped score is not exactly +-20"
            assert not (got["gh"][hit].any() or got["gr"][hit].any() or got["gt"][hit].any()), tag + ": a clamped edge carries gradient"
            note = "%d of %d edges clamped" % (hit.sum(), B)
        errs = dict(score=M.worst(got["score"], ref["score"], M.score_bound(ref["score"])))
        for k in ("gh", "gr", "gt"):
            errs[k] = M.worst(M.masked(got[k], ref[k], edges), ref[k], M.grad_bound(ref[k]))
        _record("score_pos", tag, note, **errs)
        _check(errs, tag)
        res.update({"%s B%d" % (k, B): v for k, v in got.items()})
    return res


@pytest.mark.parametrize("c", M.POS_CASES, ids=lambda c: c["id"])
def test_score_pos_matches_float64(c):
    """kge_score_pos / kge_score_pos_bwd (edge_bwd with clamp_pos = 1; RESCAL: matvec, two axpy, outer product) at
    B = 1, 37, 1000, 4101: score, gh, gr, gt"""
    run_pos_case(c)


# --------------------------------------------------------------------------------------------------------------------------
# (c) pnorm_pow
# --------------------------------------------------------------------------------------------------------------------------
def run_pnorm_case(p, zeros, shapes=None):
    """the body of test_pnorm_pow_value_and_gradient at M.PNORM_SHAPES (or `shapes`); -> value and gradient, by shape"""
    from dglke_amd import ops
    coef = 0.37
    res = {}
    for n, dim in shapes or M.PNORM_SHAPES:
        tag = "p=%d n=%s dim=%d%s" % (p, n, dim, " zeros" if zeros else "")
        x = M.pnorm_input(n, dim, zeros)
        val, grad = M.pnorm_ref(x, p, coef)
        xt = _dev(x, True)
        y = ops.pnorm_pow(xt, p)
        (coef * y).backward()
        g = xt.grad.cpu().numpy()
        assert g.shape == x.shape
        errs = dict(value=M.worst(np.array([y.item()]), np.array([val]), x.size * 2.0 ** -24 * val),
                    grad=M.worst(g, grad, 1e-6 * np.abs(grad) + 1e-45))
        _record("pnorm_pow", tag, **errs)
        assert not g[x == 0].any(), tag + ": gradient at an exact zero"
        _check(errs, tag)
        res.update({"value " + tag: y.detach().cpu().numpy().reshape(1), "grad " + tag: g})
    return res


@pytest.mark.parametrize("zeros", [False, True], ids=["dense", "zeros"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_pnorm_pow_value_and_gradient(p, zeros):
    """x.norm(p) ** p and its gradient.  Value: n * dim * 2^-24 * sum |x|^p (one rounding per term of a fixed-order sum, at most
    n * dim of them deep).  Gradient: 1e-6 relative per element; exactly 0 at x == 0 for every p."""
    run_pnorm_case(p, zeros)


# --------------------------------------------------------------------------------------------------------------------------
# (d) mask_diag
# --------------------------------------------------------------------------------------------------------------------------
def run_mask_diag_case(shape):
    """the body of test_mask_diag_forward_and_backward_bit_exact; -> output and gradient"""
    from dglke_amd import ops
    C, chunk, Np = shape
    rng = np.random.RandomState(5)
    x = (rng.rand(C, chunk, Np) + 0.5).astype(np.float32)
    g = (rng.rand(C, chunk, Np) + 0.5).astype(np.float32)
    xt = _dev(x, True)
    y = ops.mask_diag(xt, C, chunk, Np)
    y.backward(_dev(g))
    assert np.array_equal(y.detach().cpu().numpy(), M.mask_diag_ref(x, C, chunk, Np))
    assert np.array_equal(xt.grad.cpu().numpy(), M.mask_diag_ref(g, C, chunk, Np))
    assert np.array_equal(xt.detach().cpu().numpy(), x)
    _record("mask_diag", "C=%d chunk=%d Np=%d" % shape, "bit-exact")
    return dict(y=y.detach().cpu().numpy(), grad=xt.grad.cpu().numpy())


@pytest.mark.parametrize("shape", M.MASK_SHAPES, ids=lambda s: "C%d-chunk%d-Np%d" % s)
def test_mask_diag_forward_and_backward_bit_exact(shape):
    """only the [c, i, i] elements change (i < min(chunk, Np)), the gradient is masked at the same places, the input is kept"""
    run_mask_diag_case(shape)


# --------------------------------------------------------------------------------------------------------------------------
# (e) gather_local
# --------------------------------------------------------------------------------------------------------------------------
def run_gather_case(case):
    """the body of test_gather_local_forward_bit_exact_backward_inside_the_atomic_bound; -> gathered rows and scattered gradient"""
    from dglke_amd import ops
    kind, rows, n_idx, dim = case
    block, idx, g = M.gather_input(*case)
    bt = _dev(block, True)
    out = ops.gather_local(bt, _dev(idx))
    assert np.array_equal(out.detach().cpu().numpy(), block[idx])
    _poison((rows, dim))
    out.backward(_dev(g))
    ref, bound = M.scatter_add_ref(rows, idx, g)
    got = bt.grad.cpu().numpy()
    assert not got[np.bincount(idx, minlength=rows) == 0].any(), "a row nobody gathered has a gradient"
    errs = dict(grad=M.worst(got, ref, bound + 1e-300))
    _record("gather_local", "%s rows=%d idx=%d dim=%d" % case, "forward bit-exact", **errs)
    _check(errs, str(case))
    return dict(out=out.detach().cpu().numpy(), grad=got)


@pytest.mark.parametrize("case", M.GATHER_CASES, ids=lambda c: "%s-rows%d-idx%d-dim%d" % c)
def test_gather_local_forward_bit_exact_backward_inside_the_atomic_bound(case):
    """forward kge_gather_rows: bit-exact.  Backward kge_scatter_add_rows (float atomics, any order): per element within
    count * 2^-24 * sum |terms| of the float64 np.add.at - the worst case of any summation order, no margin"""
    run_gather_case(case)


# --------------------------------------------------------------------------------------------------------------------------
# (f) adagrad_scatter and adagrad_apply_rows
# --------------------------------------------------------------------------------------------------------------------------
def run_adagrad_scatter_case(dim, dup):
    """the body of test_adagrad_scatter_matches_float64; -> table and state"""
    from dglke_amd import ops
    table, state, idx, grad = M.adagrad_input(dim, dup)
    t_d, s_d = _dev(table), _dev(state)
    ops.adagrad_scatter(t_d, s_d, _dev(idx), _dev(grad), 0.3)
    t64, s64 = table.astype(np.float64), state.astype(np.float64)
    O.adagrad_update(t64, s64, idx, grad.astype(np.float64), 0.3)
    errs = dict(state=M.worst(s_d.cpu().numpy(), s64, 1e-7 + 1e-5 * np.abs(s64)), table=M.worst(t_d.cpu().numpy(), t64, 1e-5 + 1e-5 * np.abs(t64)))
    _record("adagrad_scatter", "dim=%d %s" % (dim, "duplicates" if dup else "unique"), **errs)
    untouched = np.ones(len(table), bool)
    untouched[idx] = False
    assert np.array_equal(t_d.cpu().numpy()[untouched], table[untouched]) and np.array_equal(s_d.cpu().numpy()[untouched], state[untouched])
    _check(errs, "adagrad_scatter dim %d" % dim)
    return dict(table=t_d, state=s_d)


@pytest.mark.parametrize("dup", [False, True], ids=["unique", "duplicates"])
@pytest.mark.parametrize("dim", M.ADAGRAD_DIMS)
def test_adagrad_scatter_matches_float64(dim, dup):
    """3 000 (index, gradient) rows, with duplicates and a hub of five rows: tolerances of test_adagrad_scatter_duplicate_semantics"""
    run_adagrad_scatter_case(dim, dup)


def run_adagrad_apply_rows_case(dim):
    """the body of test_adagrad_apply_rows_matches_float64_and_skips; -> table and state"""
    from dglke_amd import ops
    table, state, idx, grad = M.adagrad_input(dim, False)
    gs = (grad.astype(np.float64) ** 2).mean(1).astype(np.float32)
    rng = np.random.RandomState(9)
    drop, zero = rng.rand(len(idx)) < 0.1, rng.rand(len(idx)) < 0.1
    zero &= ~drop
    idx_in = np.where(drop, -1, idx)
    gs[zero] = 0.0                                        # (their gradient rows stay non-zero: the skip is what keeps the row)
    t_d, s_d = _dev(table), _dev(state)
    ops.adagrad_apply_rows(t_d, s_d, _dev(idx_in), _dev(grad), _dev(gs), 0.3)
    keep = ~(drop | zero)
    t64, s64 = table.astype(np.float64), state.astype(np.float64)
    O.adagrad_update(t64, s64, idx[keep], grad[keep].astype(np.float64), 0.3)
    got_t, got_s = t_d.cpu().numpy(), s_d.cpu().numpy()
    skipped = np.ones(len(table), bool)
    skipped[idx[keep]] = False
    assert drop.sum() > 100 and zero.sum() > 100
    assert np.array_equal(got_t[skipped], table[skipped]) and np.array_equal(got_s[skipped], state[skipped]), "a skipped row changed"
    errs = dict(state=M.worst(got_s, s64, 1e-7 + 1e-5 * np.abs(s64)), table=M.worst(got_t, t64, 1e-5 + 1e-5 * np.abs(t64)))
    _record("adagrad_rows", "dim=%d" % dim, "%d idx=-1 and %d gs=0 rows untouched bit for bit" % (drop.sum(), zero.sum()), **errs)
    assert (got_t[idx[keep]] != table[idx[keep]]).any(1).all(), "a kept row did not move"
    _check(errs, "adagrad_apply_rows dim %d" % dim)
    return dict(table=t_d, state=s_d)


@pytest.mark.parametrize("dim", M.ADAGRAD_DIMS)
def test_adagrad_apply_rows_matches_float64_and_skips(dim):
    """unique ids; rows with idx = -1 and rows with gs = 0 are skipped: their table rows and states stay bit for bit"""
    run_adagrad_apply_rows_case(dim)


# --------------------------------------------------------------------------------------------------------------------------
# (g) rank_from_scores
# --------------------------------------------------------------------------------------------------------------------------
def run_rank_case(shape, with_bias):
    """the body of test_rank_from_scores_equals_numpy; -> ranks"""
    from dglke_amd import ops
    neg, pos, bias = M.rank_input(shape[0], shape[1], with_bias)
    got = ops.rank_from_scores(_dev(neg), _dev(pos), None if bias is None else _dev(bias))
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), M.rank_ref(neg, pos, bias))
    _record("rank", "E=%d N=%d %s" % (shape + ("bias" if with_bias else "nobias",)), "equal")
    return dict(ranks=got)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", M.RANK_SHAPES, ids=lambda s: "E%d-N%d" % s)
def test_rank_from_scores_equals_numpy(shape, with_bias):
    """1 + #{j: neg[i, j] >= pos[i], bias[i, j] != -1}: exact ties count, masked candidates do not; integer equality"""
    run_rank_case(shape, with_bias)


# --------------------------------------------------------------------------------------------------------------------------
# (h) the drop-in model at the recipes' shapes
# --------------------------------------------------------------------------------------------------------------------------
def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("shape,reg", M.DROPIN, ids=[s for s, _ in M.DROPIN])
def test_dropin_model_matches_oracle_at_recipe_shapes(shape, reg):
    """KEModel.forward -> loss.backward() -> update, one C call per op (gather_local / scatter_add_rows atomics, pnorm_pow on the
    traces, adagrad_scatter on ~3 000 rows with duplicates), two steps against O.train_step restarted from the model's own
    float32 tables - quantities and tolerances of test_fused_step_matches_oracle_at_config_shapes; then forward_test (chunk = 64
    test triples, N = every entity, kge_rank_from_scores) inside the band of O.rank_eval(tol=1e-4)"""
    from dglke_amd import plan
    from dglke_amd.dataloader import NegGraph, PosGraph
    from dglke_amd.general_models import KEModel
    c = L.case("dropin-" + shape, shape, reg_coef=reg)
    cfg = L.config(c)
    ent, rel, _ = L.tables(c)
    m = KEModel(make_args(c), c["model"], c["n_ent"], c["n_rel"], c["hidden"], c["gamma"], double_entity_emb=c["de"], double_relation_emb=c["dr"])
    m.entity_emb.emb.copy_(torch.from_numpy(ent))
    m.relation_emb.emb.copy_(torch.from_numpy(rel))
    m.entity_emb.state_sum.zero_()
    m.relation_emb.state_sum.zero_()
    chunk, N, lr = c["chunk"], c["N"], c["lr"]
    bts = L.batches(c)
    for step, bt in enumerate(bts, 1):
        tag = "dropin %s step %d" % (shape, step)
        ent64, rel64 = _f64(m.entity_emb.emb), _f64(m.relation_emb.emb)
        es64, rs64 = _f64(m.entity_emb.state_sum), _f64(m.relation_emb.state_sum)
        amb = dict(slots=[], edges=[], pos_local=[], ent=[], rel=[])
        if c["model"] == "TransE_l1":
            amb = _l1_ambiguous(bt, ent64, rel64, chunk, N, tau=M.dropin_l1_tau(ent64, rel64))
            for what, rows, total in (("g_neg", amb["slots"], len(bt["neg"])), ("g_rel", amb["edges"], c["B"]), ("g_pos_ent", amb["pos_local"], len(bt["nid"])),
                                      ("entity table", amb["ent"], c["n_ent"]), ("relation table", amb["rel"], c["n_rel"])):
                M.check_row_cap(rows, total, tag + " " + what)
        b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], chunk, N, bt["neg_head"], DEV)
        pos_g, neg_g = PosGraph(b), NegGraph(b)
        loss, log = m.forward(pos_g, neg_g, 0)
        with torch.no_grad():
            neg_score = m.predict_neg_score(pos_g, neg_g, gpu_id=0, trace=False)
        out = O.train_step(cfg, ent64, es64, rel64, rs64, bt["nid"], bt["h_local"], bt["t_local"], bt["r"], bt["neg"], bt["neg_head"], chunk, N)
        _close(pos_g.edata["score"].detach().cpu(), out["pos_score"], 1e-4, 1e-4, tag + " pos_score")
        _close(neg_score.cpu().reshape(out["neg_score"].shape), out["neg_score"], 1e-4, 1e-4, tag + " neg_score")
        _close([log["pos_loss"], log["neg_loss"], log["loss"]], out["log"][:3], 1e-4, 1e-5, tag + " loss")
        _close(log["regularization"], out["log"][3], 1e-3, 1e-7, tag + " reg")
        loss.backward()
        et, rt = m.entity_emb.trace, m.relation_emb.trace
        assert len(et) == 2 and len(rt) == 1
        g_pos, g_neg, g_rel = et[0][1].grad.cpu().numpy(), et[1][1].grad.cpu().numpy(), rt[0][1].grad.cpu().numpy()
        q = {}
        for k, got, rows in (("g_pos_ent", g_pos, amb["pos_local"]), ("g_neg", g_neg, amb["slots"]), ("g_rel", g_rel, amb["edges"])):
            _close(_masked(got, out[k], rows), out[k], 3e-4, grad_tol(out[k]), tag + " " + k)
            q[k] = M.worst(_masked(got, out[k], rows), out[k], M.grad_bound(out[k]))
        m.update(0)
        got_e, got_r = _f64(m.entity_emb.emb), _f64(m.relation_emb.emb)
        _close(_masked(_f64(m.entity_emb.state_sum), es64, amb["ent"]), es64, 2e-3, 1e-9, tag + " ent state")
        _close(_masked(_f64(m.relation_emb.state_sum), rs64, amb["rel"]), rs64, 2e-3, 1e-9, tag + " rel state")
        _close(_masked(got_e, ent64, amb["ent"]), ent64, 1e-4, 1e-3 * lr, tag + " entity rows")
        _close(_masked(got_r, rel64, amb["rel"]), rel64, 1e-4, 1e-3 * lr, tag + " relation rows")
        q["score"] = M.worst(neg_score.cpu().numpy().reshape(out["neg_score"].shape), out["neg_score"], M.score_bound(out["neg_score"]))
        q["ent_rows"] = M.worst(_masked(got_e, ent64, amb["ent"]), ent64, 1e-3 * lr + 1e-4 * np.abs(ent64))
        q["rel_rows"] = M.worst(_masked(got_r, rel64, amb["rel"]), rel64, 1e-3 * lr + 1e-4 * np.abs(rel64))
        _record("dropin", tag, "%d + %d table rows excluded" % (len(amb["ent"]), len(amb["rel"])) if c["model"] == "TransE_l1" else "", **q)
    # ---- forward_test: 64 of the last batch's triples against every entity, one chunk
    E, n_ent = 64, c["n_ent"]
    bt = bts[-1]
    h, r, t = bt["h"][:E], bt["r"][:E], bt["t"][:E]
    ent64, rel64 = _f64(m.entity_emb.emb), _f64(m.relation_emb.emb)
    for neg_head in (False, True):
        b = plan.make_batch(h, t, r, np.arange(n_ent), E, n_ent, neg_head, DEV)
        logs = []
        m.forward_test(PosGraph(b), NegGraph(b), logs, 0)
        got = np.array([lg["MR"] for lg in logs])
        lo, hi = np.empty(E, np.int64), np.empty(E, np.int64)
        for k in range(0, E, 8):          # (8 triples at a time: a pairwise [8, n_ent, D] float64 block)
            (lo[k:k + 8], hi[k:k + 8]), _, _ = O.rank_eval(c["model"], ent64, rel64, h[k:k + 8], r[k:k + 8], t[k:k + 8], neg_head, c["gamma"],
                                                           cfg.emb_init, tol=1e-4)
        assert ((got >= lo) & (got <= hi)).all(), "dropin %s forward_test neg_head=%d: ranks %r outside [%r, %r]" % (shape, neg_head, got, lo, hi)
        assert hi.max() > 10, "the positives all rank first: nothing is ranked"
        _record("forward_test", "dropin %s neg_head=%d" % (shape, neg_head), "64 ranks inside the oracle's band, widest band %d" % int((hi - lo).max()))
