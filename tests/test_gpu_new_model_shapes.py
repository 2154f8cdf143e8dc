"""QuatE, PairRE, TransH and TransD on the GPU across the tile, slab and list boundaries of their kernels, against the float64
statements of tests/quate_cases.py, tests/pairre_cases.py, tests/transh_cases.py and tests/transd_cases.py (cases:
tests/new_model_shape_cases.py; their inputs are guarded on the CPU by tests/test_new_model_shape_inputs.py):
  1. the fused step at boundary shapes: several row tiles, column tiles and k slabs at once, degenerate and odd edges,
     --neg_deg_sample with a chunk that is no multiple of 16, streamed loss rows, the recipe width, relation rows beyond the
     register-resident update; QuatE on its three negative-score routes; TransD's column-sum workgroups with several column tiles
     and several rows per row group, its stacked operand across row tiles; TransH and TransD on either side of the threshold
     between the backward GEMM tiles and the pairwise backward products (s7a, s7b beyond it, s7c the last shape on the tiles);
  2. the fused step at random shapes (KGE_NEW_MODEL_FUZZ_N cases per model, 24 by default);
  3. the fused step with hub entities and a dominant relation: update lists well beyond 64 entries, with and without the regulariser;
  4. every ranking entry and the top-K selection over several row and column tiles, with Ranker batches that reach into the filter
     lists at e0 > 0: EQUAL to the float64 ranks / order on integer-grid tables; inside the float64 band on random tables.
Each step starts from the case's fixed tables (tail, then head corruption) and is compared with the float64 step started from the
GPU's own float32 tables: scores, loss terms, the three trace gradients, both Adagrad states, both tables.  Bounds are the suite's
(tests/modular_op_cases.py); where the float32 statement itself is over one (new_model_shape_cases.bound_factors, measured on the
CPU) the bound is 3 x that statement's error.  Rows left out: PairRE's sign-ambiguous ones (at most pairre_cases.ROW_CAP) and
hinge flips under the rule and caps of tests/test_gpu_loss_options.py (TransD: nothing else, and no bound factor).

new_model_shape_errors.txt, written next to the suite's other reports, records per part, case and quantity the largest error over
its bound, the rows left out, any bound factor taken from the float32 statement, and the wall time of this file."""
import os
import time

import numpy as np
import pytest
import torch

import loss_option_cases as L
import new_model_shape_cases as S
from test_gpu_eval import TOL
from test_gpu_infer import accept
from test_gpu_loss_options import _f64, _report_dir
from test_gpu_parity import DEV, _close, _skewed_batch

pytestmark = pytest.mark.gpu

ERRORS = {}          # (part, case) -> {quantity: (err / bound, err, bound)}
NOTES = {}           # (part, case) -> str
T0 = time.time()


def _record(part, case, note="", **q):
    rec = ERRORS.setdefault((part, case), {})
    for k, v in q.items():
        if k not in rec or v[0] >= rec[k][0]:
            rec[k] = v
    if note:
        NOTES[(part, case)] = note
    try:
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "new_model_shape_errors.txt"), "w") as f:
            f.write("QuatE, PairRE, TransH and TransD at boundary, random and heavy-list shapes against float64: largest |error| / bound per part, case "
                    "and quantity (<= 1 passes), that error, its bound\n(wall time of this file up to the last record: %.0f s)\n" % (time.time() - T0))
            top = max(((v[0], p, c, k) for (p, c), r in ERRORS.items() for k, v in r.items()), default=None)
            if top:
                f.write("worst: %.4f of its bound (%s %s %s)\n" % top)
            for key in sorted(set(ERRORS) | set(NOTES)):
                f.write("%-9s %s   %s\n" % (key + (NOTES.get(key, ""),)))
                for k in sorted(ERRORS.get(key, {})):
                    f.write("    %-10s err/bound %8.4f   err %.3e   bound %.3e\n" % ((k,) + tuple(ERRORS[key][k])))
    except OSError:
        pass


def _check(errs, tag):
    for k, (ratio, err, bound) in errs.items():
        assert ratio <= 1.0, "%s %s: %.2f bounds off (error %.3e, bound %.3e)" % (tag, k, ratio, err, bound)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # (a copy: the case tables are read-only)


# --------------------------------------------------------------------------------------------------------------------------
# the fused step
# --------------------------------------------------------------------------------------------------------------------------
def _engine(c):
    from dglke_amd.engine import StepEngine
    model = c["model"]
    td = model == "TransD"           # hidden dimension k, both tables doubled: rows of d_e = 2 k floats
    eng = StepEngine(model, c["n_ent"], c["n_rel"], c["d_e"] // 2 if td else c["d_e"], S.engine_gamma(model), c["lr"], DEV, td,
                     model != "QuatE", c["adv"],
                     c["adv_temp"], c["reg_coef"], c["reg_norm"], loss_genre=c["genre"], pairwise=c["pairwise"], margin=c["margin"],
                     flags=int(c["flags"]) | (S.PR.NEG_DEG if c["neg_deg"] else 0))
    eng.load_tables(*S.tables(c))
    return eng


def _run_step(c, bt, step):
    """one fused step of case `c` from its fixed tables: (engine, batch, outputs, float64 reference, tables before, tag)"""
    from dglke_amd import plan
    eng = _engine(c)
    ent0, rel0 = eng.ent.cpu().numpy(), eng.rel.cpu().numpy()
    assert not eng.ent_state.any() and not eng.rel_state.any()
    b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV, bt["w"])
    want = eng.alloc_outputs(b)
    eng.step(b, want)
    torch.cuda.synchronize()
    ref = S.statement_step(c, bt, ent0, rel0)
    tag = "%s %s" % (c["id"], "head" if bt["neg_head"] else "tail")
    assert not np.array_equal(ent0, eng.ent.cpu().numpy()), tag + ": the step did not move the entity table"
    assert not np.array_equal(rel0, eng.rel.cpu().numpy()), tag + ": the step did not move the relation table"
    return eng, b, want, ref, (ent0, rel0), tag


def _loss_terms(c, eng, out, tag):
    l4 = eng.read_loss()
    if c["pairwise"] or c["genre"] == "Softmax":
        assert np.isnan(l4[0]) and np.isnan(l4[1]), tag
    else:
        _close(l4[0], out["log"][0], 1e-4, 1e-5, tag + " pos_loss")
        _close(l4[1], out["log"][1], 1e-4, 1e-5, tag + " neg_loss")
    _close(l4[2], out["log"][2], 1e-4, 1e-5, tag + " loss")
    _close(l4[3], out["log"][3], 1e-3, 1e-7, tag + " reg")


def run_case(c, part):
    """two fused steps of case `c` (tail then head corruption, each from the fixed tables) against the float64 statement: every
    optional output of kge_step_out, the loss terms, both Adagrad states and both tables"""
    for step, bt in enumerate(S.batches(c)):
        eng, b, want, ref, (ent0, rel0), tag = _run_step(c, bt, step)
        out = ref[0]
        if c["model"] == "TransH":
            assert out["share"] >= S.TH.DIST_SHARE and S.TH.residual_rows(out) == 0, tag + ": a step input outside the conditions of transh_cases.py"
        if c["model"] == "TransD":
            assert out["share"] >= S.TD.DIST_SHARE and S.TD.residual_rows(out) == 0 and out["cmax"] < S.TD.C_MAX, \
                tag + ": a step input outside the conditions of transd_cases.py"
            assert not S.bound_factors(c, step), tag
        gp, gn = want["pos_score"].cpu().numpy(), want["neg_score"].cpu().numpy()
        excl, note = dict(S.NO_ROWS), ""
        if c["model"] == "PairRE":
            excl, n_amb = S.pairre_excluded(c, bt, ent0, rel0)
            S.check_row_cap(c, bt, excl, S.PR.ROW_CAP, tag)
            note += " ambiguous pairs %d" % n_amb
        fl = L.hinge_flips(c, bt, gp, gn, out["pos_score"], out["neg_score"])
        if fl is not None:
            L.check_flip_caps(c, bt, fl, tag)
            excl = S.union(excl, fl)
            note += " hinge flips %d" % fl["n_flips"]
        factor = S.bound_factors(c, step)
        if factor:
            note += " bound x " + ", ".join("%s %.2f" % kv for kv in sorted(factor.items())) + " (3 x the float32 statement's error)"
        if any(excl.values()):
            note += " rows left out: " + ", ".join("%s %d" % (k, len(v)) for k, v in sorted(excl.items()) if v)
        _loss_terms(c, eng, out, tag)
        sel = np.searchsorted(b.p["ue_id"], bt["nid"])
        got = dict(pos_score=gp, neg_score=gn, g_pos_ent=want["g_pos_ent"].cpu().numpy()[sel], g_neg=want["g_neg"].cpu().numpy(),
                   g_rel=want["g_rel"].cpu().numpy(), ent=_f64(eng.ent), rel=_f64(eng.rel), ent_state=_f64(eng.ent_state),
                   rel_state=_f64(eng.rel_state))
        assert all(np.isfinite(v).all() for v in got.values()), tag + ": non-finite output"
        errs = S.step_errors(c, bt, got, ref, excl, factor, ent0=ent0.astype(np.float64))
        _record(part, tag, note.strip(), **errs)
        _check(errs, tag)


@pytest.mark.parametrize("c", S.BOUNDARY_CASES, ids=lambda c: c["id"])
def test_step_at_boundary_shapes_matches_float64(c):
    """part 1: the shapes of new_model_shape_cases.SHAPES - what each crosses is named there and asserted by the CPU file"""
    run_case(c, "boundary")


@pytest.mark.parametrize("seed", range(S.FUZZ_N))
@pytest.mark.parametrize("model", S.MODELS)
def test_step_random_shapes_match_float64(model, seed):
    """part 2: random (C, chunk, N, d_e, option set, edge importance, QuatE route) - ragged tiles of every kernel of the four models"""
    c = S.fuzz_case(model, seed)
    bad, _ = S.conditions(c)
    assert not bad, "\n".join(bad)
    run_case(c, "random")


@pytest.mark.parametrize("c", S.HEAVY_CASES, ids=lambda c: c["id"])
def test_step_heavy_lists_match_float64(c):
    """part 3: hub entity 7 and dominant relation 1 - update lists of hundreds of entries on an entity row and on a 2 d_e wide relation
    row (TransD: both rows 104 floats, chunk 100 no multiple of its 8 row groups) - compared as tests/test_gpu_parity.py::test_fused_step_heavy_lists_match_oracle compares, at its tolerances, nothing left out"""
    for step, bt in enumerate(S.batches(c, skewed=_skewed_batch)):
        eng, b, want, ref, _, tag = _run_step(c, bt, step)
        out, ent64, es64, rel64, rs64 = ref
        assert min(S.list_lengths(bt)) > 64
        gn = want["neg_score"].cpu().numpy().reshape(out["neg_score"].shape)
        _close(gn, out["neg_score"], 1e-4, 1e-4, tag + " neg_score")
        _close(eng.read_loss()[:3], out["log"][:3], 1e-4, 1e-5, tag + " loss")
        _close(eng.ent_state.cpu(), es64, 2e-3, 1e-9, tag + " ent state")
        _close(eng.rel_state.cpu(), rs64, 2e-3, 1e-9, tag + " rel state")
        _close(eng.ent.cpu(), ent64, 1e-4, 5e-3 * c["lr"], tag + " entity rows")
        _close(eng.rel.cpu(), rel64, 1e-4, 5e-3 * c["lr"], tag + " relation rows")
        rows = lambda g, r: (float(np.abs(g - r).max() / (5e-3 * c["lr"])), float(np.abs(g - r).max()), 5e-3 * c["lr"])
        _record("heavy", tag, "lists %d / %d entries, nothing left out" % S.list_lengths(bt),
                neg_score=S.worst(gn, out["neg_score"], S.score_bound(out["neg_score"])),
                ent_rows=rows(_f64(eng.ent), ent64), rel_rows=rows(_f64(eng.rel), rel64))


# --------------------------------------------------------------------------------------------------------------------------
# ranking and top-K over several tiles
# --------------------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: %d of %d ranks differ, first at triple %d (got %d, float64 %d)" % (
        what, len(bad), len(want), bad[0] if len(bad) else -1, got[bad[0]] if len(bad) else 0, want[bad[0]] if len(bad) else 0)


def _topk(model, c, ent, rel, side, K, filt=None):
    """kge_topk_select / _filtered over all entities: (ids [E, K], scores [E, K])"""
    from dglke_amd import _lib
    Q = S.MOD[model]
    Lb = _lib.lib()
    E, n, d_e = len(c.h), c.n, c.d_e
    h, r, t, cd = _dev(c.h), _dev(c.r), _dev(c.t), torch.arange(n, dtype=torch.int64, device=DEV)
    res_s = torch.zeros(E, K, dtype=torch.float32, device=DEV)
    res_o = torch.full((E, K), -1, dtype=torch.int64, device=DEV)
    base = torch.zeros(E, dtype=torch.int64, device=DEV)
    ws = torch.empty(_lib.topk_workspace_bytes(Q.MODEL_ID, E, n, d_e, K), dtype=torch.uint8, device=DEV)
    a = (Q.MODEL_ID, side, _lib.ptr(ent), n, _lib.ptr(rel), n, _lib.ptr(h), _lib.ptr(r), _lib.ptr(t), E, d_e, S.rel_width(model, d_e),
         S.rank_gamma(model), 1.0, _lib.ptr(cd), n, _lib.ptr(base), 1, 1, K, _lib.ptr(res_s), _lib.ptr(res_o), _lib.ptr(ws), ws.numel())
    if filt is not None:
        fr, fi = _dev(filt[0].reshape(-1)), _dev(filt[1])
        _lib.check(Lb.kge_topk_select_filtered(*a, _lib.ptr(fr), _lib.ptr(fi), _lib.stream_ptr()))
    else:
        _lib.check(Lb.kge_topk_select(*a, _lib.stream_ptr()))
    return res_o.cpu().numpy(), res_s.cpu().numpy()


def _entries(model, c, ent, rel, check, check_pos):
    """every ranking entry the model has, at both Ranker batches: check(got ranks, neg_head, lists, columns, what)"""
    from dglke_amd import eval as kev
    E = len(c.h)
    cols = S.rank_list()
    for flags in ((0, S.QE.FORCE_PAIRWISE) if model == "QuatE" else (0,)):
        for batch in S.RANK_BATCHES:
            rk = kev.Ranker(model, ent, rel, S.rank_gamma(model), 1.0, batch=batch, flags=flags)
            for neg_head in (False, True):
                lists = S.PR.filter_lists(c, neg_head)
                for filt in (None, lists):
                    what = "flags=%d batch=%d neg_head=%d %s" % (flags, batch, neg_head, "filtered" if filt else "raw")
                    fl = None if filt is None else (_dev(filt[0]), _dev(filt[1]))
                    got, pos = rk.ranks(c.h, c.r, c.t, neg_head, filt=fl, want_pos_score=True)
                    check(got.cpu().numpy(), neg_head, filt, None, "Ranker.ranks " + what)
                    check_pos(pos.cpu().numpy(), neg_head, "Ranker.ranks " + what)
                    got = rk.chunked_ranks(c.h, c.r, c.t, neg_head, S.RANK_CHUNK, filt=fl)
                    check(got.cpu().numpy(), neg_head, filt, None, "Ranker.chunked_ranks " + what)
                    fc = None if filt is None else kev.filter_columns(cols, filt, 0, E)
                    got = rk.ranks(c.h, c.r, c.t, neg_head, filt=fc, cand=cols)
                    check(got.cpu().numpy(), neg_head, filt, cols, "Ranker.ranks list " + what)


@pytest.mark.parametrize("d_e", S.RANK_WIDTHS)
@pytest.mark.parametrize("model", S.MODELS)
def test_ranking_entries_equal_float64_over_several_tiles(model, d_e):
    """part 4, exact tables: Ranker.ranks raw, filtered and on an explicit candidate list, Ranker.chunked_ranks with chunks that span
    two row tiles (PairRE, TransH, TransD: per-chunk lists with -1 pads and self_cand too), QuatE's relation ranking (TransD has
    none: that entry is closed) and kge_topk_select (PairRE, TransH, TransD: _filtered too) for K in 1, 10, 128: ranks and order
    EQUAL the float64 ones, scores the float32 statement's bits.  TransD: the parameter is the half-width k"""
    from dglke_amd import eval as kev
    Q = S.MOD[model]
    c = Q.tie_inputs(S.RANK_N, d_e, S.RANK_E)
    ent, rel = _dev(c.ent), _dev(c.rel)
    E = len(c.h)
    sc = {nh: (Q.tie_scores(c, c.h, c.r, c.t, nh), Q.tie_scores(c, c.h, c.r, c.t, nh, np.float32)) for nh in (False, True)}

    def check(got, neg_head, lists, cols, what):
        p, Sc = sc[neg_head][0]
        lo, hi, _ = S.rank_band(c, p, Sc, neg_head, lists, cols, 0.0)
        assert np.array_equal(lo, hi)
        _same(got, lo, what)

    def check_pos(pos, neg_head, what):
        assert np.array_equal(pos, sc[neg_head][1][0]), what + ": positive scores"

    _entries(model, c, ent, rel, check, check_pos)
    if model != "QuatE":
        cand = S.PR.tie_candidates(S.RANK_N, E, S.RANK_CHUNK)
        rk = kev.Ranker(model, ent, rel, S.rank_gamma(model), 1.0, batch=E)
        for neg_head in (False, True):
            p, Sc = sc[neg_head][0]
            for self_cand in (False, True):
                what = "Ranker.chunked_ranks lists neg_head=%d self_cand=%d" % (neg_head, self_cand)
                got, pos = rk.chunked_ranks(c.h, c.r, c.t, neg_head, S.RANK_CHUNK, cand=_dev(cand), self_cand=self_cand, want_pos_score=True)
                _same(got.cpu().numpy(), S.PR.chunked_ranks_of(c, p, Sc, neg_head, cand, self_cand, S.RANK_CHUNK), what)
                check_pos(pos.cpu().numpy(), neg_head, what)
            got = rk.chunked_ranks(c.h, c.r, c.t, neg_head, S.RANK_CHUNK, self_cand=True)
            _same(got.cpu().numpy(), S.PR.chunked_ranks_of(c, p, Sc, neg_head, None, True, S.RANK_CHUNK), "Ranker.chunked_ranks all entities self_cand")
    else:
        p, Sr = Q.rel_tie_scores(c, c.h, c.r, c.t)
        for flags in (0, Q.FORCE_PAIRWISE):
            for batch in S.RANK_BATCHES:
                rk = kev.Ranker(model, ent, rel, 0.0, 1.0, batch=batch, flags=flags)
                for filtered in (False, True):
                    lists = Q.relation_lists(c, filtered)
                    got, pos = rk.relation_ranks(c.h, c.r, c.t, (_dev(lists[0]), _dev(lists[1])), want_pos_score=True)
                    what = "Ranker.relation_ranks flags=%d batch=%d %s" % (flags, batch, "filtered" if filtered else "raw")
                    _same(got.cpu().numpy(), Q.ranks_of(p, Sr, lists), what)
                    assert np.array_equal(pos.cpu().numpy(), p.astype(np.float32)), what + ": positive scores"
    for side in (0, 1):
        Sc, S32 = sc[bool(side)][0][1], sc[bool(side)][1][1]
        frng, fids = S.PR.filter_lists(c, bool(side))
        for filtered in ((False,) if model == "QuatE" else (False, True)):
            for K in S.RANK_TOPK:
                go, gs = _topk(model, c, ent, rel, side, K, (frng, fids) if filtered else None)
                for i in range(E):
                    keep = np.ones(S.RANK_N, bool)
                    if filtered:
                        keep[fids[frng[i, 0]:frng[i, 1]]] = False
                    ids = np.nonzero(keep)[0]
                    order = ids[np.argsort(-Sc[i, ids], kind="stable")][:K]
                    what = "kge_topk_select%s side=%d K=%d row %d" % ("_filtered" if filtered else "", side, K, i)
                    assert np.array_equal(go[i], order), what + ": order"
                    assert np.array_equal(gs[i], S32[i, order]), what + ": scores"


@pytest.mark.parametrize("d_e", S.RANK_WIDTHS)
@pytest.mark.parametrize("model", S.MODELS)
def test_ranking_entries_stay_inside_the_float64_band_on_random_tables(model, d_e):
    """part 4, random tables: every rank inside [lo, hi] of the float64 scores under the score tolerance of tests/test_gpu_eval.py
    (at least 90 % of the intervals hold one rank: asserted on the CPU), top-K under `accept` of tests/test_gpu_infer.py"""
    c = S.rank_random_inputs(model, d_e)
    ent, rel = _dev(c.ent), _dev(c.rel)
    E = len(c.h)
    sc = {nh: S.rank_scores(model, c, nh) for nh in (False, True)}

    def check(got, neg_head, lists, cols, what):
        p, Sc = sc[neg_head]
        lo, hi, _ = S.rank_band(c, p, Sc, neg_head, lists, cols, TOL)
        bad = np.nonzero((got < lo) | (got > hi))[0]
        assert not len(bad), "%s: %d ranks outside the band, first at triple %d (got %d, band %d .. %d)" % (
            what, len(bad), bad[0], got[bad[0]], lo[bad[0]], hi[bad[0]])

    def check_pos(pos, neg_head, what):
        p = sc[neg_head][0]
        _close(pos, p, 1e-4, 1e-4, what + ": positive scores")

    _entries(model, c, ent, rel, check, check_pos)
    for side in (0, 1):
        Sc = sc[bool(side)][1]
        frng, fids = S.PR.filter_lists(c, bool(side))
        for filtered in ((False,) if model == "QuatE" else (False, True)):
            for K in S.RANK_TOPK:
                go, gs = _topk(model, c, ent, rel, side, K, (frng, fids) if filtered else None)
                for i in range(E):
                    keep = np.ones(S.RANK_N, bool)
                    if filtered:
                        keep[fids[frng[i, 0]:frng[i, 1]]] = False
                    exact = {int(j): [float(Sc[i, j])] for j in np.nonzero(keep)[0]}
                    assert np.all(go[i] >= 0), "row %d: empty slots among %d candidates" % (i, len(exact))
                    accept(exact, [int(j) for j in go[i]], [float(v) for v in gs[i]], K, None)
