"""The two column layouts of the register-resident loss rows (kge_loss_body.hpp) against the float64 oracle: packs of four
consecutive columns per lane when N % 4 == 0 (16-byte row accesses; one pack up to 256 columns, two up to 512) and the strided
lane + 64 u form otherwise - at every width where the live-lane predicate changes (one lane, the last live lane partial and full,
the exact fill of one and two packs), through kge_loss_fwd_bwd (the generic instances: every genre, the pairwise forms, edge
importance, saturated rows) and through the fused step (the raw-product TransE_l2 instance with and without per-step outputs,
a distance on its 1e-30 floor, the masked diagonal column of --neg_deg_sample).

Tolerances: those of tests/test_gpu_loss_entry.py and tests/test_gpu_parity.py (loss 1e-4 / 1e-5, gradients 3e-4 of the largest
component, rows 5e-3 lr on the first Adagrad steps, states 2e-3)."""
import numpy as np
import pytest
import torch

from oracle import kge_oracle as O
from test_gpu_loss_entry import _entry, _scores
from test_gpu_parity import DEV, _close, grad_tol

pytestmark = pytest.mark.gpu

B = 37                                                              # not a multiple of the four wavefronts of a workgroup
PACKED = [4, 8, 60, 64, 68, 128, 132, 200, 252, 256, 260, 512]
STRIDED = [1, 3, 6, 130, 201, 255]


def _check(pos, neg, w, genre, adv, T, pairwise, margin, tag):
    loss3, dpos, dneg = _entry(pos, neg, w, genre, adv, T, pairwise, margin)
    (pl, nl, loss), dp64, dn64 = O.loss_fwd_bwd(pos.astype(np.float64), neg.astype(np.float64),
                                                None if w is None else w.astype(np.float64), genre, adv, T, pairwise, margin)
    assert np.isfinite(loss) and np.isfinite(dp64).all() and np.isfinite(dn64).all(), tag
    assert np.isfinite(dneg).all() and np.isfinite(dpos).all() and np.isfinite(loss3[2]), tag + ": not finite"
    if pairwise:
        _close(loss3[2], loss, 1e-4, 1e-5, tag + " loss")
        act32 = (np.float32(margin) - (pos[:, None] - neg)) >= 0        # (the float32 / float64 hinge kink: test_gpu_loss_entry.py)
        act64 = (margin - (pos.astype(np.float64)[:, None] - neg.astype(np.float64))) >= 0
        flip = act32 != act64
        assert flip.sum() <= 1e-4 * flip.size, tag
        if genre == "Hinge" and flip.any():
            dneg = np.where(flip, dn64, dneg)
            dpos = np.where(flip.any(1), dp64, dpos)
    else:
        _close(loss3, [pl, nl, loss], 1e-4, 1e-5, tag + " loss3")
    _close(dpos, dp64, 3e-4, grad_tol(dp64), tag + " dpos")
    _close(dneg, dn64, 3e-4, grad_tol(dn64), tag + " dneg")
    return loss3, dpos, dneg


@pytest.mark.parametrize("N", PACKED + STRIDED, ids=lambda n: "N%d" % n)
def test_logsigmoid_rows_at_every_layout_width(N):
    """Logsigmoid with and without -adv, with and without edge importance; rows 0-3 of the scores are saturated (+-40)."""
    rng = np.random.RandomState(7000 + N)
    w_all = rng.uniform(0.5, 1.5, size=B).astype(np.float32)
    pos, neg = _scores(rng, B, N, 1.0)
    for adv in (False, True):
        for w in (None, w_all):
            tag = "N%d Logsigmoid adv=%s w=%s" % (N, adv, w is not None)
            first = _check(pos, neg, w, "Logsigmoid", adv, 1.0, False, 1.0, tag)
    again = _entry(pos, neg, w_all, "Logsigmoid", True, 1.0, False, 1.0)       # deterministic run to run
    for a, b in zip(first, again):
        assert np.array_equal(a, b), "N%d: run-to-run difference" % N


@pytest.mark.parametrize("N", [200, 201], ids=lambda n: "N%d" % n)
def test_every_other_genre_and_the_pairwise_forms(N):
    rng = np.random.RandomState(7500 + N)
    w_all = rng.uniform(0.5, 1.5, size=B).astype(np.float32)
    for genre in ("Logistic", "Hinge", "BCE"):
        pos, neg = _scores(rng, B, N, 1.0)
        for w in (None, w_all):
            for adv in (False, True):
                _check(pos, neg, w, genre, adv, 1.0, False, 1.0, "N%d %s adv=%s w=%s" % (N, genre, adv, w is not None))
            if genre != "BCE":
                _check(pos, neg, w, genre, False, 1.0, True, 1.0, "N%d %s pairwise w=%s" % (N, genre, w is not None))


def _engine(model, n_ent, n_rel, D, gamma, lr, ent, rel, flags=0, adv=True):
    from dglke_amd.engine import StepEngine
    eng = StepEngine(model, n_ent, n_rel, D, gamma, lr, DEV, False, False, adv, 1.0, 0.0, 3, flags=flags)
    eng.load_tables(ent, rel)
    return eng


def _step_against_oracle(eng, cfg, bt, chunk, N, with_outputs, tag, lr):
    """one fused step against the float64 oracle started from the engine's tables; returns the outputs (or None)"""
    from dglke_amd import plan
    ent64, rel64 = eng.ent.cpu().numpy().astype(np.float64), eng.rel.cpu().numpy().astype(np.float64)
    es64, rs64 = eng.ent_state.cpu().numpy().astype(np.float64), eng.rel_state.cpu().numpy().astype(np.float64)
    b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], chunk, N, bt["neg_head"], DEV)
    want = eng.alloc_outputs(b) if with_outputs else None
    eng.step(b, want)
    torch.cuda.synchronize()
    out = O.train_step(cfg, ent64, es64, rel64, rs64, bt["nid"], bt["h_local"], bt["t_local"], bt["r"], bt["neg"], bt["neg_head"],
                       chunk, N)
    if with_outputs:
        _close(want["neg_score"].cpu(), out["neg_score"], 1e-4, 1e-4, tag + " neg_score")
        _close(eng.read_loss()[:3], out["log"][:3], 1e-4, 1e-5, tag + " loss")
        if not cfg.neg_deg:
            _close(want["g_neg"].cpu(), out["g_neg"], 3e-4, grad_tol(out["g_neg"]), tag + " g_neg")
        _close(want["g_rel"].cpu(), out["g_rel"], 3e-4, grad_tol(out["g_rel"]), tag + " g_rel")
    for got, ref, what in ((eng.ent_state, es64, "ent state"), (eng.rel_state, rs64, "rel state")):
        _close(got.cpu(), ref, 2e-3, 1e-9, tag + " " + what)
    _close(eng.ent.cpu(), ent64, 1e-4, 5e-3 * lr, tag + " entity rows")
    _close(eng.rel.cpu(), rel64, 1e-4, 5e-3 * lr, tag + " relation rows")
    return want


@pytest.mark.parametrize("with_outputs", [False, True], ids=["lean", "outputs"])
@pytest.mark.parametrize("N", [16, 40], ids=lambda n: "N%d" % n)
def test_raw_product_rows_through_the_fused_step(N, with_outputs):
    """TransE_l2 at its smallest shapes (D 32, B 48): the loss launch rebuilds the scores from the raw products of the merged
    forward launch in the packed layout - without per-step outputs (the lean instance) and with them; tail then head corruption."""
    n_ent, n_rel, D, lr, gamma = 300, 7, 32, 0.25, 19.9
    cfg = O.Config("TransE_l2", gamma, D, lr, adv=True, adv_temp=1.0)
    rng = np.random.RandomState(8100 + N)
    ent = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(n_ent, D)).astype(np.float32)
    rel = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(n_rel, D)).astype(np.float32)
    eng = _engine("TransE_l2", n_ent, n_rel, D, gamma, lr, ent, rel)
    for step in (1, 2):
        bt = O.synth_batch(rng, n_ent, n_rel, 48, N, 16, step)      # three chunks of 16 positives
        _step_against_oracle(eng, cfg, bt, 16, N, with_outputs, "N%d step %d" % (N, step), lr)


@pytest.mark.parametrize("with_outputs", [False, True], ids=["lean", "outputs"])
def test_distance_on_its_floor_has_no_gradient(with_outputs):
    """a negative that equals h + r exactly (zero relation row, the head itself among the negatives; row values whose squares
    and products sum exactly in float32 and float64): |a|^2 + |b|^2 - 2 a.b = 0, the distance sits on the 1e-30 floor, gamma - n
    is 0 and the guarded reciprocal gives gradient 0 - everything finite, equal to the oracle (which has no gradient there)."""
    n_ent, n_rel, D, N, lr, gamma = 300, 7, 32, 16, 0.25, 19.9
    cfg = O.Config("TransE_l2", gamma, D, lr, adv=True, adv_temp=1.0)
    rng = np.random.RandomState(8200)
    ent = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(n_ent, D)).astype(np.float32)
    rel = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(n_rel, D)).astype(np.float32)
    bt = O.synth_batch(rng, n_ent, n_rel, 48, N, N, 1)              # step 1: tails corrupted, a = h + r
    h0 = int(bt["h"][0])
    assert int(bt["t"][0]) != h0
    row = np.zeros(D, np.float32)
    row[rng.permutation(D)[:16]] = rng.choice([-0.5, 0.5], size=16)  # |row|^2 = 4: sqrt, squares and dot products all exact
    ent[h0] = row
    rel[int(bt["r"][0])] = 0.0
    bt["neg"][5] = h0                                                # column 5 of chunk 0 (edge 0 is row 0 of that chunk)
    eng = _engine("TransE_l2", n_ent, n_rel, D, gamma, lr, ent, rel)
    want = _step_against_oracle(eng, cfg, bt, N, N, with_outputs, "floor", lr)
    assert np.isfinite(eng.ent.cpu().numpy()).all() and np.isfinite(eng.ent_state.cpu().numpy()).all()
    if with_outputs:
        assert float(want["neg_score"][0, 0, 5]) == np.float32(gamma)
        assert np.isfinite(want["g_neg"].cpu().numpy()).all()


def test_masked_diagonal_column_inside_a_pack():
    """--neg_deg_sample: column i % chunk of row i is the edge's own positive - score 0 and dL/dn exactly 0, its neighbours in the
    same pack of four columns not.  chunk 4 + 12 sampled = 16 columns against the oracle; chunk 1 + 7 sampled = 8 columns, where
    the in-batch negative row of a chunk receives ONLY the masked entry: its gradient row is exactly 0, the next three are not."""
    from dglke_amd import plan, _lib
    n_ent, n_rel, D, lr, gamma = 300, 7, 32, 0.25, 19.9
    cfg = O.Config("TransE_l2", gamma, D, lr, adv=True, adv_temp=1.0, neg_deg=True)
    rng = np.random.RandomState(8300)
    ent = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(n_ent, D)).astype(np.float32)
    rel = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(n_rel, D)).astype(np.float32)
    eng = _engine("TransE_l2", n_ent, n_rel, D, gamma, lr, ent, rel, flags=_lib.FLAG_NEG_DEG_SAMPLE)
    for step in (1, 2):
        bt = O.synth_batch(rng, n_ent, n_rel, 24, 12, 4, step)
        _step_against_oracle(eng, cfg, bt, 4, 12, True, "nd chunk 4 step %d" % step, lr)
    eng = _engine("TransE_l2", n_ent, n_rel, D, gamma, lr, ent, rel, flags=_lib.FLAG_NEG_DEG_SAMPLE)
    bt = O.synth_batch(rng, n_ent, n_rel, 6, 7, 1, 1)
    b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], 1, 7, bt["neg_head"], DEV)
    want = eng.alloc_outputs(b)
    eng.step(b, want)
    torch.cuda.synchronize()
    sc = want["neg_score"].cpu().numpy().reshape(6, 8)
    gn = want["g_neg"].cpu().numpy().reshape(6, 8, -1)
    assert np.all(sc[:, 0] == 0) and np.all(sc[:, 1:4] != 0)
    assert np.all(gn[:, 0] == 0), "the masked column carries a gradient"
    assert np.all(np.abs(gn[:, 1:4]).max(-1) > 0), "the masked column's neighbours in the pack lost their gradient"
    assert np.isfinite(gn).all()
