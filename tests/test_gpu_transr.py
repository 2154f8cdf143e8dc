"""TransR on the HIP path (kge_transr.hip): the fused step against the goldens recorded from the reference -
scores, loss terms, the three trace gradients, Adagrad state and rows of the entity, relation AND projection
tables (two projection traces per step, score_fun.py:131-166, :173-174)."""
import numpy as np
import pytest
import torch

from golden_util import golden_names, load_golden
from test_gpu_parity import DEV, _close, build_model, golden_batch, grad_tol

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", golden_names(transr=True, nd=None))
def test_transr_fused_step_matches_reference(name):
    """transr_*: the strict step; nd_transr_* (round 6, VERDICT r05 missing 2): --neg_deg_sample on the fused TransR step
    (KGE_FLAG_NEG_DEG_SAMPLE) - the chunk's own corrupted-side entities are projected like every other negative, the diagonal is
    masked, their gradients join the positive trace (general_models.py:396-402, 417-432) - against the reference run with
    args.neg_deg_sample = True."""
    from oracle import kge_oracle as O
    z, case = load_golden(name)
    m = build_model(case, z)
    pe = m.score_func.projection_emb
    pe.emb.copy_(torch.from_numpy(z["init_projection"]))
    pe.state_sum.zero_()
    eng = m.engine
    assert eng.proj.data_ptr() == pe.emb.data_ptr()
    nd = bool(case.get("neg_deg", False))
    if nd:
        eng.hp.flags = 32
    prev_ent = z["init_entity"]
    for s in range(1, case["steps"] + 1):
        p = "s%d_" % s
        b = golden_batch(z, case, s)
        want = eng.alloc_outputs(b)
        eng.step(b, want)
        torch.cuda.synchronize()
        if nd:
            # the sampled negatives are rows chunk.. of every chunk's N' block of g_neg; their regulariser is added by the update
            # kernel in this mode (the reference's trace gradient includes it)
            chunk, De = case["chunk"], want["g_neg"].shape[1]
            assert tuple(want["neg_score"].shape) == z[p + "neg_score"].shape
            gn = want["g_neg"].cpu().numpy().reshape(-1, chunk + case["N"], De)[:, chunk:].reshape(-1, De)
            if case["reg_coef"] > 0:
                gn = gn + O.reg_grad(prev_ent[z[p + "neg"]].astype(np.float64), case["reg_coef"], case["reg_norm"])
            want["g_neg"] = torch.from_numpy(gn.astype(np.float32))
        prev_ent = None
        _close(want["pos_score"].cpu(), z[p + "pos_score"], 1e-4, 1e-4, name + " pos_score")
        _close(want["neg_score"].cpu(), z[p + "neg_score"], 1e-4, 1e-4, name + " neg_score")
        l4 = eng.read_loss()
        ref_log = z[p + "log"]
        _close(l4[0], ref_log[0], 1e-4, 1e-5, name + " pos_loss")
        _close(l4[1], ref_log[1], 1e-4, 1e-5, name + " neg_loss")
        _close(l4[2], ref_log[2], 1e-4, 1e-5, name + " loss")
        _close(l4[3], ref_log[3], 1e-4, 1e-7, name + " reg")
        ue = b.p["ue_id"]
        sel = np.searchsorted(ue, z[p + "nid"])
        _close(want["g_pos_ent"].cpu().numpy()[sel], z[p + "g_pos_ent"], 3e-4, grad_tol(z[p + "g_pos_ent"]), name + " g_pos_ent")
        _close(want["g_neg"].cpu(), z[p + "g_neg"], 3e-4, grad_tol(z[p + "g_neg"]), name + " g_neg")
        _close(want["g_rel"].cpu(), z[p + "g_rel"], 3e-4, grad_tol(z[p + "g_rel"]), name + " g_rel")
        _close(eng.ent_state.cpu(), z[p + "entity_state"], 2e-3, 1e-9, name + " ent state")
        _close(eng.rel_state.cpu(), z[p + "relation_state"], 2e-3, 1e-9, name + " rel state")
        _close(eng.proj_state.cpu(), z[p + "projection_state"], 2e-3, 1e-9, name + " projection state")
        _close(eng.proj.cpu(), z[p + "projection"], 1e-4, 5e-3 * case["lr"], name + " projection rows")
        if (p + "entity") in z:
            _close(eng.ent.cpu(), z[p + "entity"], 1e-4, 5e-3 * case["lr"], name + " entity rows")
            _close(eng.rel.cpu(), z[p + "relation"], 1e-4, 5e-3 * case["lr"], name + " relation rows")
        prev_ent = eng.ent.cpu().numpy()
    _close(eng.ent.cpu(), z["final_entity"], 1e-4, 1e-2 * case["lr"], name + " final entity")
    _close(eng.rel.cpu(), z["final_relation"], 1e-4, 1e-2 * case["lr"], name + " final relation")


# (adversarial weighting only in the first case: with it a negative row can end up with a gradient that is a few fp32 roundings of
#  cancelling terms, and Adagrad's first steps move a row by lr * g / rms(g) whatever the size of g - no digits to compare)
TILE_SHAPES = [
    # n_ent, n_rel, hidden, double_rel, B, N, chunk, adversarial
    (500, 9, 72, True, 70, 70, 35, True),        # De 72 / Dr 144: the 64 x 208 tiles, 5 and 9 column blocks (instances 7 and 13), ragged rows
    (500, 9, 108, True, 48, 40, 24, False),      # Dr 216 > 208: the 64 x 64 tiles (16-byte loads), 4 column tiles with a partial last one
    (300, 5, 18, True, 24, 10, 12, False),       # De 18 / Dr 36, De % 4 != 0: the 64 x 64 tiles with scalar loads
    (2000, 40, 200, False, 128, 256, 64, False), # the FB15k recipe's operands (13 column blocks), 4 row tiles of negatives, 2 chunks
    (300, 5, 64, False, 32, 130, 16, False),     # 4 column blocks; N = 130: a row tile with 2 real rows
]


@pytest.mark.parametrize("shape", TILE_SHAPES, ids=lambda c: "De%d-%s-B%d-N%d" % (c[2], "dr" if c[3] else "sq", c[4], c[5]))
def test_transr_fused_step_matches_oracle_at_tile_shapes(shape):
    """dims that span several tiles and do not divide them, through every tile routine of kge_transr.hip / kge_transr_wide.hpp."""
    from dglke_amd import plan
    from dglke_amd.engine import StepEngine
    from oracle import kge_oracle as O
    n_ent, n_rel, hidden, dr, B, N, chunk, adv = shape
    rng = np.random.RandomState(4)
    eng = StepEngine("TransR", n_ent, n_rel, hidden, 10.0, 0.05, DEV, False, dr, adv, 1.0, 1e-6, 3)
    d_r = 2 * hidden if dr else hidden
    assert eng.proj.shape == (n_rel, hidden * d_r)
    cfg = O.Config("TransR", 10.0, hidden, 0.05, adv=adv, adv_temp=1.0, reg_coef=1e-6, reg_norm=3, double_rel=dr)
    ent, rel, proj = (x.cpu().numpy().astype(np.float64) for x in (eng.ent, eng.rel, eng.proj))
    es, rs, ps = np.zeros(n_ent), np.zeros(n_rel), np.zeros(n_rel)
    for step in range(1, 3):
        bt = O.synth_batch(rng, n_ent, n_rel, B, N, chunk, step)
        b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], chunk, N, bt["neg_head"], DEV)
        want = eng.alloc_outputs(b)
        eng.step(b, want)
        out = O.transr_train_step(cfg, ent, es, rel, rs, proj, ps, bt["nid"], bt["h_local"], bt["t_local"], bt["r"],
                                  bt["neg"], bt["neg_head"], chunk, N)
        torch.cuda.synchronize()
        _close(want["pos_score"].cpu(), out["pos_score"], 1e-4, 1e-4, "pos")
        _close(want["neg_score"].cpu(), out["neg_score"], 1e-4, 2e-4, "neg")
        _close(want["g_neg"].cpu(), out["g_neg"], 3e-4, grad_tol(out["g_neg"]), "g_neg")
        _close(want["g_rel"].cpu(), out["g_rel"], 3e-4, grad_tol(out["g_rel"]), "g_rel")
        sel = np.searchsorted(b.p["ue_id"], bt["nid"])
        _close(want["g_pos_ent"].cpu().numpy()[sel], out["g_pos_ent"], 3e-4, grad_tol(out["g_pos_ent"]), "g_pos_ent")
        _close(eng.proj_state.cpu(), ps, 2e-3, 1e-9, "projection state")
        _close(eng.rel_state.cpu(), rs, 2e-3, 1e-9, "relation state")
        _close(eng.proj.cpu(), proj, 1e-4, 5e-3 * 0.05, "projection rows")
        _close(eng.rel.cpu(), rel, 1e-4, 5e-3 * 0.05, "relation rows")
        # a row whose whole trace gradient is rounding residue of cancelling terms (an edge with h == t: (h - t) P = 0 in exact
        # arithmetic) has no digits to compare - Adagrad's first steps move it by lr * g / rms(g) whatever the size of g
        starved = bt["nid"][np.abs(out["g_pos_ent"]).max(axis=1) < 1e-6 * np.abs(out["g_pos_ent"]).max()]
        starved = np.setdiff1d(starved, bt["neg"])
        assert len(starved) <= 2, starved
        got_ent = eng.ent.cpu().numpy().astype(np.float64)
        got_ent[starved] = ent[starved]
        _close(got_ent, ent, 1e-4, 5e-3 * 0.05, "entity rows")
        # re-synchronise the fp64 oracle on the fp32 tables so that drift does not accumulate
        ent, rel, proj = (x.cpu().numpy().astype(np.float64) for x in (eng.ent, eng.rel, eng.proj))
        es, rs, ps = (x.cpu().numpy().astype(np.float64) for x in (eng.ent_state, eng.rel_state, eng.proj_state))


def run_projection_ops_case(C, chunk, N, De, Dr):
    """the body of test_transr_projection_ops_match_torch_autograd; -> the two projections and the three gradients"""
    from dglke_amd import ops
    g = torch.Generator().manual_seed(C * 100 + N)
    B = C * chunk
    x = torch.randn(B, De, generator=g)
    proj = torch.randn(B, De * Dr, generator=g) * 0.3
    neg = torch.randn(C * N, De, generator=g)
    wy = torch.randn(B, Dr, generator=g)
    wY = torch.randn(C, chunk, N, Dr, generator=g)
    # reference formulation, fp64
    x64, p64, n64 = (t.double().requires_grad_(True) for t in (x, proj, neg))
    P = p64.reshape(C, chunk, De, Dr)
    y_ref = torch.matmul(x64.reshape(C, chunk, 1, De), P).reshape(B, Dr)
    Y_ref = torch.matmul(n64.reshape(C, 1, N, De), P)
    ((y_ref * wy.double()).sum() + (Y_ref * wY.double()).sum()).backward()
    xd, pd, nd = (t.to(DEV).requires_grad_(True) for t in (x, proj, neg))
    y = ops.transr_project(xd, pd, De, Dr)
    Y = ops.transr_project_neg(nd, pd, C, chunk, N, De, Dr)
    ((y * wy.to(DEV)).sum() + (Y * wY.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(y.detach().cpu().numpy(), y_ref.detach().numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(Y.detach().cpu().numpy(), Y_ref.detach().numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), x64.grad.numpy(), rtol=2e-5, atol=3e-5)
    np.testing.assert_allclose(nd.grad.cpu().numpy(), n64.grad.numpy(), rtol=2e-5, atol=2e-4)
    np.testing.assert_allclose(pd.grad.cpu().numpy(), p64.grad.numpy(), rtol=2e-5, atol=2e-4)
    return dict(y=y.detach(), Y=Y.detach(), gx=xd.grad, gneg=nd.grad, gproj=pd.grad)


@pytest.mark.parametrize("C,chunk,N,De,Dr", [(2, 8, 12, 16, 16), (1, 5, 7, 10, 6), (3, 33, 70, 64, 40), (2, 64, 64, 128, 72)])
def test_transr_projection_ops_match_torch_autograd(C, chunk, N, De, Dr):
    """the per-op route's HIP projections (kge_transr_project / _neg and their analytic backward) against the reference's
    th.matmul formulation (score_fun.py:131-166) in fp64 with torch autograd."""
    run_projection_ops_case(C, chunk, N, De, Dr)


@pytest.mark.parametrize("shape", [TILE_SHAPES[0], TILE_SHAPES[3], TILE_SHAPES[4]],
                         ids=lambda c: "nd-De%d-%s-B%d-N%d" % (c[2], "dr" if c[3] else "sq", c[4], c[5]))
def test_transr_neg_deg_sample_matches_oracle_at_tile_shapes(shape):
    """round 6: --neg_deg_sample on the fused TransR step at shapes that span several tiles (N' = chunk + N: 105, 320, 146 negative rows per
    chunk through the wide and the 64 x 64 routines) - scores incl. the masked diagonal, the three trace gradients (in-batch rows in the
    positive trace), the three tables - against the fp64 oracle (`transr_forward_backward` with neg_deg, pinned by the nd_transr_* goldens)."""
    from dglke_amd import plan
    from dglke_amd.engine import StepEngine
    from oracle import kge_oracle as O
    n_ent, n_rel, hidden, dr, B, N, chunk, adv = shape
    rng = np.random.RandomState(6)
    eng = StepEngine("TransR", n_ent, n_rel, hidden, 10.0, 0.05, DEV, False, dr, adv, 1.0, 1e-6, 3, flags=32)
    cfg = O.Config("TransR", 10.0, hidden, 0.05, adv=adv, adv_temp=1.0, reg_coef=1e-6, reg_norm=3, double_rel=dr, neg_deg=True)
    ent, rel, proj = (x.cpu().numpy().astype(np.float64) for x in (eng.ent, eng.rel, eng.proj))
    es, rs, ps = np.zeros(n_ent), np.zeros(n_rel), np.zeros(n_rel)
    Np = chunk + N
    for step in range(1, 3):
        bt = O.synth_batch(rng, n_ent, n_rel, B, N, chunk, step)
        b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], chunk, N, bt["neg_head"], DEV)
        want = eng.alloc_outputs(b)
        eng.step(b, want)
        negrows = ent[bt["neg"]].copy()
        out = O.transr_train_step(cfg, ent, es, rel, rs, proj, ps, bt["nid"], bt["h_local"], bt["t_local"], bt["r"],
                                  bt["neg"], bt["neg_head"], chunk, N)
        torch.cuda.synchronize()
        assert tuple(want["neg_score"].shape) == (B // chunk, chunk, Np)
        _close(want["pos_score"].cpu(), out["pos_score"], 1e-4, 1e-4, "pos")
        _close(want["neg_score"].cpu(), out["neg_score"], 1e-4, 2e-4, "neg (masked diagonal = 0)")
        gn = want["g_neg"].cpu().numpy().reshape(-1, Np, hidden)[:, chunk:].reshape(-1, hidden)       # the sampled rows of every chunk's block
        gn = gn + O.reg_grad(negrows, 1e-6, 3)                                                          # (their regulariser: added by the update kernel)
        _close(gn, out["g_neg"], 3e-4, grad_tol(out["g_neg"]), "g_neg")
        _close(want["g_rel"].cpu(), out["g_rel"], 3e-4, grad_tol(out["g_rel"]), "g_rel")
        sel = np.searchsorted(b.p["ue_id"], bt["nid"])
        _close(want["g_pos_ent"].cpu().numpy()[sel], out["g_pos_ent"], 3e-4, grad_tol(out["g_pos_ent"]), "g_pos_ent (+ in-batch negative rows)")
        _close(eng.proj_state.cpu(), ps, 2e-3, 1e-9, "projection state")
        _close(eng.proj.cpu(), proj, 1e-4, 5e-3 * 0.05, "projection rows")
        _close(eng.rel.cpu(), rel, 1e-4, 5e-3 * 0.05, "relation rows")
        _close(eng.ent_state.cpu(), es, 2e-3, 1e-9, "entity state")
        ent[:], rel[:], proj[:] = (x.cpu().numpy().astype(np.float64) for x in (eng.ent, eng.rel, eng.proj))
        es[:], rs[:], ps[:] = (x.cpu().numpy().astype(np.float64) for x in (eng.ent_state, eng.rel_state, eng.proj_state))
