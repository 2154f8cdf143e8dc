"""The backward GEMM tiles' operand addressing (kge_neg_gemm.hip, neg_bwd_gemm_tile) against float64.

The tiles keep the ELEMENT OFFSET row * D of every reduction row in their LDS table and carry the dense operand's and W's
offsets along the macro steps (no multiply in the loop).  What can go wrong with that: a wrong offset in the predicated tail or in
the single remainder step, a stride taken for the wrong operand, a 32-bit product, a gathered id used where a dense row number was
meant.  The shapes are the smallest that reach each of those places:

  N = 24, chunk = 8      GA: one full macro step + a tail of 8, GN: the tail alone - fewer than two macro steps on both products
  N = 40, chunk = 56     GA: the loop runs once (2 macro steps) + tail, GN: loop once + the single remainder step + tail
  D = 72                 the second 64-column tile has 8 live columns
  N = chunk = 200, D = 400   the flagship step's own tile counts, one chunk
  gathered negatives with repeated ids, in descending order
  the dense instance (KGE_FLAG_DENSE_BWD) and the path without ids (kge_score_neg_bwd: the negatives ARE the operand)
  DistMult and ComplEx (D = 64): the GA tiles that write the per-edge gradient rows, both corruption sides
  an entity table of 2 800 000 x 400 floats: every row the step touches lies beyond 2^32 BYTES (the table is uninitialised but
  for its last thousand rows; 64-bit offsets are the only form built, so there is no case that selects a 32-bit one)

Entry points: kge_step_fused through StepEngine.step and kge_score_neg_fwd / kge_score_neg_bwd through ops.score_neg, as in
test_gpu_parity.py / test_gpu_modular_ops.py; reference: oracle/kge_oracle.py in float64 from the same float32 inputs;
tolerances: the suite's (scores 1e-4 abs + 1e-4 rel, gradients 3e-4 rel + 3e-4 of the largest component)."""
import numpy as np
import pytest
import torch

from oracle import kge_oracle as O
from test_gpu_parity import DEV, _close, grad_tol

pytestmark = pytest.mark.gpu

FLAG_DENSE_BWD = 256


def _descending_with_repeats(rng, n_ent, C, N):
    """C * N negative ids, every chunk in descending order with every third id repeated"""
    out = []
    for _ in range(C):
        ids = np.sort(rng.randint(0, n_ent, size=N))[::-1].copy()
        ids[1::3] = ids[0::3][:len(ids[1::3])]
        out.append(ids)
    return np.concatenate(out).astype(np.int64)


def _step_vs_oracle(model, hidden, dbl, B, chunk, N, flags=0, n_ent=500, n_rel=20, gamma=12.0, neg_ids=None, id_offset=0, tables=None,
                    steps=(1, 2), seed=7):
    """one fused step per corruption side from the same float32 tables as the float64 oracle; scores and the three gradient arrays.
    `id_offset`: the batch's entity ids are shifted by it (the oracle sees the table's last n_ent rows)"""
    from dglke_amd import plan
    from dglke_amd.engine import StepEngine
    lr = 0.1
    cfg = O.Config(model, gamma, hidden, lr, adv=True, adv_temp=1.0, reg_coef=1e-9, reg_norm=3, double_ent=dbl, double_rel=dbl)
    rng = np.random.RandomState(seed)
    rel = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(n_rel, cfg.rel_dim)).astype(np.float32)
    ent = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(n_ent, cfg.ent_dim)).astype(np.float32)
    if tables is None:
        eng = StepEngine(model, n_ent, n_rel, hidden, gamma, lr, DEV, dbl, dbl, True, 1.0, 1e-9, 3, flags=flags)
        eng.load_tables(ent, rel)
    else:
        big = tables[0]
        big[id_offset:].copy_(torch.from_numpy(ent))
        tables[2].copy_(torch.from_numpy(rel))
        eng = StepEngine(model, big.shape[0], n_rel, hidden, gamma, lr, DEV, dbl, dbl, True, 1.0, 1e-9, 3, flags=flags, tables=tables)
    for step in steps:
        ent64 = eng.ent[id_offset:].cpu().numpy().astype(np.float64)
        rel64 = eng.rel.cpu().numpy().astype(np.float64)
        es64 = eng.ent_state[id_offset:].cpu().numpy().astype(np.float64)
        rs64 = eng.rel_state.cpu().numpy().astype(np.float64)
        bt = O.synth_batch(rng, n_ent, n_rel, B, N, chunk, step)
        if neg_ids is not None:
            bt["neg"] = neg_ids(rng, n_ent, B // chunk, N)
        b = plan.make_batch(bt["h"] + id_offset, bt["t"] + id_offset, bt["r"], bt["neg"] + id_offset, chunk, N, bt["neg_head"], DEV)
        want = eng.alloc_outputs(b)
        for v in want.values():
            v.fill_(float("nan"))                  # an element no tile wrote must not pass as a stale value
        eng.step(b, want)
        torch.cuda.synchronize()
        out = O.train_step(cfg, ent64, es64, rel64, rs64, bt["nid"], bt["h_local"], bt["t_local"], bt["r"], bt["neg"], bt["neg_head"],
                           chunk, N)
        tag = "%s D%d B%d chunk%d N%d flags%d neg_head=%d" % (model, cfg.ent_dim, B, chunk, N, flags, bt["neg_head"])
        _close(want["neg_score"].cpu(), out["neg_score"], 1e-4, 1e-4, tag + " neg_score")
        sel = np.searchsorted(b.p["ue_id"], bt["nid"] + id_offset)
        _close(want["g_neg"].cpu(), out["g_neg"], 3e-4, grad_tol(out["g_neg"]), tag + " g_neg")                        # the GN product
        _close(want["g_pos_ent"].cpu().numpy()[sel], out["g_pos_ent"], 3e-4, grad_tol(out["g_pos_ent"]), tag + " g_pos_ent")   # GA ...
        _close(want["g_rel"].cpu(), out["g_rel"], 3e-4, grad_tol(out["g_rel"]), tag + " g_rel")                        # ... and its epilogue


SHAPES = [  # (hidden, B, chunk, N)
    (72, 16, 8, 24),
    (72, 112, 56, 40),
    (400, 200, 200, 200),
]


@pytest.mark.parametrize("hidden,B,chunk,N", SHAPES, ids=lambda v: str(v))
def test_gathered_tiles_match_float64(hidden, B, chunk, N):
    """TransE_l2, negatives gathered through neg_ids (the strict step's own instance), both corruption sides"""
    _step_vs_oracle("TransE_l2", hidden, False, B, chunk, N)


def test_gathered_tiles_with_repeated_descending_ids():
    """the LDS table is filled from the ids as they come: repeated rows and falling addresses"""
    _step_vs_oracle("TransE_l2", 72, False, 112, 56, 40, neg_ids=_descending_with_repeats)


@pytest.mark.parametrize("hidden,B,chunk,N", SHAPES[:2], ids=lambda v: str(v))
def test_dense_instance_matches_float64(hidden, B, chunk, N):
    """KGE_FLAG_DENSE_BWD: no table, the four rows of a lane and the wave-uniform step are arithmetic"""
    _step_vs_oracle("TransE_l2", hidden, False, B, chunk, N, flags=FLAG_DENSE_BWD)


@pytest.mark.parametrize("model,hidden,dbl", [("DistMult", 72, False), ("ComplEx", 32, True)], ids=["DistMult-D72", "ComplEx-D64"])
@pytest.mark.parametrize("flags", [0, FLAG_DENSE_BWD], ids=["gathered", "dense"])
def test_edge_writing_tiles_match_float64(model, hidden, dbl, flags):
    """DistMult / ComplEx: the GA tiles chain the per-edge gradient rows in their epilogue; tail- and head-corrupted step"""
    _step_vs_oracle(model, hidden, dbl, 112, 56, 40, flags=flags, gamma=20.0)


@pytest.mark.parametrize("model", ["TransE_l2", "DistMult"])
def test_tiles_without_ids_match_float64(model):
    """kge_score_neg_bwd: the negative rows are a dense [C * N, D] array and there are no ids - the table holds (c * N + k) * D"""
    from dglke_amd import ops
    C, chunk, N, D, gamma = 2, 56, 40, 72, 12.0
    rng = np.random.RandomState(3)
    x = rng.uniform(-0.2, 0.2, size=(C * chunk, D)).astype(np.float32)
    r = rng.uniform(-0.2, 0.2, size=(C * chunk, D)).astype(np.float32)
    nb = rng.uniform(-0.2, 0.2, size=(C * N, D)).astype(np.float32)
    W = rng.standard_normal((C, chunk, N)).astype(np.float32)
    for neg_head in (False, True):
        xt, rt, nt = (torch.from_numpy(v).to(DEV).requires_grad_() for v in (x, r, nb))
        s = ops.score_neg(model, neg_head, xt, rt, nt, C, chunk, N, gamma)
        (s * torch.from_numpy(W).to(DEV)).sum().backward()
        x64, r64, n64 = x.astype(np.float64), r.astype(np.float64), nb.astype(np.float64)
        a = O.pos_side(model, neg_head, x64, r64, 1.0)
        ga, gn = O.score_neg_bwd(model, a, n64, W.astype(np.float64), C, chunk, N, gamma)
        gx, gr = O.pos_side_bwd(model, neg_head, x64, r64, ga, 1.0)
        tag = "%s neg_head=%d" % (model, neg_head)
        _close(s.detach().cpu(), O.score_neg(model, a, n64, C, chunk, N, gamma), 1e-4, 1e-4, tag + " score")
        _close(nt.grad.cpu(), gn, 3e-4, grad_tol(gn), tag + " g_neg")
        _close(xt.grad.cpu(), gx, 3e-4, grad_tol(gx), tag + " g_pos_side")
        _close(rt.grad.cpu(), gr, 3e-4, grad_tol(gr), tag + " g_rel")


def test_offsets_beyond_4_gib():
    """2 800 000 x 400 floats: the rows of the table's last thousand sit 4.48e9 bytes behind its base, so `row * D * 4` does not fit
    32 bits - both products (GN reads its own rows there, GA the gathered ones), tail-corrupted step, N = 24: 48 gathered rows.
    The table is allocated uninitialised; only its last thousand rows are written."""
    n_big, tail_rows, D, n_rel = 2_800_000, 1000, 400, 20
    assert (n_big - tail_rows) * D * 4 > 2 ** 32
    big = torch.empty(n_big, D, dtype=torch.float32, device=DEV)
    tables = (big, torch.zeros(n_big, dtype=torch.float32, device=DEV), torch.empty(n_rel, D, dtype=torch.float32, device=DEV),
              torch.zeros(n_rel, dtype=torch.float32, device=DEV))
    _step_vs_oracle("TransE_l2", D, False, 32, 16, 24, n_ent=tail_rows, n_rel=n_rel, id_offset=n_big - tail_rows, tables=tables, steps=(1,))
    del big, tables
    torch.cuda.empty_cache()
