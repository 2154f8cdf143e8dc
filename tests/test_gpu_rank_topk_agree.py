"""Full-table ranking (kge_rank_eval) and top-K selection (kge_topk_select) score a (query row, candidate) pair through the same
128 x 128 x 32 MFMA main loop (csrc/kge_tile_gemm.hpp), so for the raw-product models their answers agree exactly: for every row i

    min(rank_i - 1, K) == #{k : topk_score[i, k] >= pos_score_i}

with rank_i the unfiltered rank, pos_score_i what kge_rank_eval itself compared against (pos_score_out) and the top K = 128
(KGE_TOPK_MAX) scores over the same candidate list.  DistMult and ComplEx; TransE_l2 is left out on purpose: its selected scores
are recomputed in the difference form by topk_l2_fix_kernel.

Shapes, the smallest at which the loop can still go wrong: 130 query rows (two row blocks, the second nearly empty), 300 candidates
(three column tiles, the last partial) through an id list into a larger table, d_e = 4 (a single short stage; top-K takes its VALU
tile below d_e = 32, so this width pins the two FORMS against each other), 36 (a tail stage after a full one), 64 (exactly two full
stages); both corruption sides."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, N_CAND, N_ENT, N_REL, K = 130, 300, 340, 5, 128
GAMMA, EMB_INIT = 12.0, 1.0


def _inputs(d_e):
    rng = np.random.default_rng(20261018 + d_e)
    ent = rng.uniform(-1.0, 1.0, (N_ENT, d_e)).astype(np.float32)
    rel = rng.uniform(-1.0, 1.0, (N_REL, d_e)).astype(np.float32)
    h = rng.integers(0, N_ENT, ROWS).astype(np.int64)
    r = rng.integers(0, N_REL, ROWS).astype(np.int64)
    t = rng.integers(0, N_ENT, ROWS).astype(np.int64)
    cand = rng.permutation(N_ENT)[:N_CAND].astype(np.int64)
    return ent, rel, h, r, t, cand


def _scores64(model, ent, rel, h, r, t, cand, side):
    """float64: [ROWS, N_CAND] candidate scores, [ROWS] positive scores, and the sums of the absolute terms of both (what an fp32
    evaluation's rounding error scales with); side 1: the head is replaced"""
    e, q = ent.astype(np.float64), rel.astype(np.float64)
    H, R, T, C = e[h], q[r], e[t], e[cand]
    if model == "DistMult":
        a, own = (T if side else H) * R, (H if side else T)
        return a @ C.T, (a * own).sum(1), np.abs(a) @ np.abs(C).T, np.abs(a * own).sum(1)
    d = ent.shape[1] // 2
    hr, hi, rr, ri, tr, ti = H[:, :d], H[:, d:], R[:, :d], R[:, d:], T[:, :d], T[:, d:]
    if side:        # coefficients of (c_re, c_im) with the candidate as head
        a = np.concatenate([rr * tr + ri * ti, rr * ti - ri * tr], 1)
        am = np.abs(np.concatenate([rr * tr, rr * ti], 1)) + np.abs(np.concatenate([ri * ti, ri * tr], 1))
    else:
        a = np.concatenate([hr * rr - hi * ri, hi * rr + hr * ri], 1)
        am = np.abs(np.concatenate([hr * rr, hi * rr], 1)) + np.abs(np.concatenate([hi * ri, hr * ri], 1))
    own = H if side else T
    return a @ C.T, (a * own).sum(1), am @ np.abs(C).T, (am * np.abs(own)).sum(1)


def _ranks(model, side, ent, rel, h, r, t, cand):
    from dglke_amd import _lib
    L = _lib.lib()
    d_e = ent.shape[1]
    ranks = torch.zeros(ROWS, dtype=torch.int32, device=DEV)
    pos = torch.zeros(ROWS, dtype=torch.float32, device=DEV)
    ws = torch.empty(L.kge_rank_workspace_bytes(ROWS, N_CAND, d_e), dtype=torch.uint8, device=DEV)
    _lib.check(L.kge_rank_eval(_lib.MODEL_IDS[model], side, _lib.ptr(ent), N_ENT, _lib.ptr(rel), N_REL, _lib.ptr(h), _lib.ptr(r),
                               _lib.ptr(t), ROWS, d_e, d_e, GAMMA, EMB_INIT, _lib.ptr(cand), N_CAND, None, None, ROWS,
                               _lib.ptr(ranks), _lib.ptr(pos), _lib.ptr(ws), ws.numel(), 0, _lib.stream_ptr()))
    return ranks.cpu().numpy().astype(np.int64), pos.cpu().numpy()


def _topk(model, side, ent, rel, h, r, t, cand):
    from dglke_amd import _lib
    L = _lib.lib()
    d_e = ent.shape[1]
    res_s = torch.zeros(ROWS, K, dtype=torch.float32, device=DEV)
    res_o = torch.full((ROWS, K), -1, dtype=torch.int64, device=DEV)
    base = torch.zeros(ROWS, dtype=torch.int64, device=DEV)
    ws = torch.empty(L.kge_topk_workspace_bytes(ROWS, N_CAND, d_e, K), dtype=torch.uint8, device=DEV)
    _lib.check(L.kge_topk_select(_lib.MODEL_IDS[model], side, _lib.ptr(ent), N_ENT, _lib.ptr(rel), N_REL, _lib.ptr(h), _lib.ptr(r),
                                 _lib.ptr(t), ROWS, d_e, d_e, GAMMA, EMB_INIT, _lib.ptr(cand), N_CAND, _lib.ptr(base), 1, 1, K,
                                 _lib.ptr(res_s), _lib.ptr(res_o), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return res_s.cpu().numpy(), res_o.cpu().numpy()


@pytest.mark.parametrize("d_e", [4, 36, 64])
@pytest.mark.parametrize("model", ["DistMult", "ComplEx"])
def test_rank_minus_one_is_the_count_of_topk_scores_at_or_above_the_positive(model, d_e):
    host = _inputs(d_e)
    dev = [torch.from_numpy(x).to(DEV) for x in host]
    for side in (0, 1):
        rank, pos = _ranks(model, side, *dev)
        top_s, top_o = _topk(model, side, *dev)
        assert np.all(top_o >= 0)                                      # 300 candidates: every list is full
        want = np.minimum(rank - 1, K)
        got = (top_s >= pos[:, None]).sum(1)
        inside = (rank - 1 > 0) & (rank - 1 < K)
        # the device ranks are the ranks of these tables: inside the float64 bounds whose slack is the fp32 rounding of a d_e-term
        # sum of products of up to three factors, (d_e + 8) u sum |terms| on either side of a comparison
        S, p, Sm, pm = _scores64(model, *host, side)
        tol = (d_e + 8) * 2.0 ** -24 * (Sm + pm[:, None])
        lo, hi = 1 + (S > p[:, None] + tol).sum(1), 1 + (S >= p[:, None] - tol).sum(1)
        print(model, d_e, "side", side, "rows with 0 < rank - 1 < K:", int(inside.sum()), "of", ROWS, "| rows that differ:",
              int((want != got).sum()), "| rows outside the float64 bounds:", int(((rank < lo) | (rank > hi)).sum()),
              "| hi - lo max", int((hi - lo).max()))
        assert inside.sum() * 4 >= ROWS                                # not vacuous: a quarter of the rows is decided inside the list
        assert np.all((lo <= rank) & (rank <= hi))
        assert np.array_equal(want, got), (side, np.nonzero(want != got)[0][:8], want[:8], got[:8])
