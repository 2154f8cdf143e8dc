"""CPU guard of the QuatE tests (tests/quate_cases.py): the float64 statement against torch.autograd on the same formulas and its
identities, the cases of the tables do what they are listed for, the integer-grid ranking inputs are exact in float32 and hold the
ties the device tests need, and the refusals - widths and flag combinations on the command lines, dimensions and the closed
entries in the C ABI (no GPU: argument errors are reported before any launch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import quate_cases as Q
from oracle import kge_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib
    return _lib


# --------------------------------------------------------------------------------------------------------------------------
# the statement
# --------------------------------------------------------------------------------------------------------------------------
def _t_quarters(x):
    q = x.shape[-1] // 4
    return x[..., :q], x[..., q:2 * q], x[..., 2 * q:3 * q], x[..., 3 * q:]


def _t_hamilton(x, y):
    a, b, c, d = _t_quarters(x)
    p, q, u, v = _t_quarters(y)
    return torch.cat([a * p - b * q - c * u - d * v, a * q + b * p + c * v - d * u, a * u - b * v + c * p + d * q,
                      a * v + b * u - c * q + d * p], -1)


def _t_unit(r):
    a, b, c, d = _t_quarters(r)
    n = torch.sqrt(a * a + b * b + c * c + d * d)
    return torch.cat([p / n for p in (a, b, c, d)], -1)


def _t_pos_side(neg_head, x, r):
    ru = _t_unit(r)
    if neg_head:
        a, b, c, d = _t_quarters(ru)
        ru = torch.cat([a, -b, -c, -d], -1)
    return _t_hamilton(x, ru)


@pytest.mark.parametrize("d_e", [4, 36, 32])
@pytest.mark.parametrize("neg_head", [False, True])
def test_statement_gradients_equal_autograd(d_e, neg_head):
    """score, both pos-side vectors and the full adjoint (through the normalisation) in float64, to 1e-10"""
    C_, chunk, N = 2, 5, 7
    rng = np.random.RandomState(d_e + neg_head)
    inp = dict(x=rng.uniform(-1, 1, (C_ * chunk, d_e)), y=rng.uniform(-1, 1, (C_ * chunk, d_e)), r=rng.uniform(-1, 1, (C_ * chunk, d_e)),
               nb=rng.uniform(-1, 1, (C_ * N, d_e)), W=rng.uniform(-1, 1, (C_, chunk, N)), dp=rng.uniform(-1, 1, C_ * chunk))
    ref = Q.op_reference(inp, C_, chunk, N, neg_head)
    x, y, r, nb = (torch.tensor(inp[k], dtype=torch.float64, requires_grad=True) for k in ("x", "y", "r", "nb"))
    h, t = (y, x) if neg_head else (x, y)
    pos = (_t_hamilton(h, _t_unit(r)) * t).sum(-1)
    assert np.abs(pos.detach().numpy() - ref["pos"]).max() < 1e-10
    (pos * torch.tensor(inp["dp"])).sum().backward()
    for got, want in ((h.grad, ref["gh"]), (r.grad, ref["grp"]), (t.grad, ref["gt"])):
        assert np.abs(got.numpy() - want).max() < 1e-10
    for v in (x, y, r):
        v.grad = None
    a = _t_pos_side(neg_head, x, r)
    s = torch.einsum("cik,cjk->cij", a.reshape(C_, chunk, d_e), nb.reshape(C_, N, d_e))
    assert np.abs(s.detach().numpy() - ref["score"]).max() < 1e-10
    (s * torch.tensor(inp["W"])).sum().backward()
    for got, want in ((x.grad, ref["gx"]), (r.grad, ref["gr"]), (nb.grad, ref["gn"])):
        assert np.abs(got.numpy() - want).max() < 1e-10


def test_statement_identities():
    rng = np.random.RandomState(5)
    h, r, t = (rng.uniform(-1, 1, (9, 24)) for _ in range(3))
    ru = Q.unit(r)
    # <h (x) r, t> == <h, t (x) conj(r)>: the two pos-side vectors give one score
    s = Q.score(h, r, t)
    assert np.abs((h * Q.hamilton(t, Q.conj(ru))).sum(-1) - s).max() < 1e-12
    assert np.abs((Q.pos_side(True, t, r) * h).sum(-1) - s).max() < 1e-12 and np.abs((Q.pos_side(False, h, r) * t).sum(-1) - s).max() < 1e-12
    # the relation-ranking query: <conj(h) (x) t, r^>
    assert np.abs((Q.rel_query(h, t) * ru).sum(-1) - s).max() < 1e-12
    # unit quaternions, and a positive scale per relation quaternion changes no score
    assert np.abs(Q.norms(ru) - 1).max() < 1e-12
    scale = rng.uniform(0.1, 10.0, (9, 6))
    assert np.abs(Q.score(h, r * np.tile(scale, (1, 4)), t) - s).max() < 1e-12


def test_statement_reduces_to_complex_on_the_first_two_quarters():
    """c = d = 0 everywhere and unit-modulus relations: the score is the oracle's ComplEx score on the [a | b] halves"""
    rng = np.random.RandomState(6)
    B, q = 11, 5
    z = np.zeros((B, 2 * q))
    h2, t2 = rng.uniform(-1, 1, (B, 2 * q)), rng.uniform(-1, 1, (B, 2 * q))
    ph = rng.uniform(-np.pi, np.pi, (B, q))
    r2 = np.concatenate([np.cos(ph), np.sin(ph)], -1)
    got = Q.score(np.concatenate([h2, z], -1), np.concatenate([r2, z], -1), np.concatenate([t2, z], -1))
    assert np.abs(got - O.score_pos("ComplEx", h2, r2, t2, 0.0)).max() < 1e-12


def test_zero_relation_quaternion_gives_no_score_and_no_gradient():
    rng = np.random.RandomState(7)
    h, r, t = (rng.uniform(-1, 1, (3, 8)) for _ in range(3))
    r[:, ::2] = 0.0                                       # column 0 of every quarter: quaternion 0 is all zero
    hz, tz = h.copy(), t.copy()
    hz[:, ::2], tz[:, ::2] = 0.0, 0.0                     # ... so column 0 of h and t must not matter
    assert np.array_equal(Q.score(h, r, t), Q.score(hz, r, tz))
    dp = np.ones(3)
    gh, gr, gt = Q.score_bwd(h, r, t, dp)
    gx, gr2 = Q.pos_side_bwd(False, h, r, rng.uniform(-1, 1, (3, 8)))
    for g in (gh, gr, gt, gx, gr2):
        assert np.isfinite(g).all() and not g[:, ::2].any()
    inp = Q.op_inputs(36, 2, 8, 24, False)
    assert not inp["r"][0, ::9].any() and inp["r"][1, ::9].all(), "the per-op inputs plant one all-zero relation quaternion"
    ref = Q.op_reference(inp, 2, 8, 24, False)
    assert all(np.isfinite(v).all() for v in ref.values()) and not ref["gr"][0, ::9].any() and not ref["gx"][0, ::9].any()


# --------------------------------------------------------------------------------------------------------------------------
# the case tables
# --------------------------------------------------------------------------------------------------------------------------
def test_op_widths_reach_the_instances_they_are_listed_for():
    assert [Q.vector_packs(d) for d in Q.OP_WIDTHS] == [False, False, True, True, True]
    assert (1040 // 4) // 4 > 64, "the widest case needs a second round of 64 packs"
    assert all(Q.neg_route(d, 0) == "gemm" for d in Q.OP_WIDTHS)          # every width is a multiple of 4: matrix cores
    assert [Q.neg_route(d, Q.FORCE_PAIRWISE) for d in Q.OP_WIDTHS] == ["pair32", "pair32", "bcast", "bcast", "bcast"]
    assert any(N % 16 and chunk % 16 == 0 for _, chunk, N in Q.OP_SHAPES) and any(C_ > 1 for C_, _, _ in Q.OP_SHAPES)


def test_step_cases_do_what_they_are_listed_for():
    from dglke_amd import plan
    ids = [c["id"] for c in Q.STEP_CASES]
    assert len(set(ids)) == len(ids)
    assert {(c["genre"], c["adv"], c["pairwise"]) for c in Q.STEP_CASES} >= {("Logsigmoid", True, False), ("Hinge", False, True),
                                                                            ("BCE", False, False), ("Softmax", False, False)}
    assert {c["reg_norm"] for c in Q.STEP_CASES if c["reg_coef"] > 0} == {2, 3}
    assert any(c["neg_deg"] for c in Q.STEP_CASES) and any(c["impts"] for c in Q.STEP_CASES)
    for d_e in Q.STEP_WIDTHS:
        ent, rel = Q.step_tables(d_e)
        for c in Q.STEP_CASES:
            bts = Q.step_batches(c)
            assert [bt["neg_head"] for bt in bts] == [False, True], "tail then head corruption"
            for bt in bts:
                p = plan.build_plan(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], bt["w"])
                # owner-computes lists longer than one: an entity with several positive ends and negative slots, a relation with several edges
                assert np.diff(p["ue_pos_ptr"]).max() > 1 and np.diff(p["ue_neg_ptr"]).max() > 1 and np.diff(p["ur_ptr"]).max() > 1
                out = Q.forward_backward(c, ent.astype(np.float64), rel.astype(np.float64), bt)
                assert np.isfinite(out["log"][2]) and out["log"][2] > 0
                for k in ("g_pos_ent", "g_neg", "g_rel"):
                    assert np.isfinite(out[k]).all() and np.abs(out[k]).max() > 1e-4, (c["id"], k)
                if c["neg_deg"]:
                    n = out["neg_score"].reshape(c["B"], -1)
                    assert n.shape[1] == c["chunk"] + c["N"] and np.all(n[np.arange(c["B"]), np.arange(c["B"]) % c["chunk"]] == 0.0)
                if c["reg_coef"] > 0:
                    plain = Q.forward_backward(dict(c, reg_coef=0.0), ent.astype(np.float64), rel.astype(np.float64), bt)
                    share = np.abs(out["g_rel"] - plain["g_rel"]).max() / np.abs(out["g_rel"]).max()
                    assert share >= 0.01, "%s: the regulariser does not show in the gradients (%.3g)" % (c["id"], share)
                if c["genre"] == "Hinge":
                    act = c["margin"] - (out["pos_score"][:, None] - out["neg_score"].reshape(c["B"], -1))
                    assert 0.2 < (act > 0).mean() < 0.98, "the hinge is active for some pairs and not for others"


def test_planted_known_pairs_take_their_columns_out():
    c = Q.STEP_CASES[0]
    ent, rel = Q.step_tables(32)
    for bt in Q.step_batches(c):
        K, known = Q.planted_known(bt, c["chunk"], c["N"])
        assert known[0, 3] and known[c["chunk"], c["N"] - 1] and 2 <= known.sum() < known.size // 4
        out = Q.forward_backward(c, ent.astype(np.float64), rel.astype(np.float64), bt, known)
        plain = Q.forward_backward(c, ent.astype(np.float64), rel.astype(np.float64), bt)
        assert np.all(out["neg_score"].reshape(known.shape)[known] == Q.KNOWN_SCORE)
        assert np.abs(out["g_neg"] - plain["g_neg"]).max() > 1e-6, "the planted pairs carried gradient"


# --------------------------------------------------------------------------------------------------------------------------
# the integer-grid ranking inputs
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d_e", Q.TIE_CASES, ids=["n%d-D%d" % c for c in Q.TIE_CASES])
def test_grid_inputs_are_exact_in_float32_and_hold_ties(n, d_e, wide_e=None):
    c = Q.tie_inputs(n, d_e) if wide_e is None else Q.tie_inputs(n, d_e, wide_e)      # (the several-tile size)
    assert c.ent.min() == -3 and c.ent.max() == 3 and np.array_equal(c.ent, np.rint(c.ent))
    nr = Q.norms(c.rel.astype(np.float64))
    assert np.array_equal(np.log2(nr), np.rint(np.log2(nr))), "every relation norm is a power of two"
    ru = Q.unit(c.rel)
    assert ru.dtype == np.float32 and set(np.unique(np.abs(ru)).tolist()) <= {0.0, 0.5, 1.0}, "float32 normalisation is exact"
    assert np.array_equal(ru.astype(np.float64), Q.unit(c.rel.astype(np.float64)))
    E = len(c.h)
    tied_rows, filt_ties = 0, 0
    for neg_head in (False, True):
        p, S = Q.tie_scores(c, c.h, c.r, c.t, neg_head)
        assert np.array_equal(2 * S, np.rint(2 * S)) and np.abs(S).max() < 2 ** 20, "scores are small multiples of 1/2"
        p32, _ = Q.tie_scores(c, c.h, c.r, c.t, neg_head, np.float32)
        assert p32.dtype == np.float32 and np.array_equal(p32.astype(np.float64), p)
        for s32 in Q.f32_scores_three_orders(c, c.h, c.r, c.t, neg_head):
            assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), S), "a float32 summation order is not exact"
        own = c.h if neg_head else c.t
        assert np.array_equal(S[np.arange(E), own], p)
        m = S == p[:, None]
        m[np.arange(E), own] = False
        tied_rows = max(tied_rows, int(m.any(1).sum()))
        assert m.any(1).sum() * 10 >= E, "fewer than one row in ten has a candidate that ties its positive (neg_head=%d)" % neg_head
        lists = Q.filter_lists(c, neg_head)
        raw, filt = Q.ranks_of(p, S), Q.ranks_of(p, S, lists)
        assert np.any(raw != Q.ranks_of(p, S, strict=True) + 1), "`>=` and `>` must differ by more than the own column"
        for i in range(E):
            ids = lists[1][lists[0][i, 0]:lists[0][i, 1]]
            assert own[i] in ids
            filt_ties += int(((S[i, ids] == p[i]) & (ids != own[i])).sum())
        assert np.all(filt <= raw - 1)
    assert filt_ties >= 1, "no tie on the filtered side"
    p, S = Q.rel_tie_scores(c, c.h, c.r, c.t)
    assert np.array_equal(2 * S, np.rint(2 * S))
    S32 = (Q.rel_query(c.ent[c.h], c.ent[c.t]) @ Q.unit(c.rel).T)
    assert S32.dtype == np.float32 and np.array_equal(S32.astype(np.float64), S)
    pt, _ = Q.tie_scores(c, c.h, c.r, c.t, False)
    assert np.array_equal(p, pt), "the relation-ranking form gives the positive score of the entity form"
    m = S == p[:, None]
    m[np.arange(E), c.r] = False
    assert m.any(1).sum() * 10 >= E, "fewer than one row in ten has a relation that ties the true one"
    raw, filt = Q.ranks_of(p, S, Q.relation_lists(c, False)), Q.ranks_of(p, S, Q.relation_lists(c, True))
    assert np.all(filt <= raw) and np.any(filt < raw)


def test_interface_reference_is_the_statement_on_every_triple():
    ent, rel = Q.interface_tables()
    S = Q.all_scores(ent, rel)
    assert S.shape == (Q.IF_ENT, Q.IF_REL, Q.IF_ENT)
    assert np.abs(S[3, 2, 5] - Q.score(ent[3:4].astype(np.float64), rel[2:3].astype(np.float64), ent[5:6].astype(np.float64))[0]) < 1e-12


# --------------------------------------------------------------------------------------------------------------------------
# the refusals
# --------------------------------------------------------------------------------------------------------------------------
def test_c_abi_takes_model_8_and_refuses_bad_dimensions_without_a_gpu():
    lib = _lib()
    h = lib.lib()
    assert lib.MODEL_IDS["QuatE"] == Q.MODEL_ID == 8 and lib.MODEL_IDS["TransR"] == 7 and h.kge_abi_version() == 8
    one = 1                                                       # (a non-NULL pointer that is never dereferenced)
    rc = h.kge_score_pos(8, one, one, one, 2, 8, 4, 1.0, 1.0, one, None)           # d_r != d_e
    assert rc == -1 and b"QuatE" in h.kge_last_error()
    rc = h.kge_score_pos(8, one, one, one, 2, 6, 6, 1.0, 1.0, one, None)           # no multiple of 4
    assert rc == -1 and b"QuatE" in h.kge_last_error()
    rc = h.kge_score_pos(8, one, one, one, 2, 0, 0, 1.0, 1.0, one, None)
    assert rc == -1 and b"QuatE" in h.kge_last_error()
    rc = h.kge_score_pos(8, None, None, None, 2, 8, 8, 1.0, 1.0, None, None)       # accepted: the next check speaks
    assert rc == -1 and b"QuatE" not in h.kge_last_error() and b"kge_score_pos" in h.kge_last_error()
    rc = h.kge_score_pos(9, one, one, one, 2, 4, 4, 1.0, 1.0, one, None)
    assert rc == -1 and b"unknown model" in h.kge_last_error()
    # relation ranking: the size function answers for the ids up to TransR; a QuatE workspace is the DistMult layout + the
    # normalised relation table, and a workspace one byte short of that is refused before any launch
    assert h.kge_rank_rel_workspace_bytes(8, 4, 10, 8, 8) == 0
    need = lib.rank_rel_workspace_bytes(8, 4, 10, 8, 8)
    assert need == h.kge_rank_rel_workspace_bytes(2, 4, 10, 8, 8) + 512 and lib.rank_rel_workspace_bytes(8, 4, 10, 6, 6) == 0
    assert lib.rank_rel_workspace_bytes(2, 4, 10, 8, 8) == h.kge_rank_rel_workspace_bytes(2, 4, 10, 8, 8)

    def rel_eval(ws_bytes):
        return h.kge_rank_rel_eval(8, one, 5, one, 10, None, one, one, one, 4, 8, 8, 0.0, 1.0, one, one, 4, one, None, one, ws_bytes, 0, None)
    assert rel_eval(need - 1) == -2 and b"workspace too small" in h.kge_last_error()
    assert h.kge_score_neg_workspace_bytes(8, 2, 8, 24, 32) == h.kge_score_neg_workspace_bytes(3, 2, 8, 24, 32)
    # top-K: the id is known, TransR still is not
    rc = h.kge_topk_select(8, 0, one, 5, one, 2, one, one, one, 1, 8, 4, 0.0, 1.0, None, 5, one, 1, 1, 3, one, one, one, 1 << 20, None)
    assert rc == -1 and b"do not fit model 8" in h.kge_last_error()
    rc = h.kge_topk_select(7, 0, one, 5, one, 2, one, one, one, 1, 8, 8, 0.0, 1.0, None, 5, one, 1, 1, 3, one, one, one, 1 << 20, None)
    assert rc == -1 and b"unknown score function 7" in h.kge_last_error()


def test_closed_entries_refuse_quate_before_any_launch():
    lib = _lib()
    h = lib.lib()
    one = 1
    hp, tb, b, sh, em = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch(), lib.KgeShards(), lib.KgeEmit()
    hp.model, hp.d_e, hp.d_r = 8, 8, 8
    b.B, b.C, b.chunk, b.N = 4, 1, 4, 3
    assert h.kge_step_sharded(C.byref(hp), C.byref(sh), C.byref(b), None, one, 1 << 20, None) == -1
    assert b"QuatE" in h.kge_last_error() and b"kge_step_sharded" in h.kge_last_error()
    assert h.kge_step_grads(C.byref(hp), C.byref(tb), C.byref(b), None, C.byref(em), one, 1 << 20, None) == -1
    assert b"QuatE" in h.kge_last_error() and b"kge_step_grads" in h.kge_last_error()
    pipe = C.c_void_p()
    assert h.kge_pipe_create(C.byref(pipe)) == 0
    assert h.kge_step_async(pipe, C.byref(hp), C.byref(tb), C.byref(b), None, None, one, 1 << 20, None) == -1
    assert b"QuatE" in h.kge_last_error() and b"kge_step_async" in h.kge_last_error()
    h.kge_pipe_destroy(pipe)
    rc = h.kge_rank_eval_split(8, 0, one, 5, one, 5, one, 2, None, one, one, one, 1, 8, 8, 0.0, 1.0, None, 0, None, None, 1, one, None,
                               one, 1 << 20, 0, None)
    assert rc == -1 and b"QuatE" in h.kge_last_error() and b"kge_rank_eval_split" in h.kge_last_error()
    # the strict step takes the id: the next check speaks (null tables)
    assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20, None) == -1
    assert b"QuatE" not in h.kge_last_error() and b"unknown model" not in h.kge_last_error()


def test_command_lines_refuse_widths_and_flag_combinations(tmp_path):
    _lib()
    from dglke_amd import eval_cli, train as T
    from dglke_amd._lib import KgeError
    base = ["--model_name", "QuatE", "--dataset", "toy", "--data_path", str(tmp_path / "none"), "--save_path", str(tmp_path / "ckpts"),
            "--gpu", "0"]
    assert T.ArgParser().parse_args(base).model_name == "QuatE"
    for extra, word in ((["--hidden_dim", "30"], "entity width"), (["--hidden_dim", "32", "-de"], "relation width"),
                        (["--hidden_dim", "32", "-dr"], "relation width"), (["--hidden_dim", "15", "-de", "-dr"], "entity width"),
                        (["--hidden_dim", "32", "--async_update", "--async_update_pipeline"], "one-step-stale pipeline"),
                        (["--hidden_dim", "32", "--async_update", "--async_update_rel"], "one-step-stale pipeline")):
        with pytest.raises(KgeError, match="QuatE.*" + word):
            T.main(base + extra)
    with pytest.raises(KgeError, match="QuatE is not available on more than one GPU"):
        T.main(base[:-1] + ["0", "0", "--hidden_dim", "32"])
    assert not os.path.exists(str(tmp_path / "ckpts")), "refused before anything is loaded or created"
    ev = ["--model_name", "QuatE", "--dataset", "toy", "--data_path", str(tmp_path / "none"), "--model_path", str(tmp_path), "--gpu", "0"]
    with pytest.raises(KgeError, match="QuatE.*entity width"):
        eval_cli.main(ev + ["--hidden_dim", "30"])
    with pytest.raises(KgeError, match="QuatE.*relation width"):
        eval_cli.main(ev + ["--hidden_dim", "32", "-de"])
    with pytest.raises(KgeError, match="QuatE is not available on sharded tables"):
        eval_cli.main(ev[:-1] + ["0", "0", "--hidden_dim", "32"])
    with pytest.raises(SystemExit):
        T.ArgParser().parse_args(["--model_name", "Quate"])


def test_python_layers_check_the_widths_before_touching_a_device():
    lib = _lib()
    from dglke_amd import ke_model, score_fun
    assert score_fun.QuatEScore.model_name == "QuatE" and lib.model_id("QuatE") == 8
    assert issubclass(ke_model.QuatEModel, ke_model.KGEModel)
    from dglke_amd.train import check_model_widths
    check_model_widths("QuatE", 32, False, False)
    check_model_widths("QuatE", 18, True, True)
    check_model_widths("DistMult", 30, True, False)
