"""dglke_amd.infer on the GPU (csrc/kge_topk.hip): every top-K against an fp64 statement of the reference's score forms
(models/pytorch/score_fun.py `infer` methods, tensor_models.py:59-100 similarities), written here with torch float64.

Acceptance rule for a top-K (it tolerates fp32 ties): with s the exact scores and tol = 1e-4 * max(1, |s|), the returned
combinations are distinct, each has s >= s_(K) - tol, each reported score equals s within tol, the order is non-increasing
within tol, and wherever s_(K) and s_(K+1) differ by more than tol the returned set is the exact set."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))

pytestmark = pytest.mark.gpu

MODELS = ["TransE_l1", "TransE_l2", "DistMult", "ComplEx", "RotatE", "SimplE", "RESCAL"]
DEV = "cuda:0"


def _tables(model, n_ent, n_rel, hidden, seed):
    rng = np.random.RandomState(seed)
    d_e = hidden * (2 if model in ("ComplEx", "RotatE", "SimplE") else 1)
    d_r = hidden * hidden if model == "RESCAL" else hidden * (2 if model in ("ComplEx", "SimplE") else 1)
    ent = rng.uniform(-1, 1, (n_ent, d_e)).astype(np.float32)
    rel = rng.uniform(-1, 1, (n_rel, d_r)).astype(np.float32)
    if model == "RESCAL":
        rel *= 1.0 / math.sqrt(hidden)
    return ent, rel


def _save(tmp, model, ent, rel, hidden, gamma):
    np.save(os.path.join(tmp, "toy_%s_entity.npy" % model), ent)
    np.save(os.path.join(tmp, "toy_%s_relation.npy" % model), rel)
    return {"model_name": model, "dataset": "toy", "hidden_dim": hidden, "gamma": gamma,
            "double_ent": model in ("ComplEx", "RotatE", "SimplE"), "double_rel": model in ("ComplEx", "SimplE")}


def exact_scores(model, ent, rel, h, r, t, gamma, emb_init):
    """[H, R, T] float64 scores of every combination (the reference's `infer` forms)"""
    E = th.as_tensor(ent, dtype=th.float64, device=DEV)
    Rl = th.as_tensor(rel, dtype=th.float64, device=DEV)
    hh, rr, tt = E[th.as_tensor(h, device=DEV)], Rl[th.as_tensor(r, device=DEV)], E[th.as_tensor(t, device=DEV)]
    H, R, T = len(h), len(r), len(t)
    out = th.empty(H, R, T, dtype=th.float64, device=DEV)
    for i in range(H):
        a = hh[i:i + 1]
        if model in ("TransE_l1", "TransE_l2"):
            x = (a + rr).unsqueeze(1) - tt.unsqueeze(0)
            out[i] = gamma - x.norm(p=1 if model == "TransE_l1" else 2, dim=-1)
        elif model == "DistMult":
            out[i] = (a * rr) @ tt.T
        elif model == "ComplEx":
            d = hh.shape[1] // 2
            hre, him, rre, rim = a[:, :d], a[:, d:], rr[:, :d], rr[:, d:]
            qre, qim = hre * rre - him * rim, hre * rim + him * rre
            out[i] = qre @ tt[:, :d].T + qim @ tt[:, d:].T
        elif model == "RotatE":
            d = hh.shape[1] // 2
            ph = rr / (emb_init / math.pi)
            c, s = th.cos(ph), th.sin(ph)
            qre, qim = a[:, :d] * c - a[:, d:] * s, a[:, :d] * s + a[:, d:] * c
            dre = qre.unsqueeze(1) - tt[:, :d].unsqueeze(0)
            dim = qim.unsqueeze(1) - tt[:, d:].unsqueeze(0)
            out[i] = gamma - th.sqrt(dre * dre + dim * dim).sum(-1)
        elif model == "SimplE":
            d = hh.shape[1] // 2
            q = th.cat([a[:, d:] * rr[:, d:], a[:, :d] * rr[:, :d]], dim=1)      # . [t_i | t_j]
            out[i] = 0.5 * (q @ tt.T)
        else:
            D = hh.shape[1]
            M = rr.view(R, D, D)
            out[i] = th.einsum("rbc,tc,b->rt", M, tt, a[0])
    return out


def exact_sim(sim, emb, left, right):
    E = th.as_tensor(emb, dtype=th.float64, device=DEV)
    x, y = E[th.as_tensor(left, device=DEV)], E[th.as_tensor(right, device=DEV)]
    dot = x @ y.T
    if sim == "dot":
        return dot
    if sim == "cosine":
        return dot / (x.norm(dim=1)[:, None] * y.norm(dim=1)[None, :])
    if sim == "ext_jaccard":
        nx, ny = (x * x).sum(1)[:, None], (y * y).sum(1)[None, :]
        return dot / (nx + ny - dot)
    p = 2 if sim == "l2" else 1
    return -th.cdist(x, y, p=p)


def accept(exact, ret_keys, ret_scores, K, key_of):
    """exact: dict combination-key -> list of exact scores (one per position); ret_keys: returned combination keys in order"""
    flat = sorted((s for v in exact.values() for s in v), reverse=True)
    m = min(K, len(flat))
    assert len(ret_keys) == m == len(ret_scores)
    if m == 0:
        return
    sK = flat[m - 1]
    tol_k = 1e-4 * max(1.0, abs(sK))
    seen = {}
    for key, v in zip(ret_keys, ret_scores):
        seen[key] = seen.get(key, 0) + 1
        assert seen[key] <= len(exact[key]), "combination %r returned more often than it occurs" % (key,)
        s = exact[key][0]
        tol = 1e-4 * max(1.0, abs(s))
        assert s >= sK - tol_k - tol, (key, s, sK)
        assert abs(v - s) <= tol, (key, v, s)
    for a, b in zip(ret_scores[:-1], ret_scores[1:]):
        assert b <= a + 1e-4 * max(1.0, abs(a))
    if m < len(flat) and flat[m - 1] - flat[m] > tol_k:
        want = {}
        for key, v in exact.items():
            for s in v:
                if s >= flat[m - 1]:
                    want[key] = want.get(key, 0) + 1
        assert seen == want


def _exact_dict(S, h, r, t, groups):
    """split [H, R, T] exact scores into the groups of an exec mode: list of dicts (h, r, t) -> [scores]"""
    S = S.cpu().numpy()
    out = []
    for sel in groups:
        d = {}
        for (i, j, k) in sel:
            d.setdefault((int(h[i]), int(r[j]), int(t[k])), []).append(float(S[i, j, k]))
        out.append(d)
    return out


def _groups(mode, H, R, T):
    import itertools
    if mode == "all":
        return [list(itertools.product(range(H), range(R), range(T)))]
    if mode == "batch_head":
        return [[(i, j, k) for j in range(R) for k in range(T)] for i in range(H)]
    if mode == "batch_rel":
        return [[(i, j, k) for i in range(H) for k in range(T)] for j in range(R)]
    return [[(i, j, k) for i in range(H) for j in range(R)] for k in range(T)]


def _check_result(res, exact_groups, K):
    assert len(res) == len(exact_groups)
    for (hl, rl, tl, sl), ex in zip(res, exact_groups):
        keys = list(zip(hl.tolist(), rl.tolist(), tl.tolist()))
        accept(ex, keys, [float(x) for x in sl], K, None)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("sfunc", ["none", "logsigmoid"])
def test_predict_modes_fp64(tmp_path, model, sfunc):
    from dglke_amd.infer import ScoreInfer
    # d_e 36 for every model but RESCAL (64): the MFMA tile for the matrix forms (a ragged last k stage at 36); TransE_l1 and
    # RotatE take the VALU tile whatever d is.  (d below 32 or not a multiple of 4 - the VALU tile for every form - is
    # covered by the reference goldens below and by the d 6 similarity cases.)
    hidden = 64 if model == "RESCAL" else (18 if model in ("ComplEx", "RotatE", "SimplE") else 36)
    ent, rel = _tables(model, 300, 5, hidden, 1)
    gamma = 12.0
    cfg = _save(str(tmp_path), model, ent, rel, hidden, gamma)
    m = ScoreInfer(0, cfg, str(tmp_path), sfunc)
    m.load_model()
    rng = np.random.RandomState(2)
    h = rng.randint(0, 300, 13)
    h[5] = h[2]                                          # a repeated id
    r = np.array([4, 0, 2])
    t = rng.permutation(300)[:290]
    g = gamma if sfunc == "logsigmoid" else 0.0
    S = exact_scores(model, ent, rel, h, r, t, g, (gamma + 2.0) / hidden)
    if sfunc == "logsigmoid":
        S = th.nn.functional.logsigmoid(S)
    for mode in ("all", "batch_head", "batch_rel", "batch_tail"):
        ex = _exact_dict(S, h, r, t, _groups(mode, len(h), len(r), len(t)))
        for K in (1, 10, 128):
            _check_result(m.topK(h, r, t, mode, K), ex, K)
    # triplet_wise (SimplE clamped to +-20 in this mode only)
    hw, rw, tw = h[:12], rng.randint(0, 5, 12), t[:12]
    Sw = th.stack([exact_scores(model, ent, rel, [a], [b], [c], g, (gamma + 2.0) / hidden)[0, 0, 0]
                   for a, b, c in zip(hw, rw, tw)])
    if model == "SimplE":
        Sw = Sw.clamp(-20, 20)
    if sfunc == "logsigmoid":
        Sw = th.nn.functional.logsigmoid(Sw)
    for K in (1, 5, 128):
        (hl, rl, tl, sl), = m.topK(hw, rw, tw, "triplet_wise", K)
        ex = {}
        for i, (a, b, c) in enumerate(zip(hw, rw, tw)):
            ex.setdefault((int(a), int(b), int(c)), []).append(float(Sw[i]))
        accept(ex, list(zip(hl.tolist(), rl.tolist(), tl.tolist())), [float(x) for x in sl], K, None)


@pytest.mark.parametrize("model", ["TransE_l2", "DistMult", "ComplEx", "SimplE", "TransE_l1", "RotatE"])
def test_predict_fb15k_shape(tmp_path, model):
    """1000 queries x 14 951 candidates x d 400 (the pairwise forms at 1000 x 3000): crosses tiles and segments"""
    from dglke_amd.infer import ScoreInfer
    n_ent = 14951
    hidden = 400 if model in ("TransE_l2", "DistMult", "TransE_l1") else 200
    ent, rel = _tables(model, n_ent, 2, hidden, 3)
    ent *= 0.1
    cfg = _save(str(tmp_path), model, ent, rel, hidden, 12.0)
    m = ScoreInfer(0, cfg, str(tmp_path), "none")
    m.load_model()
    rng = np.random.RandomState(4)
    h = rng.randint(0, n_ent, 1000)
    t = np.arange(n_ent) if model not in ("TransE_l1", "RotatE") else rng.randint(0, n_ent, 3000)
    S = exact_scores(model, ent, rel, h[:40], [1], t, 0.0, 14.0 / hidden)          # the first 40 groups against fp64
    ex = _exact_dict(S, h[:40], [1], t, _groups("batch_head", 40, 1, len(t)))
    for K in (1, 10, 128):
        res = m.topK(h, [1], t, "batch_head", K)
        _check_result(res[:40], ex, K)
        assert len(res) == 1000


@pytest.mark.parametrize("model", ["DistMult", "TransE_l1"])
def test_rising_scores_every_tile_survives(tmp_path, model):
    """candidates ordered so that scores rise with the index: every tile passes the threshold (queue merges each tile)"""
    from dglke_amd.infer import ScoreInfer
    ent, rel = _tables(model, 5000, 1, 32, 5)
    cfg = _save(str(tmp_path), model, ent, rel, 32, 12.0)
    m = ScoreInfer(0, cfg, str(tmp_path), "none")
    m.load_model()
    h = np.array([7, 11])
    S = exact_scores(model, ent, rel, h[:1], [0], np.arange(5000), 0.0, 14.0 / 32)[0, 0]
    t = th.argsort(S).cpu().numpy()                       # rising for the first query
    for K in (10, 128):
        res = m.topK(h, [0], t, "batch_head", K)
        Sx = exact_scores(model, ent, rel, h, [0], t, 0.0, 14.0 / 32)
        _check_result(res, _exact_dict(Sx, h, [0], t, _groups("batch_head", 2, 1, len(t))), K)


def test_all_over_row_batches_and_determinism(tmp_path):
    from dglke_amd.infer import ScoreInfer
    ent, rel = _tables("DistMult", 400, 4, 36, 6)
    cfg = _save(str(tmp_path), "DistMult", ent, rel, 36, 12.0)
    m = ScoreInfer(0, cfg, str(tmp_path), "none")
    m.load_model()
    h, r, t = np.arange(100), np.arange(4), np.arange(400)
    one = m.topK(h, r, t, "all", 128)
    m.max_rows = 128                                      # 400 rows -> four calls carrying the running result
    split = m.topK(h, r, t, "all", 128)
    again = m.topK(h, r, t, "all", 128)
    for a, b, c in zip(one[0], split[0], again[0]):
        assert np.array_equal(a, b) and np.array_equal(b, c)
    S = exact_scores("DistMult", ent, rel, h, r, t, 0.0, 1.0)
    _check_result(split, _exact_dict(S, h, r, t, _groups("all", 100, 4, 400)), 128)
    m.max_rows = 64                                       # batch_rel groups of 100 rows over two calls each
    br = m.topK(h, r, t, "batch_rel", 10)
    _check_result(br, _exact_dict(S, h, r, t, _groups("batch_rel", 100, 4, 400)), 10)


def test_ties_ordered_by_position(tmp_path):
    """equal scores: (head, rel, tail) position order, whichever side the kernel used"""
    from dglke_amd.infer import ScoreInfer
    ent = np.ones((50, 8), np.float32)
    rel = np.ones((2, 8), np.float32)
    cfg = _save(str(tmp_path), "DistMult", ent, rel, 8, 1.0)
    m = ScoreInfer(0, cfg, str(tmp_path), "none")
    m.load_model()
    for h, t in ((np.arange(20), np.arange(30)), (np.arange(30), np.arange(20))):
        (hl, rl, tl, sl), = m.topK(h, [1, 0], t, "all", 25)
        pos = [(int(a), [1, 0].index(int(b)), int(c)) for a, b, c in zip(hl, rl, tl)]
        assert pos == sorted(pos)
        assert np.all(sl == 8.0)


@pytest.mark.parametrize("d", [6, 36])
@pytest.mark.parametrize("sim", ["cosine", "l2", "l1", "dot", "ext_jaccard"])
def test_emb_sim_fp64(tmp_path, sim, d):
    from dglke_amd.infer import EmbSimInfer
    rng = np.random.RandomState(7)
    emb = rng.uniform(-1, 1, (300, d)).astype(np.float32)
    f = os.path.join(str(tmp_path), "e.npy")
    np.save(f, emb)
    m = EmbSimInfer(0, f, sim)
    m.load_emb()
    left, right = rng.randint(0, 300, 130), rng.permutation(300)
    left[3] = left[9]
    S = exact_sim(sim, emb, left, right).cpu().numpy()
    for K in (1, 10, 128):
        (hl, tl, sl), = m.topK(left, right, bcast=False, k=K)
        ex = {}
        for i in range(len(left)):
            for j in range(len(right)):
                ex.setdefault((int(left[i]), int(right[j])), []).append(float(S[i, j]))
        accept(ex, list(zip(hl.tolist(), tl.tolist())), [float(x) for x in sl], K, None)
        res = m.topK(left, right, bcast=True, k=K)
        assert len(res) == len(left)
        for i, (hl, tl, sl) in enumerate(res):
            assert np.all(hl == left[i])
            ex = {(int(left[i]), int(right[j])): [float(S[i, j])] for j in range(len(right))}
            accept(ex, [(int(left[i]), int(b)) for b in tl], [float(x) for x in sl], K, None)
        pl, pr = left[:100], right[:100]
        (hl, tl, sl), = m.topK(pl, pr, pair_ws=True, k=K)
        Sp = exact_sim(sim, emb, pl, pr).diagonal().cpu().numpy()
        ex = {}
        for i in range(100):
            ex.setdefault((int(pl[i]), int(pr[i])), []).append(float(Sp[i]))
        accept(ex, list(zip(hl.tolist(), tl.tolist())), [float(x) for x in sl], K, None)


def test_emb_sim_self_l2_direct_form(tmp_path):
    """an entity against itself tops an l2 list: the reported score is the direct |a - b| form (0), not the GEMM form"""
    from dglke_amd.infer import EmbSimInfer
    emb = np.random.RandomState(8).uniform(-1, 1, (500, 400)).astype(np.float32)
    f = os.path.join(str(tmp_path), "e.npy")
    np.save(f, emb)
    m = EmbSimInfer(0, f, "l2")
    m.load_emb()
    res = m.topK(np.arange(64), None, bcast=True, k=3)
    for i, (hl, tl, sl) in enumerate(res):
        assert tl[0] == i and abs(sl[0]) <= 1e-4


def test_cosine_zero_row_is_nan_and_last(tmp_path):
    from dglke_amd.infer import EmbSimInfer
    emb = np.random.RandomState(9).uniform(-1, 1, (40, 12)).astype(np.float32)
    emb[5] = 0.0
    f = os.path.join(str(tmp_path), "e.npy")
    np.save(f, emb)
    m = EmbSimInfer(0, f, "cosine")
    m.load_emb()
    for hl, tl, sl in m.topK(np.array([5, 6]), None, bcast=True, k=40):
        nan = np.isnan(sl)
        if hl[0] == 5:
            assert nan.all() and list(tl) == list(range(40))
        else:
            assert nan.sum() == 1 and nan[-1] and tl[-1] == 5
            assert np.all(np.diff(sl[:-1]) <= 1e-6)


def test_cli_end_to_end(tmp_path):
    """dglke_train (a 'TransE' model on a tiny built-in-layout dataset written by kgdataset's writer) -> dglke_predict
    --raw_data and dglke_emb_sim as subprocesses: their TSVs equal the Python API's results with ids mapped to names"""
    from dglke_amd import kgdataset
    from dglke_amd.infer import EmbSimInfer, ScoreInfer
    from dglke_amd.predict_cli import load_model_config, read_map
    tmp = str(tmp_path)
    rng = np.random.RandomState(11)
    n_ent, n_rel = 60, 4
    trip = [rng.randint(0, n, 300) for n in (n_ent, n_rel, n_ent)]
    split = lambda a, b: [x[a:b] for x in trip]
    d = kgdataset.write_built_in_layout(os.path.join(tmp, "data"), "FB15k", n_ent, n_rel, split(0, 260), split(260, 280),
                                        split(280, 300))
    subprocess.run([sys.executable, os.path.join(ROOT, "dgl-ke_amd", "dglke_train"), "--model_name", "TransE",
                    "--dataset", "FB15k", "--data_path", os.path.join(tmp, "data"), "--format", "built_in",
                    "--save_path", os.path.join(tmp, "ckpts"), "--gpu", "0", "--hidden_dim", "16", "-g", "6",
                    "--lr", "0.1", "--batch_size", "64", "--neg_sample_size", "16", "--max_step", "50",
                    "--log_interval", "25"], check=True, timeout=600)
    model_path = os.path.join(tmp, "ckpts", "TransE_FB15k_0")
    emap, rmap = os.path.join(d, "entities.dict"), os.path.join(d, "relations.dict")
    _, id2e = read_map(emap)
    _, id2r = read_map(rmap)
    with open(os.path.join(tmp, "head.list"), "w") as f:
        f.write("/e/3\n/e/17\n/e/3\n")
    with open(os.path.join(tmp, "rel.list"), "w") as f:
        f.write("/r/2\n/r/0\n")
    out = os.path.join(tmp, "pred.tsv")
    subprocess.run([sys.executable, os.path.join(ROOT, "dgl-ke_amd", "dglke_predict"), "--model_path", model_path,
                    "--format", "h_r_*", "--data_files", os.path.join(tmp, "head.list"), os.path.join(tmp, "rel.list"),
                    "--raw_data", "--entity_mfile", emap, "--rel_mfile", rmap, "--exec_mode", "batch_head", "--topK", "7",
                    "--score_func", "logsigmoid", "--output", out, "--gpu", "0"], check=True, timeout=300)
    m = ScoreInfer(0, load_model_config(os.path.join(model_path, "config.json")), model_path, "logsigmoid")
    m.load_model()
    want = ["head\trel\ttail\tscore"]
    for hl, rl, tl, sl in m.topK(np.array([3, 17, 3]), np.array([2, 0]), None, "batch_head", 7):
        for a, b, c, x in zip(hl.tolist(), rl.tolist(), tl.tolist(), sl.tolist()):
            want.append("{}\t{}\t{}\t{}".format(id2e[a], id2r[b], id2e[c], x))
    with open(out) as f:
        assert f.read().splitlines() == want
    out2 = os.path.join(tmp, "sim.tsv")
    efile = os.path.join(model_path, "FB15k_TransE_entity.npy")
    subprocess.run([sys.executable, os.path.join(ROOT, "dgl-ke_amd", "dglke_emb_sim"), "--emb_file", efile, "--format", "*",
                    "--raw_data", "--mfile", emap, "--exec_mode", "batch_left", "--sim_func", "l1", "--topK", "4",
                    "--output", out2, "--gpu", "0"], check=True, timeout=300)
    e = EmbSimInfer(0, efile, "l1")
    e.load_emb()
    want = ["left\tright\tscore"]
    for hl, tl, sl in e.topK(None, None, bcast=True, k=4):
        for a, b, x in zip(hl.tolist(), tl.tolist(), sl.tolist()):
            want.append("{}\t{}\t{}".format(id2e[a], id2e[b], x))
    with open(out2) as f:
        assert f.read().splitlines() == want


# ---- the unmodified reference's own results (tests/golden/gen_golden_infer.py) ------------------------------------------------
GOLDEN_INFER = os.path.join(ROOT, "tests", "golden", "infer")
GOLDEN_MODELS = {"transe_l2": "TransE_l2", "transe_l1": "TransE_l1", "distmult": "DistMult", "complex": "ComplEx",
                 "rotate": "RotatE", "simple": "SimplE", "rescal": "RESCAL"}


def _ref_groups(z, key):
    """the reference's result tuples of one case, split back into groups"""
    n = z[key + "_n"]
    cols = [c for c in ("h", "l", "r", "t", "s") if key + "_" + c in z]
    off = np.concatenate([[0], np.cumsum(n)])
    return [tuple(z[key + "_" + c][off[g]:off[g + 1]] for c in cols) for g in range(len(n))]


@pytest.mark.parametrize("sfunc", ["none", "logsigmoid"])
@pytest.mark.parametrize("name", sorted(GOLDEN_MODELS))
def test_predict_against_reference_goldens(tmp_path, name, sfunc):
    from dglke_amd.infer import ScoreInfer
    z = dict(np.load(os.path.join(GOLDEN_INFER, "infer_%s.npz" % name)))
    model = GOLDEN_MODELS[name]
    hidden, K = int(z["hidden"]), int(z["K"])
    np.save(os.path.join(str(tmp_path), "toy_%s_entity.npy" % model), z["entity"])
    np.save(os.path.join(str(tmp_path), "toy_%s_relation.npy" % model), z["relation"])
    cfg = {"model_name": model, "dataset": "toy", "hidden_dim": hidden, "gamma": float(z["gamma"]),
           "double_ent": bool(z["de"]), "double_rel": bool(z["dr"])}
    m = ScoreInfer(0, cfg, str(tmp_path), sfunc)
    m.load_model()
    h, r, t = z["h"], z["r"], z["t"]
    full = z["%s_full" % sfunc].astype(np.float64).reshape(len(h), len(r), len(t))        # the reference's own scores
    for mode in ("all", "batch_head", "batch_rel", "batch_tail"):
        got = m.topK(h, r, t, mode, K)
        ref = _ref_groups(z, "%s_%s" % (sfunc, mode))
        assert len(got) == len(ref)
        ex = _exact_dict(th.as_tensor(full), h, r, t, _groups(mode, len(h), len(r), len(t)))
        for (hl, rl, tl, sl), (rh, rr, rt, rs), e in zip(got, ref, ex):
            assert len(sl) == len(rs) == min(K, sum(len(v) for v in e.values()))
            accept(e, list(zip(hl.tolist(), rl.tolist(), tl.tolist())), [float(x) for x in sl], K, None)
            # the reference's own returned set, wherever its K-th score is clear of the next one
            accept(e, list(zip(rh.tolist(), rr.tolist(), rt.tolist())), [float(x) for x in rs], K, None)
            np.testing.assert_allclose(sl, rs, rtol=1e-4, atol=1e-4)
    hw, rw, tw = z["hw"], z["rw"], z["tw"]
    (hl, rl, tl, sl), = m.topK(hw, rw, tw, "triplet_wise", K)
    (rh, rr, rt, rs), = _ref_groups(z, "%s_triplet_wise" % sfunc)
    fw = z["%s_fullw" % sfunc]
    e = {}
    for i in range(len(hw)):
        e.setdefault((int(hw[i]), int(rw[i]), int(tw[i])), []).append(float(fw[i]))
    accept(e, list(zip(hl.tolist(), rl.tolist(), tl.tolist())), [float(x) for x in sl], K, None)
    np.testing.assert_allclose(sl, rs, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("sim", ["cosine", "l2", "l1", "dot", "ext_jaccard"])
def test_emb_sim_against_reference_goldens(tmp_path, sim):
    from dglke_amd.infer import EmbSimInfer
    z = dict(np.load(os.path.join(GOLDEN_INFER, "infer_sim.npz")))
    f = os.path.join(str(tmp_path), "emb.npy")
    np.save(f, z["emb"])
    m = EmbSimInfer(0, f, sim)
    m.load_emb()
    K, left, right, pl, pr = int(z["K"]), z["left"], z["right"], z["pl"], z["pr"]
    full, fw = z["%s_full" % sim].astype(np.float64), z["%s_fullw" % sim].astype(np.float64)
    cases = (("pairwise", dict(pair_ws=True), pl, pr), ("all", {}, left, right), ("batch_left", dict(bcast=True), left, right))
    for mode, kw, a, b in cases:
        got = m.topK(a, b, k=K, **kw)
        ref = _ref_groups(z, "%s_%s" % (sim, mode))
        assert len(got) == len(ref)
        for g, ((gl, gr, gs), (rl, rr, rs)) in enumerate(zip(got, ref)):
            if mode == "pairwise":
                e = {}
                for i in range(len(a)):
                    e.setdefault((int(a[i]), int(b[i])), []).append(float(fw[i]))
            elif mode == "all":
                e = {}
                for i in range(len(a)):
                    for j in range(len(b)):
                        e.setdefault((int(a[i]), int(b[j])), []).append(float(full[i, j]))
            else:
                e = {(int(a[g]), int(b[j])): [float(full[g, j])] for j in range(len(b))}
            accept(e, list(zip(gl.tolist(), gr.tolist())), [float(x) for x in gs], K, None)
            accept(e, list(zip(rl.tolist(), rr.tolist())), [float(x) for x in rs], K, None)
            np.testing.assert_allclose(gs, rs, rtol=1e-4, atol=1e-4)


def test_library_calls_run_on_the_objects_device(tmp_path, monkeypatch):
    """every library call of ScoreInfer / EmbSimInfer is made with the object's GPU as the current device and on that
    device's current stream (the last GPU of the box: on a multi-GPU box not the default one)"""
    from dglke_amd import _lib
    from dglke_amd.infer import EmbSimInfer, ScoreInfer
    dev = th.cuda.device_count() - 1
    real, calls = _lib.lib(), []

    class Probe(object):
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("kge_") or name in ("kge_last_error", "kge_topk_workspace_bytes"):
                return fn

            def call(*a):
                calls.append((name, th.cuda.current_device(), _lib.stream_ptr() == th.cuda.current_stream(dev).cuda_stream))
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Probe())
    ent, rel = _tables("DistMult", 200, 3, 36, 12)
    cfg = _save(str(tmp_path), "DistMult", ent, rel, 36, 12.0)
    m = ScoreInfer(dev, cfg, str(tmp_path), "none")
    m.load_model()
    m.topK([1, 2], [0], None, "batch_head", 5)
    m.topK([1, 2], [0, 1], [3, 4], "triplet_wise", 2)
    e = EmbSimInfer(dev, os.path.join(str(tmp_path), "toy_DistMult_entity.npy"), "cosine")
    e.load_emb()
    e.topK([1, 2], None, bcast=True, k=3)
    e.topK([1, 2], [3, 4], pair_ws=True, k=1)
    assert {c[0] for c in calls} == {"kge_topk_select", "kge_score_pos", "kge_topk_vector", "kge_sim_pairwise"}
    assert all(d == dev and same for _, d, same in calls), calls
