"""dglke_amd.ke_model.link_predict on the GPU: known-edge exclusion inside the top-K selection (kge_topk_select_filtered) and the
known flags (kge_triples_known), against the fp64 statement of the scores of tests/test_gpu_infer.py WITH THE KNOWN
COMBINATIONS REMOVED.  Acceptance rule: the one stated at the top of tests/test_gpu_infer.py (tolerance 1e-4 * max(1, |s|),
the exact set wherever the K-th and (K+1)-th exact scores are further apart than that)."""
import os
import sys

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gpu_infer import MODELS, _exact_dict, _groups, _save, _tables, accept, exact_scores      # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("all", "batch_head", "batch_rel", "batch_tail")
GAMMA = 12.0


def _model(model, gamma, path, ent, rel):
    from dglke_amd import ke_model as K
    np.save(os.path.join(path, "entity.npy"), ent)
    np.save(os.path.join(path, "relation.npy"), rel)
    cls = getattr(K, model + "Model")
    m = cls(0, gamma) if model in ("TransE_l1", "TransE_l2", "RotatE") else cls(0)
    m.load(path)
    return m


def _hidden_of(model, ent):
    return ent.shape[1] // 2 if model in ("ComplEx", "RotatE", "SimplE") else ent.shape[1]


def _without(ex, known):
    return {key: v for key, v in ex.items() if key not in known}


def _clear(ex, K):
    """whether the K-th and (K+1)-th exact scores of a group are further apart than the tolerance (the exact-set clause of
    `accept` applies)"""
    flat = sorted((s for v in ex.values() for s in v), reverse=True)
    m = min(K, len(flat))
    return m > 0 and m < len(flat) and flat[m - 1] - flat[m] > 1e-4 * max(1.0, abs(flat[m - 1]))


def _check(res, exact_groups, K, known=None, want_mask=False, tally=None):
    assert len(res) == len(exact_groups)
    for (hl, rl, tl, sl, ml), ex in zip(res, exact_groups):
        keys = list(zip(hl.tolist(), rl.tolist(), tl.tolist()))
        assert all(a >= 0 and c >= 0 for a, _, c in keys)                       # an empty slot (ordinal -1) never leaks out
        accept(ex, keys, [float(x) for x in sl], K, None)
        if want_mask:
            assert ml is not None and ml.dtype == np.bool_ and ml.tolist() == [key in known for key in keys]
        else:
            assert ml is None
        if tally is not None:
            tally.append(_clear(ex, K))


@pytest.mark.parametrize("model", MODELS)
def test_link_predict_planted_graph_fp64(tmp_path, model):
    """the attached graph holds the 3K best combinations of every batch_head group (by the fp64 scores) plus 2 % random
    triples: the unfiltered answer consists of known triples, so 'exclude' cannot pass by accident"""
    K, n_ent, n_rel = 10, 300, 5
    tally = []
    for hidden in (6, 36):                                   # the VALU tile and the MFMA tile
        ent, rel = _tables(model, n_ent, n_rel, hidden, 21 + hidden)
        path = os.path.join(str(tmp_path), "d%d" % hidden)
        os.makedirs(path)
        m = _model(model, GAMMA, path, ent, rel)
        rng = np.random.RandomState(22)
        h = rng.permutation(n_ent)[:40]
        r = np.array([4, 0, 2, 1, 3])
        t = rng.permutation(n_ent)
        S = exact_scores(model, ent, rel, h, r, t, GAMMA, (GAMMA + 2.0) / _hidden_of(model, ent))
        Sn = S.cpu().numpy()
        kh, kr, kt = [], [], []
        for i in range(len(h)):
            best = np.argsort(-Sn[i].reshape(-1), kind="stable")[:3 * K]
            kh += [h[i]] * len(best); kr += list(r[best // len(t)]); kt += list(t[best % len(t)])
        n_rand = n_ent * n_rel * n_ent * 2 // 100
        kh += list(rng.randint(0, n_ent, n_rand)); kr += list(rng.randint(0, n_rel, n_rand)); kt += list(rng.randint(0, n_ent, n_rand))
        known = set(zip((int(x) for x in kh), (int(x) for x in kr), (int(x) for x in kt)))
        m.attach_graph((np.array(kh), np.array(kr), np.array(kt)))
        assert m.graph is not None
        for mode in MODES:
            ex = _exact_dict(S, h, r, t, _groups(mode, len(h), len(r), len(t)))
            plain = m.link_predict(h, r, t, mode, "none", K, None)
            _check(plain, ex, K, tally=tally)
            if mode == "batch_head":                         # the plant: every unfiltered result is a known triple
                assert all((a, b, c) in known for g in plain for a, b, c in zip(g[0].tolist(), g[1].tolist(), g[2].tolist()))
            masked = m.link_predict(h, r, t, mode, "none", K, "mask")
            for a, b in zip(plain, masked):
                assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
            _check(masked, ex, K, known, want_mask=True)
            excl = m.link_predict(h, r, t, mode, "none", K, "exclude")
            _check(excl, [_without(e, known) for e in ex], K, tally=tally)
            assert all((a, b, c) not in known for g in excl for a, b, c in zip(g[0].tolist(), g[1].tolist(), g[2].tolist()))
        # triplet_wise: 150 query positions of the block, 60 of them known triples
        kn_pos = [(i, j, k) for i in range(len(h)) for j in range(len(r)) for k in range(len(t))
                  if (int(h[i]), int(r[j]), int(t[k])) in known]
        kn_pos = kn_pos[::len(kn_pos) // 60][:60]
        pos = kn_pos + [(int(rng.randint(40)), int(rng.randint(5)), int(rng.randint(300))) for _ in range(90)]
        assert len(kn_pos) == 60
        hw, rw, tw = (np.array([x[c] for x in pos]) for c in range(3))
        Sw = S[th.as_tensor(hw, device=S.device), th.as_tensor(rw, device=S.device), th.as_tensor(tw, device=S.device)]
        if model == "SimplE":
            Sw = Sw.clamp(-20, 20)
        ex = {}
        for i, (a, b, c) in enumerate(zip(h[hw], r[rw], t[tw])):
            ex.setdefault((int(a), int(b), int(c)), []).append(float(Sw[i]))
        plain = m.link_predict(h[hw], r[rw], t[tw], "triplet_wise", "none", K, None)
        _check(plain, [ex], K, tally=tally)
        masked = m.link_predict(h[hw], r[rw], t[tw], "triplet_wise", "none", K, "mask")
        assert all(np.array_equal(x, y) for x, y in zip(plain[0][:4], masked[0][:4]))
        _check(masked, [ex], K, known, want_mask=True)
        _check(m.link_predict(h[hw], r[rw], t[tw], "triplet_wise", "none", K, "exclude"), [_without(ex, known)], K, tally=tally)
    clear = sum(tally) / float(len(tally))
    print("%s: %d of %d groups had a clear K-th gap (%.1f %%)" % (model, sum(tally), len(tally), 100 * clear))
    assert clear >= 0.9, "too many tied groups for the exact-set clause to mean anything: %.3f" % clear


@pytest.mark.parametrize("model", ["DistMult", "TransE_l1"])
def test_hub_and_boundaries_fb15k_shape(tmp_path, model):
    """1000 heads x 14 951 candidates, d 400: a hub (h, r) with 5 000 known tails (its 4K best, both ends of a 128-candidate
    tile and of a segment, the last candidate), an (h, r) with all but 3 tails known, rows with short lists and rows with
    empty lists in the same call"""
    K, n_ent, hidden = 10, 14951, 400
    ent, rel = _tables(model, n_ent, 2, hidden, 31)
    ent *= 0.1
    m = _model(model, GAMMA, str(tmp_path), ent, rel)
    rng = np.random.RandomState(32)
    h = rng.permutation(n_ent)[:1000]
    t = np.arange(n_ent)
    S = exact_scores(model, ent, rel, h[:40], [1], t, GAMMA, 1.0)
    Sn = S.cpu().numpy()[:, 0, :]
    hub = set(np.argsort(-Sn[0], kind="stable")[:4 * K].tolist())
    hub |= {0, 127, 128, 255, 639, 640, 5 * 128 * 2 - 1, 5 * 128 * 2, n_ent - 1}     # tile ends; segment ends (5 tiles each)
    hub = sorted(hub | set([x for x in rng.permutation(n_ent).tolist() if x not in hub][:5000 - len(hub)]))
    assert len(hub) == 5000
    left3 = set(np.argsort(-Sn[1], kind="stable")[[5, 700, 14000]].tolist())          # row 1 keeps three candidates
    kh = [h[0]] * len(hub) + [h[1]] * (n_ent - 3)
    kt = list(hub) + [x for x in range(n_ent) if x not in left3]
    for i in range(2, 12):                                   # short lists (the broadcast path): the row's 5 best + 15 others
        mine = set(np.argsort(-Sn[i], kind="stable")[:5].tolist()) | set(rng.randint(0, n_ent, 15).tolist())
        kh += [h[i]] * len(mine); kt += sorted(mine)
    kr = [1] * len(kh)
    # the same pairs under the other relation and a few triples of heads that are not queried: must not matter
    kh += [h[20]] * 50 + [h[999]] * 50; kr += [0] * 100; kt += list(range(50)) * 2
    known = set(zip((int(x) for x in kh), kr, (int(x) for x in kt)))
    m.attach_graph((np.array(kh), np.array(kr), np.array(kt)))
    ex = _exact_dict(S, h[:40], [1], t, _groups("batch_head", 40, 1, n_ent))
    res = m.link_predict(h, [1], None, "batch_head", "none", K, "exclude")
    assert len(res) == 1000
    _check(res[:40], [_without(e, known) for e in ex], K)
    assert len(res[1][0]) == 3 and set(res[1][2].tolist()) == left3
    assert all(len(g[0]) == K for i, g in enumerate(res) if i != 1)
    assert not (set(res[0][2].tolist()) & set(hub))
    plain = m.link_predict(h, [1], None, "batch_head", "none", K, None)
    _check(plain[:40], ex, K)
    for i in range(12, 1000):                                # rows with empty lists: the unfiltered result, array for array
        assert all(np.array_equal(x, y) for x, y in zip(plain[i][:4], res[i][:4]))
    masked = m.link_predict(h, [1], None, "batch_head", "none", K, "mask")
    _check(masked[:40], ex, K, known, want_mask=True)
    assert masked[0][4].all() and not any(g[4].any() for g in masked[12:])
    assert masked[1][4].tolist() == [i != 5 for i in range(K)]          # (row 1's sixth best is one of its three unknown tails)


@pytest.mark.parametrize("model,hidden", [("DistMult", 36), ("TransE_l1", 6), ("TransE_l2", 36)])
def test_explicit_candidate_lists_unsorted_with_repeats(tmp_path, model, hidden):
    """a candidate list that is unsorted and repeats ids: every position of a known id is left out, both positions of an
    unknown one may be returned; with more heads than tails the kernel scores the head side (lists of known heads)"""
    K, n_ent, n_rel = 10, 200, 3
    ent, rel = _tables(model, n_ent, n_rel, hidden, 41)
    m = _model(model, GAMMA, str(tmp_path), ent, rel)
    rng = np.random.RandomState(42)
    r = np.array([2, 0])
    for H, T in ((6, 90), (90, 12)):
        h, t = rng.randint(0, n_ent, H), rng.randint(0, n_ent, T)
        h[1], t[3], t[7] = h[0], t[0], t[0]                  # repeated ids on both sides
        S = exact_scores(model, ent, rel, h, r, t, GAMMA, 1.0)
        Sn = S.cpu().numpy()
        top = np.argsort(-Sn.reshape(-1), kind="stable")[:40]          # the 40 best combinations + the repeated pair + noise
        hp, rp, tp = top // (len(r) * T), (top // T) % len(r), top % T
        kh = list(h[hp]) + [h[0], h[0]] + list(rng.randint(0, n_ent, 400))
        kr = list(r[rp]) + [2, 0] + list(rng.choice(r, 400))
        kt = list(t[tp]) + [t[0], t[0]] + list(rng.randint(0, n_ent, 400))
        known = set(zip((int(x) for x in kh), (int(x) for x in kr), (int(x) for x in kt)))
        m.attach_graph((kh, kr, kt))
        for mode in MODES:
            ex = _exact_dict(S, h, r, t, _groups(mode, H, len(r), T))
            _check(m.link_predict(h, r, t, mode, "none", K, "exclude"), [_without(e, known) for e in ex], K)
            _check(m.link_predict(h, r, t, mode, "none", K, "mask"), ex, K, known, want_mask=True)
        # nothing left: every combination of the group is known
        full = [(int(h[0]), int(b), int(c)) for b in r for c in t]
        m.attach_graph(tuple(np.array([x[c] for x in full]) for c in range(3)))
        res = m.link_predict(h[:1], r, t, "batch_head", "none", K, "exclude")
        assert len(res) == 1 and all(len(x) == 0 for x in res[0][:4])


def test_groups_over_several_calls_and_determinism(tmp_path):
    K = 128
    ent, rel = _tables("DistMult", 400, 4, 36, 51)
    m = _model("DistMult", GAMMA, str(tmp_path), ent, rel)
    h, r, t = np.arange(100), np.arange(4), np.arange(400)
    S = exact_scores("DistMult", ent, rel, h, r, t, 0.0, 1.0)
    top = th.topk(S.reshape(-1), 500).indices.cpu().numpy()
    kh, kr, kt = h[top // 1600], r[(top // 400) % 4], t[top % 400]
    known = set(zip(kh.tolist(), kr.tolist(), kt.tolist()))
    m.attach_graph((kh, kr, kt))
    one = m.link_predict(h, r, t, "all", "none", K, "exclude")
    m.max_rows = 128                                         # 400 rows -> four calls carrying the running result
    split = m.link_predict(h, r, t, "all", "none", K, "exclude")
    again = m.link_predict(h, r, t, "all", "none", K, "exclude")
    for a, b, c in zip(one[0][:4], split[0][:4], again[0][:4]):
        assert np.array_equal(a, b) and np.array_equal(b, c)
    _check(split, [_without(e, known) for e in _exact_dict(S, h, r, t, _groups("all", 100, 4, 400))], K)
    m.max_rows = 64                                          # batch_rel groups of 100 rows over two calls each
    for mode in ("batch_rel", "batch_tail"):
        ex = [_without(e, known) for e in _exact_dict(S, h, r, t, _groups(mode, 100, 4, 400))]
        a = m.link_predict(h, r, t, mode, "none", 10, "exclude")
        b = m.link_predict(h, r, t, mode, "none", 10, "exclude")
        _check(a, ex, 10)
        for x, y in zip(a, b):
            assert all(np.array_equal(p, q) for p, q in zip(x[:4], y[:4]))


@pytest.mark.parametrize("model", ["TransE_l2", "RotatE", "DistMult"])
def test_no_exclusion_equals_score_infer(tmp_path, model):
    """exclude_mode None is the existing path: array for array what ScoreInfer.topK returns (logsigmoid: the same gamma)"""
    from dglke_amd.infer import ScoreInfer
    hidden = 18 if model == "RotatE" else 36
    ent, rel = _tables(model, 300, 5, hidden, 61)
    cfg = _save(str(tmp_path), model, ent, rel, hidden, GAMMA)
    s = ScoreInfer(0, cfg, str(tmp_path), "logsigmoid")
    s.load_model()
    m = _model(model, GAMMA, str(tmp_path), ent, rel)
    assert m.num_entity == 300 and m.num_rel == 5 and m.model_name == model
    assert th.equal(m.entity_embed, s.ent) and m.relation_embed.shape == s.rel.shape
    rng = np.random.RandomState(62)
    h, r, t = rng.randint(0, 300, 13), np.array([4, 0, 2]), rng.permutation(300)[:290]
    for mode in MODES:
        want, got = s.topK(h, r, t, mode, 10), m.link_predict(h, r, t, mode, "logsigmoid", 10)
        assert len(want) == len(got)
        for a, b in zip(want, got):
            assert b[4] is None and all(np.array_equal(x, y) for x, y in zip(a, b[:4]))
    rw = rng.randint(0, 5, 13)
    (a,), (b,) = s.topK(h, rw, t[:13], "triplet_wise", 5), m.link_predict(h, rw, t[:13], "triplet_wise", "logsigmoid", 5)
    assert b[4] is None and all(np.array_equal(x, y) for x, y in zip(a, b[:4]))
    # the trainer's own file names through config.json
    import json
    alt = os.path.join(str(tmp_path), "alt")
    os.makedirs(alt)
    _save(alt, model, ent, rel, hidden, GAMMA)
    with open(os.path.join(alt, "config.json"), "w") as f:
        json.dump({"dataset": "toy", "model_name": model}, f)
    from dglke_amd import ke_model as K
    m2 = getattr(K, model + "Model")(0, GAMMA) if model != "DistMult" else K.DistMultModel(0)
    m2.load(alt)
    assert th.equal(m2.entity_embed, m.entity_embed)


def test_triples_known_kernel_and_embed_sim(tmp_path):
    """kge_triples_known against a Python set (one-key and two-key index), and embed_sim = EmbSimInfer on the loaded table"""
    from dglke_amd import eval as E
    from dglke_amd.infer import EmbSimInfer
    from dglke_amd.known import KnownIndex
    rng = np.random.RandomState(71)
    NE, R = 500, 7
    kh, kr, kt = rng.randint(0, NE, 3000), rng.choice([0, 1, 2, 4, 5, 6], 3000), rng.randint(0, NE, 3000)
    kh[:4], kr[:4], kt[:4] = [0, 0, NE - 1, NE - 1], [0, 6, 0, 6], [0, NE - 1, 0, NE - 1]
    known = set(zip(kh.tolist(), kr.tolist(), kt.tolist()))
    qh, qr, qt = (np.concatenate([a[:1500], b]) for a, b in zip((kh, kr, kt), (rng.randint(0, NE, 1500), rng.randint(0, R, 1500), rng.randint(0, NE, 1500))))
    want = [x in known for x in zip(qh.tolist(), qr.tolist(), qt.tolist())]
    for two_key in (False, True):
        E._FORCE_TWO_KEY_SORT = two_key
        try:
            ix = KnownIndex((kh, kr, kt), NE, R, "cuda:0")
            got = ix.known(*(th.as_tensor(x, device="cuda:0") for x in (qh, qr, qt)))
        finally:
            E._FORCE_TWO_KEY_SORT = False
        assert got.dtype == th.uint8 and got.cpu().numpy().astype(bool).tolist() == want
    ent, rel = _tables("DistMult", 300, 5, 36, 72)
    m = _model("DistMult", GAMMA, str(tmp_path), ent, rel)
    for etype, tab in (("entity", ent), ("relation", rel)):
        f = os.path.join(str(tmp_path), etype + "_tab.npy")
        np.save(f, tab)
        e = EmbSimInfer(0, f, "l2")
        e.load_emb()
        left = np.arange(min(20, tab.shape[0]))
        for kw in (dict(bcast=True), dict(), dict(pair_ws=True)):
            want = e.topK(left, left if kw.get("pair_ws") else None, k=4, **kw)
            got = m.embed_sim(left, left if kw.get("pair_ws") else None, etype, "l2", topk=4, **kw)
            assert len(want) == len(got)
            for a, b in zip(want, got):
                assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the unmodified reference's link_predict (tests/golden/gen_golden_link_predict.py) ------------------------------------------
GOLDEN_LP = os.path.join(ROOT, "tests", "golden", "link_predict")
GOLDEN_LP_MODELS = {"transe_l2": "TransE_l2", "distmult": "DistMult"}


def _ref_groups(z, key):
    n = z[key + "_n"]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    cols = [c for c in ("h", "r", "t", "s", "m") if key + "_" + c in z]
    return [tuple(z[key + "_" + c][off[g]:off[g + 1]] for c in cols) for g in range(len(n))]


@pytest.mark.parametrize("sfunc", ["none", "logsigmoid"])
@pytest.mark.parametrize("name", sorted(GOLDEN_LP_MODELS))
def test_link_predict_against_reference_goldens(tmp_path, name, sfunc):
    """both the reference's result and ours are accepted against the reference's OWN full scores with the known triples removed"""
    z = dict(np.load(os.path.join(GOLDEN_LP, "lp_%s.npz" % name)))
    model = GOLDEN_LP_MODELS[name]
    K = int(z["K"])
    m = _model(model, float(z["gamma"]), str(tmp_path), z["entity"], z["relation"])
    kh, kr, kt = z["known_h"], z["known_r"], z["known_t"]
    known = set(zip(kh.tolist(), kr.tolist(), kt.tolist()))
    m.attach_graph((kh, kr, kt))
    h, r, t = z["h"], z["r"], z["t"]
    full = z["%s_full" % sfunc].astype(np.float64).reshape(len(h), len(r), len(t))
    for mode in MODES:
        ex = _exact_dict(th.as_tensor(full), h, r, t, _groups(mode, len(h), len(r), len(t)))
        for emode in (None, "mask", "exclude"):
            got = m.link_predict(h, r, t, mode, sfunc, K, emode)
            ref = _ref_groups(z, "%s_%s_%s" % (sfunc, mode, emode))
            assert len(got) == len(ref)
            exg = [_without(e, known) for e in ex] if emode == "exclude" else ex
            _check(got, exg, K, known, want_mask=emode == "mask")
            for g, rf, e in zip(got, ref, exg):
                accept(e, list(zip(rf[0].tolist(), rf[1].tolist(), rf[2].tolist())), [float(x) for x in rf[3]], K, None)
                np.testing.assert_allclose(g[3], rf[3], rtol=1e-4, atol=1e-4)
                if emode == "mask":
                    assert rf[4].astype(bool).tolist() == [x in known for x in zip(rf[0].tolist(), rf[1].tolist(), rf[2].tolist())]
