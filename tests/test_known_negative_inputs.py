"""CPU guard of tests/known_negative_cases.py: the float64 statement of the masked step and the planted batches the GPU tests
(tests/test_gpu_known_negatives.py) rely on."""
import numpy as np
import pytest

import known_negative_cases as KN
import loss_option_cases as L
from oracle import kge_oracle as O

IDS = [c["id"] for c in KN.CASES]


@pytest.fixture(scope="module")
def built():
    return {c["id"]: KN.build(c) for c in KN.CASES}


def _tables64(c):
    ent, rel, proj = L.tables(c)
    return ent.astype(np.float64), rel.astype(np.float64), None if proj is None else proj.astype(np.float64)


@pytest.mark.parametrize("c", KN.CASES, ids=IDS)
def test_empty_known_set_is_the_oracle_step(c, built):
    ent, rel, proj = _tables64(c)
    for bt in built[c["id"]][0]:
        none = np.zeros((c["B"], c["N"]), bool)
        got = KN.masked_forward_backward(c, ent, rel, proj, bt, none)
        ref = L.oracle_forward_backward(c, ent, rel, proj, bt)
        for k in ("pos_score", "neg_score", "g_pos_ent", "g_neg", "g_rel") + (("g_proj0", "g_proj1") if proj is not None else ()):
            assert np.abs(np.asarray(got[k]) - np.asarray(ref[k])).max() <= 1e-12, k
        lg, lr_ = np.array(got["log"], float), np.array(ref["log"], float)
        ok = ~np.isnan(lr_)
        assert (np.isnan(lg) == np.isnan(lr_)).all() and np.abs(lg[ok] - lr_[ok]).max() <= 1e-12


@pytest.mark.parametrize("adv,pw", [(False, False), (True, False), (False, True)], ids=["plain", "adv", "pw"])
@pytest.mark.parametrize("genre", ["Logsigmoid", "Logistic", "Hinge", "BCE"])
def test_minus_1e6_entries_are_exact_zeros_in_float64(genre, adv, pw):
    """a known pair = a negative at -1e6: loss term 0, gradient 0, no softmax weight, denominators 1 / N and 1 / B unchanged; an
    all-known row adds 0 and stays finite"""
    rng = np.random.RandomState(5)
    B, N, T = 6, 9, 0.7
    pos, neg = rng.normal(0, 2, B), rng.normal(0, 2, (B, N))
    known = rng.rand(B, N) < 0.4
    known[0], known[1] = True, False
    w = rng.uniform(0.5, 1.5, B)
    nm = np.where(known, KN.KNOWN_SCORE, neg)
    (pl, nl, loss), dpos, dneg = O.loss_fwd_bwd(pos, nm, w, genre, adv, T, pw, 1.0)
    assert np.isfinite(loss) and np.isfinite(dpos).all() and np.isfinite(dneg).all()
    assert (dneg[known] == 0.0).all() and (dneg[~known] != 0.0).any() and dneg[0].tolist() == [0.0] * N
    el, _ = O._criterion(genre, (pos[:, None] - nm) if pw else nm, 1 if pw else (0 if genre == "BCE" else -1), 1.0)
    assert (el[known] == 0.0).all()
    # the same loss from the unknown pairs alone
    rows = np.zeros(B)
    for i in range(B):
        u = ~known[i]
        if not u.any():
            continue
        if adv:
            e = np.exp((neg[i, u] - neg[i, u].max()) * T)
            rows[i] = (e / e.sum() * el[i, u]).sum() * w[i]
        else:
            rows[i] = el[i, u].sum() / N * w[i]
    assert abs((loss if pw else nl) - rows.mean()) <= 1e-12


@pytest.mark.parametrize("c", KN.CASES, ids=IDS)
def test_every_case_plants_the_edge_cases(c, built):
    bts, K, notes = built[c["id"]]
    B, chunk, N = c["B"], c["chunk"], c["N"]
    assert [bt["neg_head"] for bt in bts] == [False, True]
    for bt, note in zip(bts, notes):
        kn = KN.known_matrix(K, bt, chunk, N)
        assert kn[0].all() and not kn[1].any()
        assert kn[:, N - 1].any() and kn[:, min(32, N - 1):].any()
        assert kn[2, N - 1] and kn[2, min(32, N - 1)]
        share = kn.mean()
        assert 0.05 <= share <= 0.60, share
        # a list longer than 64 entities: row 0's key
        x, y = KN.corrupted(bt)
        keyed = (K[2] if bt["neg_head"] else K[0]) == x[0]
        assert int((keyed & (K[1] == bt["r"][0])).sum()) > 64
        # an entity that occurs in the batch only as a known negative
        lone, slot = note["lone"], note["lone_slot"]
        assert (bt["neg"] == lone).sum() == 1 and bt["neg"][slot] == lone
        assert lone not in bt["h"] and lone not in bt["t"]
        assert slot // N == B // chunk - 1 and kn[B - chunk:, slot % N].all()
        # the row's own corrupted entity as a negative, and the ids 0 and n_ent - 1
        assert bt["neg"][(3 // chunk) * N + 1] == y[3] and kn[3, 1]
        assert x[0] == 0 and (bt["neg"] == c["n_ent"] - 1).any()
        if c["model"] == "TransR":
            assert (bt["h"] != bt["t"]).all()


def test_masked_pairs_leave_their_rows_alone_in_float64(built):
    """with reg_coef 0 the lone known negative's row and state do not move, and its slot's gradient is exactly zero"""
    for c in KN.CASES:
        if c["reg_coef"] > 0:
            continue
        ent, rel, proj = _tables64(c)
        bts, K, notes = built[c["id"]]
        for bt, note in zip(bts, notes):
            e, r = ent.copy(), rel.copy()
            es, rs = np.zeros(len(e)), np.zeros(len(r))
            pj = None if proj is None else proj.copy()
            ps = None if proj is None else np.zeros(len(r))
            out = KN.masked_step(c, e, es, r, rs, pj, ps, bt, KN.known_matrix(K, bt, c["chunk"], c["N"]))
            assert (out["g_neg"][note["lone_slot"]] == 0.0).all()
            assert (e[note["lone"]] == ent[note["lone"]]).all() and es[note["lone"]] == 0.0
