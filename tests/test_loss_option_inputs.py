"""Input guard of the loss-option tests (CPU): the cases of tests/loss_option_cases.py and the loss-option goldens must actually
exercise their criterion - a hinge whose scores all sit on one side of the kink, or a sigmoid sampled where it is linear, lets a
wrong kernel pass (the five older genre goldens did exactly that).  Also checks, between the float32 and the float64 oracle, the
caps under which the GPU test may exclude rows fed by a hinge pair that flips side (tests/test_gpu_loss_options.py)."""
import functools

import numpy as np
import pytest

import loss_option_cases as L
from golden_util import load_golden

# the goldens added with this family (tests/golden/gen_golden.py) and their genre; every one must meet the activity condition
GENRE_GOLDENS = ["distmult_hinge_adv", "transe_l2_bce_adv", "complex_logistic_adv", "rotate_hinge", "transe_l1_hinge_adv",
                 "transe_l2_hinge_pairwise_impts", "rescal_hinge_adv", "transr_bce_adv", "simple_logistic", "nd_distmult_hinge_adv"]
REG_GOLDENS = ["transe_l2_reg2", "rotate_reg2", "distmult_reg1", "complex_reg4"]


@functools.lru_cache(maxsize=4)
def _scores(shape_key, seed, neg_deg):
    """float32 and float64 oracle scores of both batches from the initial tables; shared by the cases of one shape"""
    c = next(c for c in L.CASES + [L.fuzz_case(s) for s in range(48)]
             if (c["id"] if c["shape"] == "fuzz" else c["shape"]) == shape_key and c["seed"] == seed and c["neg_deg"] == neg_deg)
    ent, rel, proj = L.tables(c)
    out = []
    for bt in L.batches(c):
        per = []
        for dt in (np.float32, np.float64):
            per.append(L.oracle_scores(c, ent.astype(dt), rel.astype(dt), None if proj is None else proj.astype(dt), bt))
        out.append((bt, per[0], per[1]))
    return out


def _case_scores(c):
    return _scores(c["id"] if c["shape"] == "fuzz" else c["shape"], c["seed"], c["neg_deg"])


@pytest.mark.parametrize("c", L.CASES, ids=lambda c: c["id"])
def test_case_inputs_exercise_the_criterion_and_stay_inside_the_flip_caps(c):
    for step, (bt, (p32, n32), (p64, n64)) in enumerate(_case_scores(c), 1):
        tag = "%s step %d" % (c["id"], step)
        assert p32.dtype == np.float32 and p64.dtype == np.float64
        assert L.activity_ok(c, p64, n64), "%s: the %s criterion is not exercised: %r" % (tag, c["genre"], L.activity(c, p64, n64))
        L.check_flip_caps(c, bt, L.hinge_flips(c, bt, p32, n32, p64, n64), tag)


@pytest.mark.parametrize("seed", range(48))
def test_fuzz_inputs_stay_inside_the_flip_caps(seed):
    """the small random cases are not held to the activity shares (a 4 x 2 batch cannot be), only to the flip caps"""
    c = L.fuzz_case(seed)
    for step, (bt, (p32, n32), (p64, n64)) in enumerate(_case_scores(c), 1):
        L.check_flip_caps(c, bt, L.hinge_flips(c, bt, p32, n32, p64, n64), "%s step %d" % (c["id"], step))


def test_fuzz_covers_every_axis():
    cs = [L.fuzz_case(s) for s in range(48)]
    assert {c["genre"] for c in cs} == {"Hinge", "BCE", "Logistic", "Logsigmoid"}
    assert {c["reg_norm"] for c in cs if c["reg_coef"] > 0} == {1, 2, 3, 4}
    assert {c["adv_temp"] for c in cs if c["adv"]} == {0.5, 1.0, 2.0}
    assert {c["margin"] for c in cs if c["genre"] == "Hinge"} == {0.5, 1.0, 2.0}
    assert any(c["pairwise"] for c in cs) and any(c["impts"] for c in cs) and any(c["neg_deg"] for c in cs)
    assert all(not (c["pairwise"] and c["adv"]) for c in cs)


@pytest.mark.parametrize("c", [c for c in L.CASES if c["reg_norm"] != 3], ids=lambda c: c["id"])
def test_regulariser_is_a_visible_share_of_the_gradient(c):
    """reg_norm cases: the regulariser's largest gradient component is >= 1 % of the largest gradient component (fp64 oracle)"""
    ent, rel, proj = (None if x is None else x.astype(np.float64) for x in L.tables(c))
    bt = L.batches(c)[0]
    out = L.oracle_forward_backward(c, ent, rel, proj, bt)
    assert L.reg_share(c, out, ent, rel, bt) >= 0.01, "%s: regulariser share %.3g" % (c["id"], L.reg_share(c, out, ent, rel, bt))


@pytest.mark.parametrize("name", GENRE_GOLDENS)
def test_genre_goldens_exercise_the_criterion(name):
    """read from the recorded reference scores: Hinge - in at least one step 20 - 80 % of the positives AND of the negatives
    (pairwise: of the pairs) are active; BCE / Logistic - the recorded scores span at least [-3, 3]"""
    z, case = load_golden(name)
    c = dict(genre=case["loss_genre"], pairwise=case.get("pairwise", False), margin=case.get("margin", 1.0))
    steps = [(z["s%d_pos_score" % s], z["s%d_neg_score" % s]) for s in range(1, case["steps"] + 1)]
    if c["genre"] == "Hinge":
        assert any(L.activity_ok(c, p, n) for p, n in steps), [L.activity(c, p, n) for p, n in steps]
    else:
        allsc = np.concatenate([np.concatenate([p.ravel(), n.ravel()]) for p, n in steps])
        assert allsc.min() <= -3.0 and allsc.max() >= 3.0, (allsc.min(), allsc.max())


@pytest.mark.parametrize("name", REG_GOLDENS)
def test_reg_goldens_show_the_regulariser_in_the_gradients(name):
    from oracle import kge_oracle as O
    z, case = load_golden(name)
    assert case["reg_norm"] != 3
    rg = np.abs(O.reg_grad(z["init_entity"][z["s1_nid"]].astype(np.float64), case["reg_coef"], case["reg_norm"])).max()
    assert rg >= 0.01 * np.abs(z["s1_g_pos_ent"]).max()
    assert z["s1_log"][3] >= 0.01 * abs(z["s1_log"][2])


@pytest.mark.parametrize("neg_deg", [False, True])
def test_hinge_flip_exclusion_names_exactly_the_rows_a_flipped_pair_feeds(neg_deg):
    """hinge_flips on scores with planted flips: one negative pair and one positive nudged across the kink in float32"""
    c = L.case("flip-check", "midD", "Hinge", neg_deg=neg_deg)
    ent, rel, _ = (None if x is None else x.astype(np.float64) for x in L.tables(c))
    bt = L.batches(c)[0]
    p64, n64 = L.oracle_scores(c, ent, rel, None, bt)
    p32, n32 = p64.astype(np.float32), n64.astype(np.float32)
    assert L.hinge_flips(c, bt, p32, n32, p64, n64)["n_flips"] == 0
    chunk, N = c["chunk"], c["N"]
    i, j = 50, (chunk + 3 if neg_deg else 3)                  # edge 50 (chunk 1), a SAMPLED negative column
    n64 = n64.copy()
    n64[i, j] = -c["margin"] - 3e-5                             # float64: just inactive ...
    n32[i, j] = np.float32(-c["margin"] + 3e-5)                 # ... float32: just active
    p64 = p64.copy()
    p64[7], p32[7] = c["margin"] - 2e-5, np.float32(c["margin"] + 2e-5)
    fl = L.hinge_flips(c, bt, p32, n32, p64, n64)
    slot = (i // chunk) * N + 3
    assert fl["n_flips"] == 2 and fl["worst_v"] <= 1.0
    assert fl["slots"] == [slot] and fl["edges"] == [7, i]
    want_ent = {int(bt["neg"][slot]), int(bt["h"][i]), int(bt["t"][i]), int(bt["h"][7]), int(bt["t"][7])}
    assert set(fl["ent"]) == want_ent and set(fl["rel"]) == {int(bt["r"][i]), int(bt["r"][7])}
    assert set(bt["nid"][fl["pos_local"]].tolist()) == want_ent & set(bt["nid"].tolist())
    with pytest.raises(AssertionError):
        L.check_flip_caps(c, bt, fl, "planted")               # 2 flips among 4 700 pairs: over the 1e-4 cap
    if neg_deg:     # a flip in an in-batch column feeds the chunk's own corrupted-side entity (positive trace), no g_neg slot
        n32[i, j] = n64[i, j]
        n64[i, 2], n32[i, 2] = -c["margin"] - 3e-5, np.float32(-c["margin"] + 3e-5)
        fl = L.hinge_flips(c, bt, p32, n32, p64, n64)
        own = (bt["h"] if bt["neg_head"] else bt["t"])[(i // chunk) * chunk + 2]
        assert fl["slots"] == [] and int(own) in fl["ent"]
    # far from the kink is not a legitimate flip
    n64[i, j], n32[i, j] = -c["margin"] - 0.1, np.float32(-c["margin"] + 0.1)
    assert L.hinge_flips(c, bt, p32, n32, p64, n64)["worst_v"] > 1.0
