"""Input guard of the gradient-message tests (CPU): every host-planned case of tests/emit_message_cases.py through the float64 and
the float32 statement of the messages.  Asserted from the reference alone, before any GPU run:
  * the float32 statement (the oracle's own formulation and precision) meets every bound the GPU file applies - so a kernel that
    misses one is wrong, not the bound;
  * emit_message_cases.update_instance over the case table and its layouts reaches every instance launch_update can pick for an
    emitting step: update_kernel<4>, update_kernel<1> and update_kernel_reg<NIT, false, LEAN> for LEAN 0, 4, 6, 7 x NIT 1, 2, 4;
  * the planted lists are there: the hub's negative list is longer than 64 entries (the body's one-at-a-time loop) and it has a
    positive list too, the planted relation's list is at least COOP_MIN_R edges (the shared-list instance), several entities sit in
    exactly 2 and exactly 3 negative slots, and the batch has entries in both traces, only the positive and only the negative one;
  * in every case some row's sum_k mean(g_k^2) and mean((sum_k g_k)^2) are more than 10 bounds apart - the GPU comparison tells the
    two meanings of a summed increment apart;
  * the --neg_deg_sample flag, the regulariser and the edge weights move the messages by more than their bound.
The two device-planned cases get their ids on the GPU (kge_sample_batches); here only their geometry is checked.
"""
import numpy as np
import pytest

import emit_message_cases as E

HOST = [c for c in E.CASES if not c["device_plan"]]


def _ids(cs):
    return [c["id"] for c in cs]


@pytest.mark.parametrize("c", HOST, ids=_ids(HOST))
def test_float32_statement_stays_inside_every_bound(c):
    ent, rel, proj = E.tables(c)
    bt = E.host_ids(c)
    r64 = E.messages(c, ent, rel, proj, bt, np.float64)
    r32 = E.messages(c, ent, rel, proj, bt, np.float32)
    assert r32["g1"].dtype == np.float32 and r64["g1"].dtype == np.float64
    assert all(np.isfinite(v).all() for v in r64.values()), c["id"]
    excl = E.exclusions(c, ent, rel, bt)
    for k, (ratio, err, bound) in E.message_errors(r32, r64, excl).items():
        assert ratio <= 1.0, "%s %s: the float32 statement is %.2f bounds (%.3e, bound %.3e) from the float64 one" % (c["id"], k, ratio, err, bound)
    # a row without a list carries exact zeros, a row with one a non-zero increment
    for g, gs, n in (("g0", "gs0", "n_pos"), ("g1", "gs1", "n_neg")):
        assert not r64[g][r64[n] == 0].any() and not r64[gs][r64[n] == 0].any() and (r64[gs][r64[n] > 0] > 0).all(), c["id"]


@pytest.mark.parametrize("c", HOST, ids=_ids(HOST))
def test_planted_lists_and_trace_membership(c):
    bt = E.host_ids(c)
    ue_id, ur_id = E.union(bt)
    assert 64 <= c["B"] <= 128 and c["chunk"] in (16, 32) and 16 <= c["N"] <= 32 and c["n_ent"] <= 400 and c["n_rel"] <= 8
    cnt = np.bincount(bt["neg"], minlength=c["n_ent"])
    in_pos = np.zeros(c["n_ent"], bool)
    in_pos[bt["nid"]] = True
    assert cnt[E.HUB] >= 66 and cnt[E.HUB] > E.LONG_LIST and in_pos[E.HUB], "the hub's list does not reach the loop from i = 64"
    assert all(cnt[x] == 2 for x in E.TWOS) and all(cnt[x] == 3 for x in E.THREES)
    assert in_pos[E.TWOS[0]] and not in_pos[E.TWOS[1]]
    nit = int(E.update_instance(c)[-1]) if E.update_instance(c).startswith("reg") else 1
    assert int((bt["r"] == E.PLANTED_REL).sum()) >= max(13, E.COOP_MIN_R[nit])
    assert (in_pos & (cnt > 0)).sum() >= 2 and (in_pos & (cnt == 0)).any() and (~in_pos & (cnt > 0)).any()
    assert not (bt["h"] == bt["t"]).any()
    assert len(ue_id) > 4 * 4, "one workgroup (four wavefronts) would cover every entity row"


def test_cases_reach_every_update_instance_and_option():
    reached = {E.instance_of(c, lay) for c in E.CASES for lay in E.layouts_of(c)}
    assert reached == set(E.INSTANCES), "missing %r, unexpected %r" % (set(E.INSTANCES) - reached, reached - set(E.INSTANCES))
    for c in E.CASES:
        assert c["id"].endswith(c["instance"]) and c["instance"] == E.instance_of(c, E.layouts_of(c)[0])
    ids = [c["id"] for c in E.CASES]
    assert len(set(ids)) == len(ids)
    assert {"TransE_l2", "TransE_l1", "DistMult", "ComplEx", "RotatE", "TransR", "RESCAL"} == {c["model"] for c in E.CASES}
    assert {c["neg_head"] for c in E.CASES} == {False, True}
    assert any(c["reg_norm"] == 2 and c["reg_coef"] > 0 for c in E.CASES) and any(c["reg_norm"] == 3 and c["reg_coef"] > 0 for c in E.CASES)
    assert any(c["neg_deg"] for c in E.CASES) and any(c["impts"] for c in E.CASES) and any(c["device_plan"] for c in E.CASES)
    assert {16, 320, 768, 1028, 30, 18} <= {c["d_e"] for c in E.CASES}
    assert all(c["d_r"] == c["d_e"] // 2 for c in E.CASES if c["model"] == "RotatE")
    # every layout on the NIT 1 body, a wide body and both generic kernels; the packed layout exists on the body alone
    for lay in E.LAYOUTS:
        inst = {E.instance_of(c, lay) for c in E.CASES if lay in E.layouts_of(c)}
        assert any(i.endswith("nit1") for i in inst) and any(i.endswith("nit4") for i in inst) and {"generic4", "generic1"} <= inst, lay
    assert [E.packed_supported(c) for c in E.CASES if c["d_e"] in (1028, 30, 18)] == [False, False, False]
    assert all(E.layouts_of(c) == ("dense_rel_inplace",) for c in E.CASES if c["model"] in ("TransR", "RESCAL"))
    # a device-built plan bounds its unique relations by B: more rows than the graph has relations
    assert all(c["B"] > c["n_rel"] for c in E.CASES if c["device_plan"])


@pytest.mark.parametrize("c", HOST, ids=_ids(HOST))
def test_the_two_meanings_of_a_summed_increment_are_bounds_apart(c):
    ent, rel, proj = E.tables(c)
    gap = E.meaning_gap(E.messages(c, ent, rel, proj, E.host_ids(c)))
    # the negative trace (the hub's list) in every case; the relation trace where the per-edge rows of a relation are correlated
    assert gap["gs1"] > 10.0, "%s: sum of means and mean of the squared sum are only %.2f bounds apart" % (c["id"], gap["gs1"])
    assert max(gap.values()) > 10.0


def _moved(c, other, quantities):
    ent, rel, proj = E.tables(c)
    bt = E.host_ids(c)
    a, b = E.messages(c, ent, rel, proj, bt), E.messages(other, ent, rel, proj, bt)
    bd = E.bounds(a)
    return {k: float((np.abs(a[k] - b[k]) / np.maximum(bd[k], 1e-300)).max()) for k in quantities}


@pytest.mark.parametrize("c", [c for c in HOST if c["neg_deg"] or c["reg_coef"] > 0 or c["impts"]],
                         ids=_ids([c for c in HOST if c["neg_deg"] or c["reg_coef"] > 0 or c["impts"]]))
def test_options_move_the_messages_by_more_than_the_bound(c):
    if c["neg_deg"]:          # the in-batch rows' gradients join the positive trace
        assert _moved(c, dict(c, neg_deg=False), ("g0",))["g0"] > 1.0
    if c["reg_coef"] > 0:
        mv = _moved(c, dict(c, reg_coef=0.0), ("g0", "g1", "gr"))
        assert min(mv.values()) > 1.0, mv
    if c["impts"]:
        ent, rel, proj = E.tables(c)
        bt = E.host_ids(c)
        a, b = E.messages(c, ent, rel, proj, bt), E.messages(c, ent, rel, proj, dict(bt, w=None))
        assert (np.abs(a["g0"] - b["g0"]) / E.bounds(a)["g0"]).max() > 1.0
