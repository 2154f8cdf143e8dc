"""Known triples left out of the training negatives (dglke_train --exclude_positive; include/kge_hip.h kge_known): the pair-mask
kernel against numpy set membership, the whole step against the float64 statement of tests/known_negative_cases.py (inputs guarded
on the CPU by tests/test_known_negative_inputs.py), the exact zeros, and the new entry points next to the old ones.

Tolerances of the whole-step test are those tests/test_gpu_loss_options.py applies to the same quantities (scores 1e-4 / 1e-4,
loss 1e-4 / 1e-5, gradients 3e-4 / grad_tol, states 2e-3 / 1e-9, rows 1e-4 / rows * lr): a known pair adds exact zeros, so no new
margin is due.  The hinge-flip and L1-sign exclusions of that suite apply under its own caps (loss_option_cases.FLIP_CAP, ROW_CAP)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import known_negative_cases as KN
import loss_option_cases as L
from test_gpu_parity import DEV, _close, _l1_ambiguous, _masked, grad_tol

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------------------------------------------
def _index(K, n_ent, n_rel):
    from dglke_amd.known import KnownIndex
    return KnownIndex(K, n_ent, n_rel, DEV)


def _known_struct(idx):
    from dglke_amd import _lib
    (kt, vt), (kh, vh) = idx.side(False), idx.side(True)
    k = _lib.KgeKnown()
    k.keys_tail, k.vals_tail, k.m_tail = _lib.ptr(kt), _lib.ptr(vt), kt.numel()
    k.keys_head, k.vals_head, k.m_head = _lib.ptr(kh), _lib.ptr(vh), kh.numel()
    k.n_rel = idx.n_rel
    return k


def _mask_bits(kb, k, B, N):
    """kge_known_neg_mask on a buffer pre-filled with ones -> ([B, N] bool, the bits of every row's last word beyond column N)"""
    from dglke_amd import _lib
    W = (N + 31) // 32
    assert _lib.lib().kge_known_mask_bytes(B, N) == 4 * B * W
    m = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().kge_known_neg_mask(C.byref(kb), C.byref(k), _lib.ptr(m), m.numel() * 4, _lib.stream_ptr()))
    torch.cuda.synchronize()
    words = m.cpu().numpy().view(np.uint32)
    bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, W * 32).astype(bool)
    return bits[:, :N], bits[:, N:]


def _membership(K, h, r, t, neg, neg_head, chunk, N):
    bt = dict(h=h, r=r, t=t, neg=neg, neg_head=neg_head)
    return KN.known_matrix(K, bt, chunk, N)


# --------------------------------------------------------------------------------------------------------------------------
# 1. the mask kernel
# --------------------------------------------------------------------------------------------------------------------------
MASK_ENT, MASK_REL = 500, 7


@functools.lru_cache(maxsize=None)
def _mask_graph():
    """a graph whose (entity, relation) lists are long on the tail side - 20 head entities (0 and n_ent - 1 among them), up to 300
    tails each: hub lists, so that uniform negatives hit them - and short on the head side"""
    rng = np.random.RandomState(77)
    pool = np.concatenate([[0, MASK_ENT - 1], rng.choice(np.arange(1, MASK_ENT - 1), 18, replace=False)])
    h = np.repeat(pool, MASK_REL * 300)
    r = np.tile(np.repeat(np.arange(MASK_REL), 300), len(pool))
    t = rng.randint(0, MASK_ENT, size=len(h))
    t[:300] = np.arange(300)                                # (0, 0, ?): a list of exactly 300, holding entity 0 itself
    t[-1] = MASK_ENT - 1
    k = np.unique(np.stack([h, r, t], 1), axis=0).astype(np.int64)
    return k[:, 0].copy(), k[:, 1].copy(), k[:, 2].copy()


@pytest.mark.parametrize("chunk", [1, 8])
@pytest.mark.parametrize("N", [1, 31, 33, 64, 65, 200])
def test_mask_kernel_equals_set_membership(N, chunk):
    from dglke_amd import _lib, plan
    from dglke_amd.dataloader import DeviceSampler
    K = _mask_graph()
    idx = _index(K, MASK_ENT, MASK_REL)
    k = _known_struct(idx)
    B = 3 * chunk if chunk > 1 else 5                        # more than one block of four wavefronts
    rng = np.random.RandomState(N * 10 + chunk)
    hits = 0
    # ---- host-built plans, both corruption sides (kge_batch.neg_head, counts_dev NULL)
    for neg_head in (False, True):
        sel = rng.randint(0, len(K[0]), size=B)
        h, r, t = K[0][sel].copy(), K[1][sel].copy(), K[2][sel].copy()
        neg = rng.randint(0, MASK_ENT, size=(B // chunk) * N).astype(np.int64)
        neg[0], neg[-1] = 0, MASK_ENT - 1
        h[0], r[0] = 0, 0                                     # the list of 300 (tail side)
        b = plan.make_batch(h, t, r, neg, chunk, N, neg_head, DEV)
        got, spill = _mask_bits(b.c, k, B, N)
        want = _membership(K, h, r, t, neg, neg_head, chunk, N)
        assert np.array_equal(got, want), "host plan, neg_head=%s" % neg_head
        assert not spill.any(), "bits beyond column N must be 0"
        hits += int(want.sum())
    # ---- device-built plans: the corrupt-head flag is counts_dev[2], whatever the host field says
    smp = DeviceSampler(K[0], K[1], K[2], MASK_ENT, B, N, DEV, n_slots=2, neg_chunk_size=chunk, seed=N)
    bs = smp.sample(2)
    torch.cuda.synchronize()
    for slot, b in enumerate(bs):
        a = smp.slot_arrays(slot)
        neg_head = bool(a["counts"][2])
        assert neg_head == b.neg_head == (slot == 1)
        kb = _lib.KgeBatch.from_buffer_copy(b.c)
        kb.neg_head = int(not neg_head)                      # a wrong host flag: the kernel must not read it
        got, spill = _mask_bits(kb, k, B, N)
        want = _membership(K, a["h_gid"], a["rel_ids"], a["t_gid"], a["neg_ids"], neg_head, chunk, N)
        assert np.array_equal(got, want), "device plan, slot %d" % slot
        assert not spill.any()
        hits += int(want.sum())
    assert hits > 0, "no known pair at all: the case tests nothing"


def test_mask_kernel_empty_index_and_empty_lists():
    from dglke_amd import _lib, plan
    rng = np.random.RandomState(3)
    B, chunk, N = 16, 8, 65
    h, t, r = (rng.randint(0, MASK_ENT, B).astype(np.int64), rng.randint(0, MASK_ENT, B).astype(np.int64),
               rng.randint(0, MASK_REL, B).astype(np.int64))
    neg = rng.randint(0, MASK_ENT, (B // chunk) * N).astype(np.int64)
    empty = _lib.KgeKnown()
    empty.n_rel = MASK_REL                                   # m_tail = m_head = 0, null arrays
    # every key absent: triples whose entities the batch (ids < 500 of a 1000-entity space) never names
    far = (np.arange(500, 900, dtype=np.int64), np.zeros(400, np.int64), np.arange(501, 901, dtype=np.int64))
    idx = _index(far, 1000, MASK_REL)
    for neg_head in (False, True):
        b = plan.make_batch(h, t, r, neg, chunk, N, neg_head, DEV)
        for k in (empty, _known_struct(idx)):
            got, spill = _mask_bits(b.c, k, B, N)
            assert not got.any() and not spill.any()


# --------------------------------------------------------------------------------------------------------------------------
# 2. + 3. the whole step against the float64 statement, and the exact zeros
# --------------------------------------------------------------------------------------------------------------------------
def _engine(c, flags=0):
    from dglke_amd.engine import StepEngine
    eng = StepEngine(c["model"], c["n_ent"], c["n_rel"], c["hidden"], c["gamma"], c["lr"], DEV, c["de"], c["dr"], c["adv"],
                     c["adv_temp"], c["reg_coef"], c["reg_norm"], loss_genre=c["genre"], pairwise=c["pairwise"], margin=c["margin"],
                     flags=int(flags))
    ent, rel, proj = L.tables(c)
    eng.load_tables(ent, rel)
    if proj is not None:
        eng.proj.copy_(torch.from_numpy(proj))
        eng.proj_state.zero_()
    return eng


def _batch(c, bt):
    from dglke_amd import plan
    return plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV)


def _f64(t):
    return None if t is None else t.cpu().numpy().astype(np.float64)


def _union(a, b):
    return {k: sorted(set(a[k]) | set(b[k])) for k in ("slots", "edges", "pos_local", "ent", "rel")}


@functools.lru_cache(maxsize=None)
def _run(cid):
    """two steps (tail, then head corruption) of case `cid` with the index attached; the float64 statement restarted from the GPU's
    own float32 tables each step.  Computed once, shared by the tests below and left unchanged."""
    c = [x for x in KN.CASES if x["id"] == cid][0]
    bts, K, notes = KN.build(c)
    eng = _engine(c)
    eng.attach_known(_index(K, c["n_ent"], c["n_rel"]))
    recs = []
    for bt, note in zip(bts, notes):
        ent64, rel64, es64, rs64 = _f64(eng.ent), _f64(eng.rel), _f64(eng.ent_state), _f64(eng.rel_state)
        pj64, ps64 = _f64(eng.proj), _f64(eng.proj_state)
        before = dict(ent=eng.ent.cpu().numpy().copy(), es=eng.ent_state.cpu().numpy().copy(), ent64=ent64.copy(), rel64=rel64.copy())
        b = _batch(c, bt)
        want = eng.alloc_outputs(b)
        eng.step(b, want)
        torch.cuda.synchronize()
        known = KN.known_matrix(K, bt, c["chunk"], c["N"])
        out = KN.masked_step(c, ent64, es64, rel64, rs64, pj64, ps64, bt, known)
        got = {k: v.cpu().numpy() for k, v in want.items()}
        got.update(loss4=eng.read_loss(), ue_id=b.p["ue_id"], ent=eng.ent.cpu().numpy(), es=eng.ent_state.cpu().numpy(),
                   rel=eng.rel.cpu().numpy(), rs=eng.rel_state.cpu().numpy(), proj=None if eng.proj is None else eng.proj.cpu().numpy(),
                   ps=None if eng.proj is None else eng.proj_state.cpu().numpy())
        recs.append(dict(bt=bt, note=note, known=known, out=out, got=got, before=before,
                         ref=dict(ent=ent64, es=es64, rel=rel64, rs=rs64, proj=pj64, ps=ps64)))
    return c, recs


IDS = [c["id"] for c in KN.CASES]


@pytest.mark.parametrize("cid", IDS)
def test_step_with_known_index_matches_float64_statement(cid):
    c, recs = _run(cid)
    chunk, N, lr = c["chunk"], c["N"], c["lr"]
    for step, rec in enumerate(recs, 1):
        bt, out, got, ref = rec["bt"], rec["out"], rec["got"], rec["ref"]
        tag = "%s step %d" % (cid, step)
        gp, gn = got["pos_score"], got["neg_score"]
        _close(gp, out["pos_score"], 1e-4, 1e-4, tag + " pos_score")
        _close(gn, out["neg_score"], 1e-4, 1e-4, tag + " neg_score")
        excl = dict(slots=[], edges=[], pos_local=[], ent=[], rel=[])
        fl = L.hinge_flips(c, bt, gp, gn, out["pos_score"], out["neg_score"])
        if fl is not None:
            L.check_flip_caps(c, bt, fl, tag)
            excl = _union(excl, fl)
        if c["model"] == "TransE_l1":
            e0 = rec["before"]["ent64"]
            amb = _l1_ambiguous(bt, e0, rec["before"]["rel64"], chunk, N, tau=1.1 * 2.0 ** -24 * float(max(np.abs(e0).max(), 1e-30)) * 2)
            assert len(amb["ent"]) <= 30 and len(amb["rel"]) <= 15, "too many sign-ambiguous rows to call this a comparison: %r" % amb
            excl = _union(excl, amb)
        l4 = got["loss4"]
        if c["pairwise"]:
            assert np.isnan(l4[0]) and np.isnan(l4[1])
            _close(l4[2], out["log"][2], 1e-4, 1e-5, tag + " loss")
        else:
            _close(l4[:3], out["log"][:3], 1e-4, 1e-5, tag + " loss")
        _close(l4[3], out["log"][3], 1e-3, 1e-7, tag + " reg")
        sel = np.searchsorted(got["ue_id"], bt["nid"])
        g_pos = got["g_pos_ent"][sel]
        _close(_masked(g_pos, out["g_pos_ent"], excl["pos_local"]), out["g_pos_ent"], 3e-4, grad_tol(out["g_pos_ent"]), tag + " g_pos_ent")
        _close(_masked(got["g_neg"], out["g_neg"], excl["slots"]), out["g_neg"], 3e-4, grad_tol(out["g_neg"]), tag + " g_neg")
        _close(_masked(got["g_rel"], out["g_rel"], excl["edges"]), out["g_rel"], 3e-4, grad_tol(out["g_rel"]), tag + " g_rel")
        _close(_masked(got["es"], ref["es"], excl["ent"]), ref["es"], 2e-3, 1e-9, tag + " ent state")
        _close(_masked(got["rs"], ref["rs"], excl["rel"]), ref["rs"], 2e-3, 1e-9, tag + " rel state")
        _close(_masked(got["ent"], ref["ent"], excl["ent"]), ref["ent"], 1e-4, c["rows"] * lr, tag + " entity rows")
        _close(_masked(got["rel"], ref["rel"], excl["rel"]), ref["rel"], 1e-4, c["rows"] * lr, tag + " relation rows")
        if c["model"] == "TransR":
            _close(_masked(got["ps"], ref["ps"], excl["rel"]), ref["ps"], 2e-3, 1e-9, tag + " projection state")
            _close(_masked(got["proj"], ref["proj"], excl["rel"]), ref["proj"], 1e-4, c["rows"] * lr, tag + " projection rows")


@pytest.mark.parametrize("cid", IDS)
def test_known_pairs_are_exact(cid):
    from dglke_amd import _lib
    c, recs = _run(cid)
    chunk, N, B = c["chunk"], c["N"], c["B"]
    sentinel = np.float32(_lib.KNOWN_SCORE)
    assert sentinel == np.float32(KN.KNOWN_SCORE)
    for rec in recs:
        bt, known, got, note = rec["bt"], rec["known"], rec["got"], rec["note"]
        # the sentinel exactly at the known pairs and nowhere else
        ns = got["neg_score"].reshape(B, N)
        assert np.array_equal(ns == sentinel, known)
        # nothing is NaN or Inf anywhere - the all-known row 0 under -adv included (loss4[0:2] of the pairwise form is NaN by definition)
        for k in ("pos_score", "neg_score", "g_pos_ent", "g_neg", "g_rel", "ent", "es", "rel", "rs"):
            assert np.isfinite(got[k]).all(), k
        assert np.isfinite(got["loss4"][2:]).all() and (c["pairwise"] or np.isfinite(got["loss4"][:2]).all())
        if c["reg_coef"] > 0:                                # the regulariser moves every row the batch names
            continue
        # slots whose every pair is known: gradient rows of all 0.0f
        dead = np.nonzero(known.reshape(B // chunk, chunk, N).all(1).reshape(-1))[0]
        assert note["lone_slot"] in dead
        assert (got["g_neg"][dead] == 0.0).all()
        # the entity that occurs only as a known negative keeps its row and its state bit for bit
        e = note["lone"]
        assert np.array_equal(got["ent"][e].view(np.uint32), rec["before"]["ent"][e].view(np.uint32))
        assert got["es"][e].tobytes() == rec["before"]["es"][e].tobytes()


# --------------------------------------------------------------------------------------------------------------------------
# 4. a null index through the new entries = the old entries, bit for bit
# --------------------------------------------------------------------------------------------------------------------------
def _raw_steps(c, bts, entry):
    from dglke_amd import _lib
    lib = _lib.lib()
    eng = _engine(c)
    for bt in bts:
        b = _batch(c, bt)
        ws = eng.workspace_for(b)
        out = _lib.KgeStepOut()
        out.loss_accum = _lib.ptr(eng.loss_accum)
        a = (C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(ws), eng._ws_bytes)
        s = _lib.stream_ptr()
        if entry == "fused":
            _lib.check(lib.kge_step_fused(*a, s))
        elif entry == "fused_known":
            _lib.check(lib.kge_step_fused_known(*a, None, None, None, 0, s))
        else:
            for ph in (_lib.PHASE_GATHER, _lib.PHASE_FORWARD, _lib.PHASE_BACKWARD, _lib.PHASE_UPDATE):
                if entry == "phase":
                    _lib.check(lib.kge_step_phase(*a, ph, s))
                else:
                    _lib.check(lib.kge_step_phase_known(*a, ph, None, None, 0, s))
        torch.cuda.synchronize()
    tabs = [eng.ent, eng.ent_state, eng.rel, eng.rel_state] + ([eng.proj, eng.proj_state] if eng.proj is not None else [])
    return [x.cpu().numpy().copy() for x in tabs] + [np.array(eng.read_loss_sums(), np.float32)]


@pytest.mark.parametrize("cid", ["l2-d400-n200-adv", "rotate-d32-n40-adv", "transr-12x24-n40-adv"])
def test_null_index_is_the_old_entry_bit_for_bit(cid):
    c = [x for x in KN.CASES if x["id"] == cid][0]
    bts = KN.build(c)[0]
    bts = bts + bts[:1]                                      # 3 steps
    for old, new in (("fused", "fused_known"), ("phase", "phase_known")):
        a, b = _raw_steps(c, bts, old), _raw_steps(c, bts, new)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), "%s vs %s" % (old, new)


# --------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [L.FUSED_LOSS, L.LOSS_IN_FWD, L.NEG_DEG], ids=["fused_loss", "loss_in_fwd", "neg_deg_sample"])
def test_refused_flag_combinations_leave_the_tables_alone(flag):
    from dglke_amd import _lib
    c = KN.CASES[1]
    bts, K, _ = KN.build(c)
    eng = _engine(c, flag)
    eng.attach_known(_index(K, c["n_ent"], c["n_rel"]))
    before = [x.clone() for x in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)]
    b = _batch(c, bts[0])
    with pytest.raises(_lib.KgeError) as e:
        eng.step(b)
    assert "(status -1)" in str(e.value) and "known-triple exclusion" in str(e.value)
    with pytest.raises(_lib.KgeError) as e:
        eng.step_timed(b)
    assert "(status -1)" in str(e.value)
    torch.cuda.synchronize()
    for x, y in zip(before, (eng.ent, eng.ent_state, eng.rel, eng.rel_state)):
        assert torch.equal(x, y)


def test_bad_known_arguments_are_refused():
    from dglke_amd import _lib
    lib = _lib.lib()
    c = KN.CASES[1]
    bts, K, _ = KN.build(c)
    eng = _engine(c)
    idx = _index(K, c["n_ent"], c["n_rel"])
    k = _known_struct(idx)
    b = _batch(c, bts[0])
    ws = eng.workspace_for(b)
    out = _lib.KgeStepOut()
    need = lib.kge_known_mask_bytes(b.B, b.N)
    m = torch.zeros(need, dtype=torch.uint8, device=DEV)
    before = eng.ent.clone()
    a = (C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(ws), eng._ws_bytes)
    assert lib.kge_step_fused_known(*a, None, C.byref(k), _lib.ptr(m), need - 1, _lib.stream_ptr()) == -1      # mask too small
    assert b"mask" in lib.kge_last_error()
    assert lib.kge_step_fused_known(*a, None, C.byref(k), None, need, _lib.stream_ptr()) == -1                  # no mask
    assert lib.kge_known_neg_mask(C.byref(b.c), C.byref(k), _lib.ptr(m), need - 1, _lib.stream_ptr()) == -1
    bad = _known_struct(idx)
    bad.n_rel = 0
    assert lib.kge_step_phase_known(*a, _lib.PHASE_FORWARD, C.byref(bad), _lib.ptr(m), need, _lib.stream_ptr()) == -1
    bad = _known_struct(idx)
    bad.keys_head = None
    assert lib.kge_known_neg_mask(C.byref(b.c), C.byref(bad), _lib.ptr(m), need, _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert torch.equal(before, eng.ent)
    with pytest.raises(_lib.KgeError):
        eng.attach_known(_index(K, c["n_ent"] + 1, c["n_rel"]))      # an index of another graph
    eng.attach_known(idx)
    with pytest.raises(_lib.KgeError):
        eng.step_async(b)


# --------------------------------------------------------------------------------------------------------------------------
# 6. captured path
# --------------------------------------------------------------------------------------------------------------------------
def test_captured_groups_with_device_sampler_equal_eager_steps():
    """StepEngine.capture over a device sampler with an index attached: 2 replays of [sampler launch + 4 steps] = the same 8 steps
    launched eagerly, bit for bit"""
    from dglke_amd.dataloader import DeviceSampler
    c = dict(KN.CASES[1], n_ent=MASK_ENT, n_rel=MASK_REL)
    K = _mask_graph()
    idx = _index(K, MASK_ENT, MASK_REL)
    res = []
    for captured in (True, False):
        eng = _engine(c)
        eng.attach_known(idx)
        smp = DeviceSampler(K[0], K[1], K[2], MASK_ENT, c["B"], c["N"], DEV, n_slots=4, neg_chunk_size=c["chunk"], seed=11)
        if captured:
            g = eng.capture(4, sampler=smp)
            for _ in range(2):
                g.replay()
                smp.host_step += 4
        else:
            for _ in range(2):
                for b in smp.sample(4):
                    eng.step(b)
        torch.cuda.synchronize()
        res.append([x.cpu().numpy().copy() for x in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)] +
                   [np.array(eng.read_loss_sums(), np.float32), smp.state.cpu().numpy().copy()])
    assert res[0][-1][1] == 9                                # both samplers stand at step 9
    for x, y in zip(*res):
        assert x.tobytes() == y.tobytes()
    assert res[0][1].max() > 0
