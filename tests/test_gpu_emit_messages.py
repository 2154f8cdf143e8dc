"""The gradient-emitting step's MESSAGES against float64 (cases, statement and bounds: tests/emit_message_cases.py; their inputs
are guarded on the CPU by tests/test_emit_message_inputs.py).

kge_step_grads (StepEngine.step(batch, want, emit=KgeEmit)) is run on every case in every documented layout of kge_emit:
  dense              g0 / gs0 / g1 / gs1 / gr / gsr / rid as seven dense arrays addressed by union entry, g_pos_ent asked for too;
  strided            one interleaved message [g0 | g1 | gs0 gs1 pad pad] per entity at row ue_id[u] (ent_by_id = 1) and one relation
                     message [gr | gsr | rid_lo rid_hi pad] per unique relation (ld_r = d_r + 4) - what dglke_amd/dist.py builds;
  packed             single-trace messages [g | gs | link pad pad] at the rows kge_route_build assigns (world = 3);
  dense_rel_inplace  the dense layout with gr == NULL: the relation trace is applied in place.
Every buffer is pre-filled with a NaN bit pattern.  Per case and layout: gradients and increments against the float64 statement
(bounds derived in emit_message_cases), rid words exact, every float the layout does not name still the sentinel, the entity table
and state bit-unchanged, the relation table bit-unchanged (gr given) or equal to kge_step_fused's (gr NULL), scores bit-equal to
kge_step_fused's.  The strided and packed messages are then applied to a copy of the tables (kge_adagrad_apply_packed /
kge_adagrad_apply_merged) and compared with kge_step_fused and with the float64 train_step.

Further down: kge_adagrad_apply_packed on its own against float64, and the argument contract of kge_step_grads.

emit_message_errors.txt, written next to the suite's other reports, records per case, layout and quantity the largest error next
to its bound.
"""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import emit_message_cases as E
import loss_option_cases as L
import modular_op_cases as M
from test_gpu_loss_options import _engine, _report_dir
from test_gpu_parity import DEV, _close

pytestmark = pytest.mark.gpu

SENT = 0x7FA5A5A5        # a quiet-NaN bit pattern no kernel computes
ERRORS = {}
T0 = []                  # the time this file's first test started


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """a lost GPU context fails every later call: end the session instead of running the rest of the file against it"""
    T0.append(time.time()) if not T0 else None
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU context is lost (%s): nothing more is run" % (e,), returncode=3)


def _record(case, layout, note="", **q):
    rec = ERRORS.setdefault((case, layout), dict(q={}, note=""))
    rec["q"].update(q)
    rec["note"] = note or rec["note"]
    try:
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "emit_message_errors.txt"), "w") as f:
            f.write("gradient messages of kge_step_grads against float64: largest |error| / bound per case, layout and quantity (<= 1 passes), "
                    "that error, its bound\n(wall time of this file up to the last record: %.0f s)\n" % (time.time() - T0[0]))
            for (cs, lay) in sorted(ERRORS):
                r = ERRORS[(cs, lay)]
                f.write("%-44s %-18s %s\n" % (cs, lay, r["note"]))
                for k in sorted(r["q"]):
                    f.write("    %-14s err/bound %8.4f   err %.3e   bound %.3e\n" % ((k,) + tuple(r["q"][k])))
    except OSError:
        pass


def _sent(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device=DEV)


def _np(t):
    return t.cpu().numpy()


def _f(a):
    """int32 words read as floats"""
    return np.ascontiguousarray(a).view(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(errs, tag):
    for k, (ratio, err, bound) in errs.items():
        assert ratio <= 1.0, "%s %s: %.2f bounds off (error %.3e, bound %.3e)" % (tag, k, ratio, err, bound)


# --------------------------------------------------------------------------------------------------------------------------
# per case: the batch, the float64 statement, the fused step and the float64 train step - computed once, shared by the layouts
# --------------------------------------------------------------------------------------------------------------------------
_SHARED = {}


def _device_batch(c):
    """a plan built by kge_sample_batches on a small graph: UE / UR are bounds, the counts live on the device"""
    from dglke_amd.dataloader import DeviceSampler
    rng = np.random.RandomState(c["seed"])
    n = 2000
    h, t = rng.randint(0, c["n_ent"], n), rng.randint(0, c["n_ent"], n)
    t = np.where(h == t, (t + 1) % c["n_ent"], t)
    smp = DeviceSampler(h, rng.randint(0, c["n_rel"], n), t, c["n_ent"], c["B"], c["N"], DEV, n_slots=2, neg_chunk_size=c["chunk"], seed=c["seed"])
    b = smp.sample()[0]
    torch.cuda.synchronize()
    a = smp.slot_arrays(0)
    bt = E.ids_dict(c, a["h_gid"], a["t_gid"], a["rel_ids"], a["neg_ids"], b.neg_head)
    ue_id, ur_id = E.union(bt)
    assert np.array_equal(a["ue_id"][:a["counts"][0]], ue_id) and np.array_equal(a["ur_id"][:a["counts"][1]], ur_id)
    assert b.UE > len(ue_id) and b.UR > len(ur_id), "the bounds of a device-built plan do not exceed its counts"
    return b, bt


def _shared(c):
    if c["id"] in _SHARED:
        return _SHARED[c["id"]]
    while len(_SHARED) >= 2:
        _SHARED.pop(next(iter(_SHARED)))
    from dglke_amd import plan
    if c["device_plan"]:
        b, bt = _device_batch(c)
    else:
        bt = E.host_ids(c)
        b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV, bt["w"])
    ent, rel, proj = E.tables(c)
    ref = E.messages(c, ent, rel, proj, bt)
    excl = E.exclusions(c, ent, rel, bt)
    # kge_step_fused on the same batch
    fe = _engine(c, c["flags"])
    Np = c["N"] + (c["chunk"] if c["neg_deg"] else 0)
    want = dict(pos_score=torch.empty(c["B"], device=DEV), neg_score=torch.empty(b.C, c["chunk"], Np, device=DEV))
    fe.step(b, want)
    torch.cuda.synchronize()
    fused = dict(ent=fe.ent.clone(), ent_state=fe.ent_state.clone(), rel=fe.rel.clone(), rel_state=fe.rel_state.clone(),
                 pos_score=want["pos_score"].clone(), neg_score=want["neg_score"].clone())
    # the float64 train step
    t64 = dict(ent=ent.astype(np.float64), es=np.zeros(len(ent)), rel=rel.astype(np.float64), rs=np.zeros(len(rel)),
               proj=None if proj is None else proj.astype(np.float64), ps=None if proj is None else np.zeros(len(proj)))
    L.oracle_step(c, t64["ent"], t64["es"], t64["rel"], t64["rs"], t64["proj"], t64["ps"], bt)
    excl_tab = dict(ent=[], rel=[])
    if c["model"] == "TransE_l1":
        excl_tab = dict(ent=ref["ue_id"][excl["ent"]].tolist(), rel=ref["ur_id"][excl["rel"]].tolist())
        M.check_row_cap(excl_tab["ent"], c["n_ent"], c["id"] + " entity table")
    _SHARED[c["id"]] = dict(b=b, bt=bt, ref=ref, excl=excl, fused=fused, t64=t64, excl_tab=excl_tab)
    return _SHARED[c["id"]]


# --------------------------------------------------------------------------------------------------------------------------
# layouts: buffers, the kge_emit that points into them, and how to read the messages back
# --------------------------------------------------------------------------------------------------------------------------
def _route(c, b, ref, world=3):
    """kge_route_build with packed message rows (ue_msg) and the numpy statement of its two words per union entry"""
    from dglke_amd import dist as kd
    ue = ref["ue_id"]
    per = (c["n_ent"] + world - 1) // world
    owner = np.minimum(ue // per, world - 1)
    both = (ref["n_pos"] > 0) & (ref["n_neg"] > 0)
    cap = int(np.bincount(owner, minlength=world).max()) + 3
    cap2 = int(np.bincount(owner[both], minlength=world).max()) + 2
    bf = type("S", (), {})()
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=DEV)
    bf.req_ids, bf.h_loc, bf.t_loc, bf.neg_loc = z(world * cap, torch.int64), z(b.B, torch.int64), z(b.B, torch.int64), z(b.C * b.N, torch.int64)
    bf.ue_loc, bf.ue_rec_loc, bf.overflow, bf.ue_msg = z(b.UE, torch.int64), z(b.UE * 8, torch.int32), z(1, torch.int32), z(b.UE * 2, torch.int32)
    lb = kd.HipOps().route(b, world, per, cap, bf, cap2=cap2)
    torch.cuda.synchronize()
    assert int(bf.overflow.item()) == 0
    start = np.searchsorted(owner, np.arange(world + 1))
    pos = np.arange(len(ue)) - start[owner]
    rank = np.zeros(len(ue), np.int64)
    for o in range(world):
        m = owner == o
        rank[m] = np.cumsum(both[m]) - both[m]
    capT = cap + cap2
    got = _np(bf.ue_msg).reshape(-1, 2)[:len(ue)]
    assert np.array_equal(got[:, 0], owner * capT + pos) and np.array_equal(got[:, 1], np.where(both, rank, -1))
    assert both.sum() >= 2 and (both & (rank > 0)).any(), "no bucket with two both-trace rows"
    return dict(bf=bf, lb=lb, world=world, per=per, cap=cap, cap2=cap2, capT=capT, owner=owner, pos=pos, rank=rank, both=both)


def _layout(c, lay, b, ref):
    """(kge_emit, {name: int32 sentinel buffer}, route or None)"""
    from dglke_amd import _lib
    d_e, d_r = c["d_e"], c["d_r"]
    em = _lib.KgeEmit()
    bufs, route = {}, None
    rows_e, rows_r = b.UE + 2, b.UR + 2
    if lay in ("dense", "dense_rel_inplace", "packed"):
        bufs.update(g0=_sent(rows_e, d_e), gs0=_sent(rows_e), g1=_sent(rows_e, d_e), gs1=_sent(rows_e))
        em.g0, em.gs0, em.g1, em.gs1 = (bufs[k].data_ptr() for k in ("g0", "gs0", "g1", "gs1"))
    if lay == "dense":
        bufs.update(gr=_sent(rows_r, d_r), gsr=_sent(rows_r), rid=_sent(rows_r, d_r))
        em.gr, em.gsr, em.rid = bufs["gr"].data_ptr(), bufs["gsr"].data_ptr(), bufs["rid"].data_ptr()
    if lay in ("strided", "packed"):
        bufs["rel_msg"] = _sent(rows_r, d_r + 4)
        r0 = bufs["rel_msg"].data_ptr()
        em.gr, em.gsr, em.rid, em.ld_r = r0, r0 + 4 * d_r, r0 + 4 * d_r + 4, d_r + 4
    if lay == "strided":
        bufs["ent_msg"] = _sent(c["n_ent"] + 2, 2 * d_e + 4)
        e0 = bufs["ent_msg"].data_ptr()
        em.g0, em.g1, em.gs0, em.gs1 = e0, e0 + 4 * d_e, e0 + 8 * d_e, e0 + 8 * d_e + 4
        em.ld_e, em.ent_by_id = 2 * d_e + 4, 1
    if lay == "packed":
        route = _route(c, b, ref)
        bufs["ent_msg"] = _sent(route["world"] * route["capT"] + 1, d_e + 4)       # (+ the dump row of an entry that does not fit: never written here)
        em.g0, em.ld_e = bufs["ent_msg"].data_ptr(), d_e + 4
        em.msg_rows, em.msg_cap, em.msg_cap_extra = route["bf"].ue_msg.data_ptr(), route["cap"], route["cap2"]
    return em, bufs, route


def _read(c, lay, b, ref, bufs, route, tag):
    """the messages as arrays by union entry / unique relation, after asserting that every word the layout does not name still
    holds the sentinel (and the exact words: rid, link, pad ids)"""
    d_e, d_r = c["d_e"], c["d_r"]
    UE, UR = len(ref["ue_id"]), len(ref["ur_id"])
    host = {k: _np(v).copy() for k, v in bufs.items()}
    named = {k: np.zeros(v.shape, bool) for k, v in host.items()}
    got = {}
    lo, hi = (ref["ur_id"] & 0xFFFFFFFF).astype(np.uint32).view(np.int32), (ref["ur_id"] >> 32).astype(np.int32)
    if lay in ("dense", "dense_rel_inplace"):
        for k in ("g0", "gs0", "g1", "gs1"):
            named[k][:UE] = True
            got[k] = _f(host[k][:UE])
    if lay == "dense":
        named["gr"][:UR] = named["gsr"][:UR] = True
        named["rid"][:UR, :2] = True
        got.update(gr=_f(host["gr"][:UR]), gsr=_f(host["gsr"][:UR]))
        assert np.array_equal(host["rid"][:UR, 0], lo) and np.array_equal(host["rid"][:UR, 1], hi), tag + ": rid"
        if c["device_plan"]:
            named["rid"][UR:b.UR, :2] = True
            assert (host["rid"][UR:b.UR, :2] == -1).all(), tag + ": pad relation rows of a device-built plan do not hold id -1"
    if lay in ("strided", "packed"):
        rm = host["rel_msg"]
        named["rel_msg"][:UR, :d_r + 3] = True
        got.update(gr=_f(rm[:UR, :d_r]), gsr=_f(rm[:UR, d_r]))
        assert np.array_equal(rm[:UR, d_r + 1], lo) and np.array_equal(rm[:UR, d_r + 2], hi), tag + ": rid"
        if c["device_plan"]:
            named["rel_msg"][UR:b.UR, d_r + 1:d_r + 3] = True
            assert (rm[UR:b.UR, d_r + 1:d_r + 3] == -1).all(), tag + ": pad relation rows of a device-built plan do not hold id -1"
    if lay == "strided":
        em_ = host["ent_msg"]
        rows = ref["ue_id"]
        named["ent_msg"][rows, :2 * d_e + 2] = True
        got.update(g0=_f(em_[rows, :d_e]), g1=_f(em_[rows, d_e:2 * d_e]), gs0=_f(em_[rows, 2 * d_e]), gs1=_f(em_[rows, 2 * d_e + 1]))
    if lay == "packed":
        em_ = host["ent_msg"]
        r, capT, cap = route, route["capT"], route["cap"]
        mr0 = r["owner"] * capT + r["pos"]
        mr1 = r["owner"] * capT + cap + r["rank"]
        has_pos, both = ref["n_pos"] > 0, r["both"]
        named["ent_msg"][mr0, :d_e + 2] = True
        named["ent_msg"][mr1[both], :d_e + 2] = True
        # a row with a positive list carries its positive trace and the link, any other row its negative trace and link -1
        assert np.array_equal(em_[mr0, d_e + 1], np.where(both, r["rank"], -1)), tag + ": link words"
        assert (em_[mr1[both], d_e + 1] == -1).all(), tag + ": the header of a second message is not {gs1, -1}"
        first_g, first_gs = _f(em_[mr0, :d_e]), _f(em_[mr0, d_e])
        got.update(g0=np.where(has_pos[:, None], first_g, 0.0), gs0=np.where(has_pos, first_gs, 0.0),
                   g1=np.where(has_pos[:, None], 0.0, first_g), gs1=np.where(has_pos, 0.0, first_gs))
        got["g1"][both], got["gs1"][both] = _f(em_[mr1[both], :d_e]), _f(em_[mr1[both], d_e])
        # (a positive-only row has no negative trace anywhere: its g1 / gs1 of the statement are exact zeros)
        assert not ref["gs1"][has_pos & ~both].any()
    for k in host:
        assert (host[k][~named[k]] == SENT).all(), "%s: %d words of %s outside the documented layout were written" % (
            tag, int((host[k][~named[k]] != SENT).sum()), k)
    return got


LAYOUT_CASES = [pytest.param(c, lay, id="%s-%s-%s" % (c["id"], lay, E.instance_of(c, lay))) for c in E.CASES for lay in E.layouts_of(c)]


@pytest.mark.parametrize("c,lay", LAYOUT_CASES)
def test_messages_match_the_float64_statement(c, lay):
    from dglke_amd import _lib
    sh = _shared(c)
    b, bt, ref, excl, fused, t64 = sh["b"], sh["bt"], sh["ref"], sh["excl"], sh["fused"], sh["t64"]
    tag = "%s %s" % (c["id"], lay)
    eng = _engine(c, c["flags"])
    before = dict(ent=eng.ent.clone(), ent_state=eng.ent_state.clone(), rel=eng.rel.clone(), rel_state=eng.rel_state.clone())
    em, bufs, route = _layout(c, lay, b, ref)
    Np = c["N"] + (c["chunk"] if c["neg_deg"] else 0)
    want = dict(pos_score=torch.empty(c["B"], device=DEV), neg_score=torch.empty(b.C, c["chunk"], Np, device=DEV))
    if lay in ("dense", "dense_rel_inplace"):
        bufs["g_pos_ent"] = _sent(b.UE + 2, c["d_e"])
        want["g_pos_ent"] = bufs["g_pos_ent"].view(torch.float32)
    if lay == "packed" and not E.packed_supported(c):
        # the generic update kernel knows the two-trace layouts only: refused before anything is launched, nothing written
        with pytest.raises(_lib.KgeError, match="multiples of 4 and at most 1024"):
            eng.step(b, want, emit=em)
        torch.cuda.synchronize()
        assert _lib.lib().kge_last_error()
        assert all((_np(v) == SENT).all() for v in bufs.values()), tag + ": a refused call wrote messages"
        assert all(_bits_equal(getattr(eng, k), before[k]) for k in before), tag + ": a refused call changed a table"
        _record(c["id"], lay, "refused (KGE_ERR_ARG): packed messages at a width of the generic update kernel")
        return
    eng.step(b, want, emit=em)
    torch.cuda.synchronize()
    g_pos_ent = bufs.pop("g_pos_ent", None)
    got = _read(c, lay, b, ref, bufs, route, tag)
    assert all(np.isfinite(v).all() for v in got.values()), tag + ": non-finite message"
    errs = E.message_errors(got, ref, excl)
    UE = len(ref["ue_id"])
    if g_pos_ent is not None:      # out->g_pos_ent next to a dense emit: the same rows as g0, nothing beyond the bound
        gp = _np(g_pos_ent)
        assert np.array_equal(gp[:UE], _np(bufs["g0"])[:UE]) and (gp[b.UE:] == SENT).all(), tag + ": g_pos_ent is not g0"
    note = "%s; hub list %d, longest relation list %d" % (E.instance_of(c, lay), int(ref["n_neg"].max()), int(ref["n_rel"].max()))
    if c["model"] == "TransE_l1":
        note += "; %d + %d sign-ambiguous message rows excluded" % (len(excl["ent"]), len(excl["rel"]))
    # ---- the tables: the entity side never changes; the relation side only when its trace is applied in place
    assert _bits_equal(eng.ent, before["ent"]) and _bits_equal(eng.ent_state, before["ent_state"]), tag + ": the entity table changed"
    if lay != "dense_rel_inplace":
        assert _bits_equal(eng.rel, before["rel"]) and _bits_equal(eng.rel_state, before["rel_state"]), tag + ": the relation table changed"
    else:
        assert not _bits_equal(eng.rel, before["rel"]), tag + ": the relation trace was not applied"
        same = E.instance_of(c, lay).startswith(("generic", "reg0")) or c["model"] in ("RESCAL", "TransR")
        if same:      # the fused step runs the same update instance: bit for bit
            assert _bits_equal(eng.rel, fused["rel"]) and _bits_equal(eng.rel_state, fused["rel_state"]), tag + ": relation table vs kge_step_fused"
        else:
            _close(eng.rel.cpu(), fused["rel"].cpu(), 1e-5, 5e-6, tag + " relation table vs kge_step_fused")
            _close(eng.rel_state.cpu(), fused["rel_state"].cpu(), 1e-5, 1e-8, tag + " relation state vs kge_step_fused")
        note += "; relation table %s kge_step_fused" % ("bit-equal to" if same else "within 1e-5 of")
    assert _bits_equal(want["pos_score"], fused["pos_score"]) and _bits_equal(want["neg_score"], fused["neg_score"]), tag + ": scores vs kge_step_fused"
    # ---- composition: the messages applied on a copy of the tables
    if lay in ("strided", "packed"):
        errs.update(_compose(c, lay, b, ref, bufs, route, before, fused, t64, sh["excl_tab"], tag))
    _record(c["id"], lay, note, **errs)
    _check(errs, tag)


def _apply_packed(table, state, idx, msg, ld, n, T, lr):
    from dglke_amd import _lib
    _lib.check(_lib.lib().kge_adagrad_apply_packed(_lib.ptr(table), _lib.ptr(state), table.shape[0], table.shape[1],
                                                   None if idx is None else _lib.ptr(idx), _lib.ptr(msg), int(ld), int(n), int(T), float(lr),
                                                   1e-10, _lib.stream_ptr()))


def _compose(c, lay, b, ref, bufs, route, before, fused, t64, excl_tab, tag):
    """strided: kge_adagrad_apply_packed (T = 2 with idx; the relation message with the ids inside).  packed: kge_adagrad_apply_merged
    with cap_extra = cap2, one source per owner bucket.  Against kge_step_fused (the world-1 engine test's tolerances) and the
    float64 train step (the suite's row tolerance)."""
    from dglke_amd import dist as kd
    d_e, d_r, lr = c["d_e"], c["d_r"], c["lr"]
    ent, es, rel, rs = (before[k].clone() for k in ("ent", "ent_state", "rel", "rel_state"))
    fl = lambda t: t.view(torch.float32)
    if lay == "strided":
        ue = _dev(ref["ue_id"])
        _apply_packed(ent, es, ue, fl(bufs["ent_msg"])[ue].contiguous(), 2 * d_e + 4, len(ref["ue_id"]), 2, lr)
    else:
        r = route
        for o in range(r["world"]):
            lo, hi = o * r["per"], min((o + 1) * r["per"], c["n_ent"])
            kd.HipOps().apply_merged(ent[lo:hi], es[lo:hi], 1, r["cap"], r["bf"].req_ids[o * r["cap"]:(o + 1) * r["cap"]], lo,
                                     fl(bufs["ent_msg"])[o * r["capT"]:(o + 1) * r["capT"]], 1, lr, cap_extra=r["cap2"])
    # (device-built plans: the pad rows with id -1 are part of the call)
    n_rel_msg = b.UR if c["device_plan"] else len(ref["ur_id"])
    _apply_packed(rel, rs, None, fl(bufs["rel_msg"]), d_r + 4, n_rel_msg, 1, lr)
    torch.cuda.synchronize()
    for got_t, k, rt, at in ((ent, "ent", 1e-5, 5e-6), (es, "ent_state", 1e-5, 1e-8), (rel, "rel", 1e-5, 5e-6), (rs, "rel_state", 1e-5, 1e-8)):
        _close(got_t.cpu(), fused[k].cpu(), rt, at, "%s applied %s vs kge_step_fused" % (tag, k))
    touched = np.zeros(c["n_ent"], bool)
    touched[ref["ue_id"]] = True
    assert _bits_equal(ent[_dev(~touched)], before["ent"][_dev(~touched)]), tag + ": a row outside the batch changed"
    res = {}
    for got_t, want64, rows, name, bound in ((ent, t64["ent"], excl_tab["ent"], "applied_ent", c["rows"] * lr + 1e-4 * np.abs(t64["ent"])),
                                             (es, t64["es"], excl_tab["ent"], "applied_es", 1e-9 + 2e-3 * np.abs(t64["es"])),
                                             (rel, t64["rel"], excl_tab["rel"], "applied_rel", c["rows"] * lr + 1e-4 * np.abs(t64["rel"])),
                                             (rs, t64["rs"], excl_tab["rel"], "applied_rs", 1e-9 + 2e-3 * np.abs(t64["rs"]))):
        res[name] = M.worst(M.masked(_np(got_t), want64, rows), want64, bound)
    return res


# --------------------------------------------------------------------------------------------------------------------------
# kge_adagrad_apply_packed on its own
# --------------------------------------------------------------------------------------------------------------------------
def _packed_reference(table, state, ids, g, gs, lr, eps=1e-10):
    """float64, sequential: trace t of message k: inc == 0 -> skipped; s += inc; row += -lr g_t / (sqrt(s) + eps)"""
    t64, s64 = table.astype(np.float64), state.astype(np.float64)
    for k, i in enumerate(ids):
        if i < 0:
            continue
        for t in range(g.shape[1]):
            if gs[k, t] == 0.0:
                continue
            s64[i] += np.float64(gs[k, t])
            t64[i] += -lr * g[k, t].astype(np.float64) / (np.sqrt(s64[i]) + eps)
    return t64, s64


def run_apply_packed_case(dim, T, inside):
    """the body of test_adagrad_apply_packed_matches_float64_and_skips; -> table and state, by ld"""
    res = {}
    rng = np.random.RandomState(M._seed("packed", dim, T, inside))
    n_tab, n, lr = 700, 500, 0.3
    need = T * dim + T + (2 if inside else 0)
    for ld in ((need + 3) // 4 * 4, (need + 3) // 4 * 4 + 1):
        table = rng.uniform(-0.1, 0.1, (n_tab, dim)).astype(np.float32)
        state = (rng.rand(n_tab) * 1e-3).astype(np.float32)
        ids = rng.permutation(n_tab)[:n].astype(np.int64)
        drop = rng.rand(n) < 0.1
        ids_in = np.where(drop, -1, ids)
        g = (rng.randn(n, T, dim) * 0.01).astype(np.float32)
        gs = (g.astype(np.float64) ** 2).mean(2).astype(np.float32)
        zero = rng.rand(n, T) < 0.15
        zero[:20, 0] = True                                  # (their gradient rows stay non-zero: the skip is what keeps the row)
        zero[:20, T - 1] = T == 1
        gs[zero] = 0.0
        msg = np.full((n, ld), SENT, np.int32)
        msg[:, :T * dim] = g.reshape(n, T * dim).view(np.int32)
        msg[:, T * dim:T * dim + T] = gs.view(np.int32)
        if inside:
            msg[:, T * dim + T] = (ids_in & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
            msg[:, T * dim + T + 1] = (ids_in >> 32).astype(np.int32)
        t_d, s_d = _dev(table), _dev(state)
        _apply_packed(t_d, s_d, None if inside else _dev(ids_in), _dev(msg).view(torch.float32), ld, n, T, lr)
        torch.cuda.synchronize()
        t64, s64 = _packed_reference(table, state, ids_in, g, gs, lr)
        got_t, got_s = _np(t_d), _np(s_d)
        applied = ~drop & ~zero.all(1)
        skipped = np.ones(n_tab, bool)
        skipped[ids[applied]] = False
        assert drop.sum() > 20 and (zero[:, 0] & ~zero.all(1) & ~drop).sum() >= (10 if T > 1 else 0)
        assert np.array_equal(got_t[skipped], table[skipped]) and np.array_equal(got_s[skipped], state[skipped]), "a skipped row changed"
        assert (got_t[ids[applied]] != table[ids[applied]]).any(1).all(), "an applied row did not move"
        errs = dict(state=M.worst(got_s, s64, 1e-7 + 1e-5 * np.abs(s64)), table=M.worst(got_t, t64, 1e-5 + 1e-5 * np.abs(t64)))
        _record("apply_packed dim=%d T=%d %s" % (dim, T, "ids inside" if inside else "idx"), "ld=%d" % ld,
                "%d negative ids, %d zero-increment traces" % (drop.sum(), zero.sum()), **errs)
        _check(errs, "apply_packed dim %d T %d ld %d" % (dim, T, ld))
        res.update({"table ld%d" % ld: t_d, "state ld%d" % ld: s_d})
    return res


@pytest.mark.parametrize("inside", [False, True], ids=["idx", "ids_inside"])
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("dim", [8, 30, 1028])
def test_adagrad_apply_packed_matches_float64_and_skips(dim, T, inside):
    """msg = [g_0 | .. | g_{T-1} | gs_0 .. gs_{T-1} | (id_lo id_hi)]: the T traces in order, ids from idx or from the message, negative
    ids skipped (row and state bit-unchanged), a trace with increment exactly 0 skipped while the later traces of the row are applied.
    Twice per case: an ld that is a multiple of 4 (dim 8 / 1028: the 16-byte instance) and one that is not (the scalar instance, as
    for dim 30).  Bounds of test_adagrad_apply_rows_matches_float64_and_skips.  Ids at or above 2^31 are out of scope: a table with
    that many rows does not fit this test (the id is read as two int32 words and widened, see apply_packed_kernel)."""
    run_apply_packed_case(dim, T, inside)


def test_adagrad_apply_packed_argument_errors():
    from dglke_amd import _lib
    f = _lib.lib().kge_adagrad_apply_packed
    t, s, m, i = (torch.zeros(n, device=DEV) for n in (64, 8, 64, 1))
    i = torch.zeros(4, dtype=torch.int64, device=DEV)
    tp, sp, mp, ip, st = t.data_ptr(), s.data_ptr(), m.data_ptr(), i.data_ptr(), _lib.stream_ptr()
    for args in ((None, sp, 8, 8, ip, mp, 12, 4, 1), (tp, None, 8, 8, ip, mp, 12, 4, 1), (tp, sp, 8, 8, ip, None, 12, 4, 1),
                 (tp, sp, 8, 0, ip, mp, 12, 4, 1), (tp, sp, -1, 8, ip, mp, 12, 4, 1), (tp, sp, 8, 8, ip, mp, 12, 4, 0),
                 (tp, sp, 8, 8, ip, mp, 8, 4, 1),             # ld < T * dim + T
                 (tp, sp, 8, 8, None, mp, 10, 4, 1),          # ids inside the message: two more words
                 (tp, sp, 8, 8, ip, mp, 17, 4, 2)):           # two traces
        assert f(*(args + (0.1, 1e-10, st))) == -1 and _lib.lib().kge_last_error(), args
    assert f(tp, sp, 8, 8, ip, None, 12, 0, 1, 0.1, 1e-10, st) == 0          # nothing to apply: no message pointer needed
    torch.cuda.synchronize()
    assert not t.any() and not s.any()


# --------------------------------------------------------------------------------------------------------------------------
# the argument contract of kge_step_grads: one call per `fail` of its path, nothing launched
# --------------------------------------------------------------------------------------------------------------------------
def _copy(st):
    return type(st).from_buffer_copy(st)


def test_step_grads_argument_contract():
    from dglke_amd import _lib, plan
    lib = _lib.lib()
    c = E.CASES[5]                                   # DistMult, d_e = d_r = 16
    assert c["model"] == "DistMult" and c["d_e"] == 16
    bt = E.host_ids(c)
    b = plan.make_batch(bt["h"], bt["t"], bt["r"], bt["neg"], c["chunk"], c["N"], bt["neg_head"], DEV)
    eng = _engine(c, 0)
    ws = eng.workspace_for(b)
    ref = dict(ue_id=E.union(bt)[0])
    bufs = dict(g0=_sent(b.UE, 20), gs0=_sent(b.UE), g1=_sent(b.UE, 20), gs1=_sent(b.UE), gr=_sent(b.UR, 20), gsr=_sent(b.UR),
                msg_rows=torch.zeros(2 * b.UE, dtype=torch.int32, device=DEV), gp=_sent(b.UE, 16))
    em = _lib.KgeEmit()
    em.g0, em.gs0, em.g1, em.gs1, em.gr, em.gsr = (bufs[k].data_ptr() for k in ("g0", "gs0", "g1", "gs1", "gr", "gsr"))
    out = _lib.KgeStepOut()
    before = dict(ent=eng.ent.clone(), rel=eng.rel.clone())

    def call(status, text, hp=eng.hp, tb=eng.tb, kb=b.c, out=out, em=em, ws_ptr=ws.data_ptr(), ws_bytes=eng._ws_bytes):
        rc = lib.kge_step_grads(C.byref(hp) if hp is not None else None, C.byref(tb) if tb is not None else None,
                                C.byref(kb) if kb is not None else None, C.byref(out), C.byref(em) if em is not None else None, ws_ptr, ws_bytes,
                                _lib.stream_ptr())
        msg = lib.kge_last_error().decode()
        assert rc == status and msg and text in msg, (rc, msg, text)

    def emit(**kw):
        e = _copy(em)
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    def hparams(**kw):
        h = _copy(eng.hp)
        for k, v in kw.items():
            setattr(h, k, v)
        return h

    def batch(**kw):
        k_ = _copy(b.c)
        for k, v in kw.items():
            setattr(k_, k, v)
        return k_

    ARG, WSP = -1, -2
    # ---- kge_step_grads itself
    call(ARG, "emit buffers", em=None)
    call(ARG, "emit buffers", em=emit(g0=None))
    call(ARG, "emit buffers", em=emit(gs1=None))
    call(ARG, "emit buffers", em=emit(msg_rows=bufs["msg_rows"].data_ptr(), g0=None))
    call(ARG, "gr and gsr", em=emit(gsr=None))
    call(ARG, "gr and gsr", em=emit(gr=None))
    # ---- Step::setup
    call(ARG, "null argument", hp=None)
    call(ARG, "null argument", tb=None)
    call(ARG, "null argument", kb=None)
    call(ARG, "null argument", ws_ptr=None)
    call(ARG, "unknown model", hp=hparams(model=99))
    call(ARG, "RESCAL", hp=hparams(model=_lib.MODEL_IDS["RESCAL"], d_r=256))                        # relation messages for RESCAL
    call(ARG, "RESCAL", hp=hparams(model=_lib.MODEL_IDS["RESCAL"], d_r=16), em=emit(gr=None, gsr=None))      # d_r != d_e * d_e
    call(ARG, "C*chunk == B", kb=batch(chunk=c["chunk"] + 1))
    call(ARG, "C*chunk == B", kb=batch(N=0))
    call(ARG, "bad dims", hp=hparams(d_e=0))
    call(ARG, "needs d_r == d_e", hp=hparams(d_r=20))
    call(ARG, "ComplEx needs even d_e", hp=hparams(model=_lib.MODEL_IDS["ComplEx"], d_r=20))
    call(ARG, "RotatE needs d_r == d_e/2", hp=hparams(model=_lib.MODEL_IDS["RotatE"]))
    call(ARG, "TransR needs 0 < d_r <= 1024", hp=hparams(model=_lib.MODEL_IDS["TransR"], d_r=2000))
    call(ARG, "unknown loss genre", hp=hparams(loss_genre=17))
    call(ARG, "pairwise and adversarial", hp=hparams(pairwise=1, adv=1, loss_genre=_lib.LOSS_IDS["Hinge"]))
    call(ARG, "cannot be applied to pairwise", hp=hparams(pairwise=1, adv=0))
    tb = _copy(eng.tb)
    tb.ent_state = None
    call(ARG, "null table / batch pointer", tb=tb)
    call(ARG, "null table / batch pointer", kb=batch(ue_rec=None))
    call(ARG, "neg_deg_sample for RESCAL / TransR", hp=hparams(model=_lib.MODEL_IDS["TransR"], flags=E.NEG_DEG), em=emit(gr=None, gsr=None))
    call(ARG, "TransR: the gradient-emitting step needs the relation trace in place", hp=hparams(model=_lib.MODEL_IDS["TransR"]))
    call(ARG, "TransR needs kge_tables.proj", hp=hparams(model=_lib.MODEL_IDS["TransR"]), em=emit(gr=None, gsr=None))
    # ---- packed messages: the width rule (found by this file: the generic update kernel ignored msg_rows) and the geometry
    packed = dict(msg_rows=bufs["msg_rows"].data_ptr(), msg_cap=b.UE, msg_cap_extra=b.UE, ld_e=20)
    call(ARG, "multiples of 4 and at most 1024", hp=hparams(d_e=18, d_r=18), em=emit(**dict(packed, ld_e=22)))
    call(ARG, "multiples of 4 and at most 1024", hp=hparams(d_e=1028, d_r=1028), em=emit(**dict(packed, ld_e=1032)))
    call(ARG, "bucket geometry", em=emit(**dict(packed, ld_e=19)))
    call(ARG, "bucket geometry", em=emit(**dict(packed, msg_cap=0)))
    call(ARG, "bucket geometry", em=emit(**dict(packed, msg_cap_extra=0)))
    # ---- g_pos_ent next to a strided emit, or next to messages addressed by row id (the [UE, d_e] output has no such rows)
    o2 = _copy(out)
    o2.g_pos_ent = bufs["gp"].data_ptr()
    call(ARG, "g_pos_ent", out=o2, em=emit(ld_e=20))
    call(ARG, "g_pos_ent", out=o2, em=emit(ent_by_id=1))
    # ---- workspace
    call(WSP, "workspace too small", ws_bytes=1024)
    torch.cuda.synchronize()
    assert all((_np(bufs[k]) == SENT).all() for k in bufs if k != "msg_rows"), "a refused call wrote messages"
    assert _bits_equal(eng.ent, before["ent"]) and _bits_equal(eng.rel, before["rel"])
    # ... and the same structs are accepted once nothing is wrong with them
    assert lib.kge_step_grads(C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), C.byref(em), ws.data_ptr(), eng._ws_bytes,
                              _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.isfinite(_f(_np(bufs["g0"]).reshape(-1)[:len(ref["ue_id"]) * 16])).all()          # (dense rows: 16 floats apart)


def test_dist_engine_says_the_width_rule_up_front():
    """DistEngine with the library's arithmetic moves messages that kge_step_grads / kge_adagrad_apply_merged write and read for row
    widths that are multiples of 4 and at most 1024 floats only: said when the engine is built, not by the first apply"""
    from dglke_amd import _lib
    from dglke_amd import dist as kd

    class _NoComm(object):
        world, rank = 2, 0
    for d_e, d_r, ok in ((30, 30, False), (1028, 1028, False), (16, 18, False), (16, 16, True)):
        eng = type("E", (), {})()
        eng.lr, eng.rel = 0.1, torch.zeros(5, d_r, device=DEV)
        spec = kd.ShardSpec(300, 2, 0)
        mk = lambda: kd.DistEngine(eng, spec, torch.zeros(spec.n_local, d_e, device=DEV), torch.zeros(spec.n_local, device=DEV),
                                   ops=kd.HipOps(), comm=_NoComm(), cap=64)
        if ok:
            mk()
        else:
            with pytest.raises(_lib.KgeError, match="multiples of 4 and at most 1024"):
                mk()
