"""The head of the update wavefronts' chain (kge_update_body.hpp, update_head): one scalar round for the plan record, the four
device-side counts and the arguments, in front of the entity / relation branch and of both exit tests.

What can go wrong with that, and the smallest shapes that reach it:

  a count below its bound      the record of an entry in [count, bound) is loaded (the head is branch-free) but must never be
                               used.  Batches built by hand from a host plan: UE / UR enlarged, counts_dev = {UE_true, UR_true,
                               flag, longest relation list}, the pad records copies of a VALID record whose id is a row outside
                               the batch - ids and list bounds stay in range, so a wrong build updates that row and does not
                               fault.  UE_true, UR_true in {1, 4, 5}: one wavefront, a full workgroup, one past it.
  a host plan                  counts_dev null: the head reads the record in place of the counts and must select UE / UR; the same
                               batch in both forms gives the same tables bit for bit.
  the relation instance        counts[3] either side of the shared-list threshold (13, 14, 15 for rows <= 512 floats, 5, 6, 7 for
                               1024), with one relation list of exactly that length.
  the corrupt-head flag        counts[2] is in the same 16 bytes.  The update reads the corruption side from the HOST field
                               (kge_batch.neg_head; only the known-pair mask reads counts[2]), so a step whose counts[2] says the
                               opposite of the host field computes what the host field says.
  widths                       4, 252, 256, 260, 400, 512, 516, 1024: every NIT and the one-live-lane second pack.
  instances                    TransE_l2 (LEAN 3), DistMult (LEAN 2), TransE_l1 (LEAN 5), regularization_norm = 2 (generic), one
                               gradient-emitting step (kge_step_grads) and one kge_step_async group (the body inside the fused
                               forward launch).

Reference: oracle/kge_oracle.py in float64 from the same float32 tables.  Tolerance of the post-update rows: 1e-4 * lr, the floor of
the suite's bound max(1e-4 * lr, 3 x the float32 reference's own distance from float64) (DESIGN.md 3.2 "Numerics") - the distance
itself is not measured for hand-made batches, so the floor alone stands (+ 1e-6 of the largest row element: one float32 rounding of
the stored row).  Rows that are not in the batch, the pad row among them, must be unchanged bit for bit."""

import numpy as np
import pytest
import torch

from oracle import kge_oracle as O
from test_gpu_parity import DEV, grad_tol

pytestmark = pytest.mark.gpu

N_ENT, N_REL = 48, 12
OUT_ENT, OUT_REL = N_ENT - 1, N_REL - 1        # the rows the pad records name: never in a batch


def _ids(rng, B, chunk, N, ue_true=None, ur_true=None, rel_list=None, neg_head=False):
    """h, t, r, neg of one batch: entities from a pool of ue_true ids (all of them used), relations from a pool of ur_true;
    rel_list = L: relation 0 gets exactly L edges and every other relation fewer"""
    ne = ue_true if ue_true is not None else N_ENT - 1
    nr = ur_true if ur_true is not None else N_REL - 1
    Cn = B // chunk
    pool = rng.permutation(N_ENT - 1)[:ne]
    flat = pool[rng.randint(0, ne, size=2 * B + Cn * N)]
    flat[:ne] = pool                                        # every pool entity appears
    flat = flat[rng.permutation(flat.shape[0])]
    h, t, neg = flat[:B], flat[B:2 * B], flat[2 * B:]
    rpool = rng.permutation(N_REL - 1)[:nr]
    if rel_list is None:
        r = rpool[rng.randint(0, nr, size=B)]
        r[:nr] = rpool
    else:
        assert nr > 1 and rel_list <= B and (B - rel_list) <= (nr - 1) * (rel_list - 1)
        r = np.concatenate([np.full(rel_list, rpool[0]), rpool[1 + np.arange(B - rel_list) % (nr - 1)]])
    r = r[rng.permutation(B)]
    return dict(h=h.astype(np.int64), t=t.astype(np.int64), r=r.astype(np.int64), neg=neg.astype(np.int64), neg_head=bool(neg_head),
                chunk=chunk, N=N)


def _oracle_view(bt):
    nid, inv = np.unique(np.concatenate([bt["h"], bt["t"]]), return_inverse=True)
    B = bt["h"].shape[0]
    return dict(bt, nid=nid, h_local=inv[:B], t_local=inv[B:])


def _batch(bt, form, pad_e=0, pad_r=0, flag=None, maxrel=None):
    """form 'host': the plan as built.  form 'dev': UE / UR enlarged by pad_e / pad_r entries and counts_dev set; the pad records
    are copies of record 0 with the id of OUT_ENT / OUT_REL"""
    from dglke_amd import plan
    p = plan.build_plan(bt["h"], bt["t"], bt["r"], bt["neg"], bt["chunk"], bt["N"], bt["neg_head"])
    if form == "host":
        return plan.upload([p], DEV)[0], p
    ue, ur = p["UE"], p["UR"]
    longest = int(np.diff(p["ur_ptr"]).max())
    counts = np.array([ue, ur, int(bt["neg_head"]) if flag is None else flag, longest if maxrel is None else maxrel], np.int32)

    def padded(rec, n, out_id):
        rec = rec.reshape(-1, 8)
        pads = np.repeat(rec[:1], n, axis=0)
        pads[:, 0], pads[:, 1] = out_id, 0
        return np.concatenate([rec, pads]).reshape(-1)

    q = dict(p)
    q["UE"], q["UR"] = ue + pad_e, ur + pad_r
    q["ue_rec"], q["ur_rec"] = padded(p["ue_rec"], pad_e, OUT_ENT), padded(p["ur_rec"], pad_r, OUT_REL)
    q["ue_id"] = np.concatenate([p["ue_id"], np.full(pad_e, OUT_ENT, np.int64)])
    q["ur_id"] = np.concatenate([p["ur_id"], np.full(pad_r, OUT_REL, np.int64)])
    for k, n in (("ue_pos_ptr", pad_e), ("ue_neg_ptr", pad_e), ("ur_ptr", pad_r)):
        q[k] = np.concatenate([p[k], np.full(n, p[k][-1], np.int32)])
    b = plan.upload([q], DEV)[0]
    b.counts = torch.from_numpy(counts).to(DEV)             # (kept alive by the batch)
    b.c.counts_dev = b.counts.data_ptr()
    return b, p


def _engine(model, hidden, lr=0.1, reg_coef=1e-9, reg_norm=3, gamma=12.0, seed=5):
    from dglke_amd.engine import StepEngine
    cfg = O.Config(model, gamma, hidden, lr, adv=True, adv_temp=1.0, reg_coef=reg_coef, reg_norm=reg_norm)
    rng = np.random.RandomState(seed)
    ent = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(N_ENT, cfg.ent_dim)).astype(np.float32)
    rel = rng.uniform(-cfg.emb_init, cfg.emb_init, size=(N_REL, cfg.rel_dim)).astype(np.float32)
    es = rng.uniform(0.0, 1e-3, size=N_ENT).astype(np.float32)      # (a state of 0 hides a wrong state row)
    rs = rng.uniform(0.0, 1e-3, size=N_REL).astype(np.float32)
    eng = StepEngine(model, N_ENT, N_REL, hidden, gamma, lr, DEV, False, False, True, 1.0, reg_coef, reg_norm)
    eng.load_tables(ent, rel, es, rs)
    return eng, cfg, (ent, rel, es, rs)


def _tables(eng):
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy().copy() for x in (eng.ent, eng.rel, eng.ent_state, eng.rel_state))


def _check_step(got, start, cfg, bts, tag, async_group=False):
    """tables after the step(s) against the float64 oracle from the same start; untouched rows bit for bit"""
    e64, r64, es64, rs64 = (x.astype(np.float64) for x in start)
    if async_group:
        O.train_steps_async(cfg, e64, es64, r64, rs64, [_oracle_view(bt) for bt in bts])
    else:
        for bt in bts:
            v = _oracle_view(bt)
            O.train_step(cfg, e64, es64, r64, rs64, v["nid"], v["h_local"], v["t_local"], v["r"], v["neg"], v["neg_head"], v["chunk"], v["N"])
    in_e = np.zeros(N_ENT, bool)
    in_r = np.zeros(N_REL, bool)
    for bt in bts:
        in_e[np.concatenate([bt["h"], bt["t"], bt["neg"]])] = True
        in_r[bt["r"]] = True
    assert not in_e[OUT_ENT] and not in_r[OUT_REL]
    for name, g, s, ref, inside in (("entity", got[0], start[0], e64, in_e), ("relation", got[1], start[1], r64, in_r)):
        assert np.array_equal(g[~inside].view(np.uint32), s[~inside].view(np.uint32)), "%s: a %s row outside the batch changed" % (tag, name)
        err = np.abs(g[inside].astype(np.float64) - ref[inside])
        tol = 1e-4 * cfg.lr + 1e-6 * np.abs(ref).max()
        print("%s %s rows: max|err| %.3e = %.3e lr (bound %.3e lr)" % (tag, name, err.max(), err.max() / cfg.lr, tol / cfg.lr))
        assert np.all(np.isfinite(g)) and err.max() <= tol, "%s %s rows: max|err| %.3e lr > %.3e lr" % (tag, name, err.max() / cfg.lr, tol / cfg.lr)
    for name, g, s, ref, inside in (("entity", got[2], start[2], es64, in_e), ("relation", got[3], start[3], rs64, in_r)):
        assert np.array_equal(g[~inside].view(np.uint32), s[~inside].view(np.uint32)), "%s: a %s state outside the batch changed" % (tag, name)
        assert np.allclose(g[inside], ref[inside], rtol=1e-4, atol=1e-9), "%s %s state" % (tag, name)


def _run(eng, start, b):
    eng.load_tables(*start)
    eng.step(b)
    return _tables(eng)


def _both_forms(model, hidden, bt, tag, pad_e=3, pad_r=2, flag=None, maxrel=None, **kw):
    """one step on the device-counted form against the oracle, and the host plan of the same batch bit for bit"""
    eng, cfg, start = _engine(model, hidden, **kw)
    bd, _ = _batch(bt, "dev", pad_e, pad_r, flag, maxrel)
    bh, _ = _batch(bt, "host")
    got_d = _run(eng, start, bd)
    _check_step(got_d, start, cfg, [bt], tag + " device counts")
    got_h = _run(eng, start, bh)
    for name, x, y in zip(("entity rows", "relation rows", "entity state", "relation state"), got_d, got_h):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: %s differ between the host plan and the device-counted form" % (tag, name)


@pytest.mark.parametrize("ur_true", [1, 4, 5])
@pytest.mark.parametrize("ue_true", [1, 4, 5])
def test_counts_below_the_bounds(ue_true, ur_true):
    """bounds 7 entity and 6 relation entries above the counts: pad wavefronts in the last real workgroup and whole pad workgroups"""
    rng = np.random.RandomState(100 * ue_true + ur_true)
    bt = _ids(rng, 16, 8, 8, ue_true=ue_true, ur_true=ur_true, neg_head=bool(ue_true & 1))
    _both_forms("TransE_l2", 64, bt, "UE %d UR %d" % (ue_true, ur_true), pad_e=7, pad_r=6)


@pytest.mark.parametrize("hidden,longest", [(256, 13), (256, 14), (256, 15), (512, 13), (512, 14), (512, 15), (1024, 5), (1024, 6), (1024, 7)],
                         ids=lambda v: str(v))
def test_relation_instance_switch(hidden, longest):
    """counts[3] = the longest relation list, either side of COOP_MIN_R; relation 0's list has exactly that length"""
    rng = np.random.RandomState(hidden + longest)
    bt = _ids(rng, 32, 16, 8, ur_true=8, rel_list=longest, neg_head=bool(longest & 1))
    _both_forms("TransE_l2", hidden, bt, "D%d longest list %d" % (hidden, longest))
    if hidden == 256:
        _both_forms("DistMult", hidden, bt, "DistMult D%d longest list %d" % (hidden, longest), gamma=20.0)


@pytest.mark.parametrize("flag", [0, 1])
def test_corrupt_head_flag_word_is_not_the_updates_side(flag):
    """counts[2] set against the host field: the step computes what kge_batch.neg_head says"""
    rng = np.random.RandomState(40 + flag)
    bt = _ids(rng, 16, 8, 8, neg_head=not flag)
    _both_forms("TransE_l2", 64, bt, "counts[2] = %d, host neg_head = %d" % (flag, not flag), flag=flag)


WIDTHS = [4, 252, 256, 260, 400, 512, 516, 1024]
INSTANCES = [("TransE_l2", w, {}) for w in WIDTHS] + \
            [("DistMult", w, dict(gamma=20.0)) for w in (4, 260, 516, 1024)] + \
            [("TransE_l1", w, {}) for w in (4, 260, 512, 1024)] + \
            [("TransE_l2", w, dict(reg_norm=2, reg_coef=1e-7)) for w in (252, 516, 1024)]


@pytest.mark.parametrize("model,hidden,kw", INSTANCES, ids=lambda v: str(v).replace(" ", ""))
def test_widths_and_instances(model, hidden, kw):
    """every NIT of every update instance the strict step launches, both corruption sides, device counts with pad entries"""
    rng = np.random.RandomState(hidden)
    for neg_head in (False, True):
        bt = _ids(rng, 16, 8, 8, neg_head=neg_head)
        _both_forms(model, hidden, bt, "%s D%d neg_head=%d %s" % (model, hidden, neg_head, kw), **kw)


def test_gradient_emitting_step():
    """kge_step_grads, dense layout: the messages of the entries below the counts are the host plan's bit for bit, pad relation
    messages carry id -1, the entity gradients are the oracle's, and no table row moves"""
    from dglke_amd import _lib
    hidden = 260
    eng, cfg, start = _engine("TransE_l2", hidden)
    rng = np.random.RandomState(9)
    bt = _ids(rng, 16, 8, 8, neg_head=True)
    res = {}
    for form in ("host", "dev"):
        b, p = _batch(bt, form, 3, 2)
        bufs = dict(g0=torch.full((b.UE, hidden), float("nan"), device=DEV), gs0=torch.full((b.UE,), float("nan"), device=DEV),
                    g1=torch.full((b.UE, hidden), float("nan"), device=DEV), gs1=torch.full((b.UE,), float("nan"), device=DEV),
                    gr=torch.full((b.UR, hidden), float("nan"), device=DEV), gsr=torch.full((b.UR,), float("nan"), device=DEV),
                    rid=torch.full((b.UR, hidden), 7, dtype=torch.int32, device=DEV))
        em = _lib.KgeEmit()
        for k, v in bufs.items():
            setattr(em, k, v.data_ptr())
        eng.load_tables(*start)
        eng.step(b, eng.alloc_outputs(b), emit=em)
        got = _tables(eng)
        assert np.array_equal(got[0].view(np.uint32), start[0].view(np.uint32)), "the emitting step moved an entity row"
        res[form] = ({k: v.cpu().numpy() for k, v in bufs.items()}, p)
    (h, p), (d, _) = res["host"], res["dev"]
    ue, ur = p["UE"], p["UR"]
    for k in ("g0", "gs0", "g1", "gs1"):
        assert np.array_equal(h[k][:ue].view(np.uint32), d[k][:ue].view(np.uint32)), k
    for k in ("gr", "gsr"):
        assert np.array_equal(h[k][:ur].view(np.uint32), d[k][:ur].view(np.uint32)), k
    assert np.array_equal(d["rid"][:ur, :2], h["rid"][:ur, :2]) and np.all(d["rid"][ur:, :2] == -1)
    assert np.all(np.isnan(d["g0"][ue:])) and np.all(np.isnan(d["gr"][ur:])), "a pad entry wrote a message"
    v = _oracle_view(bt)
    out = O.forward_backward(cfg, start[0].astype(np.float64), start[1].astype(np.float64), v["nid"], v["h_local"], v["t_local"], v["r"],
                             v["neg"], v["neg_head"], v["chunk"], v["N"])
    sel = np.searchsorted(p["ue_id"], v["nid"])
    err = np.abs(d["g0"][sel] - out["g_pos_ent"]).max()
    print("emitted positive-trace gradients: max|err| %.3e (bound %.3e)" % (err, grad_tol(out["g_pos_ent"])))
    assert err <= grad_tol(out["g_pos_ent"])


def test_async_group():
    """kge_step_async: the update of step s - 1 runs inside step s's forward launch; three steps, device counts with pad entries"""
    eng, cfg, start = _engine("TransE_l2", 260)
    rng = np.random.RandomState(21)
    bts = [_ids(rng, 16, 8, 8, neg_head=bool(k & 1)) for k in range(3)]
    res = []
    for form in ("dev", "host"):
        bs = [_batch(bt, form, 3, 2)[0] for bt in bts]
        eng.load_tables(*start)
        eng.steps_async(bs)
        res.append(_tables(eng))
    _check_step(res[0], start, cfg, bts, "async group, device counts", async_group=True)
    for x, y in zip(*res):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "async group: host plan and device-counted form differ"
