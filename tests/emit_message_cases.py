"""Case table, input builders and float64 statement of the gradient-emitting step's MESSAGES (test infrastructure; a plain module,
not a conftest).

kge_step_grads runs the kernels of the fused step, but its update kernel applies nothing to the entity table: per union entry u
of the batch's plan it writes the two trace gradients and their Adagrad increments (include/kge_hip.h, kge_emit), and an owner
applies them later.  The cases below are shared by
  tests/test_emit_message_inputs.py   (CPU): every case through the statement in float32 and float64 - the reference alone stays
                                      inside every bound, the cases reach every instance of the update kernel, the two meanings of a
                                      summed increment are further apart than the bound;
  tests/test_gpu_emit_messages.py     (GPU): the messages of every case in every layout against the float64 statement.

Statement (messages(): built from oracle.kge_oracle.forward_backward / transr_forward_backward on the same float32 tables and
the batch's plan):
  g0[u]  = row of g_pos_ent of union entry u (zero without a positive list)      gs0[u] = mean(g0[u]^2)      (0 without one)
  g1[u]  = sum_k g_neg[slot_k] over ue_neg_slot                                   gs1[u] = sum_k mean(g_neg[slot_k]^2)
  gr[u]  = sum_k g_rel[edge_k] over ur_edge                                       gsr[u] = sum_k mean(g_rel[edge_k]^2)
with the regulariser as the oracle includes it and, under --neg_deg_sample, the in-batch rows' gradients inside g0.
A summed increment is NOT mean((sum_k g_k)^2): messages() returns that second form too (gs1_alt, gsr_alt) so that the tests can
show that their bound tells the two apart.

Bounds.  Gradients: GRAD_RTOL (3e-4) of the largest component of the compared array.  Increments: with tau = GRAD_RTOL and gmax
the largest component of the array whose rows are squared (g0, the per-slot g_neg, the per-edge g_rel), a component g + e with
|e| <= tau gmax has |(g + e)^2 - g^2| <= (2 tau + tau^2) gmax^2, so one mean(g^2) is off by at most that and a sum over a list
by that times the list's length (a row with an empty list: exactly 0).

Exclusions (conditions on the float64 operands, ROW_CAP of loss_option_cases.py): TransE_l1 elements whose sign(a - b) float32
cannot resolve (test_gpu_parity._l1_ambiguous with modular_op_cases.dropin_l1_tau) - the message rows they feed.
"""
import zlib

import numpy as np

import loss_option_cases as L
import modular_op_cases as M
from oracle import kge_oracle as O

GRAD_RTOL = M.GRAD_RTOL
TAU2 = 2.0 * GRAD_RTOL + GRAD_RTOL ** 2
ROW_CAP = L.ROW_CAP
NEG_DEG = L.NEG_DEG                      # include/kge_hip.h KGE_FLAG_NEG_DEG_SAMPLE
COOP_MIN_R = {1: 13, 2: 13, 4: 5}        # kge_update_body.hpp: 2 * LBR + 1 edges put a relation list on the shared-list instance
LONG_LIST = 64                           # kge_update_body.hpp: list entries beyond 64 take the loop `for (i = 64; ...)`
HUB, HUB_SLOTS = 7, 70                   # planted: entity 7 sits in 70 negative slots and is the head of edge 0
TWOS, THREES = (11, 12, 13), (21, 22)    # planted: entities in exactly 2 / exactly 3 negative slots; 11 is also the tail of edge 5
PLANTED_REL, PLANTED_EDGES = 0, 16       # planted: relation 0 carries at least 16 edges
LAYOUTS = ("dense", "strided", "packed", "dense_rel_inplace")       # (a) - (d) of the GPU file


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def rel_update_width(c):
    """the width launch_update sees as d_r (Step::phase_update: RESCAL's relation matrices are updated by kge_rescal.hip)"""
    return c["d_e"] if c["model"] == "RESCAL" else c["d_r"]


def transe_fast(c):
    """plan_step (kge_api.hip): the TransE fast path - the update kernel rebuilds the per-edge gradients itself"""
    dmax = max(c["d_e"], c["d_r"])
    return (c["model"] in ("TransE_l1", "TransE_l2") and not c["pairwise"] and not c["neg_deg"] and c["d_e"] % 4 == 0 and
            c["d_r"] % 4 == 0 and dmax <= 1024)


def update_instance(c, rel_messages=True):
    """the instance launch_update (kge_rowwise.hip) picks for an emitting step of case c: 'generic4' / 'generic1' (update_kernel<V>)
    or 'reg<LEAN>-nit<NIT>' (update_kernel_reg<NIT, false, LEAN>).  rel_messages: emit.gr given (False: relation trace in place)"""
    d_e, d_r = c["d_e"], rel_update_width(c)
    dmax, vec = max(d_e, d_r), d_e % 4 == 0 and d_r % 4 == 0
    if not (vec and dmax <= 1024):
        return "generic4" if vec else "generic1"
    nit = 1 if dmax <= 256 else (2 if dmax <= 512 else 4)
    reg3 = not (c["reg_coef"] > 0 and c["reg_norm"] > 0) or c["reg_norm"] == 3
    if not reg3:
        lean = 0
    elif transe_fast(c) or c["neg_deg"]:
        lean = 4
    else:
        lean = 6 if rel_messages else 7
    return "reg%d-nit%d" % (lean, nit)


def packed_supported(c):
    """kge_emit.msg_rows: the register-resident update kernel only"""
    return not update_instance(c).startswith("generic")


def rel_messages_allowed(c):
    """RESCAL / TransR emit with the relation trace applied in place only (Step::setup)"""
    return c["model"] not in ("RESCAL", "TransR")


def _table_range(model, gamma, d_e):
    """half-width s of the uniform tables: the distance models' scores around 0 (mean distance ~ gamma), the product models wide
    enough for gradients of the size of the rows"""
    if model == "TransE_l2":
        return gamma / np.sqrt(d_e)
    if model == "TransE_l1":
        return gamma / (0.8 * d_e)
    if model == "RotatE":
        return gamma / (0.5 * d_e)
    if model == "TransR":             # |x P - r - y P|_1 over d_r = d_e columns, P ~ U(-1, 1): ~1.13 d_e sqrt(d_e / 3) s
        return gamma / (1.13 * d_e * np.sqrt(d_e / 3.0))
    return 0.25 if model == "RESCAL" else 0.5


def emit_case(model, hidden, de=False, dr=False, neg_head=False, reg_coef=0.0, reg_norm=3, neg_deg=False, impts=False, device_plan=False,
              B=64, chunk=16, N=32, n_ent=300, n_rel=5, tag=""):
    gamma = 12.0
    d_e = hidden * (2 if de else 1)
    c = L.case("", "midT", reg_coef=reg_coef, reg_norm=reg_norm, impts=impts, neg_deg=neg_deg, rows=5e-3,
               model=model, n_ent=n_ent, n_rel=n_rel, hidden=hidden, de=de, dr=dr, B=B, N=N, chunk=chunk, gamma=gamma, lr=0.1)
    c["d_e"] = d_e
    c["d_r"] = d_e * d_e if model == "RESCAL" else hidden * (2 if dr else 1)
    c["scale"] = float(_table_range(model, gamma, d_e) / ((gamma + 2.0) / hidden))
    c["neg_head"], c["device_plan"] = bool(neg_head), bool(device_plan)
    c["flags"] = NEG_DEG if neg_deg else 0
    c["instance"] = update_instance(c, rel_messages_allowed(c))
    c["id"] = "%s-D%d%s-nh%d-%s" % (model, d_e, "-" + tag if tag else "", int(neg_head), c["instance"])
    c["seed"] = _seed(c["id"]) % 100000
    return c


def _cases():
    e = emit_case
    return [
        # ---- register-resident body, LEAN 4 (TransE fast path / neg_deg_sample) at NIT 1, 2, 4
        e("TransE_l2", 16), e("TransE_l2", 320, neg_head=True), e("TransE_l2", 768),
        e("TransE_l1", 16, neg_head=True),
        e("TransE_l2", 16, neg_deg=True, tag="nd"),
        # ---- LEAN 6 (per-edge gradient rows, relation messages; layout (d): LEAN 7) at NIT 1, 2, 4
        e("DistMult", 16, neg_head=True), e("DistMult", 320), e("DistMult", 768, neg_head=True),
        e("ComplEx", 160, de=True, dr=True, reg_coef=2e-3, reg_norm=3, tag="reg3"),
        e("RotatE", 8, de=True), e("RotatE", 384, de=True, neg_head=True),
        e("DistMult", 16, impts=True, tag="impts"),
        # ---- LEAN 0 (a regulariser norm other than 3) at NIT 1, 2, 4
        e("DistMult", 16, reg_coef=2e-3, reg_norm=2, tag="reg2"),
        e("TransE_l2", 320, reg_coef=2e-4, reg_norm=2, tag="reg2"),
        e("RotatE", 384, de=True, reg_coef=2e-4, reg_norm=2, tag="reg2"),
        # ---- the generic update_kernel<4> (a width above 1024) and update_kernel<1> (widths that are no multiple of 4)
        e("TransE_l2", 1028, neg_head=True), e("TransE_l2", 30), e("DistMult", 18, neg_head=True),
        # ---- the relation-matrix models: relation trace in place (emit.gr NULL), LEAN 7
        e("TransR", 32), e("RESCAL", 16, neg_head=True),
        # ---- a plan built on the device (kge_sample_batches): UE / UR are bounds, the counts live in counts_dev
        e("TransE_l2", 16, device_plan=True, n_ent=200, tag="devplan"), e("DistMult", 16, device_plan=True, n_ent=200, tag="devplan"),
    ]


CASES = _cases()
INSTANCES = tuple(["generic4", "generic1"] + ["reg%d-nit%d" % (le, n) for le in (0, 4, 6, 7) for n in (1, 2, 4)])


def layouts_of(c):
    """the layouts the GPU file runs a case in"""
    if not rel_messages_allowed(c):
        return ("dense_rel_inplace",)
    return LAYOUTS


def instance_of(c, layout):
    return update_instance(c, rel_messages=layout != "dense_rel_inplace")


def tables(c):
    return L.tables(c)


def host_ids(c):
    """the batch of a host-planned case as a dict like oracle.synth_batch's, with the planted lists: HUB in HUB_SLOTS negative slots
    and head of edge 0; TWOS / THREES in exactly 2 / 3 slots, TWOS[0] also the tail of edge 5; PLANTED_REL on the first 16 edges.
    No edge with h == t (see loss_option_cases.batches)."""
    assert not c["device_plan"]
    rng = np.random.RandomState(c["seed"])
    B, N, chunk, n_ent = c["B"], c["N"], c["chunk"], c["n_ent"]
    CN = (B // chunk) * N
    planted = (HUB,) + TWOS + THREES
    pool = np.array([x for x in range(n_ent) if x not in planted], np.int64)
    h, t = rng.choice(pool, B), rng.choice(pool, B)
    same = h == t
    t[same] = pool[(np.searchsorted(pool, t[same]) + 1) % len(pool)]
    h[0], t[5] = HUB, TWOS[0]
    r = rng.randint(0, c["n_rel"], B).astype(np.int64)
    r[:PLANTED_EDGES] = PLANTED_REL
    neg = rng.choice(pool, CN)
    slots, o = rng.permutation(CN), 0
    for ent, n in ((HUB, HUB_SLOTS),) + tuple((x, 2) for x in TWOS) + tuple((x, 3) for x in THREES):
        neg[slots[o:o + n]] = ent
        o += n
    return ids_dict(c, h, t, r, neg, c["neg_head"], rng.uniform(0.5, 1.5, B).astype(np.float32) if c["impts"] else None)


def ids_dict(c, h, t, r, neg, neg_head, w=None):
    h, t, r, neg = (np.ascontiguousarray(x, np.int64) for x in (h, t, r, neg))
    nid, inv = np.unique(np.concatenate([h, t]), return_inverse=True)
    B = len(h)
    return dict(h=h, t=t, r=r, neg=neg, neg_head=bool(neg_head), nid=nid.astype(np.int64), h_local=inv[:B].astype(np.int64),
                t_local=inv[B:].astype(np.int64), C=B // c["chunk"], w=w)


def union(bt):
    """(ue_id, ur_id): the sorted unique entity / relation ids of the batch - the rows of its plan (dglke_amd/plan.py build_plan)"""
    return np.unique(np.concatenate([bt["nid"], bt["neg"]])), np.unique(bt["r"])


def messages(c, ent, rel, proj, bt, dtype=np.float64):
    """the statement (module docstring) in `dtype` from float32 tables.  Returns a dict of arrays indexed by union entry / unique
    relation, the per-slot / per-edge gradient arrays they were summed from (g_neg, g_rel), the list lengths (n_pos, n_neg, n_rel)
    and the scores."""
    ent, rel = ent.astype(dtype), rel.astype(dtype)
    out = L.oracle_forward_backward(c, ent, rel, None if proj is None else proj.astype(dtype), bt)
    ue_id, ur_id = union(bt)
    UE, UR, d_e, d_r = len(ue_id), len(ur_id), ent.shape[1], rel.shape[1]
    sel = np.searchsorted(ue_id, bt["nid"])
    g0, gs0 = np.zeros((UE, d_e), dtype), np.zeros(UE, dtype)
    g0[sel] = out["g_pos_ent"]
    gs0[sel] = (out["g_pos_ent"] * out["g_pos_ent"]).mean(1)
    n_pos = np.zeros(UE, np.int64)
    n_pos[sel] = 1
    uneg = np.searchsorted(ue_id, bt["neg"])
    g1, gs1 = np.zeros((UE, d_e), dtype), np.zeros(UE, dtype)
    np.add.at(g1, uneg, out["g_neg"])
    np.add.at(gs1, uneg, (out["g_neg"] * out["g_neg"]).mean(1))
    urel = np.searchsorted(ur_id, bt["r"])
    m = dict(ue_id=ue_id, ur_id=ur_id, g0=g0, gs0=gs0, g1=g1, gs1=gs1, n_pos=n_pos, n_neg=np.bincount(uneg, minlength=UE),
             n_rel=np.bincount(urel, minlength=UR), g_neg=out["g_neg"], g_pos_ent=out["g_pos_ent"], g_rel=out["g_rel"],
             pos_score=out["pos_score"], neg_score=out["neg_score"], gs1_alt=(g1 * g1).mean(1))
    if c["model"] != "RESCAL":          # (RESCAL's [B, d_e * d_e] relation gradients never leave as messages)
        gr, gsr = np.zeros((UR, d_r), dtype), np.zeros(UR, dtype)
        np.add.at(gr, urel, out["g_rel"])
        np.add.at(gsr, urel, (out["g_rel"] * out["g_rel"]).mean(1))
        m.update(gr=gr, gsr=gsr, gsr_alt=(gr * gr).mean(1))
    return m


def gmax(a):
    return max(float(np.abs(a).max()) if np.size(a) else 0.0, 1e-30)


def bounds(ref):
    """{quantity: bound array} of a float64 statement `ref`"""
    b = dict(g0=GRAD_RTOL * gmax(ref["g0"]), g1=GRAD_RTOL * gmax(ref["g1"]),
             gs0=TAU2 * gmax(ref["g0"]) ** 2 * ref["n_pos"], gs1=TAU2 * gmax(ref["g_neg"]) ** 2 * ref["n_neg"])
    if "gr" in ref:
        b.update(gr=GRAD_RTOL * gmax(ref["gr"]), gsr=TAU2 * gmax(ref["g_rel"]) ** 2 * ref["n_rel"])
    return b


def exclusions(c, ent, rel, bt):
    """TransE_l1: the message rows fed by a sign-ambiguous element - dict(ent=union entries (both traces), rel=unique relations),
    checked against ROW_CAP; empty for the other models"""
    ue_id, ur_id = union(bt)
    if c["model"] != "TransE_l1":
        return dict(ent=[], rel=[])
    from test_gpu_parity import _l1_ambiguous
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    amb = _l1_ambiguous(bt, e64, r64, c["chunk"], c["N"], tau=M.dropin_l1_tau(e64, r64))
    rows = dict(ent=np.searchsorted(ue_id, sorted(amb["ent"])).tolist(), rel=np.searchsorted(ur_id, sorted(amb["rel"])).tolist())
    M.check_row_cap(rows["ent"], len(ue_id), c["id"] + " entity messages")
    M.check_row_cap(rows["rel"], len(ur_id), c["id"] + " relation messages")
    return rows


def message_errors(got, ref, excl):
    """{quantity: (largest |got - ref| / bound, that error, its bound)} over the quantities `got` holds, excluded rows replaced"""
    bd, res = bounds(ref), {}
    for k in ("g0", "gs0", "g1", "gs1", "gr", "gsr"):
        if k in got and k in ref:
            rows = excl["rel"] if k in ("gr", "gsr") else excl["ent"]
            res[k] = M.worst(M.masked(got[k], ref[k], rows), ref[k], bd[k])
    return res


def meaning_gap(ref):
    """largest (|sum_k mean(g_k^2) - mean((sum_k g_k)^2)| / the increment's bound) over the rows with a list of two or more, for the
    negative trace and (when there are relation messages) the relation trace"""
    bd = bounds(ref)
    out = {}
    for k, n in (("gs1", "n_neg"), ("gsr", "n_rel")):
        if k in ref:
            rows = ref[n] >= 2
            out[k] = float((np.abs(ref[k] - ref[k + "_alt"])[rows] / bd[k][rows]).max()) if rows.any() else 0.0
    return out
