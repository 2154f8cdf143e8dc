"""The workspace contract of include/kge_hip.h, as cases and helpers (their CPU checks: tests/test_workspace_inputs.py; the GPU
runs: tests/test_gpu_workspace_contract.py).

Every entry point that takes (ws, ws_bytes) is listed in WS_ENTRIES with the position of its workspace argument and the size
function of its arguments.  The tests hand it a guarded buffer [GUARD bytes | need bytes | GUARD bytes] with ws_bytes = need
exactly, carved with a gap of GAP bytes behind every buffer (kge_debug_carve), filled with one byte value; bytes that belong to no
carved buffer - the gaps, the alignment padding and both guards - must still hold that value after the call.
"""
import ctypes as C

import numpy as np

GAP = 256            # bytes left behind every carved buffer in the contract tests
GUARD = 4096         # bytes in front of and behind the workspace
CAP = 4096           # trace capacity in (offset, bytes) pairs
ERR_WORKSPACE = -2   # KGE_ERR_WORKSPACE
ERR_ARG = -1


def al(x, a=256):
    return (x + a - 1) // a * a


# ---- the trace ------------------------------------------------------------------------------------------------------------
class Trace(object):
    """kge_debug_carve on the calling thread: `with Trace(h, gap) as t: ...; t.pairs()`"""

    def __init__(self, h, gap=GAP, cap=CAP):
        self.h, self.gap, self.cap = h, gap, cap
        self.buf = (C.c_int64 * (2 * cap))()

    def __enter__(self):
        self.reset()
        return self

    def __exit__(self, *exc):
        assert self.h.kge_debug_carve(None, 0, 0) == 0
        return False

    def reset(self):
        assert self.h.kge_debug_carve(C.cast(self.buf, C.c_void_p), self.cap, self.gap) == 0

    def count(self):
        return int(self.h.kge_debug_carve_count())

    def pairs(self, last=None):
        """the recorded (offset, bytes) pairs; last = k: the k most recent ones (an entry may measure before it carves)"""
        n = self.count()
        assert n <= self.cap, "trace capacity %d < %d buffers" % (self.cap, n)
        p = [(int(self.buf[2 * i]), int(self.buf[2 * i + 1])) for i in range(n)]
        return p if last is None else p[n - last:]


def check_layout(pairs, need, gap):
    """what test_workspace_inputs.py asserts of a traced layout: buffers ascending and disjoint, each followed by at least `gap`
    bytes that belong to no buffer, the last one's end + gap rounded up = the size function's value"""
    assert pairs, "no buffer carved"
    end = 0
    for k, (off, n) in enumerate(pairs):
        assert off % 256 == 0, "buffer %d at offset %d is not 256-byte aligned" % (k, off)
        assert off >= end, "buffer %d at %d overlaps the previous one's end + gap %d" % (k, off, end)
        end = off + n + gap
    assert al(end) == need, "last buffer ends at %d (+ gap, rounded: %d), the size function says %d" % (end - gap, al(end), need)


def free_mask(pairs, need, halves=1, guard=GUARD):
    """bool [guard + need + guard]: True where the byte belongs to no carved buffer (guards, gaps, alignment padding).
    halves = 2: the layout sits at offset 0 and at need / 2 (the two halves of the async workspace)."""
    m = np.ones(guard + need + guard, dtype=bool)
    half = need // halves
    for k in range(halves):
        for off, n in pairs:
            assert off + n <= half, "buffer [%d, %d) leaves its workspace of %d bytes" % (off, off + n, half)
            m[guard + k * half + off:guard + k * half + off + n] = False
    return m


def stray_bytes(buf, mask, value):
    """offsets (relative to the workspace base; negative = front guard) of free bytes that no longer hold `value`"""
    buf = np.asarray(buf).view(np.uint8)
    assert buf.shape == mask.shape
    return np.nonzero(mask & (buf != value))[0] - GUARD


def describe_stray(offsets, pairs, need):
    o = int(offsets[0])
    if o < 0:
        return "%d stray bytes, first %d bytes in FRONT of the workspace" % (len(offsets), -o)
    if o >= need:
        return "%d stray bytes, first %d bytes BEHIND the workspace end" % (len(offsets), o - need)
    prev = [(k, off, n) for k, (off, n) in enumerate(pairs) if off + n <= o]
    k, off, n = prev[-1] if prev else (-1, 0, 0)
    return "%d stray bytes, first at offset %d = %d bytes past the end of buffer %d [%d, %d)" % (len(offsets), o, o - off - n, k, off, off + n)


# ---- every entry that takes a workspace ----------------------------------------------------------------------------------------
def _obj(a):
    return getattr(a, "_obj", a)          # ctypes.byref(x) -> x


def _step_need(fn, hp_at, b_at):
    def need(h, a, gap):
        b = _obj(a[b_at])
        return int(getattr(h, fn)(a[hp_at], b.B, b.C, b.chunk, b.N, b.UE, b.UR))
    return need


def _loss_need(h, a, gap):
    # kge_loss_fwd_bwd has no size function (include/kge_hip.h states the bytes): two [B] float rows, and the four staged loss
    # terms when loss3 is asked, each rounded up to 256 bytes
    B = int(a[8])
    return 2 * al(4 * B + gap) + (al(16 + gap) if a[10] else 0)


QUATE_ID, DISTMULT_ID = 8, 2      # include/kge_hip.h KGE_QUATE, KGE_DISTMULT


def rel_need(h, model, Eb, n_rel, d_e, d_r, gap):
    """kge_rank_rel_workspace_bytes answers for the ids up to TransR; a QuatE call takes the DistMult layout followed by the
    normalised relation table [n_rel, d_r] (include/kge_hip.h; _lib.rank_rel_workspace_bytes) - behind its own gap here"""
    if int(model) != QUATE_ID:
        return int(h.kge_rank_rel_workspace_bytes(model, Eb, n_rel, d_e, d_r))
    base = int(h.kge_rank_rel_workspace_bytes(DISTMULT_ID, Eb, n_rel, d_e, d_r))
    return base + al(4 * int(n_rel) * int(d_r) + gap) if base else 0


def _topk_width(model, d_e):
    from dglke_amd import _lib
    return _lib.topk_row_width(int(model), int(d_e))


class Entry(object):
    """ws: the position of `ws` in the prototype (ws_bytes follows it); phases: the position of a `phases` argument - calls of one
    step without PHASE_GATHER share the workspace of the call that had it; known: the position of `known`, followed by the pair
    mask and its bytes (guarded in a buffer of its own)"""

    def __init__(self, ws, need, halves=1, explicit=None, phases=None, known=None, more=None):
        self.ws, self.need, self.halves, self.explicit, self.phases, self.known = ws, need, halves, explicit, phases, known
        self.more = more          # more(args) -> buffers the entry carves beyond those its size function traced


WS_ENTRIES = {
    "kge_step_fused": Entry(4, _step_need("kge_step_workspace_bytes", 0, 2)),
    "kge_step_fused_sampling": Entry(4, _step_need("kge_step_workspace_bytes", 0, 2)),
    "kge_step_fused_known": Entry(4, _step_need("kge_step_workspace_bytes", 0, 2), known=7),
    "kge_step_phase": Entry(4, _step_need("kge_step_workspace_bytes", 0, 2), phases=6),
    "kge_step_phase_known": Entry(4, _step_need("kge_step_workspace_bytes", 0, 2), phases=6, known=7),
    # (hp, opt, tb, b, out, ws, ws_bytes, phases, known, mask, mask_bytes, stream)
    "kge_step_optim": Entry(5, _step_need("kge_step_workspace_bytes", 0, 3), phases=7, known=8),
    "kge_step_grads": Entry(5, _step_need("kge_step_workspace_bytes", 0, 2)),
    "kge_step_sharded": Entry(4, _step_need("kge_step_workspace_bytes", 0, 2)),
    "kge_step_async": Entry(6, _step_need("kge_step_async_workspace_bytes", 1, 3), halves=2),
    "kge_score_neg_fwd": Entry(13, lambda h, a, gap: int(h.kge_score_neg_workspace_bytes(a[0], a[5], a[6], a[7], a[8]))),
    "kge_score_neg_bwd": Entry(17, lambda h, a, gap: int(h.kge_score_neg_workspace_bytes(a[0], a[7], a[8], a[9], a[10]))),
    "kge_loss_fwd_bwd": Entry(13, _loss_need),
    # one buffer of n floats, no allocator
    "kge_pnorm_pow": Entry(5, lambda h, a, gap: 4 * max(int(a[1]), 1), explicit=lambda a: [(0, 4 * max(int(a[1]), 1))]),
    "kge_rank_eval": Entry(21, lambda h, a, gap: int(h.kge_rank_workspace_bytes(a[18], a[15], a[10]))),
    "kge_rank_eval_ex": Entry(22, lambda h, a, gap: int(h.kge_rank_workspace_bytes(a[19], a[16], a[11]))),
    "kge_rank_eval_split": Entry(24, lambda h, a, gap: int(h.kge_rank_workspace_bytes(a[21], a[18], a[13]))),
    # ONE chunk's workspace: the entry walks its blocks over it
    "kge_rank_eval_chunked": Entry(24, lambda h, a, gap: int(h.kge_rank_chunked_workspace_bytes(a[0], a[15], a[15], a[17], a[19], a[11], a[12]))),
    "kge_rank_rel_eval": Entry(19, lambda h, a, gap: rel_need(h, a[0], a[16], a[4], a[10], a[11], gap), more=lambda a: int(a[0] == QUATE_ID)),
    # (no model argument: a PairRE / TransH call keeps the pair (a, w) / (a, w^, c) per query row - _lib.topk_row_width)
    "kge_topk_select": Entry(22, lambda h, a, gap: int(h.kge_topk_workspace_bytes(a[9], a[15], _topk_width(a[0], a[10]), a[19]))),
    "kge_topk_select_filtered": Entry(22, lambda h, a, gap: int(h.kge_topk_workspace_bytes(a[9], a[15], _topk_width(a[0], a[10]), a[19]))),
    "kge_topk_vector": Entry(5, lambda h, a, gap: int(h.kge_topk_workspace_bytes(0, a[1], 0, a[2]))),
}


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _step(id, model, hidden, B=40, chunk=8, N=24, flags=0, de=False, dr=False, outputs=True, n_ent=300, n_rel=7, adv=True,
          reg=1e-6, d_r=None, genre="Logsigmoid"):
    return dict(id=id, model=model, hidden=hidden, B=B, chunk=chunk, N=N, flags=flags, de=de, dr=dr, outputs=outputs, n_ent=n_ent,
                n_rel=n_rel, adv=adv, reg=reg, gamma=8.0, lr=0.1, d_r=d_r, genre=genre)


DOUBLED = {"ComplEx": (True, True), "RotatE": (True, False)}      # rows twice the hidden width (72 at hidden 36)
MODELS = ["TransE_l1", "TransE_l2", "DistMult", "ComplEx", "RotatE", "SimplE", "RESCAL", "TransR"]


def _steps():
    out = []
    for m in MODELS:                                              # the eight models at hidden 36, packed (N = 24) loss rows
        de, dr = DOUBLED.get(m, (False, False))
        out.append(_step("%s-h36-N24" % m, m, 36, de=de, dr=dr))
    for m in ("TransE_l2", "DistMult", "ComplEx", "RotatE"):      # strided loss rows
        de, dr = DOUBLED.get(m, (False, False))
        out.append(_step("%s-h36-N21" % m, m, 36, N=21, de=de, dr=dr))
    for m in ("TransE_l2", "TransE_l1", "DistMult"):              # widths not divisible by 4: generic update and pairwise paths
        out.append(_step("%s-h30-N24" % m, m, 30))
        out.append(_step("%s-h30-N21" % m, m, 30, N=21))
    # TransR: (36, 36) above and (36, 20) take the 128 x 208-tile kernels of kge_transr_wide.hpp (widths divisible by 4, <= 208);
    # hidden 18 and d_r = 216 take the 64 x 64 tiles (scalar and 16-byte loads)
    out.append(_step("TransR-36x20", "TransR", 36, d_r=20))
    out.append(_step("TransR-36x72", "TransR", 36, dr=True))
    out.append(_step("TransR-18x36", "TransR", 18, dr=True))
    out.append(_step("TransR-108x216", "TransR", 108, dr=True, B=16, chunk=8, N=8))
    # RESCAL: d_e = 20 (more row blocks than rows per block); d_e = 12 < RESCAL_RBN = 16 row blocks; d_e = 18 (per-edge passes)
    out.append(_step("RESCAL-h20", "RESCAL", 20))
    out.append(_step("RESCAL-h12", "RESCAL", 12))
    out.append(_step("RESCAL-h18", "RESCAL", 18, N=21))
    # the shared-pair backward with GA in parts (neg_bwd_lc_splits > 1; asserted in test_workspace_inputs.py)
    out.append(_step("RotatE-lc-parts", "RotatE", 16, de=True, B=16, chunk=8, N=64))
    out.append(_step("TransE_l1-lc-parts", "TransE_l1", 32, B=16, chunk=8, N=128))
    for f in (1, 2, 4, 8, 16, 32, 33, 128, 256, 512, 768, 1024):  # every flag form of the strict step (0: above)
        out.append(_step("TransE_l2-h36-N24-f%d" % f, "TransE_l2", 36, flags=f))
    for m, f in (("DistMult", 2), ("DistMult", 8), ("DistMult", 32), ("ComplEx", 1024), ("ComplEx", 1), ("RotatE", 16), ("TransE_l1", 16),
                 ("RotatE", 32), ("RESCAL", 32), ("TransR", 32)):
        de, dr = DOUBLED.get(m, (False, False))
        out.append(_step("%s-h36-N24-f%d" % (m, f), m, 36, flags=f, de=de, dr=dr))
    for m in ("TransE_l2", "ComplEx", "RotatE", "RESCAL", "TransR"):   # the plain training step: no optional output
        de, dr = DOUBLED.get(m, (False, False))
        out.append(_step("%s-h36-N24-plain" % m, m, 36, de=de, dr=dr, outputs=False))
    for m in ("TransE_l2", "DistMult"):                           # the Softmax genre (no -adv form): the row-wise loss kernel's softmax rows
        out.append(_step("%s-h36-N24-softmax" % m, m, 36, adv=False, genre="Softmax"))
    return out


STEP_CASES = _steps()
# what the dirty fill leaves behind: a case of another model and a larger shape run on the same buffer first
DONOR = _step("donor-ComplEx", "ComplEx", 64, B=96, chunk=32, N=48, de=True, dr=True)
DONOR_ALT = _step("donor-TransE_l1", "TransE_l1", 100, B=96, chunk=32, N=48)

PHASE_CASES = [c for c in STEP_CASES if c["id"] in ("TransE_l2-h36-N24", "DistMult-h36-N21", "RotatE-h36-N24", "TransE_l1-h30-N24",
                                                      "RESCAL-h20", "TransR-36x72", "TransE_l2-h36-N24-f8", "TransE_l2-h36-N24-f128")]
ASYNC_CASES = [dict(c, id=c["id"] + ("-rel" if f else ""), flags=f) for c in STEP_CASES
               if c["id"] in ("TransE_l2-h36-N24", "DistMult-h36-N21", "ComplEx-h36-N24", "RotatE-h36-N24", "TransE_l1-h36-N24") for f in (0, 64)]


# ---- QuatE, PairRE, TransH: the steps ----------------------------------------------------------------------------------------
# Cases, float64 statements, bounds and the conditions on the inputs are those of quate_cases.py / pairre_cases.py / transh_cases.py
# (their step_case options by id, their step_tables / step_batches builders) at this file's shapes: B = 40, chunk = 8, N = 24 / 21
# on 300 entities and 7 relations.  Widths: 36 (a multiple of 4 - QuatE's matrix-core route - and a partial 32-wide k stage / slab of
# the TransH tiles and the PairRE kernels), 16 (below one k stage: TransH's top-K takes its VALU tile; QuatE's vector packs and
# broadcast kernels), 260 (past 256, q = 65 scalar packs) at B = 16, N = 8.  Every step starts from the fixed tables (as in the
# PairRE / TransH tests), so test_workspace_inputs.py can assert the conditions on the float64 statement alone.  `seed`: of the
# batches, chosen so that the conditions hold (asserted there).
NEW_MODELS = ("QuatE", "PairRE", "TransH")
FORCE_PAIRWISE, NEG_DEG = 1, 32


def model_cases(model):
    import importlib
    return importlib.import_module({"QuatE": "quate_cases", "PairRE": "pairre_cases", "TransH": "transh_cases"}[model])


def model_gamma(model):
    return 12.0 if model == "QuatE" else model_cases(model).GAMMA        # (test_gpu_quate.py's engine: 12)


def model_d_r(model, d_e):
    return d_e if model == "QuatE" else 2 * d_e


def _mstep(model, d_e, tag, base="logsigmoid-adv", N=24, flags=0, outputs=True, B=40, chunk=8, n_ent=300, n_rel=7, seed=0):
    Q = model_cases(model)
    c = dict([x for x in Q.STEP_CASES if x["id"] == base][0])
    c.update(id="%s-D%d-%s" % (model, d_e, tag), base=base, model=model, d_e=d_e, B=B, chunk=chunk, N=N, n_ent=n_ent, n_rel=n_rel,
             flags=flags, outputs=outputs, seed=seed, gamma=model_gamma(model))
    return c


# (model, tag) -> seed of the batches where 0 does not hold the model's conditions
MODEL_SEEDS = {("PairRE", "N24"): 1, ("PairRE", "w260"): 1}


def _model_steps():
    out = []
    for m in NEW_MODELS:
        k = lambda tag, **kw: _mstep(m, kw.pop("d_e", 36), tag, seed=MODEL_SEEDS.get((m, tag), 0), **kw)
        out += [k("N24"), k("N21", N=21), k("plain", outputs=False), k("neg-deg", base="neg-deg"), k("softmax", base="softmax"),
                k("hinge-pw", base="hinge-pw"), k("impts", base="impts")]
        if m == "QuatE":             # (use_mfma knows QuatE only: PairRE and TransH have one route and ignore the flag - their layout
            out.append(k("f1", flags=FORCE_PAIRWISE))        # under it is asserted equal on the CPU)
        out += [k("w16", d_e=16), k("w260", d_e=260, B=16, N=8)]
    return out


MODEL_STEP_CASES = _model_steps()
MODEL_PHASE_CASES = [c for c in MODEL_STEP_CASES if c["id"].endswith("-D36-N24")]
MODEL_KNOWN_CASES = {c["model"]: c for c in MODEL_PHASE_CASES}
# the second dirty donor: a larger TransH step (eight more buffers, four of them stacked) in front of every case that is not TransH
DONOR_TRANSH = _mstep("TransH", 64, "donor", B=96, chunk=32, N=48)


class _Shapes(object):
    """the model module's builders at a case's shapes: its STEP_ENT / STEP_REL and the batch seed of the case, for the duration"""

    def __init__(self, c):
        self.c, self.Q = c, model_cases(c["model"])

    def __enter__(self):
        Q, c = self.Q, self.c
        self.saved = (Q.STEP_ENT, Q.STEP_REL)
        Q.STEP_ENT, Q.STEP_REL = c["n_ent"], c["n_rel"]
        if hasattr(Q, "STEP_SEEDS"):
            Q.STEP_SEEDS[c["id"]] = c["seed"]
        return Q

    def __exit__(self, *exc):
        self.Q.STEP_ENT, self.Q.STEP_REL = self.saved
        getattr(self.Q, "STEP_SEEDS", {}).pop(self.c["id"], None)
        return False


def model_shapes(c):
    return _Shapes(c)


def model_tables(c):
    with _Shapes(c) as Q:
        ent, rel = Q.step_tables(c["d_e"])
    assert ent.shape == (c["n_ent"], c["d_e"]) and rel.shape == (c["n_rel"], model_d_r(c["model"], c["d_e"]))
    return ent, rel


def model_batches(c, steps=2):
    with _Shapes(c) as Q:
        if c["model"] == "QuatE" and c["seed"]:
            return Q.step_batches(dict(c, id="%s#%d" % (c["id"], c["seed"])), steps)
        return Q.step_batches(c, steps)


def model_conditions(c, out):
    """what the model's own step test asserts of its float64 statement's inputs"""
    Q = model_cases(c["model"])
    if c["model"] == "PairRE":
        assert not out["amb"], c["id"] + ": a sign-ambiguous element in a step input"
    if c["model"] == "TransH":
        assert out["share"] >= Q.DIST_SHARE, "%s: a distance at %.3f of sqrt(alpha + beta)" % (c["id"], out["share"])
        assert Q.residual_rows(out) == 0, c["id"] + ": a gradient row that is a cancellation residual"


def model_hparams(c):
    from dglke_amd import _lib
    hp = _lib.KgeHParams()
    hp.model = _lib.model_id(c["model"])
    hp.d_e, hp.d_r = c["d_e"], model_d_r(c["model"], c["d_e"])
    hp.loss_genre, hp.adv, hp.pairwise, hp.reg_norm = _lib.LOSS_IDS[c["genre"]], int(c["adv"]), int(c["pairwise"]), c["reg_norm"]
    hp.flags = c["flags"] | (NEG_DEG if c["neg_deg"] else 0)
    hp.gamma, hp.lr, hp.adv_temp, hp.reg_coef, hp.eps, hp.margin = c["gamma"], c["lr"], c["adv_temp"], c["reg_coef"], 1e-10, c["margin"]
    hp.emb_init = (c["gamma"] + 2.0) / c["d_e"]
    return hp


def model_step_size(h, c, flags=None):
    bt = model_batches(c, 1)[0]
    UE = len(np.unique(np.concatenate([bt["h"], bt["t"], bt["neg"]])))
    UR = len(np.unique(bt["r"]))
    hp = model_hparams(c)
    if flags is not None:
        hp.flags = flags
    return int(h.kge_step_workspace_bytes(C.byref(hp), c["B"], c["B"] // c["chunk"], c["chunk"], c["N"], UE, UR))


# ---- QuatE, PairRE, TransH: the per-op negative scores, ranking, top-K ---------------------------------------------------------------
# kge_score_neg_fwd / _bwd on the models' own op inputs (op_inputs / op_reference, whose conditions their CPU files assert for every
# width and shape of their tables), both corruption sides.  QuatE: the matrix-core route and, under KGE_FLAG_FORCE_PAIRWISE, the pair
# kernels; PairRE: a partial and a whole + 4 slab; TransH: below one k stage and a partial one, and (1, 12, 20), whose STACKED 24 rows
# cross a 16-row tile that the 12 rows do not
MODEL_NEG_CASES = [dict(id="%s-D%d-C%d-c%d-N%d-f%d" % ((m, d) + sh + (f,)), model=m, d_e=d, shape=sh, flags=f)
                   for m, d, sh, f in (("QuatE", 36, (2, 8, 24), 0), ("QuatE", 36, (2, 8, 24), FORCE_PAIRWISE), ("QuatE", 48, (2, 8, 24), 0),
                                       ("PairRE", 30, (2, 5, 33), 0), ("PairRE", 36, (2, 5, 33), 0),
                                       ("TransH", 8, (2, 5, 33), 0), ("TransH", 36, (2, 5, 33), 0), ("TransH", 36, (1, 12, 20), 0))]
# ranking and top-K on the models' integer-grid tables (tie_inputs: float32 scores are exact, so ranks and order EQUAL the float64
# ones) with 300 entities = relations = candidates and 90 test triples; Eb = 32 leaves a last batch of 26
TIE_N, TIE_E = 300, 90
MODEL_RANK_CASES = [dict(id="%s-D%d-%s" % (m, d, "filt" if filt else "raw"), model=m, d_e=d, filt=filt)
                    for m in NEW_MODELS for d in (16, 36) for filt in (False, True)]
# every kind of CHUNKED_CASES: (kind, chunk, n_cand)
MODEL_CHUNKED_CASES = [dict(id="%s-D36-%s" % (m, kind), model=m, d_e=36, kind=kind, chunk=chunk, n_cand=n)
                       for m in NEW_MODELS for kind, chunk, n in (("all", 8, None), ("lists", 24, 40), ("lists1", 1, 130), ("self", 24, 40))]
MODEL_REL_CASES = [dict(id="QuatE-D%d" % d, model="QuatE", d_e=d) for d in (16, 36)]
# top-K: both modes of TOPK_CASES' table (one row per group against every candidate; groups of rows merged); TransH on both tiles
MODEL_TOPK_CASES = [dict(id="%s-D%d-K%d-g%d" % (m, d, K, g), model=m, d_e=d, K=K, group=g)
                    for m, ds in (("QuatE", (36,)), ("PairRE", (36,)), ("TransH", (16, 36))) for d in ds for K, g in ((10, 1), (128, 9))]


def model_tie_inputs(model, d_e):
    """the model module's tie_inputs at TIE_N entities and TIE_E test triples"""
    Q = model_cases(model)
    saved = Q.TIE_E
    Q.TIE_E = TIE_E
    if hasattr(Q, "TIE_SEEDS"):
        Q.TIE_SEEDS.setdefault((TIE_N, d_e), 0)
    try:
        c = Q.tie_inputs(TIE_N, d_e)
    finally:
        Q.TIE_E = saved
    assert len(c.h) == TIE_E and c.ent.shape == (TIE_N, d_e)
    return c


def chunk_candidates(kind, chunk, n_cand):
    """[ceil(TIE_E / chunk), n_cand] entity ids per chunk, -1 = an empty slot (none in the first column); None: every entity"""
    if n_cand is None:
        return None
    rng = np.random.RandomState(chunk * 1000 + n_cand)
    nch = (TIE_E + chunk - 1) // chunk
    cand = np.stack([rng.choice(TIE_N, n_cand, replace=False) for _ in range(nch)]).astype(np.int64)
    cand[:, 1:][rng.rand(nch, n_cand - 1) < 0.2] = -1
    return cand


# ---- kge_step_optim ------------------------------------------------------------------------------------------------------------
# Cases of adam_cases.py (adam_cases.case at gamma 4: its ambiguity rule then takes out a few per cent of the elements at most -
# AMBIGUITY_CAP, asserted per case in test_workspace_inputs.py), two steps each.  Adam kind: one model of each update family at a
# width that is a multiple of 4 - TransE_l1 sums its GN partials in a stand-alone reduction launch under Adam (the Adagrad step folds
# that into its update) -, a width above 512 (the third instance of the update kernel), the four phase groups one by one, a known
# index.  Adagrad kind: the existing step through the new entry.
def optim_case(cid):
    import adam_cases as A
    import transh_cases as TH
    c = TH.ADAM_CASE if cid == TH.ADAM_CASE["id"] else A.by_id(cid)
    assert c["gamma"] == 4.0, cid
    return c


OPTIM_STEPS = 2
OPTIM_ADAM = [dict(id=i, case=i, phases=False) for i in ("TransE_l2-w16", "TransE_l1-w16", "DistMult-w16", "ComplEx-w16", "QuatE-w16", "PairRE-w16",
                                                         "TransH-w16", "DistMult-w516", "l2-known")] + [
    dict(id="TransE_l1-w16-phases", case="TransE_l1-w16", phases=True), dict(id="l2-known-phases", case="l2-known", phases=True)]
OPTIM_ADAGRAD = ["TransE_l2-w16", "TransE_l1-w16", "l2-known"]


def optim_size(h, cid):
    """kge_step_workspace_bytes of the case's first batch (Adam and Adagrad carve the same layout: the entry has no size of its own)"""
    import adam_cases as A
    from dglke_amd import _lib
    c = optim_case(cid)
    bt = A.batches(c, 1)[0]
    hp = _lib.KgeHParams()
    hp.model = _lib.model_id(c["model"])
    hp.d_e, hp.d_r = A.widths(c)
    hp.flags = NEG_DEG if c["neg_deg"] else 0
    UE, UR = len(np.union1d(bt["nid"], bt["neg"])), len(np.unique(bt["r"]))
    return int(h.kge_step_workspace_bytes(C.byref(hp), c["B"], c["B"] // c["chunk"], c["chunk"], c["N"], UE, UR))


def step_dims(c):
    d_e = 2 * c["hidden"] if c["de"] else c["hidden"]
    d_r = c["d_r"] or (2 * c["hidden"] if c["dr"] else c["hidden"])
    if c["model"] == "RESCAL":
        d_r = d_e * d_e
    return d_e, d_r


def step_hparams(c):
    from dglke_amd import _lib
    hp = _lib.KgeHParams()
    hp.model = _lib.model_id(c["model"])
    hp.d_e, hp.d_r = step_dims(c)
    hp.flags, hp.adv, hp.reg_norm = c["flags"], int(c["adv"]), 3
    hp.gamma, hp.lr, hp.adv_temp, hp.reg_coef, hp.eps, hp.margin = c["gamma"], c["lr"], 1.0, c["reg"], 1e-10, 1.0
    hp.emb_init = (c["gamma"] + 2.0) / c["hidden"]
    return hp


def step_batches(c, steps=2):
    """the case's id batches: tail- then head-corrupted"""
    from oracle import kge_oracle as O
    rng = np.random.RandomState(77)
    return [O.synth_batch(rng, c["n_ent"], c["n_rel"], c["B"], c["N"], c["chunk"], s) for s in range(1, steps + 1)]


def step_tables(c):
    d_e, d_r = step_dims(c)
    rng = np.random.RandomState(5)
    init = (c["gamma"] + 2.0) / c["hidden"]
    ent = rng.uniform(-init, init, (c["n_ent"], d_e)).astype(np.float32)
    rel = rng.uniform(-init, init, (c["n_rel"], d_r)).astype(np.float32)
    proj = rng.uniform(-1.0, 1.0, (c["n_rel"], d_e * d_r)).astype(np.float32) if c["model"] == "TransR" else None
    return ent, rel, proj


def step_size(h, c, which="kge_step_workspace_bytes"):
    """the size function of a step case on the CPU (UE / UR: the union sizes of the first batch)"""
    bt = step_batches(c, 1)[0]
    UE = len(np.unique(np.concatenate([bt["h"], bt["t"], bt["neg"]])))
    UR = len(np.unique(bt["r"]))
    hp = step_hparams(c)
    return int(getattr(h, which)(C.byref(hp), c["B"], c["B"] // c["chunk"], c["chunk"], c["N"], UE, UR))


# modular negative scores: every model (TransR has none), both flag forms; widths with and without the bcast kernels / 16-byte rows
def _neg_cases():
    import modular_op_cases as M
    out = []
    for m, d, N in (("TransE_l1", 48, 24), ("TransE_l1", 36, 24), ("TransE_l2", 36, 24), ("DistMult", 36, 21), ("ComplEx", 72, 24),
                    ("RotatE", 48, 24), ("RotatE", 72, 21), ("SimplE", 36, 24), ("RESCAL", 20, 24), ("TransE_l2", 30, 21), ("RotatE", 32, 64)):
        for f in (0, 1) if m in M.MATRIX_MODELS else (0, 16):
            out.append(M.neg_case(m, 2, 8, N, d, flags=f, scale=0.5, gamma=8.0))
    return out


NEG_CASES = _neg_cases()
LOSS_B, LOSS_N = 37, 21
PNORM_SHAPES = [(37, 30), (1, 7), (300, 36)]

# ranking (inputs and expected ranks: chunked_eval_cases.py - 300 entities, 90 test triples): one model each of the mask-GEMM
# (DistMult, TransE_l2 with its norms), score-block (TransE_l1, RotatE) and TransR families; n_cand below one 64-column strip and
# past one 128-column tile; Eb = 32 < E = 90: the buffers are reused across three passes
RANK_EB = 32
RANK_CASES = [dict(id="%s-h%d-n%d-%s" % (m, h, n, "filt" if filt else "raw"), model=m, hidden=h, n_cand=n, filt=filt)
              for m, h in (("DistMult", 32), ("TransE_l2", 32), ("TransE_l1", 32), ("RotatE", 16), ("TransR", 16))
              for n in (40, 130) for filt in (False, True)]
# chunked: (chunk, n_cand) of chunked_eval_cases.CONFIGS - every entity with chunks of 8 (twelve blocks walked over one chunk's
# workspace), per-chunk lists with empty slots, a ragged last chunk; self_cand
CHUNKED_CASES = [dict(id="%s-h%d-%s" % (m, h, kind), model=m, hidden=h, kind=kind, chunk=chunk, n_cand=n)
                 for m, h in (("DistMult", 32), ("TransE_l2", 32), ("RotatE", 16), ("TransR", 16), ("RESCAL", 8))
                 for kind, chunk, n in (("all", 8, None), ("lists", 24, 40), ("lists1", 1, 130), ("self", 24, 40))]
# relation ranking (relation_rank_cases.py): each kernel family, RotatE, a width not divisible by 4, TransR with d_e != d_r
REL_EB = 64
REL_CASES = [dict(id="%s-h%d-r%d" % (m, h, n), model=m, hidden=h, de=de, n_rel=n)
             for m, h, de in (("DistMult", 32, None), ("TransE_l2", 32, None), ("TransE_l1", 32, None), ("RotatE", 16, None), ("ComplEx", 16, None),
                              ("SimplE", 16, None), ("DistMult", 30, None), ("RESCAL", 12, None), ("TransR", 16, 24)) for n in (7, 130)]
# top-K: at least 1100 candidates (9 tiles: two segments per row; 2100: four).  The rows of a group merge in rounds of
# TK_MCAP / K - 1 = 2047 / 203 / 15 lists at K = 1 / 10 / 128: 2200, 210 and 16 rows take two rounds - both ping-pong halves
TOPK_CASES = [dict(id="%s-h%d-K%d-%s" % (m, h, K, mode), model=m, hidden=h, K=K, H=H, R=R, mode=mode, rows=H * R, n_cand=n)
              for m, h in (("DistMult", 36), ("TransE_l2", 36), ("TransE_l1", 30), ("RotatE", 18))
              for K, H, R, mode, n in ((1, 20, 110, "all", 1100), (10, 1, 210, "batch_head", 2100), (128, 2, 16, "batch_head", 2100))]
# (K, n): one and two merge rounds (lists of K; n / K lists against the same fan)
TOPK_VECTOR = [(1, 5), (1, 3000), (10, 1000), (10, 5000), (128, 1000), (128, 5000), (128, 5120)]


# the sampler job's tail scratch (kge_step_fused_sampling): 32-bit keys with ~30 keys per bucket and chunk != N; nine entities (long
# duplicate runs, buckets of three ids); ids sorted by popularity at NE = 3072 (one bucket takes more than 1024 keys: the
# 16-keys-per-thread instances, whose scan words and unique starts live in the scratch); 64-bit keys (n_ent > 2^20) - the carrying
# steps then train on a table of `table_ent` rows with batches of the same geometry
SAMPLING_CASES = [dict(id=i, n_ent=e, n_rel=r, B=B, N=N, chunk=ch, model=m, skewed=sk, table_ent=tab)
                  for i, e, r, B, N, ch, m, sk, tab in (("k32-spread", 500, 7, 120, 24, 40, "TransE_l2", False, None),
                                                        ("k32-nine", 9, 2, 16, 4, 4, "DistMult", False, None),
                                                        ("k32-big-bucket", 60000, 40, 1024, 256, 256, "ComplEx", True, None),
                                                        ("k64", 3000000, 40, 120, 24, 40, "DistMult", False, 2000))]
SP_CODE_BITS = 12    # csrc/kge_sampler_common.hpp: a key is id << 12 | position; ids beyond 2^(32 - 12) take 64-bit keys


# The step workspace at the geometry of the cases the GPU file takes from other tables (the id batches behind UE / UR are this
# file's): kge_step_grads (emit_message_cases.py: B 64, chunk 16, N 32), kge_step_fused_known (known_negative_cases.py, N = 24 / 40)
# and the steps that carry the sampler jobs.  kge_loss_fwd_bwd and kge_pnorm_pow have no size function and no allocator trace.
OTHER_STEP_SHAPES = (
    [_step("grads-%s-h%d%s" % (m, hd, "-f32" if f else ""), m, hd, B=64, chunk=16, N=32, flags=f, de=m == "RotatE", reg=0.0)
     for m, hd, f in (("TransE_l2", 16, 0), ("TransE_l2", 16, 32), ("DistMult", 16, 0), ("RotatE", 8, 0), ("TransE_l2", 30, 0),
                      ("TransR", 32, 0), ("RESCAL", 16, 0))]
    + [_step("known-N%d" % N, "TransE_l2", 32, B=32, chunk=16, N=N, adv=False, reg=0.0) for N in (24, 40)]
    + [_step("sampling-" + c["id"], c["model"], 32, B=c["B"], chunk=c["chunk"], N=c["N"], de=c["model"] == "ComplEx",
             dr=c["model"] == "ComplEx") for c in SAMPLING_CASES])


def tail_scratch_layout(B, CN, n_ent):
    """(offset, bytes) of the arrays of the tail scratch and its total (csrc/kge_sampler_common.hpp tail_scratch: a fixed layout,
    32-byte aligned, no allocator): header, bucket keys, sorted keys, scan words, unique starts, relation keys"""
    NE, ks = 2 * B + CN, 8 if n_ent > (1 << (32 - SP_CODE_BITS)) else 4
    out, o = [], 0
    for n in (4 * 64, ks * 4 * NE, ks * 4 * NE, 4 * 4 * NE, 4 * 4 * (NE + 1), 8 * B):
        out.append((o, n))
        o = al(o + n, 32)
    return out, al(o, 32)


def size_cases(h):
    """(id, callable() -> need) of every size function at every case's shape - what test_workspace_inputs.py traces"""
    from dglke_amd import _lib
    mid = _lib.model_id
    out = []
    for c in STEP_CASES + [DONOR, DONOR_ALT]:
        out.append(("step-" + c["id"], lambda c=c: step_size(h, c)))
    for c in OTHER_STEP_SHAPES:
        out.append(("step-" + c["id"], lambda c=c: step_size(h, c)))
    for c in MODEL_STEP_CASES + [DONOR_TRANSH]:
        out.append(("step-" + c["id"], lambda c=c: model_step_size(h, c)))
    for cid in sorted({o["case"] for o in OPTIM_ADAM} | set(OPTIM_ADAGRAD)):
        out.append(("optim-" + cid, lambda cid=cid: optim_size(h, cid)))
    for c in ASYNC_CASES:
        out.append(("async-" + c["id"], lambda c=c: step_size(h, c, "kge_step_async_workspace_bytes") // 2))
    # kge_rank_eval / kge_rank_eval_split on every entity (test_rank_eval_split_and_plain)
    out.append(("rank-every-entity", lambda: int(h.kge_rank_workspace_bytes(RANK_EB, 300, rank_dims(RANK_CASES[0])[0]))))
    for c in NEG_CASES:
        out.append(("neg-" + c["id"], lambda c=c: int(h.kge_score_neg_workspace_bytes(mid(c["model"]), c["C"], c["chunk"], c["N"], c["d_e"]))))
    for c in MODEL_NEG_CASES:
        out.append(("neg-" + c["id"], lambda c=c: int(h.kge_score_neg_workspace_bytes(mid(c["model"]), c["shape"][0], c["shape"][1], c["shape"][2], c["d_e"]))))
    for c in MODEL_RANK_CASES:
        out.append(("rank-" + c["id"], lambda c=c: int(h.kge_rank_workspace_bytes(RANK_EB, TIE_N, c["d_e"]))))
    for c in MODEL_CHUNKED_CASES:
        out.append(("chunked-" + c["id"], lambda c=c: int(h.kge_rank_chunked_workspace_bytes(
            mid(c["model"]), c["chunk"], c["chunk"], c["n_cand"] or TIE_N, int(c["kind"] == "self"), c["d_e"], model_d_r(c["model"], c["d_e"])))))
    for c in MODEL_TOPK_CASES:
        out.append(("topk-" + c["id"], lambda c=c: int(h.kge_topk_workspace_bytes(TIE_E, TIE_N, _topk_width(mid(c["model"]), c["d_e"]), c["K"]))))
    for c in RANK_CASES:
        out.append(("rank-" + c["id"], lambda c=c: int(h.kge_rank_workspace_bytes(RANK_EB, c["n_cand"], rank_dims(c)[0]))))
    for c in CHUNKED_CASES:
        d_e, d_r = rank_dims(c)
        out.append(("chunked-" + c["id"], lambda c=c, d_e=d_e, d_r=d_r: int(h.kge_rank_chunked_workspace_bytes(
            mid(c["model"]), c["chunk"], c["chunk"], c["n_cand"] or 300, int(c["kind"] == "self"), d_e, d_r))))
    for c in REL_CASES:
        d_e, d_r = rank_dims(c)
        out.append(("rel-" + c["id"], lambda c=c, d_e=d_e, d_r=d_r: int(h.kge_rank_rel_workspace_bytes(mid(c["model"]), REL_EB, c["n_rel"], d_e, d_r))))
    for c in TOPK_CASES:
        out.append(("topk-" + c["id"], lambda c=c: int(h.kge_topk_workspace_bytes(c["rows"], c["n_cand"], rank_dims(c)[0], c["K"]))))
    for K, n in TOPK_VECTOR:
        out.append(("topk-vector-K%d-n%d" % (K, n), lambda K=K, n=n: int(h.kge_topk_workspace_bytes(0, n, 0, K))))
    return out


def rank_dims(c):
    """(d_e, d_r) of an evaluation case: ComplEx rows are twice the hidden width, RotatE's entity rows are"""
    m, hdn = c["model"], c["hidden"]
    if m in ("ComplEx", "SimplE"):
        return 2 * hdn, 2 * hdn
    if m == "RotatE":
        return 2 * hdn, hdn
    if m == "RESCAL":
        return hdn, hdn * hdn
    return (c.get("de") or hdn), hdn
