"""What the library and the command lines say about each model BEFORE anything is launched: the calls behind
tests/test_model_contract.py and the recorder of its fixture, tests/golden/model_contract.json.

Three families of calls, none of which needs a device:

  refusals   every C entry that takes a model id or a kge_hparams, over MODEL_GRID x DIMS, with NULL tables (refused by the
             argument checks at the latest); the top-K entry also with dummy pointers where the widths are bad, and every entry
             with a workspace, for each model at its own widths, with dummy pointers and a workspace ONE BYTE SHORT.  The return
             code and the text of kge_last_error() are recorded; record() asserts that every one of them is a refusal.
  sizes      every *_workspace_bytes function for each model at SHAPES, with the kge_debug_carve trace: the layout entry by entry.
  python     check_model_widths / check_model_flags of dglke_amd.train and dglke_eval's checks over the flag grid: the KgeError
             text, or None.

Every distinct answer - [return code, text] - is stored once ("answers"); a call records its index, -1 where a command line said
nothing.

The fixture is recorded ONCE, from the library and package of the commit in front of the model table (KGE_LIB selects the
library): `python tests/model_contract_cases.py` writes it.  It is not recorded again from the code it checks."""
import ctypes as C
import itertools
import json
import os

import workspace_cases as W

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_contract.json")
MODEL_GRID = list(range(-1, 17)) + [99]
DIMS = [(16, 16), (16, 32), (16, 8), (8, 8), (12, 12), (4, 8), (6, 36), (0, 0), (2048, 2048)]
NAMES = ["TransE", "TransE_l1", "TransE_l2", "TransR", "RESCAL", "DistMult", "ComplEx", "RotatE", "SimplE", "QuatE", "PairRE",
         "TransH", "TransD"]
# (C, chunk, N, UE, UR, d_e); B = C * chunk
SHAPES = [(2, 8, 24, 20, 3, 32), (1, 4, 3, 5, 2, 16)]
ONE = 1                       # a non-NULL pointer that is never dereferenced
BIG = 1 << 20
NO_PATH = "no_such_model_contract_dir"


def d_r_of(name, d_e):
    """the relation width each model needs next to an entity width d_e (include/kge_hip.h, enum kge_model)"""
    return {"RotatE": d_e // 2, "RESCAL": d_e * d_e, "PairRE": 2 * d_e, "TransH": 2 * d_e}.get(name, d_e)


def topk_dims_bad(model, d_e, d_r):
    """(model, d_e, d_r) that kge_topk_select refuses for its widths: the statement of include/kge_hip.h, written out here so that
    no call with dummy pointers is made unless it is refused.  None: the id or d_e <= 0 is refused earlier, or the widths fit"""
    if model not in (0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 14) or d_e <= 0 or d_r <= 0:
        return None
    ok = {3: d_e % 2 == 0 and d_r == d_e, 5: d_e % 2 == 0 and d_r == d_e, 4: d_e % 2 == 0 and d_r == d_e // 2,
          6: d_e <= 1024 and d_r == d_e * d_e, 8: d_e % 4 == 0 and d_r == d_e, 10: d_r == 2 * d_e,
          12: d_e % 4 == 0 and d_r == 2 * d_e, 14: d_e % 8 == 0 and d_r == d_e}.get(model, d_r == d_e)
    return not ok


def _hp(L, model, d_e, d_r):
    hp = L.KgeHParams()
    hp.model, hp.d_e, hp.d_r = model, d_e, d_r
    return hp


def _batch(L, C_, chunk, N, UE, UR, ptrs):
    b = L.KgeBatch()
    b.B, b.C, b.chunk, b.N, b.UE, b.UR = C_ * chunk, C_, chunk, N, UE, UR
    if ptrs:
        for f in ("h_gid", "t_gid", "rel_ids", "neg_ids", "ue_id", "ue_pos_ptr", "ue_pos_adj", "ue_neg_ptr", "ue_neg_slot", "ur_id",
                  "ur_ptr", "ur_edge", "ue_rec", "ur_rec"):
            setattr(b, f, ONE)
    return b


def null_calls(h, L, pipe, model, d_e, d_r):
    """(entry, call) for every entry that takes a model or a kge_hparams, tables and batch arrays NULL"""
    hp, tb, b = _hp(L, model, d_e, d_r), L.KgeTables(), _batch(L, 1, 4, 3, 5, 2, False)
    sh, em, job, adagrad, adam = L.KgeShards(), L.KgeEmit(), L.KgeSamplerJob(), L.KgeOptim(), L.KgeOptim()
    adam.kind = L.OPT_ADAM
    r = C.byref
    return [
        ("kge_score_pos", lambda: h.kge_score_pos(model, None, None, None, 2, d_e, d_r, 1.0, 1.0, None, None)),
        ("kge_score_pos_bwd", lambda: h.kge_score_pos_bwd(model, None, None, None, None, 2, d_e, d_r, 1.0, 1.0, None, None, None, None)),
        ("kge_score_neg_fwd", lambda: h.kge_score_neg_fwd(model, 0, None, None, None, 2, 8, 24, d_e, d_r, 1.0, 1.0, None, ONE, BIG, 0, None)),
        ("kge_score_neg_bwd", lambda: h.kge_score_neg_bwd(model, 0, None, None, None, None, None, 2, 8, 24, d_e, d_r, 1.0, 1.0, None, None,
                                                          None, ONE, BIG, 0, None)),
        ("kge_step_fused", lambda: h.kge_step_fused(r(hp), r(tb), r(b), None, ONE, BIG, None)),
        ("kge_step_fused_sampling", lambda: h.kge_step_fused_sampling(r(hp), r(tb), r(b), None, ONE, BIG, r(job), None)),
        ("kge_step_fused_known", lambda: h.kge_step_fused_known(r(hp), r(tb), r(b), None, ONE, BIG, None, None, None, 0, None)),
        ("kge_step_phase", lambda: h.kge_step_phase(r(hp), r(tb), r(b), None, ONE, BIG, L.PHASE_ALL, None)),
        ("kge_step_phase_known", lambda: h.kge_step_phase_known(r(hp), r(tb), r(b), None, ONE, BIG, L.PHASE_ALL, None, None, 0, None)),
        ("kge_step_optim:adagrad", lambda: h.kge_step_optim(r(hp), r(adagrad), r(tb), r(b), None, ONE, BIG, L.PHASE_ALL, None, None, 0, None)),
        ("kge_step_optim:adam", lambda: h.kge_step_optim(r(hp), r(adam), r(tb), r(b), None, ONE, BIG, L.PHASE_ALL, None, None, 0, None)),
        ("kge_step_async", lambda: h.kge_step_async(pipe, r(hp), r(tb), r(b), None, None, ONE, BIG, None)),
        ("kge_step_grads", lambda: h.kge_step_grads(r(hp), r(tb), r(b), None, r(em), ONE, BIG, None)),
        ("kge_step_sharded", lambda: h.kge_step_sharded(r(hp), r(sh), r(b), None, ONE, BIG, None)),
        ("kge_rank_eval", lambda: h.kge_rank_eval(model, 0, None, 10, None, 3, None, None, None, 4, d_e, d_r, 1.0, 1.0, None, 0, None, None,
                                                  4, None, None, ONE, BIG, 0, None)),
        ("kge_rank_eval_ex", lambda: h.kge_rank_eval_ex(model, 0, None, 10, None, 3, None, None, None, None, 4, d_e, d_r, 1.0, 1.0, None, 0,
                                                        None, None, 4, None, None, ONE, BIG, 0, None)),
        ("kge_rank_eval_split", lambda: h.kge_rank_eval_split(model, 0, None, 5, None, 5, None, 3, None, None, None, None, 4, d_e, d_r, 1.0,
                                                              1.0, None, 0, None, None, 4, None, None, ONE, BIG, 0, None)),
        ("kge_rank_eval_chunked", lambda: h.kge_rank_eval_chunked(model, 0, None, 10, None, 3, None, None, None, None, 8, d_e, d_r, 1.0, 1.0,
                                                                  4, None, 0, 0, 1, None, None, None, None, ONE, BIG, 0, None)),
        ("kge_rank_rel_eval", lambda: h.kge_rank_rel_eval(model, None, 5, None, 10, None, None, None, None, 4, d_e, d_r, 1.0, 1.0, None, None,
                                                          4, None, None, ONE, BIG, 0, None)),
        ("kge_topk_select", lambda: h.kge_topk_select(model, 0, None, 5, None, 2, None, None, None, 1, d_e, d_r, 0.0, 1.0, None, 5, None, 1,
                                                      1, 3, None, None, ONE, BIG, None)),
        ("kge_topk_select_filtered", lambda: h.kge_topk_select_filtered(model, 0, None, 5, None, 2, None, None, None, 1, d_e, d_r, 0.0, 1.0,
                                                                        None, 5, None, 1, 1, 3, None, None, ONE, BIG, None, None, None)),
    ]


def short_calls(h, L, name, shape):
    """(entry, call) for every entry with a workspace: the model at its own widths, dummy pointers everywhere, ws_bytes one below
    what the size function says (0 where it says 0: the entry is closed to the model)"""
    C_, chunk, N, UE, UR, d_e = shape
    model, d_r, B = L.MODEL_IDS[name], d_r_of(name, d_e), C_ * chunk
    hp, tb, b = _hp(L, model, d_e, d_r), L.KgeTables(), _batch(L, C_, chunk, N, UE, UR, True)
    tb.ent = tb.ent_state = tb.rel = tb.rel_state = tb.proj = tb.proj_state = ONE
    r = C.byref

    def less(n):
        return max(int(n) - 1, 0)
    neg = less(h.kge_score_neg_workspace_bytes(model, C_, chunk, N, d_e))
    step = less(h.kge_step_workspace_bytes(r(hp), B, C_, chunk, N, UE, UR))
    rank = less(h.kge_rank_workspace_bytes(B, L.rank_ws_cands(model, N), d_e))
    chunked = less(h.kge_rank_chunked_workspace_bytes(model, chunk, chunk, N, 1, d_e, d_r))
    rel = less(L.rank_rel_workspace_bytes(model, B, N, d_e, d_r))
    topk = less(L.topk_workspace_bytes(model, B, N, d_e, 3))
    return [
        ("kge_score_neg_fwd", lambda: h.kge_score_neg_fwd(model, 0, ONE, ONE, ONE, C_, chunk, N, d_e, d_r, 1.0, 1.0, ONE, ONE, neg, 0, None)),
        ("kge_score_neg_bwd", lambda: h.kge_score_neg_bwd(model, 0, ONE, ONE, ONE, ONE, ONE, C_, chunk, N, d_e, d_r, 1.0, 1.0, ONE, ONE, ONE,
                                                          ONE, neg, 0, None)),
        ("kge_step_fused", lambda: h.kge_step_fused(r(hp), r(tb), r(b), None, ONE, step, None)),
        ("kge_rank_eval_ex", lambda: h.kge_rank_eval_ex(model, 0, ONE, 50, ONE, 3, ONE, ONE, ONE, ONE, B, d_e, d_r, 1.0, 1.0, ONE, N, None,
                                                        None, B, ONE, None, ONE, rank, 0, None)),
        ("kge_rank_eval_chunked", lambda: h.kge_rank_eval_chunked(model, 0, ONE, 50, ONE, 3, ONE, ONE, ONE, ONE, B, d_e, d_r, 1.0, 1.0, chunk,
                                                                  ONE, N, 0, 1, None, None, ONE, None, ONE, chunked, 0, None)),
        ("kge_rank_rel_eval", lambda: h.kge_rank_rel_eval(model, ONE, 50, ONE, N, ONE, ONE, ONE, ONE, B, d_e, d_r, 1.0, 1.0, ONE, ONE, B, ONE,
                                                          None, ONE, rel, 0, None)),
        ("kge_topk_select", lambda: h.kge_topk_select(model, 0, ONE, 50, ONE, 3, ONE, ONE, ONE, B, d_e, d_r, 0.0, 1.0, ONE, N, ONE, 1, 1, 3,
                                                      ONE, ONE, ONE, topk, None)),
    ]


def size_calls(h, L, name, shape):
    """(function, call) for every *_workspace_bytes function, the model at its own widths"""
    C_, chunk, N, UE, UR, d_e = shape
    model, d_r, B = L.MODEL_IDS[name], d_r_of(name, d_e), C_ * chunk
    hp = _hp(L, model, d_e, d_r)
    r = C.byref
    return [
        ("kge_score_neg_workspace_bytes", lambda: h.kge_score_neg_workspace_bytes(model, C_, chunk, N, d_e)),
        ("kge_step_workspace_bytes", lambda: h.kge_step_workspace_bytes(r(hp), B, C_, chunk, N, UE, UR)),
        ("kge_step_async_workspace_bytes", lambda: h.kge_step_async_workspace_bytes(r(hp), B, C_, chunk, N, UE, UR)),
        ("kge_rank_workspace_bytes", lambda: h.kge_rank_workspace_bytes(B, L.rank_ws_cands(model, N), d_e)),
        ("kge_rank_chunked_workspace_bytes:0", lambda: h.kge_rank_chunked_workspace_bytes(model, B, chunk, N, 0, d_e, d_r)),
        ("kge_rank_chunked_workspace_bytes:1", lambda: h.kge_rank_chunked_workspace_bytes(model, B, chunk, N, 1, d_e, d_r)),
        ("kge_rank_rel_workspace_bytes", lambda: L.rank_rel_workspace_bytes(model, B, N, d_e, d_r)),
        ("kge_topk_workspace_bytes", lambda: L.topk_workspace_bytes(model, B, N, d_e, 3)),
    ]


class Answers(object):
    """the answers of a run - [return code, text]; the command lines: [None, text] - each stored once; a call records its index"""

    def __init__(self):
        self.rows, self.index = [], {}

    def __call__(self, rc, text):
        if (rc, text) not in self.index:
            self.index[(rc, text)] = len(self.rows)
            self.rows.append([rc, text])
        return self.index[(rc, text)]


def collect_c(h, L):
    """{"answers", "null", "topk_dims", "short", "rel_sizes", "sizes"} of the loaded library"""
    msg = Answers()

    def refused(call):
        rc = int(call())
        return msg(rc, h.kge_last_error().decode())
    pipe = C.c_void_p()
    assert h.kge_pipe_create(C.byref(pipe)) == 0
    try:
        null = {}
        for model, (d_e, d_r) in itertools.product(MODEL_GRID, DIMS):
            for entry, call in null_calls(h, L, pipe, model, d_e, d_r):
                null.setdefault(entry, []).append(refused(call))
    finally:
        h.kge_pipe_destroy(pipe)
    topk_dims = []
    for model, (d_e, d_r) in itertools.product(MODEL_GRID, DIMS):
        if topk_dims_bad(model, d_e, d_r):
            topk_dims.append([model, d_e, d_r, refused(lambda: h.kge_topk_select(
                model, 0, ONE, 5, ONE, 2, ONE, ONE, ONE, 1, d_e, d_r, 0.0, 1.0, None, 5, ONE, 1, 1, 3, ONE, ONE, ONE, BIG, None))])
    short, sizes = {}, {}
    for name, shape in itertools.product(NAMES, SHAPES):
        for entry, call in short_calls(h, L, name, shape):
            short.setdefault(entry, []).append(refused(call))
        for fn, call in size_calls(h, L, name, shape):
            with W.Trace(h, 0) as t:
                total = int(call())
                pairs = t.pairs()
            sizes.setdefault(fn, []).append([total] + [x for p in pairs for x in p])
    rel_sizes = [int(h.kge_rank_rel_workspace_bytes(model, 4, 10, d_e, d_r)) for model, (d_e, d_r) in itertools.product(MODEL_GRID, DIMS)]
    return {"answers": msg.rows, "null": null, "topk_dims": topk_dims, "short": short, "rel_sizes": rel_sizes, "sizes": sizes}


def flag_grid():
    """(name, -de, -dr, --hidden_dim, gpus, --async_update_pipeline, --eval_relation)"""
    return itertools.product(NAMES, (False, True), (False, True), (30, 32), ([0], [0, 1]), (False, True), (False, True))


def _argv(name, de, dr, hidden, gpus, pipeline, eval_rel):
    return (["--model_name", name, "--hidden_dim", str(hidden), "--gpu"] + [str(g) for g in gpus] + (["-de"] if de else []) +
            (["-dr"] if dr else []) + (["--eval_relation"] if eval_rel else []), ["--async_update", "--async_update_pipeline"] if pipeline else [])


def collect_python():
    """{"answers", "widths", "train", "eval"}: the KgeError text of each call (an index into "answers"), or -1 for none"""
    from dglke_amd import eval_cli, train as T
    from dglke_amd._lib import KgeError
    msg = Answers()

    def text(call):
        try:
            call()
        except KgeError as e:
            return str(e)
        return None

    def said(call):
        t = text(call)
        return -1 if t is None else msg(None, t)
    widths = [said(lambda: T.check_model_widths(name, hidden, de, dr))
              for name, de, dr, hidden in itertools.product(NAMES, (False, True), (False, True), (30, 32))]
    train, ev = [], []
    for case in flag_grid():
        common, pipe = _argv(*case)
        train.append(said(lambda: T.check_model_flags(T.ArgParser().parse_args(common + pipe))))
        if not case[5]:             # dglke_eval has no update pipeline.  Nothing refused: it stops at the missing model directory
            t = text(lambda: eval_cli.main(common + ["--model_path", NO_PATH]))
            assert t is not None, "dglke_eval went past its checks: %r" % (case,)
            ev.append(-1 if t == "No existing model_path: " + NO_PATH else msg(None, t))
    return {"answers": msg.rows, "widths": widths, "train": train, "eval": ev}


def grid():
    return {"models": MODEL_GRID, "dims": [list(d) for d in DIMS], "names": NAMES, "shapes": [list(s) for s in SHAPES]}


def collect(h, L):
    out = {"grid": grid()}
    out.update(collect_c(h, L))
    out["python"] = collect_python()
    return out


def check_refusals(rec):
    """record() and the test: every recorded call was refused"""
    for section in ("null", "short"):
        for entry, rows in rec[section].items():
            for i, a in enumerate(rows):
                rc, text = rec["answers"][a]
                assert rc != 0 and text, "%s[%d] of %s was not refused" % (entry, i, section)
    for row in rec["topk_dims"]:
        rc, text = rec["answers"][row[3]]
        assert rc != 0 and "kge_topk_select: " in text, row


def record():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib as L
    rec = collect(L.lib(), L)
    check_refusals(rec)
    write(rec)
    return rec


def write(rec):
    """the fixture, one line per entry of a section"""
    def line(v):
        return json.dumps(v, separators=(",", ":"))

    def block(v):
        if isinstance(v, dict):
            return "{\n" + ",\n".join("%s:%s" % (line(k), block(x) if isinstance(x, dict) else line(x)) for k, x in v.items()) + "\n}"
        return line(v)
    with open(FIXTURE, "w") as f:
        f.write(block(rec) + "\n")


if __name__ == "__main__":
    import sys
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-ke_amd")]
    rec = record()
    print("wrote %s: %d bytes, %d answers" % (FIXTURE, os.path.getsize(FIXTURE), len(rec["answers"])))
