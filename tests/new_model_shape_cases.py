"""Case tables and builders that take QuatE, PairRE, TransH and TransD across the tile, slab and list boundaries of their kernels.
Test infrastructure; a plain module, not a conftest.  Shared by
  tests/test_new_model_shape_inputs.py  (CPU): every condition on the inputs, from the float64 statements alone;
  tests/test_gpu_new_model_shapes.py    (GPU): the fused step at these shapes against the float64 step.
The statements are those of tests/quate_cases.py, tests/pairre_cases.py, tests/transh_cases.py and tests/transd_cases.py (general
in B, chunk, N, the table sizes and the width); this module only widens the case tables.

The constants the shapes are chosen against, read from the kernels:
  kge_pairre.hip      QT = 32 (score tile edge), QK = 32 (columns of a backward tile), QS = 32 (staged slab: k of the forward tile,
                      reduction index of a backward tile); pairre_fwd_kernel decodes C * ti * tj tiles, pairre_bwd_kernel
                      C * (ti + tj) * tk, the first C * ti * tk of them row tiles
  kge_neg_pair.hip    PT = 32, PK = 32 (QuatE under FORCE_PAIRWISE where d_e % 16 != 0: `pair32`; `bcast` where d_e % 16 == 0)
  kge_tile_gemm.hpp   TILE_BK = 32 (k per stage of the matrix-core products: QuatE's `gemm` route and the TransH products)
  kge_transh.hip      TH_CT = 32 (columns of a column-sum workgroup: transh_coef_kernel's grid is nb_rows + C * tct)
  kge_transd.hip      TD_CT = 32, TD_CR = 8 (transd_cases.py: columns and row groups of a column-sum workgroup of transd_coef_kernel,
                      grid nb_rows + C * tct; row group rg sums the rows rg, rg + TD_CR, ... of its chunk); td_stack_row: the
                      stacked operand [A ; P] of 2 chunk rows per chunk, k = d_e / 2 columns, STACK_TILE = 32 rows to a row tile
  kge_own_fwd.hpp     own_bwd_products (TransH, TransD): the backward GEMM tiles while max(2 chunk, N) <= GB_MAXK = 2048
                      (kge_neg_gemm.hip; modular_op_cases.py), the pairwise kernels beyond
  kge_rowwise.hip     launch_loss: the register-resident loss rows end at N <= 512, longer rows stream (loss_kernel);
                      launch_update: the register-resident update ends at max(d_e, d_r) <= 1024 floats, 1 / 2 / 4 packs per lane
                      up to 256 / 512 / 1024; wider rows take the generic update_kernel
Relation rows are d_e wide for QuatE and TransD and 2 d_e wide for PairRE and TransH.  A TransD case's d_e is its ROW width 2 k
(rows [e | e_p], [r | r_p]); the shape tables give its half-width k, a multiple of 4.  TransD tables are uniform(-1, 1) times
transd_cases.row_scale(k), which keeps |c_j| = |m_j . n_j| of order 1; TransD leaves out no rows.

Every step starts from the case's fixed tables (tail corruption, then head corruption from the same tables), so that the CPU file
can assert every condition on the inputs of every step.

PairRE and sign ambiguity (pairre_cases.py): gradient, state and table rows fed by a sign-ambiguous element are left out as whole
rows (`pairre_excluded`), at most pairre_cases.ROW_CAP of any compared array.  The share of ambiguous elements grows with
N * d_e * (d_e + 8): uniform tables at d_e >= 400, and at the 600-edge batches of the heavy-list cases where nothing may be left
out, cannot meet the cap under any seed.  Those cases are reshaped (`separated` tables): every entity row is a random sign
vector times a random row scale in [0.5, 2), so |x^_k| = 1 / sqrt(d_e) in every column, and in every relation column one half,
chosen at random, has magnitude in [0.6, 1) and the other in [0.1, 0.45): |a_ik| and |w_ik n^_jk| differ by a factor of at least
4 / 3 and no element is ambiguous (asserted).  The sign of a - w n^ is then the sign of a where the own half dominates and the
sign of -w n^_j, which changes with the candidate, where the other half does: rows, norms, columns and candidates all still matter."""
import functools
import os
import zlib

import numpy as np

import loss_option_cases as L
import pairre_cases as PR
import quate_cases as QE
import transd_cases as TD
import transh_cases as TH
from modular_op_cases import grad_bound, score_bound, worst
from oracle import kge_oracle as O

MODELS = ("QuatE", "PairRE", "TransH", "TransD")
MOD = {"QuatE": QE, "PairRE": PR, "TransH": TH, "TransD": TD}
STACKED = ("TransH", "TransD")      # kge_own_fwd.hpp: the products run over a stacked operand of 2 chunk rows per chunk
QT = QK = QS = 32                   # kge_pairre.hip
PT = PK = 32                        # kge_neg_pair.hip
TILE_BK = 32                        # kge_tile_gemm.hpp
TH_CT = 32                          # kge_transh.hip
TD_CT, TD_CR = TD.TD_CT, TD.TD_CR   # kge_transd.hip
STACK_TILE = 32                     # rows of the stacked operand to a row tile
GB_MAXK = TD.GB_MAXK                # kge_neg_gemm.hip (KGE_NEG_BWD_GEMM_MAXK of own_bwd_products)
LOSS_REG_N = 512                    # kge_rowwise.hip launch_loss
UPDATE_REG_W = 1024                 # kge_rowwise.hip launch_update
QUANTITIES = ("pos_score", "neg_score", "g_pos_ent", "g_neg", "g_rel", "ent_rows", "rel_rows", "ent_state", "rel_state")


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def rel_width(model, d_e):
    return d_e if model in ("QuatE", "TransD") else 2 * d_e


def engine_gamma(model):
    return 12.0 if model == "QuatE" else MOD[model].GAMMA          # (QuatE's score has no margin term)


def option(model, oid):
    """one option set: an id of the model's STEP_CASES, or two or three of them joined by '+' (later ones add what they switch on)"""
    by_id = {c["id"]: c for c in MOD[model].STEP_CASES}
    parts = oid.split("+")
    c = dict(by_id[parts[0]])
    base = dict(by_id["logsigmoid-adv"])
    for p in parts[1:]:
        for k, v in by_id[p].items():
            if k != "id" and v != base[k]:
                c[k] = v
    c["id"] = oid
    return c


def make_case(model, sid, shape, oid, n_ent, n_rel, flags=0, seed=0, separated=False, lr=None):
    C, chunk, N, d_e = shape
    c = option(model, oid)
    c.update(model=model, sid=sid, C=C, B=C * chunk, chunk=chunk, N=N, d_e=d_e, n_ent=n_ent, n_rel=n_rel, flags=flags, seed=seed,
             separated=bool(separated), oid=oid)
    if lr is not None:
        c["lr"] = lr
    c["id"] = "%s-%s-%s-f%d" % (model, sid, oid, flags)
    return c


# --------------------------------------------------------------------------------------------------------------------------
# 1. the fused step at boundary shapes.  (C, chunk, N, d_e); entities / relations few enough that rows repeat inside a batch.
#    With t(x, T) = ceil(x / T) tiles, the last one ragged unless T divides x:
#    s1   (3, 40, 72, 68)   t(40, 32) = 2 row tiles, t(72, 32) = 3 column tiles, t(68, 32) = 3 k slabs / backward column tiles, all
#                           ragged, C = 3: pairre_fwd_kernel's decode with ti = 2, tj = 3, C = 3; pairre_bwd_kernel's split at
#                           nGA = 3 * 2 * 3 = 18 of 45 workgroups and three rounds of its reduction loop (S = 72); TransH's stack
#                           with chunk = 40, transh_coef_kernel with tct = 3; QuatE: quarter 17, scalar packs
#    s2a  (2, 1, 1, 4)      one row, one column, TransH's narrowest width; the stacked operand with chunk = 1
#    s2b  (1, 17, 5, 36)    odd edges inside one tile, two k slabs
#    s3   (3, 20, 28, 36)   --neg_deg_sample: Np = 20 + 28 = 48; chunk no multiple of 16; the diagonal mask; the in-batch rows'
#                           gradients go to the positive trace
#    s4   (2, 8, 520, 32)   N > 512: the loss rows stream, with the positive part in the loss kernel for PairRE and TransH;
#                           t(520, 32) = 17 column tiles
#    s5   (2, 64, 64, 400)  the recipe width: 13 k slabs (the last of 16), relation rows of 800 floats for PairRE and TransH (4 packs
#                           per lane in the update)
#    s6   (1, 32, 32, 516) for PairRE and TransH (relation rows of 1032 floats), (1, 16, 32, 1040) for QuatE (all rows 1040 floats):
#                           beyond the register-resident update
#    QuatE runs every shape under flags 0 and FORCE_PAIRWISE; the route (quate_cases.neg_route):
#      s1 68: gemm | pair32      s2a 4: gemm | pair32      s2b 36: gemm | pair32      s3 36: gemm | pair32
#      s4 32: gemm | bcast       s5 400: gemm | bcast      s6 1040: gemm | bcast
#    TransD reads the last entry as its half-width k (rows 2 k wide; s5: k = 200, the recipe's rows of 400 floats).  What its kernels
#    cross (EXPECT_TRANSD, from TD_CT, TD_CR, STACK_TILE and TILE_BK):
#    s1   the stacked operand of 80 rows per chunk - three row tiles, the last of 16 - with C = 3; tct = 3 column-sum workgroups per
#         chunk, the last of 8 columns; 5 rows per row group; 3 k-stages, the last of 4
#    s2a  m = chunk = 1 in td_stack_row; one column; the narrowest width      s2b  17 rows over 8 row groups (3, 2, 2, ..); 2 k-stages
#    s3   Np = 48: tct = 2, the last of 16; the in-batch rows' gradient joins the corrupted side (GNd of transd_edge_bwd_kernel) after
#         the candidate-row launch of its own        s4  tct = 17        s5  rows of 400 floats       s6  rows of 1032 floats, both tables
#    s7   TransH and TransD only - the route of own_bwd_products, whose stacked operand halves the threshold in chunk:
#    s7a  (1, 1032, 8, 4)   2 chunk = 2064 > GB_MAXK: the pairwise backward products
#    s7b  (1, 8, 2049, 4)   N = 2049 > GB_MAXK: the same branch from the other operand
#    s7c  (1, 1024, 8, 4)   2 chunk = 2048: the last shape on the backward GEMM tiles
#    (TransH: d_e = 4, its narrowest width; TransD: k = 4, rows of 8 floats)
# --------------------------------------------------------------------------------------------------------------------------
SHAPES = {
    #       shape               n_ent n_rel  options
    "s1": ((3, 40, 72, 68), 150, 23, ("logsigmoid-adv", "hinge-pw")),
    "s2a": ((2, 1, 1, 4), 3, 1, ("logsigmoid-adv", "softmax")),
    "s2b": ((1, 17, 5, 36), 20, 4, ("logsigmoid-adv", "softmax")),
    "s3": ((3, 20, 28, 36), 70, 11, ("neg-deg", "neg-deg+reg3")),
    "s4": ((2, 8, 520, 32), 600, 5, ("logsigmoid-adv", "bce", "softmax")),
    "s5": ((2, 64, 64, 400), 300, 13, ("impts+reg3",)),
    "s6": ((1, 32, 32, 516), 50, 6, ("logsigmoid-adv",)),
}
QUATE_S6 = (1, 16, 32, 1040)
S7_SHAPES = {
    "s7a": ((1, 1032, 8, 4), 400, 7, ("logsigmoid-adv",)),
    "s7b": ((1, 8, 2049, 4), 3000, 3, ("logsigmoid-adv",)),
    "s7c": ((1, 1024, 8, 4), 400, 7, ("logsigmoid-adv",)),
}
TRANSD_K = {"s5": 200}              # TransD's half-width where it is not the shape's last entry


def case_shape(model, sid):
    """(C, chunk, N, d_e) of shape `sid` for `model`: QuatE's own s6; TransD: the last entry is k and d_e = 2 k"""
    shape = (SHAPES.get(sid) or S7_SHAPES[sid])[0]
    if sid == "s6" and model == "QuatE":
        return QUATE_S6
    if model == "TransD":
        return shape[:3] + (2 * TRANSD_K.get(sid, shape[3]),)
    return shape


def shape_ids(model):
    return list(SHAPES) + (list(S7_SHAPES) if model in STACKED else [])


# what each shape must produce (asserted by the CPU file from the constants above): row tiles, column tiles, k slabs of the 32-wide
# tilings, and whether the last of each is ragged
EXPECT_TILES = {
    "s1": dict(ti=2, tj=3, tk=3, ragged=(True, True, True)),
    "s2a": dict(ti=1, tj=1, tk=1, ragged=(True, True, True)),
    "s2b": dict(ti=1, tj=1, tk=2, ragged=(True, True, True)),
    "s3": dict(ti=1, tj=2, tk=2, ragged=(True, True, True)),          # (tj over Np = 48)
    "s4": dict(ti=1, tj=17, tk=1, ragged=(True, True, False)),
    "s5": dict(ti=2, tj=2, tk=13, ragged=(False, False, True)),
    "s6": dict(ti=1, tj=1, tk=17, ragged=(False, False, True)),
    ("s6", "QuatE"): dict(ti=1, tj=1, tk=33, ragged=(True, False, True)),
    "s7a": dict(ti=33, tj=1, tk=1, ragged=(True, True, True)),
    "s7b": dict(ti=1, tj=65, tk=1, ragged=(True, True, True)),
    "s7c": dict(ti=32, tj=1, tk=1, ragged=(False, True, True)),
}
# TransD (`transd_tiles`): row tiles of the stacked operand, column-sum workgroups per chunk, (most, fewest) rows of a row group,
# k-stages of the products; ragged: the last row tile, the last column tile, the row groups unequal, the last k-stage
EXPECT_TRANSD = {
    "s1": dict(stack=3, tct=3, rows=(5, 5), kst=3, ragged=(True, True, False, True)),
    "s2a": dict(stack=1, tct=1, rows=(1, 0), kst=1, ragged=(True, True, True, True)),
    "s2b": dict(stack=2, tct=1, rows=(3, 2), kst=2, ragged=(True, True, True, True)),
    "s3": dict(stack=2, tct=2, rows=(3, 2), kst=2, ragged=(True, True, True, True)),          # (tct over Np = 48)
    "s4": dict(stack=1, tct=17, rows=(1, 1), kst=1, ragged=(True, True, False, False)),
    "s5": dict(stack=4, tct=2, rows=(8, 8), kst=7, ragged=(False, False, False, True)),
    "s6": dict(stack=2, tct=1, rows=(4, 4), kst=17, ragged=(False, False, False, True)),
    "s7a": dict(stack=65, tct=1, rows=(129, 129), kst=1, ragged=(True, True, False, True)),
    "s7b": dict(stack=1, tct=65, rows=(1, 1), kst=1, ragged=(True, True, False, True)),
    "s7c": dict(stack=64, tct=1, rows=(128, 128), kst=1, ragged=(False, True, False, True)),
}
# own_bwd_products (TransH, TransD): which kernels take the backward products
EXPECT_BWD = {"s7a": "pair", "s7b": "pair", "s7c": "gemm"}          # every other shape: "gemm"
EXPECT_ROUTES = {("s1", 0): "gemm", ("s1", 1): "pair32", ("s2a", 0): "gemm", ("s2a", 1): "pair32", ("s2b", 0): "gemm",
                 ("s2b", 1): "pair32", ("s3", 0): "gemm", ("s3", 1): "pair32", ("s4", 0): "gemm", ("s4", 1): "bcast",
                 ("s5", 0): "gemm", ("s5", 1): "bcast", ("s6", 0): "gemm", ("s6", 1): "bcast"}
# seeds of the batches and tables, per case id: chosen so that the conditions of the CPU file hold (0 unless listed)
BOUNDARY_SEEDS = {"PairRE-s1-hinge-pw-f0": 2, "QuatE-s2a-softmax-f1": 1, "TransH-s2a-softmax-f0": 4, "PairRE-s4-logsigmoid-adv-f0": 1,
                  "PairRE-s4-softmax-f0": 2, "QuatE-s6-logsigmoid-adv-f0": 9, "QuatE-s6-logsigmoid-adv-f1": 4,
                  "TransD-s1-hinge-pw-f0": 2,           # (seed 0: a hinge pair 0.93 safety units from the kink in the second step)
                  "TransD-s2a-softmax-f0": 5}           # (seed 0: one residual gradient row in either step)


def tiles(c):
    """(ti, tj, tk, ragged) of the 32-wide tilings of a case; columns count the in-batch rows under --neg_deg_sample"""
    Np = c["chunk"] + c["N"] if c["neg_deg"] else c["N"]
    d = c["d_e"]
    t = lambda x, T: (x + T - 1) // T
    return dict(ti=t(c["chunk"], QT), tj=t(Np, QT), tk=t(d, QS), ragged=(c["chunk"] % QT != 0, Np % QT != 0, d % QS != 0))


def transd_tiles(c):
    """what a TransD case gives transd_coef_kernel and the products over the stacked operand (EXPECT_TRANSD)"""
    Np = c["chunk"] + c["N"] if c["neg_deg"] else c["N"]
    m, k, chunk = 2 * c["chunk"], c["d_e"] // 2, c["chunk"]
    t = lambda x, T: (x + T - 1) // T
    return dict(stack=t(m, STACK_TILE), tct=t(Np, TD_CT), rows=(t(chunk, TD_CR), chunk // TD_CR), kst=t(k, TILE_BK),
                ragged=(m % STACK_TILE != 0, Np % TD_CT != 0, chunk % TD_CR != 0, k % TILE_BK != 0))


def bwd_route(c):
    """own_bwd_products' condition (kge_own_fwd.hpp), for the models of STACKED: N counts the in-batch rows under --neg_deg_sample"""
    Np = c["chunk"] + c["N"] if c["neg_deg"] else c["N"]
    return "gemm" if max(2 * c["chunk"], Np) <= GB_MAXK else "pair"


def _boundary_cases():
    out = []
    for sid, (shape, n_ent, n_rel, opts) in list(SHAPES.items()) + list(S7_SHAPES.items()):
        for model in MODELS:
            if sid not in shape_ids(model):
                continue
            sh = case_shape(model, sid)
            for oid in opts:
                for flags in ((0, QE.FORCE_PAIRWISE) if model == "QuatE" else (0,)):
                    c = make_case(model, sid, sh, oid, n_ent, n_rel, flags, separated=(model == "PairRE" and sh[3] >= 400))
                    c["seed"] = BOUNDARY_SEEDS.get(c["id"], 0)
                    out.append(c)
    return out


# --------------------------------------------------------------------------------------------------------------------------
# 2. random shapes: the draws of tests/test_gpu_parity.py::_random_step_case for the three models
# --------------------------------------------------------------------------------------------------------------------------
FUZZ_N = int(os.environ.get("KGE_NEW_MODEL_FUZZ_N", "24"))          # KGE_NEW_MODEL_FUZZ_N=500 for a longer hunt
FUZZ_CHUNK = (1, 3, 7, 8, 16, 17, 33, 40)
FUZZ_NEG = (1, 2, 5, 8, 20, 33, 64, 70)
FUZZ_WIDTH = (4, 8, 12, 20, 32, 36, 48, 64, 100)
# (model, seed) -> dict(seed=, n_ent=, n_rel=): the batch seed and, where no seed will do, the table sizes under which the
# conditions of the CPU file hold; the draws of the shape and the options never change.  (TransH 22 is hinge-pw on 30 entities: a
# sampled negative equal to the edge's own entity leaves residual rows under every seed - transh_cases.residual_rows - so it
# takes the larger entity count.  TransD 6 is hinge at (4, 17, 64, k = 100): under seed 0 one pair of its first step lies 0.94
# safety units from the kink.)  Seeds beyond the default 24 are checked where they run.
FUZZ_FIX = {("QuatE", 1): dict(seed=6), ("PairRE", 14): dict(seed=1), ("TransH", 19): dict(seed=2),
            ("TransH", 22): dict(n_ent=200), ("TransD", 6): dict(seed=1)}


def fuzz_case(model, seed):
    rng = np.random.RandomState(_seed("new-model-fuzz", model, seed))
    chunk = int(rng.choice(FUZZ_CHUNK))
    C = int(rng.randint(1, 5))
    N = int(rng.choice(FUZZ_NEG))
    d_e = int(rng.choice(FUZZ_WIDTH))
    if model == "TransD":           # the draw is the half-width k: rows of 2 k floats, multiples of 8
        d_e = 2 * d_e
    ids = [c["id"] for c in MOD[model].STEP_CASES]
    oid = ids[int(rng.randint(len(ids)))]
    impts = bool(rng.randint(4) == 0)
    flags = int(rng.choice([0, QE.FORCE_PAIRWISE])) if model == "QuatE" else 0
    n_ent, n_rel = int(rng.choice([30, 200])), int(rng.choice([3, 17]))
    fix = FUZZ_FIX.get((model, seed), {})
    c = make_case(model, "fuzz%d" % seed, (C, chunk, N, d_e), oid, fix.get("n_ent", n_ent), fix.get("n_rel", n_rel), flags,
                  seed=fix.get("seed", 0))
    c["impts"] = c["impts"] or impts
    return c


# --------------------------------------------------------------------------------------------------------------------------
# 3. heavy update lists: tests/test_gpu_parity.py::_skewed_batch at B = 600, chunk = 100, N = 64, d_e = 100 on 3000 entities and
#    11 relations, hub_frac 0.15, rel_frac 0.5: entity 7 and relation 1 collect lists well beyond 64 entries.  No -pw
#    (transh_cases.residual_rows).  Nothing is excluded: PairRE takes the `separated` tables.  TransD: k = 52, rows of 104 floats.
# --------------------------------------------------------------------------------------------------------------------------
HEAVY_SHAPE = (6, 100, 64, 100)
HEAVY_K_TRANSD = 52                 # TransD: rows of 104 floats
HEAVY_ENT, HEAVY_REL, HEAVY_HUB, HEAVY_RELF = 3000, 11, 0.15, 0.5
HEAVY_REGS = (0.0, 1e-5)


def heavy_shape(model):
    return HEAVY_SHAPE[:3] + (2 * HEAVY_K_TRANSD,) if model == "TransD" else HEAVY_SHAPE


def heavy_case(model, reg):
    c = make_case(model, "heavy", heavy_shape(model), "logsigmoid-adv", HEAVY_ENT, HEAVY_REL, separated=(model == "PairRE"))
    c.update(reg_coef=reg, reg_norm=3, heavy=True)
    c["id"] = "%s-heavy-reg%g" % (model, reg)
    return c


def skewed_batch(rng, n_ent, n_rel, B, N, chunk, step, hub_frac, rel_frac):
    from test_gpu_parity import _skewed_batch            # (numpy only; the module imports torch)
    return _skewed_batch(rng, n_ent, n_rel, B, N, chunk, step, hub_frac, rel_frac)


# --------------------------------------------------------------------------------------------------------------------------
# builders
# --------------------------------------------------------------------------------------------------------------------------
def tables(c):
    """float32 (ent [n_ent, d_e], rel [n_rel, rel_width])"""
    model, d_e = c["model"], c["d_e"]
    rng = np.random.RandomState(_seed("new-model-tables", model, c["sid"], d_e, c["seed"]))
    if c["separated"]:
        sign = lambda *s: np.where(rng.randint(0, 2, s) == 1, 1.0, -1.0)
        ent = sign(c["n_ent"], d_e) * rng.uniform(0.5, 2.0, (c["n_ent"], 1))
        big = sign(c["n_rel"], d_e) * rng.uniform(0.6, 1.0, (c["n_rel"], d_e))
        small = sign(c["n_rel"], d_e) * rng.uniform(0.1, 0.45, (c["n_rel"], d_e))
        own = rng.randint(0, 2, (c["n_rel"], d_e)) == 1
        rel = np.concatenate([np.where(own, big, small), np.where(own, small, big)], 1)
        return ent.astype(np.float32), rel.astype(np.float32)
    if model == "TransD":           # the condition under which transd_cases.py keeps |c_j| of order 1
        sc = np.float32(TD.row_scale(d_e // 2))
        return (rng.uniform(-1, 1, (c["n_ent"], d_e)).astype(np.float32) * sc,
                rng.uniform(-1, 1, (c["n_rel"], d_e)).astype(np.float32) * sc)
    return (rng.uniform(-1, 1, (c["n_ent"], d_e)).astype(np.float32),
            rng.uniform(-1, 1, (c["n_rel"], rel_width(model, d_e))).astype(np.float32))


def batches(c, steps=2, skewed=None):
    """tail then head corruption; w: edge importance or None"""
    rng = np.random.RandomState(_seed("new-model-batch", c["id"], c["seed"]))
    out = []
    for s in range(1, steps + 1):
        if c.get("heavy"):
            bt = (skewed or skewed_batch)(rng, c["n_ent"], c["n_rel"], c["B"], c["N"], c["chunk"], s, HEAVY_HUB, HEAVY_RELF)
        else:
            bt = O.synth_batch(rng, c["n_ent"], c["n_rel"], c["B"], c["N"], c["chunk"], s)
        bt["w"] = rng.uniform(0.5, 1.5, c["B"]).astype(np.float32) if c["impts"] else None
        out.append(bt)
    return out


def statement_step(c, bt, ent, rel, dtype=np.float64):
    """the model's statement from tables `ent`, `rel` cast to `dtype`, fresh Adagrad states:
    (out, ent_after, ent_state, rel_after, rel_state)"""
    e, r = ent.astype(dtype), rel.astype(dtype)
    es, rs = np.zeros(len(e), dtype), np.zeros(len(r), dtype)
    out = MOD[c["model"]].step(c, e, es, r, rs, bt)
    return out, e, es, r, rs


def list_lengths(bt):
    """(longest entity update list, longest relation update list): occurrences of one id among the edges' heads and tails and the
    sampled negatives / among the edges' relations"""
    ids = np.concatenate([bt["h"], bt["t"], bt["neg"]])
    return int(np.bincount(ids).max()), int(np.bincount(bt["r"]).max())


# --------------------------------------------------------------------------------------------------------------------------
# exclusions
# --------------------------------------------------------------------------------------------------------------------------
NO_ROWS = dict(slots=[], edges=[], pos_local=[], ent=[], rel=[])


def union(a, b):
    return {k: sorted(set(a[k]) | set(b[k])) for k in NO_ROWS}


def _rows_of(bt, edges, slots, in_batch, chunk):
    """the compared rows fed by tainted edges, sampled-negative slots and in-batch columns (chunk index, column)"""
    own = bt["h"] if bt["neg_head"] else bt["t"]
    ents = set(int(bt["neg"][s]) for s in slots)
    for ch, j in in_batch:
        ents.add(int(own[ch * chunk + j]))
    for i in edges:
        ents.update((int(bt["h"][i]), int(bt["t"][i])))
    rels = set(int(bt["r"][i]) for i in edges)
    nid = bt["nid"]
    in_pos = sorted(e for e in ents if nid[min(np.searchsorted(nid, e), len(nid) - 1)] == e)
    return dict(slots=sorted(slots), edges=sorted(edges), pos_local=np.searchsorted(nid, in_pos).tolist() if in_pos else [],
                ent=sorted(ents), rel=sorted(rels))


def pairre_excluded(c, bt, ent, rel):
    """the rows a sign-ambiguous element feeds (pairre_cases.ambiguous / ambiguous_pos on the float64 tables), and the number of
    ambiguous pairs"""
    e, r = ent.astype(np.float64), rel.astype(np.float64)
    chunk, N, B = c["chunk"], c["N"], c["B"]
    C = B // chunk
    h, t, rr, neg = e[bt["h"]], e[bt["t"]], r[bt["r"]], e[bt["neg"]]
    x = t if bt["neg_head"] else h
    a, w = PR.pair(bt["neg_head"], x, rr)
    if c["neg_deg"]:
        Np = chunk + N
        y = (h if bt["neg_head"] else t).reshape(C, chunk, -1)
        neg_all = np.concatenate([y, neg.reshape(C, N, -1)], 1).reshape(C * Np, -1)
    else:
        Np, neg_all = N, neg
    amb = PR.ambiguous(a, w, neg_all, C, chunk, Np)
    if c["neg_deg"]:
        amb[:, np.arange(chunk), np.arange(chunk)] = False           # (the masked own columns are not compared pairs)
    ap = PR.ambiguous_pos(h, rr, t)
    edges = set(np.nonzero(amb.any(2).reshape(-1) | ap)[0].tolist())
    cols = amb.any(1)                                                # [C, Np]
    slots = set((ch * N + j - (Np - N)) for ch, j in zip(*np.nonzero(cols)) if j >= Np - N)
    in_batch = [(int(ch), int(j)) for ch, j in zip(*np.nonzero(cols)) if j < Np - N]
    return _rows_of(bt, edges, slots, in_batch, chunk), int(amb.sum() + ap.sum())


def check_row_cap(c, bt, excl, cap, tag):
    C = c["B"] // c["chunk"]
    for what, rows, total in (("g_neg", excl["slots"], C * c["N"]), ("g_rel", excl["edges"], c["B"]),
                              ("g_pos_ent", excl["pos_local"], len(bt["nid"])), ("entity table", excl["ent"], c["n_ent"]),
                              ("relation table", excl["rel"], c["n_rel"])):
        assert len(rows) <= cap * total, "%s: %d of %d rows of %s excluded" % (tag, len(rows), total, what)


KINK_SAFETY = 8.0


def kink_clearance(c, out, out32):
    """Hinge: the smallest |v| over the pairs of the float64 step `out` (v: the hinge's argument, loss_option_cases.hinge_v), in
    units of KINK_SAFETY x the largest score error of the float32 statement `out32` of the same step (twice that under -pw, where v
    holds two scores).  The kernels sum in another order than the float32 statement but at the same precision over the same
    terms: above 1, a float32 evaluation does not carry a pair across the kink, and the flip rule of
    tests/test_gpu_loss_options.py (at most 1e-4 of the pairs: none, at these sizes) has nothing to exclude.  None for the other
    genres."""
    if c["genre"] != "Hinge":
        return None
    pos, neg = out["pos_score"], out["neg_score"].reshape(c["B"], -1)
    err = max(float(np.abs(out32["pos_score"] - pos).max()), float(np.abs(out32["neg_score"].reshape(neg.shape) - neg).max()))
    unit = KINK_SAFETY * max(err, 2.0 ** -24) * (2.0 if c["pairwise"] else 1.0)
    vp, vn = L.hinge_v(c, pos, neg)
    if c["neg_deg"]:          # the masked own columns score exactly 0 in every precision
        k = np.arange(c["B"])
        vn = vn.copy()
        vn[k, k % c["chunk"]] = np.inf
    clear = float(np.abs(vn).min()) / unit
    if vp is not None:
        clear = min(clear, float(np.abs(vp).min()) / unit)
    return clear


def conditions(c, skewed=None):
    """the conditions on the inputs of a case, both steps, from the float64 (and float32) statements alone:
    (violations: list of str, facts: list of dict per step)"""
    bad, facts = [], []
    ent, rel = tables(c)
    heavy = bool(c.get("heavy"))
    for k, bt in enumerate(batches(c, skewed=skewed)):
        tag = "%s step %d" % (c["id"], k + 1)
        out = statement_step(c, bt, ent, rel)[0]
        f = dict(lists=list_lengths(bt), excluded=dict(NO_ROWS), ambiguous=0)
        for key in ("pos_score", "neg_score", "g_pos_ent", "g_neg", "g_rel"):
            if not np.isfinite(out[key]).all():
                bad.append(tag + ": non-finite " + key)
        # no gradient row is a cancellation residual (transh_cases.residual_rows; model-independent), and the step moves something
        if TH.residual_rows(out):
            bad.append(tag + ": %d residual gradient rows" % TH.residual_rows(out))
        if not (np.abs(out["g_pos_ent"]).max() > 0 and np.abs(out["g_rel"]).max() > 0):
            bad.append(tag + ": an all-zero gradient trace")
        # update lists longer than one exist (where the batch is large enough to hold one)
        if f["lists"][0] < 2 and c["B"] * 2 + c["C"] * c["N"] > c["n_ent"]:
            bad.append(tag + ": no entity update list longer than one")
        if f["lists"][1] < 2 and c["B"] > c["n_rel"]:
            bad.append(tag + ": no relation update list longer than one")
        if heavy and min(f["lists"]) <= 64:
            bad.append(tag + ": heavy lists of only %r entries" % (f["lists"],))
        if c["model"] == "PairRE":
            excl, n_amb = pairre_excluded(c, bt, ent, rel)
            f["excluded"], f["ambiguous"] = excl, n_amb
            if c["separated"] and n_amb:
                bad.append(tag + ": %d sign-ambiguous pairs on separated tables" % n_amb)
            try:
                check_row_cap(c, bt, excl, PR.ROW_CAP, tag)
            except AssertionError as e:
                bad.append(str(e))
        if c["model"] == "TransH":
            f["share"] = out["share"]
            if not out["share"] >= TH.DIST_SHARE:
                bad.append(tag + ": distance share %.3g" % out["share"])
        if c["model"] == "TransD":
            f["share"], f["cmax"] = out["share"], out["cmax"]
            if not out["share"] >= TD.DIST_SHARE:
                bad.append(tag + ": distance share %.3g" % out["share"])
            if not out["cmax"] < TD.C_MAX:
                bad.append(tag + ": |c_j| reaches %.3g" % out["cmax"])
        if c["genre"] == "Hinge":
            out32 = statement_step(c, bt, ent, rel, np.float32)[0]
            f["kink"] = kink_clearance(c, out, out32)
            if not f["kink"] > 1.0:
                bad.append(tag + ": a hinge pair %.3g safety units from the kink" % f["kink"])
            fl = L.hinge_flips(c, bt, out32["pos_score"], out32["neg_score"], out["pos_score"], out["neg_score"])
            if fl["n_flips"]:
                bad.append(tag + ": the float32 statement flips %d hinge pairs" % fl["n_flips"])
        facts.append(f)
    return bad, facts


# --------------------------------------------------------------------------------------------------------------------------
# the comparison of a step (lifted from _compare_step of tests/test_gpu_quate.py / test_gpu_pairre.py / test_gpu_transh.py; the same
# quantities and bounds, with whole rows left out and a per-quantity bound factor)
# --------------------------------------------------------------------------------------------------------------------------
def _keep(n, rows):
    k = np.ones(n, bool)
    k[list(rows)] = False
    return k


def step_errors(c, bt, got, ref, excl=NO_ROWS, factor=None, kernel_layout=True, ent0=None):
    """{quantity: (error / bound, error, bound)} of `got` against the float64 step `ref` = statement_step(...).
    got: pos_score, neg_score, g_pos_ent (rows in the order of bt['nid']), g_neg, g_rel, ent, rel, ent_state, rel_state.
    kernel_layout: g_neg is the kernel's - under --neg_deg_sample [C, chunk + N] rows of which the sampled ones are compared, without
    their regulariser (the update kernel adds it in this mode; ent0: the tables the step started from)."""
    out, ent64, es64, rel64, rs64 = ref
    factor = factor or {}
    chunk, N = c["chunk"], c["N"]
    g_neg, ref_gneg = np.asarray(got["g_neg"]), out["g_neg"]
    if c["neg_deg"] and kernel_layout:
        g_neg = g_neg.reshape(-1, chunk + N, g_neg.shape[1])[:, chunk:].reshape(-1, g_neg.shape[1])
        if c["reg_coef"] > 0:
            ref_gneg = ref_gneg - O.reg_grad(ent0[bt["neg"]], c["reg_coef"], c["reg_norm"])
    pairs = (("pos_score", got["pos_score"], out["pos_score"], score_bound(out["pos_score"]), None),
             ("neg_score", np.asarray(got["neg_score"]).reshape(out["neg_score"].shape), out["neg_score"], score_bound(out["neg_score"]), None),
             ("g_pos_ent", got["g_pos_ent"], out["g_pos_ent"], grad_bound(out["g_pos_ent"]), excl["pos_local"]),
             ("g_neg", g_neg, ref_gneg, grad_bound(out["g_neg"]), excl["slots"]),
             ("g_rel", got["g_rel"], out["g_rel"], grad_bound(out["g_rel"]), excl["edges"]),
             ("ent_rows", got["ent"], ent64, grad_bound(ent64), excl["ent"]),
             ("rel_rows", got["rel"], rel64, grad_bound(rel64), excl["rel"]),
             ("ent_state", got["ent_state"], es64, grad_bound(es64), excl["ent"]),
             ("rel_state", got["rel_state"], rs64, grad_bound(rs64), excl["rel"]))
    errs = {}
    for name, g, r, bound, rows in pairs:
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        bound = np.broadcast_to(bound, r.shape) * factor.get(name, 1.0)
        if rows is not None and len(rows):
            keep = _keep(len(r), rows)
            g, r, bound = g[keep], r[keep], bound[keep]
        errs[name] = worst(g, r, bound)
    return errs


def may_relax(c):
    """the shapes whose accumulation length alone may put float32 beyond a bound of the suite"""
    return c["d_e"] >= 400 or c["N"] >= 520


@functools.lru_cache(maxsize=None)
def _f32_statement(cid, step):
    c = _CASES[cid]
    bt = batches(c)[step]
    ent, rel = tables(c)
    ref = statement_step(c, bt, ent, rel, np.float64)
    o32, e32, es32, r32, rs32 = statement_step(c, bt, ent, rel, np.float32)
    excl = pairre_excluded(c, bt, ent, rel)[0] if c["model"] == "PairRE" else NO_ROWS
    got = dict(pos_score=o32["pos_score"], neg_score=o32["neg_score"], g_pos_ent=o32["g_pos_ent"], g_neg=o32["g_neg"],
               g_rel=o32["g_rel"], ent=e32, rel=r32, ent_state=es32, rel_state=rs32)
    return step_errors(c, bt, got, ref, excl, kernel_layout=False)


_CASES = {}


def f32_statement_errors(c, step):
    """the same statement in np.float32 against float64, per quantity (error / bound, error, bound) - a measurement of what the
    accumulation length alone costs at this shape; cached per case and step"""
    _CASES[c["id"]] = c
    return _f32_statement(c["id"], step)


def bound_factors(c, step):
    """{quantity: factor on the suite's bound}: where the float32 statement itself is over the bound of a quantity (shapes of
    `may_relax` only), that bound becomes 3 x the float32 statement's own error - the rule tests/test_gpu_modular_ops.py applies to
    its coincident pair.  Never derived from a kernel's output."""
    if not may_relax(c):
        return {}
    return {k: 3.0 * v[0] for k, v in f32_statement_errors(c, step).items() if v[0] > 1.0}


BOUNDARY_CASES = _boundary_cases()
HEAVY_CASES = [heavy_case(m, reg) for m in MODELS for reg in HEAVY_REGS]


# --------------------------------------------------------------------------------------------------------------------------
# 4. ranking and top-K over several tiles: 300 entities = 300 relations (three 128-column tiles, the last of 44) and 150 test
#    triples (two 128-row tiles of rank_gemm_kernel / the pair tiles, three of rank_gemm_transh_kernel's 64-query tiles, the last
#    ragged).  Ranker batches (Eb of rank_eval_impl): 150 - one call, every row tile of it - and 64 - three calls, two of them
#    with e0 > 0 into the filter lists.  Chunked ranking takes chunks of 100 triples: the second chunk spans two row tiles.
#    TransD ranks on rank_gemm_transd_kernel's 64-query tiles too; its widths are half-widths k (rows 64 and 72 wide) and it has no
#    relation ranking.
#    Exact tables: the TIE_WIDE_CASES of the four case modules.  Random tables: uniform, same sizes; ranks must lie in the band
#    [lo, hi] of the float64 scores under the score tolerance of tests/test_gpu_eval.py.
# --------------------------------------------------------------------------------------------------------------------------
RANK_N, RANK_E, RANK_WIDTHS = 300, 150, (32, 36)
RANK_BATCHES = (150, 64)
RANK_CHUNK = 100
RANK_TOPK = (1, 10, 128)
RANK_LIST = 200                 # the explicit candidate list: 200 distinct entities in random order, two column tiles
RANK_DEGENERATE = 0.90          # share of the rank intervals that must be a single rank
RANK_ROW_TILES = {"QuatE": 128, "PairRE": 128, "TransH": 64, "TransD": 64}      # kge_tile_gemm.hpp TILE_BM; kge_rank_gemm.hip RANK_TH_BM
#                                                   (rank_gemm_transh_kernel and rank_gemm_transd_kernel: RANK_TH_BM queries)
RANK_COL_TILE = 128                                               # kge_tile_gemm.hpp TILE_BN
assert all(m.TIE_WIDE_CASES == [(RANK_N, d) for d in RANK_WIDTHS] and m.TIE_WIDE_E == RANK_E and m.TIE_WIDE_CHUNK == RANK_CHUNK
           for m in MOD.values())


def rank_list(n=RANK_N):
    return np.random.RandomState(_seed("new-model-rank-list", n)).permutation(n)[:RANK_LIST].astype(np.int64)


@functools.lru_cache(maxsize=None)
def rank_random_inputs(model, d_e):
    """uniform tables, RANK_E test triples and known triples: the test triples and, for each of the first 60 of them, two known
    corruptions of either side (so that the filter lists of a later Ranker batch are not empty)"""
    rng = np.random.RandomState(_seed("new-model-rank-random", model, d_e))
    c = PR.Case()
    if model == "TransD":           # `d_e` is the half-width k, as for transd_cases.tie_inputs: rows of 2 k floats times row_scale(k)
        c.n, c.k, c.d_e = RANK_N, d_e, 2 * d_e
        sc = np.float32(TD.row_scale(d_e))
        c.ent = rng.uniform(-1, 1, (RANK_N, 2 * d_e)).astype(np.float32) * sc
        c.rel = rng.uniform(-1, 1, (RANK_N, 2 * d_e)).astype(np.float32) * sc
    else:
        c.n, c.d_e = RANK_N, d_e
        c.ent = rng.uniform(-1, 1, (RANK_N, d_e)).astype(np.float32)
        c.rel = rng.uniform(-1, 1, (RANK_N, rel_width(model, d_e))).astype(np.float32)
    c.h, c.r, c.t = (rng.randint(0, RANK_N, RANK_E) for _ in range(3))
    extra = []
    for i in list(range(30)) + list(range(RANK_E - 30, RANK_E)):
        for e in rng.randint(0, RANK_N, 2):
            extra.append((c.h[i], c.r[i], int(e)))
        for e in rng.randint(0, RANK_N, 2):
            extra.append((int(e), c.r[i], c.t[i]))
    extra = np.array(extra, np.int64)
    c.kh, c.kr, c.kt = (np.concatenate([x, extra[:, k]]) for k, x in enumerate((c.h, c.r, c.t)))
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def rank_scores(model, c, neg_head, dtype=np.float64):
    """(p [E], S [E, n]) of the model's statement; the margin is the case module's TIE_GAMMA (QuatE has none)"""
    return MOD[model].tie_scores(c, c.h, c.r, c.t, neg_head, dtype)


def rank_gamma(model):
    return 0.0 if model == "QuatE" else MOD[model].TIE_GAMMA


def rank_band(c, p, S, neg_head, lists=None, cols=None, tol=1e-4):
    """(lo, hi, own) int64 [E]: the lowest and highest rank consistent with scores perturbed by at most `tol`
    (oracle.kge_oracle.rank_eval) among the columns `cols` (all) outside the filter lists.  own: whether the triple's own column is
    counted (it is inside the band by construction - the statement gives it the positive's score - unless the list filters it or
    `cols` leaves it out)."""
    E, n = S.shape
    keep = np.zeros((E, n), bool)
    keep[:, np.arange(n) if cols is None else cols] = True
    if lists is not None:
        for i in range(E):
            keep[i, lists[1][lists[0][i, 0]:lists[0][i, 1]]] = False
    own_col = c.h if neg_head else c.t
    own = keep[np.arange(E), own_col]
    lo = ((S >= p[:, None] + tol) & keep).sum(1) + 1
    hi = ((S >= p[:, None] - tol) & keep).sum(1) + 1
    return lo.astype(np.int64), hi.astype(np.int64), own


def degenerate_share(lo, hi, own):
    """share of the intervals that hold a single rank once the own column - whose score IS the positive's, so that it sits inside
    every band of a raw ranking - is set aside"""
    return float(((hi - lo) == own.astype(np.int64)).mean())
