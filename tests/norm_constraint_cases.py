"""Float64 statement, case table and input builders of the norm constraints (include/kge_hip.h, KGE_FLAG_ENT_NORM_* /
KGE_FLAG_REL_NORM_*; csrc/kge_constrain.hip; dglke_train --ent_norm / --rel_norm).  Test infrastructure; a plain module, not a conftest.
Shared by
  tests/test_norm_constraint_inputs.py   (CPU): the statement against a plain loop, the slice table on both sides, the flag bits, the
                                         refusals of the library and of the command line, the conditions on the inputs of every case;
  tests/test_gpu_norm_constraint.py      (GPU): the launch behind the update of every strict entry, against this statement.

The statement.  A row is `parts` equal slices, each with a mode.  Per slice x (float64 here): n = sqrt(sum x^2);
    clip: x <- x / n only when n > 1;     unit: x <- x / n when n > 0 and n != 1;     a slice that is not scaled keeps its bits.
The slices of a model's rows: dglke_amd/models.py (norm_ent, norm_rel, norm_rel_unit), the same facts as csrc/kge_models.hpp.

The value test.  The strict step is bit-reproducible, so the post-step tables T of an engine WITHOUT the flags are the input of the
constraint launch of an engine WITH them that started from the same tables and took the same batch.  Expected: T with the statement
applied to the rows of the batch's union (unique entities of h, t and the negatives; unique relations).
  1. rows outside the union equal T bit for bit (on a device-built plan this also checks the stale records behind the counts);
  2. slices the statement does not scale equal T bit for bit;
  3. an element of a scaled slice of width p: |x - x64| <= |x64| (p + 8) 2^-24.  A sum of p fp32 squares in any order is off by at
     most about p ulp, the root halves that, the division and the multiplication add one ulp each: (p / 2 + 2) ulp of 2^-24 relative,
     stated with about a factor two.
A slice whose float64 norm lies within (p + 8) 2^-24 of 1 is AMBIGUOUS under clip (fp32 may decide the other way): it is left out of
2 and 3.  At most AMBIGUOUS_CAP of the compared slices may be; and the inputs are built so that the float64 step of the CPU oracle
produces none at all - slice norms start at least NORM_GAP away from 1, between 0.5 and 1.5, and lr is 0.01
(test_norm_constraint_inputs.py asserts it for every case).  Every case also has at least MIX of its compared slices scaled and at
least MIX not scaled: a launch that does nothing, or that scales everything, fails.  Under `unit` an unscaled slice is a zero slice
or one of norm exactly 1: the unit case plants such rows among its negative-only entities and trains with the Hinge criterion at
gamma = margin = 0.1, under which a negative further than 0.2 from every a_i of its chunk has gradient exactly 0 and keeps its bits
through the update."""
import zlib

import numpy as np

import adam_cases as A
import pairre_cases as PR
import sampler_statement as S
import transd_cases as TD
import transh_cases as TH
from oracle import kge_oracle as O

ULP = 2.0 ** -24
AMBIGUOUS_CAP = 0.01
MIX = 0.10
NORM_GAP = 0.05
FLAGS = {"ent": {None: 0, "clip": 2048, "unit": 4096}, "rel": {None: 0, "clip": 8192, "unit": 16384}}      # include/kge_hip.h
# the widest slices the two register-resident instances of csrc/kge_constrain.hip hold (KGE_CONSTRAIN_REG_NARROW / _WIDE, read from
# csrc/kge_constrain.hpp by the CPU test); wider slices run the streaming two-pass instance
BOUNDARIES = (256, 1024)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def slack(p):
    return (p + 8) * ULP


# --------------------------------------------------------------------------------------------------------------------------
# the statement
# --------------------------------------------------------------------------------------------------------------------------
def project64(rows, modes):
    """rows [n, d] (any float dtype) -> (float64 rows after the projection, scaled [n, parts] bool, norms [n, parts] float64);
    modes: one of 'clip' / 'unit' per slice"""
    x = np.array(rows, np.float64)
    n_rows, d = x.shape
    parts = len(modes)
    assert parts > 0 and d % parts == 0
    v = x.reshape(n_rows, parts, d // parts)
    n = np.sqrt((v * v).sum(-1))
    unit = np.array([m == "unit" for m in modes])[None, :]
    scaled = np.where(unit, (n > 0) & (n != 1), n > 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(scaled[..., None], v / n[..., None], v)
    return out.reshape(n_rows, d), scaled, n


def ambiguous(norms, modes, p):
    """[n, parts] bool: the clip slices whose norm is within slack(p) of 1"""
    clip = np.array([m == "clip" for m in modes])[None, :]
    return clip & (np.abs(norms - 1.0) <= slack(p))


def slice_modes(c, table):
    """the modes of the slices of a row of `table` ('ent' / 'rel') in case c, [] where the table is not constrained"""
    from dglke_amd import models
    return models.norm_slices(models.MODELS[c["model"]], table, c[table + "_norm"])


# --------------------------------------------------------------------------------------------------------------------------
# cases: adam_cases.case (the option names every float64 step of the suite reads) + the constraint's own
# --------------------------------------------------------------------------------------------------------------------------
def case(cid, model, hidden, ent_norm, rel_norm, de=False, dr=False, plan="host", entry="fused", optimizer="Adagrad", plant=False, **kw):
    """plan: 'host' (dglke_amd.plan) or 'device' (DeviceSampler; the record arrays are sized for 2 B + C N entities and B relations,
    the actual counts are smaller).  entry: 'fused', 'known' (kge_step_fused_known) or 'tail' (kge_step_fused_sampling with a job)."""
    kw.setdefault("lr", 0.01)
    c = A.case(cid, model, hidden, de, dr, **kw)
    c.update(ent_norm=ent_norm, rel_norm=rel_norm, plan=plan, entry=entry, optimizer=optimizer, plant=plant)
    return c


_SMALL = dict(n_ent=24, n_rel=3, B=8, chunk=4, N=4)
# TransE_l2 entity rows of one slice: 6 (the 4-byte path), 400 (the recipe width, no multiple of 256) and one width on each side of
# both instance boundaries, on the 16-byte path and on the 4-byte path
WIDTHS = (6, 254, 256, 258, 260, 400, 1022, 1024, 1026, 1028)
WIDTH_CASES = [case("l2-w%d" % w, "TransE_l2", w, "clip", None, **_SMALL) for w in WIDTHS]
MODEL_CASES = [
    # rows of 8 in two slices of one 16-byte load each; B = 2, C = 1, N = 1 over three entities: fewer records than a workgroup has
    # wavefronts, on both tables
    case("transd-h4-tiny", "TransD", 4, "clip", "clip", True, True, n_ent=3, n_rel=2, B=2, chunk=2, N=1),
    case("transd-h8", "TransD", 8, "clip", "clip", True, True, n_ent=40, n_rel=5, B=16, chunk=8, N=8),          # four slices
    case("transh-h8", "TransH", 8, "clip", "clip", False, True, n_ent=40, n_rel=5, B=16, chunk=8, N=8),        # d clipped, w unit
    case("pairre-h6", "PairRE", 6, None, "clip", False, True, n_ent=40, n_rel=5, B=16, chunk=8, N=8),          # [rH | rT], 4-byte path
    case("distmult-rel", "DistMult", 16, None, "clip", n_ent=40, n_rel=5, B=16, chunk=8, N=8),
    case("l2-unit", "TransE_l2", 8, "unit", None, n_ent=60, n_rel=4, B=16, chunk=8, N=8, genre="Hinge", gamma=0.1, margin=0.1, plant=True),
    # unit on the other instances: the 4-byte narrow one, the 16-byte wide register one, the streaming one on the 4-byte path
    case("l2-unit-w6", "TransE_l2", 6, "unit", None, n_ent=60, n_rel=4, B=16, chunk=8, N=8, genre="Hinge", gamma=0.1, margin=0.1, plant=True),
    case("l2-unit-w400", "TransE_l2", 400, "unit", None, n_ent=60, n_rel=4, B=16, chunk=8, N=8, genre="Hinge", gamma=0.1, margin=0.1, plant=True),
    case("l2-unit-w1026", "TransE_l2", 1026, "unit", None, n_ent=60, n_rel=4, B=16, chunk=8, N=8, genre="Hinge", gamma=0.1, margin=0.1,
         plant=True),
    case("l2-several-workgroups", "TransE_l2", 16, "clip", "clip", n_ent=400, n_rel=9, B=64, chunk=32, N=32),
    case("distmult-adam", "DistMult", 16, "clip", "clip", optimizer="Adam", n_ent=40, n_rel=5, B=16, chunk=8, N=8),
    case("l2-known", "TransE_l2", 16, "clip", "clip", entry="known", n_ent=40, n_rel=5, B=16, chunk=8, N=8, known=True),
    # device-built plans: 2 B + C N = 48 entity records and 16 relation records are allocated, at most 30 / 5 are real
    case("l2-device-plan", "TransE_l2", 16, "clip", "clip", plan="device", n_ent=30, n_rel=5, B=16, chunk=8, N=8),
    case("distmult-tail", "DistMult", 32, "clip", "clip", plan="device", entry="tail", n_ent=30, n_rel=5, B=16, chunk=8, N=8),
]
CASES = WIDTH_CASES + MODEL_CASES
# a total record count (unique entities + unique relations of the constrained tables) that is no multiple of 4: asserted on the CPU
ODD_RECORDS = "l2-w6"
N_TRAIN = 48        # training triples of a device sampler's case (three batches)
SAMPLER_SEED = 5


def by_id(cid):
    return [c for c in CASES if c["id"] == cid][0]


def _spread_rows(rng, n, d, parts):
    """[n, d] float32: slice k of row i has norm 1 - u (i + k even) or 1 + u (odd), u uniform in [NORM_GAP, 0.5]"""
    p = d // parts
    v = rng.normal(size=(n, parts, p))
    v /= np.sqrt((v * v).sum(-1, keepdims=True))
    u = rng.uniform(NORM_GAP, 0.5, (n, parts))
    side = ((np.arange(n)[:, None] + np.arange(parts)[None, :]) % 2) * 2 - 1
    return (v * (1.0 + side * u)[..., None]).reshape(n, d).astype(np.float32)


def planted_rows(c):
    """the entity ids the unit case plants, none of them an end of a positive edge: (zero rows, rows that are a signed basis vector)"""
    if not c["plant"]:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    n = c["n_ent"]
    return np.arange(n - 16, n - 8), np.arange(n - 8, n)


def tables(c):
    """float32 (ent, rel): the slices the model's rows have (whether constrained or not) start with norms spread over 0.5 .. 1.5"""
    from dglke_amd import models
    m = models.MODELS[c["model"]]
    d_e, d_r = A.widths(c)
    rng = np.random.RandomState(_seed("norm-tables", c["id"], c["seed"]))
    ent, rel = _spread_rows(rng, c["n_ent"], d_e, m.norm_ent), _spread_rows(rng, c["n_rel"], d_r, max(m.norm_rel, 1))
    zero, basis = planted_rows(c)
    ent[zero] = 0.0
    for j, i in enumerate(basis):
        ent[i] = 0.0
        ent[i, j % d_e] = 1.0 if j % 2 else -1.0
    return ent, rel


def sampler_triples(c):
    """(H, R, T) of the device sampler of a plan='device' case (it does not shuffle: its batches are sampler_statement.batch_ids)"""
    rng = np.random.RandomState(_seed("norm-triples", c["id"]))
    return rng.randint(0, c["n_ent"], N_TRAIN), rng.randint(0, c["n_rel"], N_TRAIN), rng.randint(0, c["n_ent"], N_TRAIN)


def batch(c, step=1):
    """the batch of 1-based step `step` (odd: tails corrupted) as the float64 steps of the suite take it"""
    B, N, chunk = c["B"], c["N"], c["chunk"]
    if c["plan"] == "device":
        H, R, T = sampler_triples(c)
        ids = S.batch_ids(H, R, T, None, None, c["n_ent"], B, N, chunk, SAMPLER_SEED, step)
        bt = dict(h=ids["h_gid"], t=ids["t_gid"], r=ids["rel_ids"], neg=ids["neg_ids"], neg_head=bool(ids["neg_head"]), w=None)
        return A._finish(bt, B)
    rng = np.random.RandomState(_seed("norm-batch", c["id"], c["seed"], step))
    n_pos = c["n_ent"] - (16 if c["plant"] else 0)          # planted rows: negatives only
    bt = dict(h=rng.randint(0, n_pos, B).astype(np.int64), t=rng.randint(0, n_pos, B).astype(np.int64),
              r=rng.randint(0, c["n_rel"], B).astype(np.int64), neg=rng.randint(0, c["n_ent"], (B // chunk) * N).astype(np.int64),
              neg_head=step % 2 == 0, w=None)
    if c["plant"]:                  # half of the negative slots name a planted row
        planted = np.concatenate(planted_rows(c))
        bt["neg"] = np.where(rng.rand(len(bt["neg"])) < 0.5, planted[rng.randint(0, len(planted), len(bt["neg"]))], bt["neg"]).astype(np.int64)
    return A._finish(bt, B)


def known_of(c, bt):
    """([B, N] bool, triples) of the 'known' entry's planted index, None otherwise"""
    return A.known_pairs(c, bt) if c["entry"] == "known" else (None, None)


def union(bt):
    """(unique entity ids, unique relation ids) of a batch: the rows a step updates"""
    return np.union1d(np.union1d(bt["h"], bt["t"]), bt["neg"]), np.unique(bt["r"])


def gradients(c, ent, rel, bt, known=None):
    if c["model"] == "TransH":
        return TH.forward_backward(c, ent, rel, bt, known)
    if c["model"] == "TransD":
        return TD.forward_backward(c, ent, rel, bt, known)
    return A.gradients(c, ent, rel, bt, known)


def float64_step(c, ent, rel, bt, known=None):
    """(ent, rel) float64 after ONE unconstrained step of the CPU oracle from zero optimizer state (Adagrad: the reference's trace
    order; Adam: adam_cases.adam_rows on the row sums)"""
    ent, rel = np.array(ent, np.float64), np.array(rel, np.float64)
    out = gradients(c, ent, rel, bt, known)
    if c["optimizer"] == "Adam":
        st = A.zero_state(c, ent, rel)
        (ie, Ge), (ir, Gr) = A.row_sums(out, bt, c["n_ent"], c["n_rel"])
        A.adam_rows(st["ent"], st["ent_mom"], st["ent_cnt"], ie, Ge, c["lr"])
        A.adam_rows(st["rel"], st["rel_mom"], st["rel_cnt"], ir, Gr, c["lr"])
        return st["ent"], st["rel"]
    es, rs = np.zeros(c["n_ent"]), np.zeros(c["n_rel"])
    O.adagrad_update(ent, es, bt["nid"], out["g_pos_ent"], c["lr"])
    O.adagrad_update(ent, es, bt["neg"], out["g_neg"], c["lr"])
    O.adagrad_update(rel, rs, bt["r"], out["g_rel"], c["lr"])
    return ent, rel


def compare(c, table, T, X, ids):
    """the three checks of the value test on one table: T, X float32 [n, d] (post-step without / with the constraint), ids: the
    union's rows.  -> dict(slices, scaled, unscaled, exempt, ratio = largest |x - x64| / (|x64| slack(p)) over the scaled slices'
    elements).  Raises AssertionError on a violated check."""
    modes = slice_modes(c, table)
    tag = "%s %s" % (c["id"], table)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    outside = np.setdiff1d(np.arange(T.shape[0]), ids)
    assert np.array_equal(bits(T[outside]), bits(X[outside])), tag + ": a row outside the union changed"
    if not modes:
        assert np.array_equal(bits(T), bits(X)), tag + ": an unconstrained table changed"
        return dict(slices=0, scaled=0, unscaled=0, exempt=0, ratio=0.0)
    parts, p = len(modes), T.shape[1] // len(modes)
    want, scaled, norms = project64(T[ids], modes)
    amb = ambiguous(norms, modes, p)
    Tv, Xv, Wv = (a.reshape(len(ids), parts, p) for a in (T[ids], X[ids], want))
    keep = ~scaled & ~amb
    assert np.array_equal(bits(Tv[keep]), bits(Xv[keep])), tag + ": a slice the statement does not scale changed"
    sc = scaled & ~amb
    ratio = 0.0
    if sc.any():
        err, ref = np.abs(Xv[sc].astype(np.float64) - Wv[sc]), np.abs(Wv[sc])
        assert np.all(err[ref == 0] == 0), tag + ": a zero element of a scaled slice changed"
        ratio = float((err[ref > 0] / (ref[ref > 0] * slack(p))).max()) if (ref > 0).any() else 0.0
    return dict(slices=int(scaled.size), scaled=int(sc.sum()), unscaled=int(keep.sum()), exempt=int(amb.sum()), ratio=ratio)


def check_mix(c, stats):
    """the conditions on the compared slices of a case (both tables together): AMBIGUOUS_CAP and MIX"""
    tot = sum(s["slices"] for s in stats)
    exempt, scaled, unscaled = (sum(s[k] for s in stats) for k in ("exempt", "scaled", "unscaled"))
    assert tot > 0, c["id"]
    assert exempt <= AMBIGUOUS_CAP * tot, "%s: %d of %d slices are ambiguous" % (c["id"], exempt, tot)
    assert scaled >= MIX * tot and unscaled >= MIX * tot, "%s: %d scaled, %d not scaled of %d slices" % (c["id"], scaled, unscaled, tot)
    return tot, scaled, unscaled, exempt
