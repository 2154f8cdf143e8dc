"""CPU guard of the norm-constraint tests (tests/norm_constraint_cases.py): the float64 statement against a plain loop, the slice
table of dglke_amd/models.py against csrc/kge_models.hpp, the flag bits, the instance boundaries the case table names, the
conditions on the inputs of every case - no ambiguous slice and a mix of scaled and unscaled ones after the CPU oracle's float64
step - and the refusals of the C ABI and of the command line (no GPU: argument errors are reported before any launch)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import norm_constraint_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))
CSRC = os.path.join(ROOT, "dgl-ke_amd", "csrc")
BITS = dict(ENT_NORM_CLIP=2048, ENT_NORM_UNIT=4096, REL_NORM_CLIP=8192, REL_NORM_UNIT=16384)


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib
    return _lib


# --------------------------------------------------------------------------------------------------------------------------
# the statement
# --------------------------------------------------------------------------------------------------------------------------
def test_statement_equals_a_plain_loop():
    rng = np.random.RandomState(3)
    for parts, modes in ((1, ["clip"]), (1, ["unit"]), (2, ["clip", "unit"]), (2, ["unit", "clip"]), (3, ["clip"] * 3)):
        x = rng.normal(size=(9, 6 * parts)).astype(np.float32) * rng.uniform(0.05, 0.6, (9, 1)).astype(np.float32)
        x[1] = 0.0
        x[2, :6] = 0.0
        x[3] = 0.0
        x[3, 0] = -1.0                                              # slices of norm exactly 1
        x[3, 6 * (parts - 1)] = -1.0
        x[4, 2] = np.nan
        got, scaled, norms = Q.project64(x, modes)
        for i in range(len(x)):
            for k, mode in enumerate(modes):
                v = [float(a) for a in x[i, 6 * k:6 * k + 6]]
                n = sum(a * a for a in v) ** 0.5
                do = (n > 0 and n != 1) if mode == "unit" else n > 1
                want = [a / n for a in v] if do else v
                assert bool(scaled[i, k]) == do and (norms[i, k] == n or (np.isnan(n) and np.isnan(norms[i, k])))
                assert np.array_equal(got[i, 6 * k:6 * k + 6], np.array(want), equal_nan=True), (parts, modes, i, k)
        assert not scaled[1].any() and not scaled[3, 0] and not scaled[3, -1] and not scaled[4, 0]      # zero, unit and NaN slices
    # clipped rows have norm <= 1, unit rows norm 1, to the last float64 bit or two
    x = rng.normal(size=(50, 8))
    assert np.all(np.sqrt((Q.project64(x, ["clip"])[0] ** 2).sum(-1)) <= 1 + 4e-16)
    assert np.allclose(np.sqrt((Q.project64(x, ["unit"])[0] ** 2).sum(-1)), 1.0, rtol=0, atol=4e-16)
    # the ambiguity rule: clip slices only, within (p + 8) 2^-24 of 1
    n = np.array([[1.0, 1.0 + 13 * Q.ULP, 1.0 - 15 * Q.ULP, 1.0 - 13 * Q.ULP]])
    assert Q.ambiguous(n, ["clip"] * 4, 6).tolist() == [[True, True, False, True]]
    assert not Q.ambiguous(n, ["unit"] * 4, 6).any()


# --------------------------------------------------------------------------------------------------------------------------
# the slice table, the bits, the boundaries
# --------------------------------------------------------------------------------------------------------------------------
def _c_slices():
    """model name -> (ent parts, rel parts, rel unit mask, refused?) read from the rows of csrc/kge_models.hpp"""
    text = open(os.path.join(CSRC, "kge_models.hpp")).read()
    rows = re.findall(r'\{KGE_\w+, "(\w+)",[^{}]*\{(\d+), (\d+), (\d+), (nullptr|\w+)\}\}', text)
    return {name: (int(e), int(r), int(u), why != "nullptr") for name, e, r, u, why in rows}


def test_slice_tables_agree_on_both_sides():
    from dglke_amd import models
    c = _c_slices()
    py = {m.name: (m.norm_ent, m.norm_rel, m.norm_rel_unit, m.no_rel_norm is not None) for m in models.MODELS.values() if not m.alias_of}
    assert c == py and len(c) == 12
    want = dict(TransE_l1=(1, 1), TransE_l2=(1, 1), DistMult=(1, 1), ComplEx=(1, 1), SimplE=(1, 1), QuatE=(1, 1), RotatE=(1, 0),
                RESCAL=(1, 0), TransR=(1, 0), PairRE=(1, 2), TransH=(1, 2), TransD=(2, 2))
    assert {k: v[:2] for k, v in py.items()} == want
    assert {k for k, v in py.items() if v[2]} == {"TransH"} and py["TransH"][2] == 2          # w, the second half, always unit
    assert {k for k, v in py.items() if v[3]} == {"RotatE", "RESCAL", "TransR"}
    for name in ("RESCAL", "TransR"):
        assert models.own_relation_update(models.MODELS[name])
    M = models.MODELS
    assert models.norm_slices(M["TransH"], "rel", "clip") == ["clip", "unit"] and models.norm_slices(M["TransH"], "rel", "unit") == ["unit"] * 2
    assert models.norm_slices(M["TransH"], "ent", "clip") == ["clip"] and models.norm_slices(M["TransD"], "ent", "unit") == ["unit"] * 2
    assert models.norm_slices(M["PairRE"], "rel", "clip") == ["clip"] * 2 and models.norm_slices(M["TransE"], "rel", None) == []
    with pytest.raises(ValueError, match="RotatE.*phases"):
        models.norm_slices(M["RotatE"], "rel", "clip")


def test_flag_bits_on_both_sides():
    header = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define KGE_FLAG_(\w+) (\d+)u", header)}
    for name, bit in BITS.items():
        assert defs[name] == bit
    assert max(v for k, v in defs.items() if k not in BITS) < min(BITS.values())               # above every existing flag
    lib = _lib()
    assert (lib.FLAG_ENT_NORM_CLIP, lib.FLAG_ENT_NORM_UNIT, lib.FLAG_REL_NORM_CLIP, lib.FLAG_REL_NORM_UNIT) == (2048, 4096, 8192, 16384)
    assert lib.NORM_FLAGS == {"ent": {None: 0, "none": 0, "clip": 2048, "unit": 4096}, "rel": {None: 0, "none": 0, "clip": 8192, "unit": 16384}}
    assert {t: {k: v for k, v in d.items() if k != "none"} for t, d in lib.NORM_FLAGS.items()} == Q.FLAGS
    assert len(re.findall(r"\bkge_(?:\w*_)?(?:norm|constrain)\w*\s*\(", header)) == 0      # no new prototype


def test_case_table_names_the_instance_boundaries():
    hpp = open(os.path.join(CSRC, "kge_constrain.hpp")).read()
    got = tuple(int(re.search(r"#define %s (\d+)" % n, hpp).group(1)) for n in ("KGE_CONSTRAIN_REG_NARROW", "KGE_CONSTRAIN_REG_WIDE"))
    assert got == Q.BOUNDARIES
    hip = open(os.path.join(CSRC, "kge_constrain.hip")).read()
    assert re.search(r"pmax <= KGE_CONSTRAIN_REG_NARROW\) KGE_CONSTRAIN\(1\)", hip) and re.search(r"pmax <= KGE_CONSTRAIN_REG_WIDE\) KGE_CONSTRAIN\(4\)", hip)
    for b in Q.BOUNDARIES:           # one width on each side, on the 16-byte and on the 4-byte path
        assert {b - 2, b, b + 2, b + 4} <= set(Q.WIDTHS)
    assert 6 in Q.WIDTHS and 400 in Q.WIDTHS


# --------------------------------------------------------------------------------------------------------------------------
# the conditions on the inputs of every case
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", Q.CASES, ids=lambda c: c["id"])
def test_float64_step_leaves_no_ambiguous_slice_and_a_mix(c):
    _lib()
    ent, rel = Q.tables(c)
    bt = Q.batch(c)
    known = Q.known_of(c, bt)[0]
    e64, r64 = Q.float64_step(c, ent, rel, bt, known)
    ids_e, ids_r = Q.union(bt)
    assert not np.array_equal(e64[ids_e], ent[ids_e].astype(np.float64)), "the step moved nothing"
    tot = scaled = unscaled = 0
    for table, T, ids in (("ent", e64, ids_e), ("rel", r64, ids_r)):
        modes = Q.slice_modes(c, table)
        if not modes:
            continue
        _, sc, norms = Q.project64(T[ids], modes)
        assert not Q.ambiguous(norms, modes, T.shape[1] // len(modes)).any(), "%s %s: an ambiguous slice" % (c["id"], table)
        assert np.isfinite(norms).all()
        tot, scaled, unscaled = tot + sc.size, scaled + int(sc.sum()), unscaled + int((~sc).sum())
    assert scaled >= Q.MIX * tot and unscaled >= Q.MIX * tot, (c["id"], tot, scaled, unscaled)
    if c["plan"] == "device":      # the counts stay below the bounds the record arrays are sized for
        assert len(ids_e) < 2 * c["B"] + (c["B"] // c["chunk"]) * c["N"] and len(ids_r) < c["B"]
    if c["id"] == Q.ODD_RECORDS:
        assert (len(ids_e) * bool(c["ent_norm"]) + len(ids_r) * bool(c["rel_norm"])) % 4 != 0
    if c["id"] == "transd-h4-tiny":
        assert len(ids_e) < 4 and len(ids_r) < 4
    if c["id"] == "l2-several-workgroups":
        assert len(ids_e) > 16 and len(ids_r) > 4
    if c["plant"]:                 # the planted rows that stayed exactly as they were are the unscaled ones
        zero, basis = Q.planted_rows(c)
        kept = [i for i in np.concatenate([zero, basis]) if i in set(ids_e.tolist()) and np.array_equal(e64[i], ent[i].astype(np.float64))]
        assert len(kept) >= Q.MIX * len(ids_e) and any(i in zero for i in kept) and any(i in basis for i in kept)
        assert not set(np.concatenate([zero, basis]).tolist()) & set(bt["nid"].tolist())


def test_initial_slice_norms_are_spread_and_away_from_one():
    for c in Q.CASES:
        ent, rel = Q.tables(c)
        from dglke_amd import models
        m = models.MODELS[c["model"]]
        for t, parts in ((ent, m.norm_ent), (rel, max(m.norm_rel, 1))):
            n = np.sqrt((t.astype(np.float64).reshape(t.shape[0], parts, -1) ** 2).sum(-1))
            n = n[(n > 0) & (np.abs(n - 1) > 1e-6)]          # (the planted zero and basis rows)
            assert np.all((n > 0.49) & (n < 1.51)) and np.all(np.abs(n - 1) >= Q.NORM_GAP - 1e-6), c["id"]
            if n.size >= 6:
                assert (n > 1).any() and (n < 1).any()


# --------------------------------------------------------------------------------------------------------------------------
# the refusals of the C ABI
# --------------------------------------------------------------------------------------------------------------------------
def _step_args(lib, model=1, d_e=16, d_r=16, flags=0):
    hp, tb, b = lib.KgeHParams(), lib.KgeTables(), lib.KgeBatch()
    hp.model, hp.d_e, hp.d_r, hp.flags = model, d_e, d_r, flags
    b.B, b.C, b.chunk, b.N, b.UE, b.UR = 4, 1, 4, 3, 5, 2
    return hp, tb, b


def test_closed_entries_refuse_every_bit_before_any_launch():
    lib = _lib()
    h = lib.lib()
    one = 1
    for name, bit in BITS.items():
        hp, tb, b = _step_args(lib, flags=bit)
        sh, em = lib.KgeShards(), lib.KgeEmit()

        def named(entry):
            msg = h.kge_last_error()
            return entry in msg and ("KGE_FLAG_" + name).encode() in msg
        assert h.kge_step_sharded(C.byref(hp), C.byref(sh), C.byref(b), None, one, 1 << 20, None) == -1 and named(b"kge_step_sharded")
        assert h.kge_step_grads(C.byref(hp), C.byref(tb), C.byref(b), None, C.byref(em), one, 1 << 20, None) == -1 and named(b"kge_step_grads")
        pipe = C.c_void_p()
        assert h.kge_pipe_create(C.byref(pipe)) == 0
        assert h.kge_step_async(pipe, C.byref(hp), C.byref(tb), C.byref(b), None, None, one, 1 << 20, None) == -1 and named(b"kge_step_async")
        h.kge_pipe_destroy(pipe)


def _strict_entries(lib, h, hp, tb, b):
    """(entry name, return code, message) of every strict entry called with null tables: argument errors come before any launch"""
    one = 1
    a = (C.byref(hp), C.byref(tb), C.byref(b), None, one, 1 << 20)
    job, kn, opt = lib.KgeSamplerJob(), lib.KgeKnown(), lib.KgeOptim()
    job.heads = job.rels = job.tails = job.state = job.slot = job.scratch = one
    job.n_train, job.n_ent, job.B, job.C, job.chunk, job.N, job.scratch_bytes = 8, 8, 4, 1, 4, 3, 1 << 30
    out = []
    for name, call in (
            ("kge_step_fused", lambda: h.kge_step_fused(*a, None)),
            ("kge_step_fused_known", lambda: h.kge_step_fused_known(*a, None, C.byref(kn), one, 1 << 20, None)),
            ("kge_step_fused_sampling", lambda: h.kge_step_fused_sampling(*a, C.byref(job), None)),
            ("kge_step_phase", lambda: h.kge_step_phase(*a, lib.PHASE_UPDATE, None)),
            ("kge_step_phase_known", lambda: h.kge_step_phase_known(*a, lib.PHASE_UPDATE, C.byref(kn), one, 1 << 20, None)),
            ("kge_step_optim", lambda: (setattr(opt, "kind", lib.OPT_ADAM), setattr(opt, "ent_mom", one), setattr(opt, "rel_mom", one),
                                        setattr(opt, "beta1", 0.9), setattr(opt, "beta2", 0.999), setattr(opt, "eps", 1e-8),
                                        h.kge_step_optim(C.byref(hp), C.byref(opt), C.byref(tb), C.byref(b), None, one, 1 << 20,
                                                         lib.PHASE_ALL, None, None, 0, None))[-1])):
        rc = call()
        out.append((name, rc, h.kge_last_error()))
    return out


def test_strict_entries_refuse_two_modes_and_rowless_relations_before_any_launch():
    lib = _lib()
    h = lib.lib()
    # both bits of one table
    for both, word in ((2048 | 4096, b"KGE_FLAG_ENT_NORM_CLIP and KGE_FLAG_ENT_NORM_UNIT"), (8192 | 16384, b"KGE_FLAG_REL_NORM_CLIP and KGE_FLAG_REL_NORM_UNIT")):
        hp, tb, b = _step_args(lib, flags=both)
        for name, rc, msg in _strict_entries(lib, h, hp, tb, b):
            assert rc == -1 and word in msg and name.encode() in msg, (name, rc, msg)
    # a relation bit for RotatE, RESCAL, TransR: every strict entry, each bit
    for model, d_e, d_r, mname, why in ((4, 16, 8, b"RotatE", b"phases"), (6, 4, 16, b"RESCAL", b"kernels of their own"),
                                        (7, 16, 8, b"TransR", b"kernels of their own")):
        for bit, fname in ((8192, b"KGE_FLAG_REL_NORM_CLIP"), (16384, b"KGE_FLAG_REL_NORM_UNIT")):
            hp, tb, b = _step_args(lib, model, d_e, d_r, bit)
            for name, rc, msg in _strict_entries(lib, h, hp, tb, b):
                if name == "kge_step_fused_sampling" and model == 7:
                    continue                                        # (closed to the model in front of the flags)
                if name == "kge_step_optim" and model in (6, 7):
                    assert rc == -1 and b"Adam is not available" in msg          # (its own refusal comes first)
                    continue
                assert rc == -1 and fname in msg and mname in msg and why in msg and name.encode() in msg, (name, rc, msg)
            # the entity bits pass for these models: the next check speaks (null tables)
            hp.flags = 2048
            assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, 1, 1 << 20, None) == -1
            assert b"NORM" not in h.kge_last_error()


def test_bits_clear_nothing_moved_and_no_workspace_bytes_are_added():
    lib = _lib()
    h = lib.lib()
    for model, d_e, d_r in ((0, 16, 16), (1, 400, 400), (2, 16, 16), (3, 16, 16), (4, 16, 8), (5, 16, 16), (6, 4, 16), (7, 16, 8), (8, 16, 16),
                            (10, 16, 32), (12, 16, 32), (14, 16, 16)):
        hp, tb, b = _step_args(lib, model, d_e, d_r)
        base = h.kge_step_workspace_bytes(C.byref(hp), 64, 2, 32, 32, 100, 9)
        assert base > 0
        for bits in (2048, 4096, 8192 | 2048, 16384 | 4096):
            hp.flags = bits
            assert h.kge_step_workspace_bytes(C.byref(hp), 64, 2, 32, 32, 100, 9) == base, (model, bits)
        hp.flags = 0
        # the texts of the strict step's own refusals with the bits clear, and with a permitted bit set: what they were
        for flags in (0, 2048):
            hp.flags = flags
            assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, 1, 1 << 20, None) == -1
            assert h.kge_last_error() == b"kge_step: null table / batch pointer", (model, h.kge_last_error())
        hp.flags, b.B = 0, 5
        assert h.kge_step_fused(C.byref(hp), C.byref(tb), C.byref(b), None, 1, 1 << 20, None) == -1
        assert h.kge_last_error() == b"kge_step: need C*chunk == B (B=5 C=1 chunk=4)"


# --------------------------------------------------------------------------------------------------------------------------
# the command line and the engine
# --------------------------------------------------------------------------------------------------------------------------
def test_command_line_flags_and_refusals(tmp_path):
    _lib()
    from dglke_amd import train as T
    from dglke_amd._lib import KgeError
    base = ["--dataset", "toy", "--data_path", str(tmp_path / "none"), "--save_path", str(tmp_path / "ckpts"), "--gpu", "0"]
    a = T.ArgParser().parse_args(base)
    assert (a.ent_norm, a.rel_norm) == ("none", "none") and T.norm_constraints(a) == (None, None)
    a = T.ArgParser().parse_args(base + ["--ent_norm", "unit", "--rel_norm", "clip"])
    assert T.norm_constraints(a) == ("unit", "clip")
    with pytest.raises(SystemExit):
        T.ArgParser().parse_args(base + ["--ent_norm", "ball"])
    for flag in ("--ent_norm", "--rel_norm"):
        with pytest.raises(KgeError, match=flag + " is not available on more than one GPU"):
            T.main(base[:-1] + ["0", "1", flag, "clip"])
        with pytest.raises(KgeError, match=flag + " is not available with --async_update_pipeline"):
            T.main(base + [flag, "clip", "--async_update", "--async_update_pipeline"])
        with pytest.raises(KgeError, match=flag + " is not available with --async_update_rel"):
            T.main(base + [flag, "unit", "--async_update", "--async_update_rel"])
    for model, extra, why in (("RotatE", ["-de"], "phases"), ("RESCAL", [], "kernels of their own"), ("TransR", [], "kernels of their own")):
        with pytest.raises(KgeError, match="--rel_norm is not available for %s.*%s" % (model, why)):
            T.main(base + ["--model_name", model, "--rel_norm", "clip"] + extra)
        T.check_norm_constraints(T.ArgParser().parse_args(base + ["--model_name", model, "--ent_norm", "clip"] + extra))     # entities: fine
    T.check_norm_constraints(T.ArgParser().parse_args(base + ["--ent_norm", "clip", "--rel_norm", "unit", "--num_proc", "2"]))      # lanes: fine
    assert not os.path.exists(str(tmp_path / "ckpts")), "refused before anything is loaded or created"


def test_engine_maps_modes_to_bits_without_a_device():
    """StepEngine refuses a CPU device in front of everything else; the mapping it applies is _lib.NORM_FLAGS, and from_args reads the
    two flags of the namespace"""
    lib = _lib()
    from dglke_amd.engine import StepEngine
    import inspect
    sig = inspect.signature(StepEngine.__init__)
    assert sig.parameters["ent_norm"].default is None and sig.parameters["rel_norm"].default is None
    src = inspect.getsource(StepEngine.from_args)
    assert "ent_norm=arg('ent_norm')" in src and "rel_norm=arg('rel_norm')" in src
    with pytest.raises(lib.KgeError, match="no CPU fallback"):
        StepEngine("TransE_l2", 4, 2, 8, 4.0, 0.1, "cpu", ent_norm="clip")
