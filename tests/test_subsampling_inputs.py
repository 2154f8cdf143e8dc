"""CPU guard of tests/subsampling_cases.py: the graph has what the GPU tests need (duplicates, a spread of counts, the lone and the
unused relation), every sampler geometry reaches the instance it names, the new C entries are declared and bound, the ABI version
is still 8, and the UNWEIGHTED slot size of the geometries is the documented layout's - computed here, not read from the library's
own layout function."""
import os
import re

import numpy as np
import pytest

import stream_cases as S
import subsampling_cases as SC

NEW_ENTRIES = ("kge_sampler_slot_bytes_weighted", "kge_sample_batches_weighted", "kge_batch_from_slot_weighted", "kge_subsampling_weights")


def test_graph_is_what_the_table_says():
    h, r, t = SC.graph()
    assert len(h) == SC.N_TRIPLES and h.max() < SC.N_ENT and t.max() < SC.N_ENT and min(h.min(), t.min()) >= 0
    assert not (h == t).any()
    trip = list(zip(h.tolist(), r.tolist(), t.tolist()))
    mult = {}
    for x in trip:
        mult[x] = mult.get(x, 0) + 1
    assert mult[trip[SC.TRIPLED]] == 3 and trip[-1] == trip[-2] == trip[SC.TRIPLED]
    assert len(mult) < len(trip), "no duplicates"
    assert (r == SC.LONE_REL).sum() == 1 and (r == SC.UNUSED_REL).sum() == 0 and r.max() < SC.N_REL
    # Zipf: the most frequent head is seen far more often than the median one
    hc = np.bincount(h, minlength=SC.N_ENT)
    assert hc.max() >= 20 * max(1, int(np.median(hc[hc > 0])))


def test_counts_spread_so_that_weighted_differs_from_unweighted():
    h, r, t = SC.graph()
    n_hr, n_tr = SC.counts(h, r, t, SC.N_REL)
    s = n_hr + n_tr
    assert s.max() >= 10 * s.min(), (s.min(), s.max())
    w = SC.weights64(h, r, t, SC.N_REL)
    assert abs(w.mean() - 1.0) < 1e-12 and w.max() > 3 * w.min(), (w.min(), w.max())
    # the lone relation's triple is seen once on both sides: the largest raw weight, 1 / sqrt(1 + 1 + 6)
    lone = int(np.nonzero(r == SC.LONE_REL)[0][0])
    assert n_hr[lone] == n_tr[lone] == 1 and SC.raw_weights64(h, r, t, SC.N_REL)[lone] == 1.0 / np.sqrt(8.0)
    # the tripled triple counts three times on both sides; a count over unique triples would say one
    assert n_hr[SC.TRIPLED] == n_tr[SC.TRIPLED] == 3
    u = np.unique(np.stack([h, r, t], 1), axis=0)
    uh, ut = SC.counts(u[:, 0], u[:, 1], u[:, 2], SC.N_REL)
    k = int(np.nonzero((u[:, 0] == h[SC.TRIPLED]) & (u[:, 1] == r[SC.TRIPLED]) & (u[:, 2] == t[SC.TRIPLED]))[0][0])
    assert uh[k] == ut[k] == 1


def test_weight_graphs():
    g = SC.weight_graphs()
    assert set(g) == {"table", "one_relation", "keys_above_2^40"}
    h, r, t, n_ent, n_rel = g["one_relation"]
    assert n_rel == 1 and not r.any()
    h, r, t, n_ent, n_rel = g["keys_above_2^40"]
    assert (h * n_rel + r).max() > 2 ** 40 and (t * n_rel + r).max() > 2 ** 40 and n_ent * n_rel < 2 ** 62
    n_hr, n_tr = SC.counts(h, r, t, n_rel)
    assert n_hr.max() > 1 and n_tr.max() > 1, "no repeated pair: the run lengths are all one"


@pytest.mark.parametrize("g", SC.GEOMETRIES, ids=[g[0] for g in SC.GEOMETRIES])
def test_geometry_reaches_the_instance_it_names(g):
    _, B, N, n_train, n_ent, slots, inst = g
    C = B // N
    assert C * N == B and n_train >= B
    assert SC.instance(B, C, N, n_ent) == inst
    assert 2 * B + C * N <= 8192 and B <= 4096                # the sampler launch's limits
    h, r, t, w = SC.unique_triples(n_train, n_ent)
    assert len(set(zip(h.tolist(), r.tolist(), t.tolist()))) == n_train and len(np.unique(w)) == n_train and (w > 0).all()
    assert h.max() < n_ent and t.max() < n_ent


def test_geometries_cover_all_four_instances_and_four_epochs():
    assert {g[6] for g in SC.GEOMETRIES} == {(False, False), (False, True), (True, False), (True, True)}
    _, B, N, n_train, _, slots, _ = SC.GEOMETRIES[0]
    assert (SC.N_LAUNCHES * slots - 1) // (n_train // B) == 3, "the last batch is not in the fourth epoch"


def test_new_entries_are_declared_and_bound():
    from dglke_amd import _lib
    protos = S.prototypes(open(S.HEADER).read())
    for name in NEW_ENTRIES:
        assert name in protos, name
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name][1]) == len(protos[name]), name
    # the two launches take their stream last, like every entry
    for name in ("kge_sample_batches_weighted", "kge_subsampling_weights"):
        assert re.match(r"^void\s*\*\s*\w*stream$", protos[name][-1]), protos[name]
    assert any(re.search(r"const float\s*\*\s*weights", p) for p in protos["kge_sample_batches_weighted"])
    # the existing entries keep their signatures
    assert len(protos["kge_sample_batches"]) == 16 and len(protos["kge_batch_from_slot"]) == 9 and len(protos["kge_sampler_slot_bytes"]) == 3
    src = open(os.path.join(S.CSRC, "Makefile")).read()
    assert "kge_subsample.hip" in src


def test_abi_version_and_slot_sizes():
    from dglke_amd import _lib
    h = _lib.lib()
    assert h.kge_abi_version() == 8 == _lib.KGE_ABI_VERSION
    for _, B, N, _, _, _, _ in SC.GEOMETRIES:
        C = B // N
        assert h.kge_sampler_slot_bytes(B, C, N) == SC.slot_bytes(B, C * N), (B, N)
        assert h.kge_sampler_slot_bytes_weighted(B, C, N) == SC.slot_bytes(B, C * N, True) == SC.slot_bytes(B, C * N) + SC.al32(4 * B)
    # by hand for the smallest geometry: B 8, CN 8, NE 24
    assert SC.slot_bytes(8, 8) == 64 * 4 + 192 + 64 + 128 + 64 + 128 + 32 + 64 + 32 + 768 + 256 + 32
