"""Host side of link prediction with known-edge exclusion (dglke_amd.ke_model, dglke_amd.known): the refusals, the argument
errors of the two entry points (reported before any launch) and the known-triple index against a brute-force Python set
on CPU tensors.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib
    return _lib


def test_model_classes_and_refusals():
    _lib()
    from dglke_amd import ke_model as K
    from dglke_amd._lib import KgeError
    for cls in (K.TransEModel, K.TransE_l2Model, K.TransE_l1Model, K.RotatEModel, K.TransRModel):
        m = cls(0, 12.0)
        assert m._gamma == 12.0 and m.num_entity == -1 and m.num_rel == -1 and m.graph is None
    assert K.TransEModel(0, 1.0).model_name == "TransE" and K.SimplEModel(0).model_name == "SimplE"
    for cls in (K.DistMultModel, K.ComplExModel, K.RESCALModel, K.SimplEModel):
        assert isinstance(cls(torch.device("cuda:0")), K.KGEModel)
    assert K.GNNModel(0, "DistMult").model_name == "DistMult" and K.GNNModel(0, "TransE_l1", 3.0)._gamma == 3.0
    with pytest.raises(KgeError):
        K.GNNModel(0, "RotatE")
    for dev in ("cpu", -1, None, torch.device("cpu")):              # no CPU path
        with pytest.raises(KgeError):
            K.DistMultModel(dev)
    m = K.DistMultModel(0)
    with pytest.raises(KgeError, match="attach_graph"):             # exclusion without a graph
        m.link_predict([0], [0], [0], exclude_mode="exclude")
    with pytest.raises(KgeError, match="attach_graph"):
        m.link_predict([0], [0], [0], exclude_mode="mask")
    with pytest.raises(KgeError, match="exclude_mode"):
        m.link_predict([0], [0], [0], exclude_mode="filter")
    with pytest.raises(KgeError, match="execution mode"):
        m.link_predict([0], [0], [0], exec_mode="batch_all")
    with pytest.raises(KgeError, match="none or logsigmoid"):
        m.link_predict([0], [0], [0], sfunc="sigmoid")
    with pytest.raises(KgeError, match="TransR"):
        K.TransRModel(0, 12.0).link_predict([0], [0], [0])
    with pytest.raises(KgeError, match="load"):
        m.attach_graph(([0], [0], [0]))
    for fn in (m.fit, m.eval, lambda: m.save("x")):
        with pytest.raises(KgeError):
            fn()
    # ScoreInfer and the tools keep their interface: the option lives in ke_model only
    from dglke_amd.infer import ScoreInfer
    import inspect
    assert list(inspect.signature(ScoreInfer.topK).parameters) == ["self", "head", "rel", "tail", "exec_mode", "k"]


def test_entry_points_report_argument_errors_without_a_gpu():
    L = _lib()
    h = L.lib()
    assert {"kge_topk_select_filtered", "kge_triples_known"} <= set(L.EXPORTED_SYMBOLS)
    assert h.kge_abi_version() == 8
    one = 1                                                         # (a non-NULL pointer that is never dereferenced)

    def sel(func=2, K=10, d_e=8, d_r=8, filt_ptr=one, filt_ids=one):
        return h.kge_topk_select_filtered(func, 0, one, 10, one, 2, one, one, one, 4, d_e, d_r, 0.0, 1.0, one, 10, one, 1, 4, K,
                                          one, one, one, 1 << 20, filt_ptr, filt_ids, None)
    assert sel(filt_ids=None) == -1 and b"filt_ids" in h.kge_last_error()
    assert sel(K=0) == -1 and b"K = 0" in h.kge_last_error()
    assert sel(K=129) == -1 and b"K = 129" in h.kge_last_error()
    assert sel(func=7) == -1 and b"TransR" in h.kge_last_error()
    assert sel(func=3, d_e=7, d_r=7) == -1 and b"dims" in h.kge_last_error()            # ComplEx, odd dim
    assert sel(func=6, d_e=4, d_r=8) == -1 and b"dims" in h.kge_last_error()            # RESCAL, d_r != d_e^2
    assert sel(filt_ptr=None, filt_ids=None, K=0) == -1                                  # the unfiltered form's checks
    rc = h.kge_triples_known(None, None, 5, 3, one, one, one, 2, one, None)
    assert rc == -1 and b"kge_triples_known" in h.kge_last_error()
    assert h.kge_triples_known(one, one, 5, 0, one, one, one, 2, one, None) == -1       # n_rel <= 0
    assert h.kge_triples_known(one, one, 5, 3, one, one, one, 2, None, None) == -1      # no output
    assert h.kge_triples_known(one, one, 5, 3, None, None, None, 0, None, None) == 0    # nothing to do
    # the workspace formula is the unfiltered one
    assert h.kge_topk_workspace_bytes(256, 1000, 32, 10) > 0


def _known_graph():
    rng = np.random.RandomState(0)
    NE, R = 37, 5                                                   # relation 3 has no triples
    r = rng.choice([0, 1, 2, 4], 400)
    h, t = rng.randint(0, NE, 400), rng.randint(0, NE, 400)
    h[:6], t[:6] = [0, 0, NE - 1, NE - 1, 0, NE - 1], [0, NE - 1, 0, NE - 1, 0, NE - 1]      # both ends of the id range
    r[:6] = [0, 4, 4, 0, 0, 0]                                      # (triples 0 / 4 and 3 / 5 repeat)
    h, r, t = (np.concatenate([x, x[:50]]) for x in (h, r, t))       # repeated known triples
    return NE, R, h, r, t


@pytest.mark.parametrize("two_key", [False, True])
def test_known_index_against_python_sets(monkeypatch, two_key):
    _lib()
    from dglke_amd import eval as E
    from dglke_amd.known import KnownIndex
    monkeypatch.setattr(E, "_FORCE_TWO_KEY_SORT", two_key)
    NE, R, h, r, t = _known_graph()
    for graph in ((h, r, t), (torch.as_tensor(h), torch.as_tensor(r.astype(np.int32)), torch.as_tensor(t))):
        ix = KnownIndex(graph, NE, R, "cpu")
        assert len(ix) == 450
        a, rr = np.meshgrid(np.arange(NE), np.arange(R), indexing="ij")
        a, rr = torch.as_tensor(a.reshape(-1)), torch.as_tensor(rr.reshape(-1))
        for neg_head in (False, True):
            want = {}
            for x, y, z in zip(h.tolist(), r.tolist(), t.tolist()):
                want.setdefault((z, y) if neg_head else (x, y), set()).add(x if neg_head else z)
            keys, vals = ix.side(neg_head)
            assert ix.side(neg_head)[0] is keys                     # built once
            assert keys.dtype == vals.dtype == torch.int64 and keys.shape == vals.shape
            assert keys.numel() == sum(len(v) for v in want.values())
            rng = ix.ranges(neg_head, a, rr)
            assert rng.shape == (NE * R, 2) and rng.is_contiguous()
            for (ai, ri), (lo, hi) in zip(zip(a.tolist(), rr.tolist()), rng.tolist()):
                assert vals[lo:hi].tolist() == sorted(want.get((ai, ri), ())), (neg_head, ai, ri)
                if ri == 3:
                    assert lo == hi
            # what build_filter_device gives for the same queries
            frng, fids = E.build_filter_device(graph, (a, rr, a), neg_head, R, NE, "cpu")
            assert torch.equal(frng, rng) and torch.equal(fids, vals)


def test_known_index_checks_ids_on_the_host():
    _lib()
    from dglke_amd._lib import KgeError
    from dglke_amd.known import KnownIndex
    for bad in (([0, 10], [0, 0], [1, 1]), ([0, 1], [0, 2], [1, 1]), ([0, 1], [0, 0], [1, -1])):
        with pytest.raises(KgeError, match="outside"):
            KnownIndex(bad, 10, 2, "cpu")
    with pytest.raises(KgeError, match="same length"):
        KnownIndex(([0, 1], [0], [1, 1]), 10, 2, "cpu")
    with pytest.raises(KgeError, match="integers"):
        KnownIndex(([0.5], [0], [1]), 10, 2, "cpu")
    ix = KnownIndex(([], [], []), 10, 2, "cpu")                     # an empty graph filters nothing
    assert ix.side(False)[0].numel() == 0
    assert ix.ranges(False, torch.tensor([3]), torch.tensor([1])).tolist() == [[0, 0]]
    assert ix.filt_ids(False).numel() == 1
