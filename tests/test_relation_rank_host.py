"""CPU tests of the relation ranking's host side: the two C-ABI symbols, the workspace size function, the argument errors that
come back before anything touches a GPU, the filter builder's lists (its sort runs wherever its tensors live), and the
command-line refusals of --eval_relation."""
import ctypes

import numpy as np
import pytest
import torch

import relation_rank_cases as RC


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib
    return _lib


def test_both_symbols_resolve():
    L = _lib()
    h = L.lib()
    assert "kge_rank_rel_eval" in L.EXPORTED_SYMBOLS and "kge_rank_rel_workspace_bytes" in L.EXPORTED_SYMBOLS
    assert h.kge_rank_rel_eval.restype is ctypes.c_int and h.kge_rank_rel_workspace_bytes.restype is ctypes.c_size_t
    assert h.kge_abi_version() == 8


def test_workspace_size():
    ws = _lib().lib().kge_rank_rel_workspace_bytes
    for model, d_e, d_r in ((0, 32, 32), (1, 400, 400), (2, 30, 30), (3, 32, 32), (4, 64, 32), (5, 32, 32), (6, 8, 64), (7, 24, 16)):
        a = ws(model, 8, 130, d_e, d_r)
        assert a > 0
        assert ws(model, 800, 130, d_e, d_r) > a            # rows
        assert ws(model, 8, 13000, d_e, d_r) > a            # relations
    assert ws(6, 64, 130, 64, 4096) > 64 * 4096 * 4         # RESCAL: the d_e^2-wide query rows are in it
    # bad arguments: 0
    assert ws(8, 8, 130, 32, 32) == 0 and ws(-1, 8, 130, 32, 32) == 0
    assert ws(2, 0, 130, 32, 32) == 0 and ws(2, 8, 0, 32, 32) == 0 and ws(2, 8, 1 << 31, 32, 32) == 0
    assert ws(2, 8, 130, 32, 16) == 0 and ws(4, 8, 130, 32, 32) == 0 and ws(6, 8, 130, 8, 8) == 0


A = 64      # a made-up address: the checks under test come before anything is read or launched


def _call(L, model=2, ent=A, n_ent=10, rel=A, n_rel=3, proj=None, h=A, r=A, t=A, E=1, d_e=32, d_r=32, filt_ptr=A, filt_ids=A, Eb=4,
          ranks=A, ws=A, ws_bytes=1 << 30):
    return L.lib().kge_rank_rel_eval(model, ent, n_ent, rel, n_rel, proj, h, r, t, E, d_e, d_r, 8.0, 0.3, filt_ptr, filt_ids, Eb, ranks,
                                     None, ws, ws_bytes, 0, None)


@pytest.mark.parametrize("kw,word", [(dict(ent=None), "null pointer"),
                                     (dict(rel=None), "null pointer"),
                                     (dict(h=None), "null pointer"),
                                     (dict(r=None), "null pointer"),
                                     (dict(t=None), "null pointer"),
                                     (dict(ranks=None), "null pointer"),
                                     (dict(ws=None), "null pointer"),
                                     (dict(model=9), "unknown model"),
                                     (dict(d_r=16), "d_r == d_e"),
                                     (dict(model=4, d_e=32, d_r=32), "RotatE"),
                                     (dict(model=6, d_e=8, d_r=8), "RESCAL"),
                                     (dict(model=7, d_e=16, d_r=16), "TransR needs the projection table"),
                                     (dict(n_rel=1 << 31), "relation count"),
                                     (dict(Eb=0), "Eb"),
                                     (dict(Eb=-2), "Eb"),
                                     (dict(filt_ptr=None), "filt_ptr and filt_ids are required"),
                                     (dict(filt_ids=None), "filt_ptr and filt_ids are required")])
def test_argument_errors_come_back_without_a_gpu(kw, word):
    L = _lib()
    assert _call(L, **kw) == -1
    msg = L.lib().kge_last_error().decode()
    assert word in msg, msg


def test_small_workspace_and_no_triples():
    L = _lib()
    assert _call(L, ws_bytes=16) == -2                    # KGE_ERR_WORKSPACE, before any launch
    assert "workspace too small" in L.lib().kge_last_error().decode()
    assert _call(L, E=0, h=None, r=None, t=None, ranks=None) == 0


@pytest.mark.parametrize("n_rel", RC.N_RELS)
@pytest.mark.parametrize("two_key", [False, True])
def test_filter_builder_gives_the_case_tables_lists(n_rel, two_key, monkeypatch):
    _lib()
    from dglke_amd import eval as kev
    monkeypatch.setattr(kev, "_FORCE_TWO_KEY_SORT", two_key)
    c = RC.inputs("DistMult", 32, None, n_rel)
    cpu = torch.device("cpu")
    for filtered in (False, True):
        known = (c.kh[RC.E:], c.kr[RC.E:], c.kt[RC.E:]) if filtered else None      # the builder appends the test triples itself
        if known is not None:
            known = tuple(np.array(x) for x in known)
        rng, ids = kev.build_relation_filter(known, tuple(np.array(x) for x in (c.h, c.r, c.t)), RC.N_ENT, n_rel, cpu)
        wrng, wids = RC.relation_lists(n_rel, filtered)
        assert rng.dtype == ids.dtype == torch.int64 and tuple(rng.shape) == (RC.E, 2)
        for i in range(RC.E):
            assert np.array_equal(ids[rng[i, 0]:rng[i, 1]].numpy(), wids[wrng[i, 0]:wrng[i, 1]]), (filtered, i)


def test_command_line_refusals(tmp_path):
    L = _lib()
    from dglke_amd import eval_cli, train
    with pytest.raises(L.KgeError, match="--eval_relation is not available on sharded tables"):
        eval_cli.main(["--eval_relation", "--gpu", "0", "0", "--model_path", "/nonexistent"])
    with pytest.raises(L.KgeError, match="--eval_relation"):
        eval_cli.main(["--eval_relation", "--eval_candidates", "h.npy", "t.npy", "--gpu", "0", "--model_path", "/nonexistent"])
    # alone the flag is accepted: the next check (no such model directory) is reached
    with pytest.raises(L.KgeError, match="No existing model_path"):
        eval_cli.main(["--eval_relation", "--gpu", "0", "--model_path", "/nonexistent"])
    with pytest.raises(L.KgeError, match="--eval_relation is not available on sharded tables"):
        train.main(["--dataset", "toy", "--data_path", str(tmp_path), "--save_path", str(tmp_path / "ckpts"), "--eval_relation",
                    "--gpu", "0", "0"])
    assert not (tmp_path / "ckpts").exists()              # refused before anything was created
