"""CPU tests of the chunked-candidate ranking's host side: the two C-ABI symbols, the workspace size function, argument errors
that come back before anything touches a GPU, and the command-line / keyword plumbing of --neg_deg_sample_eval and
--eval_candidates."""
import ctypes

import numpy as np
import pytest
import torch


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib
    return _lib


def test_both_symbols_resolve():
    L = _lib()
    h = L.lib()
    assert "kge_rank_eval_chunked" in L.EXPORTED_SYMBOLS and "kge_rank_chunked_workspace_bytes" in L.EXPORTED_SYMBOLS
    assert h.kge_rank_eval_chunked.restype is ctypes.c_int and h.kge_rank_chunked_workspace_bytes.restype is ctypes.c_size_t
    assert h.kge_abi_version() == 8


def test_workspace_grows_with_rows_and_candidates():
    ws = _lib().lib().kge_rank_chunked_workspace_bytes
    for model, d_e, d_r in ((1, 400, 400), (4, 64, 32), (6, 8, 64), (7, 16, 16)):
        a = ws(model, 8, 8, 500, 0, d_e, d_r)
        assert a > 0
        assert ws(model, 800, 8, 500, 0, d_e, d_r) > a             # rows
        assert ws(model, 8, 8, 5000, 0, d_e, d_r) > a              # candidates
        assert ws(model, 8, 8, 500, 1, d_e, d_r) > a               # the chunk's own entities are candidates too
        assert ws(model, 9, 8, 500, 0, d_e, d_r) == ws(model, 16, 8, 500, 0, d_e, d_r)      # whole chunks


def _call(L, model=2, d_e=32, d_r=32, chunk=8, proj=None, self_cand=0, filt_ptr=None, filt_ids=None, E=0):
    # every pointer is null or a made-up address: the checks under test come before anything is read or launched
    return L.lib().kge_rank_eval_chunked(model, 0, None, 10, None, 3, proj, None, None, None, E, d_e, d_r, 8.0, 0.3, chunk, None, 0, 0,
                                         self_cand, filt_ptr, filt_ids, None, None, None, 0, 0, None)


@pytest.mark.parametrize("kw,word", [(dict(self_cand=1, filt_ptr=64, filt_ids=64), "self_cand"),
                                     (dict(chunk=0), "chunk"),
                                     (dict(chunk=-3), "chunk"),
                                     (dict(model=7, d_e=16, d_r=16), "TransR"),
                                     (dict(filt_ptr=64), "filt_ids")])
def test_argument_errors_come_back_without_a_gpu(kw, word):
    L = _lib()
    assert _call(L, **kw) == -1
    msg = L.lib().kge_last_error().decode()
    assert "kge_rank_eval_chunked" in msg and word in msg, msg


def test_eval_cli_refuses_degree_sampling_with_the_filter_on():
    L = _lib()
    from dglke_amd import eval_cli
    with pytest.raises(L.KgeError, match="if negative sampling based on degree, we can't filter positive edges."):
        eval_cli.main(["--neg_deg_sample_eval", "--gpu", "0", "--model_path", "/nonexistent"])
    # with the filter off the flag is accepted: the next check (no such model directory) is reached
    with pytest.raises(L.KgeError, match="No existing model_path"):
        eval_cli.main(["--neg_deg_sample_eval", "--no_eval_filter", "--gpu", "0", "--model_path", "/nonexistent"])
    with pytest.raises(L.KgeError, match="not available on sharded tables"):
        eval_cli.main(["--neg_deg_sample_eval", "--no_eval_filter", "--gpu", "0", "0", "--model_path", "/nonexistent"])


def test_train_cli_refuses_degree_sampling_with_the_filter_on(tmp_path):
    L = _lib()
    from dglke_amd import train
    base = ["--dataset", "toy", "--data_path", str(tmp_path), "--save_path", str(tmp_path / "ckpts"), "--neg_deg_sample_eval"]
    with pytest.raises(AssertionError, match="if negative sampling based on degree, we can't filter positive edges."):
        train.main(base + ["--gpu", "0"])
    with pytest.raises(L.KgeError, match="--neg_deg_sample_eval is not available on sharded tables"):
        train.main(base + ["--no_eval_filter", "--gpu", "0", "0"])
    assert not (tmp_path / "ckpts").exists()              # refused before anything was created


def test_eval_candidates_excludes_the_sampling_flags():
    L = _lib()
    from dglke_amd import eval_cli
    with pytest.raises(L.KgeError, match="--eval_candidates"):
        eval_cli.main(["--eval_candidates", "h.npy", "t.npy", "--neg_sample_size_eval", "5", "--gpu", "0", "--model_path", "/nonexistent"])
    with pytest.raises(L.KgeError, match="--eval_candidates"):
        eval_cli.main(["--eval_candidates", "h.npy", "t.npy", "--neg_deg_sample_eval", "--no_eval_filter", "--gpu", "0",
                       "--model_path", "/nonexistent"])
    with pytest.raises(L.KgeError, match="--eval_candidates is not available on sharded tables"):
        eval_cli.main(["--eval_candidates", "h.npy", "none", "--gpu", "0", "0", "--model_path", "/nonexistent"])


def test_evaluate_refuses_degree_sampling_with_known_triples():
    L = _lib()
    from dglke_amd import eval as kev
    ent, rel = torch.zeros(10, 8), torch.zeros(3, 8)
    trip = tuple(np.zeros(4, np.int64) for _ in range(3))
    with pytest.raises(L.KgeError, match="if negative sampling based on degree, we can't filter positive edges."):
        kev.evaluate("TransE_l2", ent, rel, 8.0, 0.3, trip, known=trip, neg_deg_sample=True)
    with pytest.raises(L.KgeError, match="at least one side"):
        kev.evaluate_candidates("TransE_l2", ent, rel, 8.0, 0.3, trip)
