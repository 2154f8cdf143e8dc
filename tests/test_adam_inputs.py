"""CPU guard of --optimizer Adam (tests/adam_cases.py): the float64 statement against torch.optim.Adam, its laziness, count
saturation and fixed point, the row classes and the ambiguity cap of every case of tests/test_gpu_adam.py, the CLI refusals
(before any file is read) and the library surface."""
import os
import re

import numpy as np
import pytest
import torch

import adam_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(c, steps=A.STEPS, preload=None):
    """the free-running float64 statement of a case: -> per step (info, state before, state after), ambiguity share per array"""
    ent, rel = A.tables(c)
    st = A.zero_state(c, ent, rel)
    for k, v in (preload or {}).items():
        st[k.replace("_state", "_cnt")] = v.astype(np.float64)
    amb = dict(ent=np.zeros(st["ent"].shape, bool), rel=np.zeros(st["rel"].shape, bool))
    hist = []
    for bt in A.batches(c, steps):
        known = A.known_pairs(c, bt)[0] if c["known"] else None
        before = {k: v.copy() for k, v in st.items()}
        info = A.step(c, st, bt, known)
        for tab in ("ent", "rel"):
            ids, G = info[tab]
            amb[tab] |= A.ambiguous(ids, G, st[tab].shape[0])
        hist.append((info, before, {k: v.copy() for k, v in st.items()}, bt))
    return hist, amb


def test_statement_equals_dense_torch_adam_where_every_row_is_touched_every_step():
    """the hub case touches all four entities and its one relation in every step: lazy Adam IS dense Adam there and the per-row
    count is the step number.  torch.optim.Adam in float64 on the same gradients, 1e-12 relative"""
    c = A.by_id("distmult-hub")
    ent, rel = A.tables(c)
    st = A.zero_state(c, ent, rel)
    pe, pr = (torch.tensor(x.astype(np.float64), requires_grad=True) for x in (ent, rel))
    opt = torch.optim.Adam([pe, pr], lr=c["lr"], betas=(A.BETA1, A.BETA2), eps=A.EPS)
    for s, bt in enumerate(A.batches(c, 6), 1):
        info = A.step(c, st, bt)
        for p, tab in ((pe, "ent"), (pr, "rel")):
            ids, G = info[tab]
            assert len(ids) == st[tab].shape[0], "not every row of %s is touched" % tab
            p.grad = torch.from_numpy(G[np.argsort(ids)].copy())
        opt.step()
        for p, tab in ((pe, "ent"), (pr, "rel")):
            want = p.detach().numpy()
            assert np.abs(st[tab] - want).max() <= 1e-12 * np.abs(want).max(), (s, tab)
            assert (st[tab + "_cnt"] == s).all()


def test_untouched_rows_moments_and_counts_keep_their_bits():
    c = A.by_id("TransE_l2-w16")
    hist, _ = _run(c, 2)
    some = 0
    for info, before, after, bt in hist:
        for tab in ("ent", "rel"):
            un = np.setdiff1d(np.arange(before[tab].shape[0]), info[tab][0])
            some += len(un)
            for k in (tab, tab + "_mom", tab + "_cnt"):
                assert np.array_equal(before[k][un].view(np.uint64), after[k][un].view(np.uint64)), (tab, k)
            assert (after[tab + "_cnt"][info[tab][0]] == before[tab + "_cnt"][info[tab][0]] + 1).all()
    assert some > 0


def test_count_saturates_at_two_to_the_24():
    x, mom = np.ones((3, 4)), np.full((3, 2, 4), 0.5)
    cnt = np.array([A.CMAX - 2, A.CMAX - 1, A.CMAX])
    for _ in range(3):
        A.adam_rows(x, mom, cnt, [0, 1, 2], np.ones((3, 4)), 0.01)
    assert cnt.tolist() == [A.CMAX, A.CMAX, A.CMAX]
    assert np.float32(A.CMAX) == A.CMAX and np.float32(A.CMAX - 1) + np.float32(1) == np.float32(A.CMAX)   # a float holds it exactly
    assert np.isfinite(x).all()


def test_all_zero_row_stays_put_and_counts():
    x, mom, cnt = np.full((2, 4), 0.3), np.zeros((2, 2, 4)), np.zeros(2)
    x0 = x.copy()
    A.adam_rows(x, mom, cnt, [1], np.zeros((1, 4)), 0.01)
    assert np.array_equal(x, x0) and not mom.any() and cnt.tolist() == [0.0, 1.0]
    # with momentum a zero gradient still moves the row and decays the moments
    mom[1, 0], mom[1, 1] = 0.1, 0.01
    A.adam_rows(x, mom, cnt, [1], np.zeros((1, 4)), 0.01)
    assert (x[1] < x0[1]).all() and np.allclose(mom[1, 0], 0.09) and np.allclose(mom[1, 1], 0.00999) and cnt[1] == 2


def test_bias_correction_of_the_first_steps():
    for beta in (0.9, 0.999):
        for c in (1, 2, 10):
            assert abs(A.bias_correction(float(c), beta) - (1 - beta ** c)) < 1e-15
    assert A.bias_correction(1.0, 0.0) == 1.0


@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c["id"])
def test_every_case_has_the_row_classes_it_names(c):
    d_e, d_r = A.widths(c)
    thr = A.rel_shared_threshold(d_r, d_e)
    for bt in A.batches(c):
        rc = A.row_classes(c, bt)
        if c["hub"]:
            assert rc["ent_pos_max"] > 66 and rc["ent_neg_max"] > 66 and rc["rel_len"].max() - 1 >= thr, rc
        else:
            assert rc["pos_only"] >= 1 and rc["neg_only"] >= 1 and rc["both"] >= 1, rc
            assert rc["rel_len"].max() - 1 >= thr and rc["rel_len"].min() - 1 < thr, rc
    assert [bt["neg_head"] for bt in A.batches(c)] == [False, True, False, True]       # alternating corruption sides


@pytest.mark.parametrize("c", A.CASES + A.GUARD_SHAPE, ids=lambda c: c["id"])
def test_ambiguity_cap(c):
    """no compared array of a case loses more than AMBIGUITY_CAP of its elements to the ambiguity rule"""
    _, amb = _run(c)
    for tab in ("ent", "rel"):
        assert amb[tab].mean() <= A.AMBIGUITY_CAP, "%s %s: %.4f of the elements are ambiguous" % (c["id"], tab, amb[tab].mean())


@pytest.mark.parametrize("cid", sorted(A.PRELOAD_CASES))
def test_ambiguity_cap_of_the_preloaded_cases(cid):
    c = A.by_id(cid)
    pre = A.preloaded(c, A.PRELOAD_CASES[cid])
    assert sorted(set(pre["ent_state"].tolist())) == [0.0, 1.0, 1000.0, 2.0 ** 24 - 1, 2.0 ** 24] and pre["ent_mom"].all()
    _, amb = _run(c, 2, pre)
    for tab in ("ent", "rel"):
        assert amb[tab].mean() <= 0.7 * A.AMBIGUITY_CAP, "%s %s: %.4f of the elements are ambiguous" % (cid, tab, amb[tab].mean())


def test_known_pairs_take_something_out():
    c = A.by_id("l2-known")
    for bt in A.batches(c):
        mask, K = A.known_pairs(c, bt)
        assert 0 < mask.mean() < 0.5 and len(K[0]) > 0


# --------------------------------------------------------------------------------------------------------------------------
# the CLI
# --------------------------------------------------------------------------------------------------------------------------
def _argv(tmp_path, model, extra):
    data = str(tmp_path / "kg")
    return ["--model_name", model, "--format", "udd_hrt", "--dataset", "toy", "--data_path", data, "--data_files",
            "e.dict", "r.dict", "train.txt", "valid.txt", "test.txt", "--save_path", str(tmp_path / "ckpts"),
            "--batch_size", "256", "--neg_sample_size", "64", "--hidden_dim", "32", "-g", "8", "--lr", "0.001", "-adv",
            "--max_step", "300", "--log_interval", "150", "--graph_steps", "100", "--optimizer", "Adam"] + extra


def test_parser_has_the_flags():
    from dglke_amd import train as T
    p = T.ArgParser()
    a = p.parse_args([])
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_eps) == ("Adagrad", 0.9, 0.999, 1e-8)
    a = p.parse_args(["--optimizer", "Adam", "--adam_beta1", "0.8", "--adam_beta2", "0.99", "--adam_eps", "1e-6"])
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_eps) == ("Adam", 0.8, 0.99, 1e-6)
    with pytest.raises(SystemExit):
        p.parse_args(["--optimizer", "SGD"])


REFUSALS = [
    ("RESCAL", ["--gpu", "0"], "RESCAL"), ("TransR", ["--gpu", "0"], "TransR"),
    ("TransE_l2", ["--gpu", "0", "1"], "more than one GPU"),
    ("TransE_l2", ["--gpu", "0", "--async_update", "--async_update_pipeline"], "pipeline"),
    ("TransE_l2", ["--gpu", "0", "--async_update", "--async_update_rel"], "pipeline"),
    ("TransE_l2", ["--gpu", "0", "--hidden_dim", "30"], "multiples of 4"),
    ("TransE_l2", ["--gpu", "0", "--hidden_dim", "1028"], "at most 1024"),
    ("ComplEx", ["--gpu", "0", "--hidden_dim", "516", "-de", "-dr"], "at most 1024"),
    ("TransE_l2", ["--gpu", "0", "--adam_beta1", "1.0"], "--adam_beta1"),
    ("TransE_l2", ["--gpu", "0", "--adam_eps", "0"], "--adam_eps"),
]


@pytest.mark.parametrize("model,extra,word", REFUSALS, ids=[r[0] + "-" + "_".join(x.strip("-") for x in r[1][2:]) for r in REFUSALS])
def test_refusals_arrive_before_any_file_is_read(tmp_path, model, extra, word):
    from dglke_amd import train as T
    from dglke_amd._lib import KgeError
    with pytest.raises(KgeError) as e:
        T.main(_argv(tmp_path, model, extra))
    assert "--optimizer Adam" in str(e.value) and word in str(e.value), str(e.value)
    assert not (tmp_path / "ckpts").exists() and not (tmp_path / "kg").exists()


def test_plain_async_update_and_adagrad_are_not_refused():
    from dglke_amd import train as T
    T.check_optimizer(T.ArgParser().parse_args(["--optimizer", "Adam", "--async_update", "--gpu", "0"]))
    T.check_optimizer(T.ArgParser().parse_args(["--model_name", "RESCAL", "--gpu", "0", "1"]))


# --------------------------------------------------------------------------------------------------------------------------
# the library surface
# --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_struct():
    src = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    assert re.search(r"#define\s+KGE_ABI_VERSION\s+8\b", src)
    assert re.search(r"#define\s+KGE_OPT_ADAGRAD\s+0\b", src) and re.search(r"#define\s+KGE_OPT_ADAM\s+1\b", src)
    m = re.search(r"typedef struct kge_optim \{(.*?)\} kge_optim;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t kind; float beta1, beta2, eps; float *ent_mom, *rel_mom;"
    proto = re.search(r"int kge_step_optim\((.*?)\);", src, re.S).group(1)
    assert re.sub(r"\s+", " ", proto).endswith("size_t mask_bytes, void *hip_stream")
    assert "Adam" in open(os.path.join(ROOT, "dgl-ke_amd", "csrc", "kge_adam.hip")).read()


def test_binding_and_symbol():
    import ctypes as C
    from dglke_amd import _lib
    assert _lib.KGE_ABI_VERSION == 8
    assert "kge_step_optim" in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES["kge_step_optim"][1]) == 12
    assert [f[0] for f in _lib.KgeOptim._fields_] == ["kind", "beta1", "beta2", "eps", "ent_mom", "rel_mom"]
    assert C.sizeof(_lib.KgeOptim) == 32 and (_lib.OPT_ADAGRAD, _lib.OPT_ADAM) == (A.OPT_ADAGRAD, A.OPT_ADAM)
    h = _lib.lib()
    assert h.kge_abi_version() == 8 and h.kge_step_optim is not None
