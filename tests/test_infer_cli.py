"""dglke_predict / dglke_emb_sim without a GPU: flag sets, input parsing, the TSV writers, the refusals (all raised before
the device is touched) and the workspace bound of the top-K kernels (kge_topk_workspace_bytes)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))

from dglke_amd import emb_sim_cli, predict_cli  # noqa: E402
from dglke_amd._lib import KgeError  # noqa: E402

PREDICT_FLAGS = {"--model_path", "--format", "--data_files", "--raw_data", "--exec_mode", "--topK", "--score_func",
                 "--output", "--entity_mfile", "--rel_mfile", "--gpu"}
EMB_SIM_FLAGS = {"--mfile", "--emb_file", "--format", "--data_files", "--raw_data", "--exec_mode", "--topK", "--sim_func",
                 "--output", "--gpu"}


def _flags(parser):
    return {s for a in parser._actions for s in a.option_strings if s.startswith("--") and s != "--help"}


def test_flag_sets_and_defaults():
    assert _flags(predict_cli.ArgParser()) == PREDICT_FLAGS
    assert _flags(emb_sim_cli.ArgParser()) == EMB_SIM_FLAGS
    a = predict_cli.ArgParser().parse_args([])
    assert (a.model_path, a.exec_mode, a.topK, a.score_func, a.output, a.gpu, a.raw_data) == \
        ("ckpts", "all", 10, "none", "result.tsv", -1, False)
    b = emb_sim_cli.ArgParser().parse_args([])
    assert (b.exec_mode, b.topK, b.sim_func, b.output, b.gpu) == ("all", 10, "cosine", "result.tsv", -1)


def _model_dir(tmp, model="DistMult"):
    with open(os.path.join(tmp, "config.json"), "w") as f:
        json.dump({"model_name": model, "dataset": "toy", "hidden_dim": 8, "gamma": 12.0, "double_ent": False,
                   "double_rel": False, "lr": 0.1}, f)
    with open(os.path.join(tmp, "e.tsv"), "w") as f:
        f.write("0\talpha\n1\tbeta\n2\tgamma delta\n")
    with open(os.path.join(tmp, "r.tsv"), "w") as f:
        f.write("0\tknows\n1\tlikes\n")
    with open(os.path.join(tmp, "h.list"), "w") as f:
        f.write("beta\ngamma delta\nbeta")                 # (no newline at the end)
    with open(os.path.join(tmp, "r.list"), "w") as f:
        f.write("likes\n")
    with open(os.path.join(tmp, "ids.list"), "w") as f:
        f.write("2\n0\n2\n")
    with open(os.path.join(tmp, "one.list"), "w") as f:
        f.write("1\n")
    return tmp


def _pargs(tmp, *extra):
    return predict_cli.ArgParser().parse_args(["--model_path", tmp, "--gpu", "0"] + list(extra))


def test_predict_inputs_raw_and_ids(tmp_path):
    tmp = _model_dir(str(tmp_path))
    a = _pargs(tmp, "--format", "h_r_*", "--data_files", tmp + "/h.list", tmp + "/r.list", "--raw_data",
               "--entity_mfile", tmp + "/e.tsv", "--rel_mfile", tmp + "/r.tsv")
    cfg, h, r, t, id2e, id2r = predict_cli.check_args(a)
    assert cfg == {"model_name": "DistMult", "dataset": "toy", "hidden_dim": 8, "gamma": 12.0, "double_ent": False,
                   "double_rel": False}
    assert h.tolist() == [1, 2, 1] and r.tolist() == [1] and t is None
    assert id2e[2] == "gamma delta" and id2r[0] == "knows"
    a = _pargs(tmp, "--format", "*_*_t", "--data_files", tmp + "/ids.list")
    _, h, r, t, id2e, _ = predict_cli.check_args(a)
    assert h is None and r is None and t.tolist() == [2, 0, 2] and id2e is None
    for fmt, n in predict_cli.FORMATS.items():
        a = _pargs(tmp, "--format", fmt, "--data_files", *([tmp + "/ids.list"] * sum(n)))
        _, h, r, t, _, _ = predict_cli.check_args(a)
        assert [x is not None for x in (h, r, t)] == list(n)


def test_emb_sim_inputs(tmp_path):
    tmp = _model_dir(str(tmp_path))
    p = emb_sim_cli.ArgParser()
    a = p.parse_args(["--emb_file", "x.npy", "--gpu", "0", "--format", "l_r", "--data_files", tmp + "/h.list", tmp + "/h.list",
                      "--raw_data", "--mfile", tmp + "/e.tsv"])
    left, right, id2e = emb_sim_cli.check_args(a)
    assert left.tolist() == [1, 2, 1] == right.tolist() and id2e[0] == "alpha"
    a = p.parse_args(["--emb_file", "x.npy", "--gpu", "0", "--format", "*"])
    assert emb_sim_cli.check_args(a) == (None, None, None)


def test_tsv_writers(tmp_path):
    out = str(tmp_path / "p.tsv")
    res = [(np.array([1, 1]), np.array([0, 1]), np.array([2, 0]), np.array([0.1, -3.25], np.float32))]
    predict_cli.write_tsv(out, res, {0: "a", 1: "b", 2: "c"}, {0: "x", 1: "y"})
    assert open(out).read() == "head\trel\ttail\tscore\nb\tx\tc\t{}\nb\ty\ta\t-3.25\n".format(float(np.float32(0.1)))
    predict_cli.write_tsv(out, res)
    assert open(out).read().splitlines()[1] == "1\t0\t2\t0.10000000149011612"
    emb_sim_cli.write_tsv(out, [(np.array([3]), np.array([4]), np.array([0.5], np.float32))])
    assert open(out).read() == "left\tright\tscore\n3\t4\t0.5\n"


@pytest.mark.parametrize("extra, msg", [
    (["--gpu", "-1"], "GPU only"),
    (["--topK", "0"], "outside 1 .. 128"),
    (["--topK", "129"], "outside 1 .. 128"),
    (["--exec_mode", "per_head"], "unknown --exec_mode"),
    (["--format", "h_t"], "unknown --format"),
    (["--score_func", "sigmoid"], "unknown --score_func"),
    (["--exec_mode", "triplet_wise", "--format", "h_r_t", "--data_files", "H", "R", "H"], "same length"),
])
def test_predict_refusals(tmp_path, extra, msg):
    tmp = _model_dir(str(tmp_path))
    argv = ["--model_path", tmp, "--gpu", "0", "--format", "h_*_*", "--data_files", tmp + "/ids.list"]
    extra = [tmp + "/h.list" if x == "H" else tmp + "/r.list" if x == "R" else x for x in extra]
    if "--raw_data" not in extra and "--data_files" in extra:
        extra = extra + ["--raw_data", "--entity_mfile", tmp + "/e.tsv", "--rel_mfile", tmp + "/r.tsv"]
    a = predict_cli.ArgParser().parse_args(argv + extra)
    with pytest.raises(KgeError, match=msg):
        predict_cli.check_args(a)


def test_predict_refuses_transr(tmp_path):
    tmp = _model_dir(str(tmp_path), "TransR")
    with pytest.raises(KgeError, match="TransR"):
        predict_cli.check_args(_pargs(tmp, "--format", "h_*_*", "--data_files", tmp + "/ids.list"))


@pytest.mark.parametrize("extra, msg", [
    (["--gpu", "-1"], "GPU only"),
    (["--topK", "0"], "outside 1 .. 128"),
    (["--topK", "1000"], "outside 1 .. 128"),
    (["--exec_mode", "batch_right"], "unknown --exec_mode"),
    (["--format", "r_l"], "unknown --format"),
    (["--sim_func", "l3"], "unknown --sim_func"),
    (["--exec_mode", "pairwise", "--format", "l_r", "--data_files", "A", "B"], "same length"),
])
def test_emb_sim_refusals(tmp_path, extra, msg):
    tmp = _model_dir(str(tmp_path))
    argv = ["--emb_file", "x.npy", "--gpu", "0", "--format", "*"]
    extra = [tmp + "/ids.list" if x == "A" else tmp + "/one.list" if x == "B" else x for x in extra]
    a = emb_sim_cli.ArgParser().parse_args(argv + extra)
    with pytest.raises(KgeError, match=msg):
        emb_sim_cli.check_args(a)


def test_api_refuses_cpu_and_transr():
    from dglke_amd.infer import EmbSimInfer, ScoreInfer
    cfg = {"model_name": "DistMult", "dataset": "toy", "hidden_dim": 8, "gamma": 1.0, "double_ent": False, "double_rel": False}
    with pytest.raises(KgeError, match="GPU only"):
        ScoreInfer(-1, cfg, ".", "none")
    with pytest.raises(KgeError, match="TransR"):
        ScoreInfer(0, dict(cfg, model_name="TransR"), ".", "none")
    with pytest.raises(KgeError, match="GPU only"):
        EmbSimInfer(-1, "x.npy", "cosine")


def test_workspace_does_not_grow_with_candidates():
    from dglke_amd import _lib
    h = _lib.lib()
    rows, D, K = 1024, 400, 128
    w5 = h.kge_topk_workspace_bytes(rows, 10 ** 5, D, K)
    w7 = h.kge_topk_workspace_bytes(rows, 10 ** 7, D, K)
    assert 0 < w7 < rows * 10 ** 7 * 4 // 100               # far below a [rows, N] score block
    norms = lambda n: (n * 4 + 255) // 256 * 256
    assert w7 - norms(10 ** 7) == w5 - norms(10 ** 5)
    assert h.kge_topk_workspace_bytes(rows, 10 ** 7, D, 129) == 0


def test_infer_applies_no_torch_ranking():
    src = open(os.path.join(ROOT, "dgl-ke_amd", "dglke_amd", "infer.py")).read()
    for op in (".topk(", ".sort(", "argsort", "matmul", "cdist", "einsum", " @ ", "import oracle", "from oracle"):
        assert op not in src, op


def test_ids_outside_the_tables_are_refused_before_the_device():
    """a head / relation / tail / left / right id outside its table raises KgeError on the host (the kernels read rows at
    these ids); nothing is loaded or launched: the objects below have no tables on any device"""
    from dglke_amd.infer import EmbSimInfer, ScoreInfer, host_ids
    cfg = {"model_name": "DistMult", "dataset": "toy", "hidden_dim": 8, "gamma": 1.0, "double_ent": False, "double_rel": False}
    m = ScoreInfer(0, cfg, ".", "none")
    m.num_entity, m.num_rel = 10, 3
    for kw, msg in ((dict(head=[1, 10]), "head id 10 is outside 0 .. 9"), (dict(rel=[-1]), "relation id -1"),
                    (dict(tail=[0, 12, 3]), "tail id 12"), (dict(rel=[3]), "relation id 3 is outside 0 .. 2")):
        for mode in ("all", "triplet_wise") if "rel" not in kw else ("batch_rel",):
            with pytest.raises(KgeError, match=msg):
                m.topK(exec_mode=mode, k=5, **kw)
    e = EmbSimInfer(0, "x.npy", "l2")

    class Shape(object):
        shape = (7, 4)
    e.emb = Shape()
    with pytest.raises(KgeError, match="left id 7"):
        e.topK([0, 7], None, k=3)
    with pytest.raises(KgeError, match="right id -2"):
        e.topK(None, [-2], bcast=True, k=3)
    assert host_ids(None, 5, "head") is None and host_ids([0, 4], 5, "head").tolist() == [0, 4]
