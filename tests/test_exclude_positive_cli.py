"""dglke_train --exclude_positive: the flag, its refusals (before anything is created) and - on the GPU - training runs on the toy
graph of tests/test_gpu_cli.py with the known training triples left out of the negatives."""
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _argv(tmp_path, model, extra):
    data = str(tmp_path / "kg")
    return ["--model_name", model, "--format", "udd_hrt", "--dataset", "toy", "--data_path", data, "--data_files",
            "e.dict", "r.dict", "train.txt", "valid.txt", "test.txt", "--save_path", str(tmp_path / "ckpts"),
            "--batch_size", "256", "--neg_sample_size", "64", "--hidden_dim", "32", "-g", "8", "--lr", "0.25", "-adv",
            "--max_step", "300", "--log_interval", "150", "--graph_steps", "100", "--exclude_positive"] + extra


def test_parser_has_the_flag():
    from dglke_amd import train as T
    p = T.ArgParser()
    assert p.parse_args([]).exclude_positive is False
    assert p.parse_args(["--exclude_positive"]).exclude_positive is True


@pytest.mark.parametrize("extra", [["--gpu", "0", "1"], ["--gpu", "0", "--neg_deg_sample"],
                                   ["--gpu", "0", "--async_update", "--async_update_pipeline"],
                                   ["--gpu", "0", "--async_update", "--async_update_rel"]],
                         ids=["two_gpus", "neg_deg_sample", "async_pipeline", "async_rel"])
def test_refused_combinations_raise_before_the_save_directory_exists(tmp_path, extra):
    from dglke_amd import train as T
    from dglke_amd._lib import KgeError
    with pytest.raises(KgeError) as e:
        T.main(_argv(tmp_path, "TransE_l2", extra))
    assert "--exclude_positive" in str(e.value)
    assert not (tmp_path / "ckpts").exists() and not (tmp_path / "kg").exists()


def test_plain_async_update_is_not_refused():
    from dglke_amd import train as T
    args = T.ArgParser().parse_args(["--exclude_positive", "--async_update", "--gpu", "0"])
    T.check_exclude_positive(args)


@pytest.mark.gpu
@pytest.mark.parametrize("model,extra", [("TransE_l2", []), ("RotatE", ["-de"]), ("TransR", ["--lr", "0.05"]),
                                         ("TransE_l2", ["--num_proc", "2"])],
                         ids=["TransE_l2", "RotatE", "TransR", "TransE_l2-num_proc2"])
def test_train_cli_with_exclude_positive(tmp_path, capsys, model, extra):
    from dglke_amd import train as T
    from test_gpu_cli import _planted
    _planted(str(tmp_path / "kg"))
    tr = T.main(_argv(tmp_path, model, ["--gpu", "0"] + extra))
    out = capsys.readouterr().out
    assert "--exclude_positive" in out and "known training triples excluded" in out
    assert tr.known is not None and all(lane.engine._known is not None for lane in tr.lanes)
    assert len(tr.lanes) == (2 if "--num_proc" in extra else 1)
    conf = json.load(open(os.path.join(tr.args.save_path, "config.json")))
    assert conf["exclude_positive"] is True and conf["model_name"] == model
    last = [l for l in out.split("\n") if "(300/300) average loss:" in l]
    assert len(last) == len(tr.lanes)
    for l in last:
        assert math.isfinite(float(l.split(":")[1]))
    assert np.isfinite(tr.model.entity_emb.emb.cpu().numpy()).all()
