"""dglke_train --k_vs_all without a GPU: the refusals of the flag, each before any dataset is read."""
import pytest

from dglke_amd import _lib, train


BASE = ["--model_name", "DistMult", "--k_vs_all", "--dataset", "no_such_dataset", "--data_path", "/nonexistent", "--gpu", "0",
        "--hidden_dim", "64"]
CLI = {
    "model": (["--model_name", "RotatE"], "DistMult and ComplEx"), "genre": (["--loss_genre", "Softmax"], "--loss_genre"),
    "one_vs_all": (["--one_vs_all"], "--one_vs_all"), "exclude": (["--exclude_positive"], "--exclude_positive"),
    "smoothing": (["--label_smoothing", "1.0"], "--label_smoothing"), "adv": (["-adv"], "-adv"),
    "adam": (["--optimizer", "Adam"], "Adam"), "ent_norm": (["--ent_norm", "clip"], "--ent_norm"),
    "lanes": (["--num_proc", "2"], "--num_proc"), "graph": (["--graph_steps", "8"], "--graph_steps"),
    "ckpt": (["--checkpoint_interval", "10"], "--checkpoint_interval"), "width": (["--hidden_dim", "514"], "entity width"),
}


@pytest.mark.parametrize("what", sorted(CLI))
def test_cli_refuses_before_loading(what):
    extra, text = CLI[what]
    with pytest.raises(_lib.KgeError) as e:
        train.main(BASE + extra)
    assert "--k_vs_all" in str(e.value) and text in str(e.value)


def test_label_smoothing_needs_the_flag():
    with pytest.raises(_lib.KgeError, match="--label_smoothing belongs to --k_vs_all"):
        train.main([a for a in BASE if a != "--k_vs_all"] + ["--label_smoothing", "0.1"])
