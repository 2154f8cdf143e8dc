"""The 1-vs-all step's host side, without a GPU: the float64 statement against torch.autograd, plans without negatives, and the
refusals of dglke_train --one_vs_all (each before any dataset is read)."""
import numpy as np
import pytest
import torch

import one_vs_all_cases as V
from dglke_amd import _lib, plan, train


@pytest.mark.parametrize("c", [V.CASES[0], V.CASES[8]], ids=lambda c: c.name)
def test_statement_agrees_with_autograd(c):
    tables, (hi, ri, ti, _) = V.inputs(c)
    ent, rel = (torch.tensor(tables[k], dtype=torch.float64, requires_grad=True) for k in (0, 2))
    w = np.linspace(0.5, 2.0, c.B)
    h, r, t = ent[hi], rel[ri], ent[ti]
    if c.model == 'DistMult':
        a, p = (t if c.neg_head else h) * r, (h * r * t).sum(1)
    else:
        cplx = lambda x: torch.complex(x[:, :c.d // 2], x[:, c.d // 2:])
        hc, rc, tc = cplx(h), cplx(r), cplx(t)
        ac = tc * rc.conj() if c.neg_head else hc * rc
        a, p = torch.cat([ac.real, ac.imag], 1), (hc * rc * tc.conj()).real.sum(1)
    S = a.detach() @ ent.detach().T                  # the statement's g and GA are gradients w.r.t. the scores and the operand
    S.requires_grad_(True)
    loss = (torch.tensor(w) * (torch.logsumexp(S, 1) - p)).sum() / c.B
    loss.backward(retain_graph=True)
    e64, r64 = tables[0].astype(np.float64), tables[2].astype(np.float64)
    l, pos, a_np, g = V.forward(c.model, c.neg_head, e64, r64, hi, ri, ti, w)
    assert abs(l - loss.item()) < 1e-12 and np.allclose(pos, p.detach().numpy(), atol=1e-12) and np.allclose(a_np, a.detach().numpy(), atol=1e-12)
    assert np.allclose(g, S.grad.numpy(), atol=1e-14)
    # the per-edge h / t / r gradients: autograd through a . GA + dp p
    GA = torch.tensor(g @ e64)
    ent.grad, rel.grad = None, None
    ((a * GA).sum() + (torch.tensor(-w / c.B) * p).sum()).backward()
    gh, gt, gr = V.edge_grads(c.model, c.neg_head, e64[hi], r64[ri], e64[ti], g @ e64, -w / c.B)
    ge, gl = np.zeros_like(e64), np.zeros_like(r64)
    np.add.at(ge, hi, gh), np.add.at(ge, ti, gt), np.add.at(gl, ri, gr)
    assert np.allclose(ge, ent.grad.numpy(), atol=1e-13) and np.allclose(gl, rel.grad.numpy(), atol=1e-13)


def test_plan_without_negatives():
    h, t, r = np.array([3, 1, 3, 5]), np.array([1, 1, 2, 3]), np.array([0, 1, 0, 1])
    p = plan.build_plan(h, t, r, np.zeros(0, np.int64), 4, 0, True)
    rec = p["ue_rec"].reshape(-1, 8)
    assert p["N"] == 0 and p["ue_neg_slot"].size == 0 and not p["ue_neg_ptr"].any() and p["UE"] == 4
    assert (rec[:, 7] == -1).all() and (rec[:, 4] == 0).all() and (rec[:, 5] == 0).all()
    assert rec[:, 6].tolist() == [1, 5, 0, 6]               # first (edge * 2 + side) of entities 1, 2, 3, 5
    # N > 0 is what it was: the records of a small example, worked out by hand
    q = plan.build_plan(h, t, r, np.array([5, 9, 1, 5]), 2, 2, False)
    assert q["ue_id"].tolist() == [1, 2, 3, 5, 9] and q["ue_neg_slot"].tolist() == [2, 0, 3, 1]
    assert q["ue_rec"].reshape(-1, 8)[:, 2:].tolist() == [[0, 3, 0, 1, 1, 2], [3, 4, 1, 1, 5, -1], [4, 7, 1, 1, 0, -1],
                                                          [7, 8, 1, 3, 6, 0], [8, 8, 3, 4, -1, 1]]


BASE = ["--model_name", "DistMult", "--one_vs_all", "--dataset", "no_such_dataset", "--data_path", "/nonexistent", "--gpu", "0",
        "--hidden_dim", "64"]
CLI = {
    "model": (["--model_name", "RotatE"], "DistMult and ComplEx"), "genre": (["--loss_genre", "Logistic"], "--loss_genre"),
    "adv": (["-adv"], "-adv"), "pw": (["-pw"], "-pw"), "neg_deg": (["--neg_deg_sample"], "--neg_deg_sample"),
    "exclude": (["--exclude_positive"], "--exclude_positive"), "subsampling": (["--subsampling_weight"], "--subsampling_weight"),
    "adam": (["--optimizer", "Adam"], "Adam"), "ent_norm": (["--ent_norm", "clip"], "--ent_norm"),
    "rel_norm": (["--rel_norm", "unit"], "--rel_norm"), "gpus": (["--gpu", "0", "1"], "--gpu"), "lanes": (["--num_proc", "2"], "--num_proc"),
    "async": (["--async_update"], "--async_update"), "graph": (["--graph_steps", "8"], "--graph_steps"),
    "ckpt": (["--checkpoint_interval", "10"], "--checkpoint_interval"), "resume": (["--resume", "latest"], "--resume"),
    "width": (["--hidden_dim", "514"], "entity width"),
}


@pytest.mark.parametrize("what", sorted(CLI))
def test_cli_refuses_before_loading(what):
    extra, text = CLI[what]
    with pytest.raises(_lib.KgeError) as e:
        train.main(BASE + extra)
    assert "--one_vs_all" in str(e.value) and text in str(e.value)
