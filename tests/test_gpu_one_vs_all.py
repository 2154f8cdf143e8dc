"""The 1-vs-all softmax step on the device: StepEngine(one_vs_all=True).step -> kge_step_fused on a batch with N == 0 (csrc/kge_onevsall.hip) against
the float64 statement of one_vs_all_cases.py.

Tolerance of a compared quantity: 8 x the error the float32 restatement of the same formulas (one_vs_all_cases.step with
dtype=float32) makes against the float64 result on that case - the kernels sum in tile order and use the hardware exponential - with
a floor of 4 fp32 ulps of the quantity's largest component.  Every measured error and its bound go to profiles/one_vs_all_errors.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import one_vs_all_cases as V
from dglke_amd import _lib, plan
from dglke_amd.engine import StepEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANT = ("loss", "pos", "g_rel", "ent", "ent_state", "rel", "rel_state")
LINES = {}


def run_step(c, tables, batch):
    eng = StepEngine(c.model, c.n_ent, V.N_REL, c.d, 12.0, V.LR, DEV, regularization_coef=c.reg_coef, loss_genre='Softmax',
                     one_vs_all=True)
    eng.load_tables(tables[0], tables[2], tables[1], tables[3])
    hi, ri, ti, w = batch
    b = plan.make_batch(hi, ti, ri, np.zeros(0, np.int64), c.B, 0, c.neg_head, DEV, edge_w=w)
    want = dict(pos_score=torch.empty(c.B, device=DEV), g_rel=torch.empty(c.B, c.d, device=DEV))
    eng.step(b, want)
    torch.cuda.synchronize()
    got = dict(loss=np.float32(eng.read_loss()[2]), pos=want["pos_score"], g_rel=want["g_rel"], ent=eng.ent, ent_state=eng.ent_state,
               rel=eng.rel, rel_state=eng.rel_state)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}, eng, b


def _report(name, rows):
    LINES[name] = rows
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "one_vs_all_errors.txt"), "w") as f:
        f.write("kge_step_fused on N == 0 batches against the float64 statement: per case and quantity the largest |error|, its bound (8 x the "
                "float32 restatement's error, floor 4 ulp of the largest component) and their ratio (<= 1 passes)\n")
        for n in sorted(LINES):
            for q, err, bound in LINES[n]:
                f.write("%-44s %-10s err %.3e  bound %.3e  ratio %.3f\n" % (n, q, err, bound, err / bound))


@pytest.mark.parametrize("c", V.CASES, ids=lambda c: c.name)
def test_step_matches_statement(c):
    tables, batch = V.inputs(c)
    ref, f32 = V.step(c, tables, batch), V.step(c, tables, batch, np.float32)
    got, _, _ = run_step(c, tables, batch)
    rows = []
    for q in QUANT:
        r = np.asarray(ref[q], np.float64)
        assert np.all(np.isfinite(got[q])), q
        err = float(np.abs(got[q] - r).max())
        bound = max(8.0 * float(np.abs(np.asarray(f32[q], np.float64) - r).max()), 4 * 2.0 ** -23 * float(np.abs(r).max()))
        rows.append((q, err, bound))
    _report(c.name, rows)
    print("\n".join("%s %s err %.3e bound %.3e" % ((c.name,) + x) for x in rows))
    for q, err, bound in rows:
        assert err <= bound, (q, err, bound)


def test_two_runs_are_bit_identical():
    c = V.DETERMINISM
    tables, batch = V.inputs(c)
    one, two = run_step(c, tables, batch)[0], run_step(c, tables, batch)[0]
    for q in QUANT:
        assert np.array_equal(one[q], two[q]), q


def _set(**kw):
    return lambda eng, b, out: [setattr(eng.hp, k, v) for k, v in kw.items()]


REFUSALS = {
    "model": (_set(model=_lib.MODEL_IDS["TransE_l2"]), "DistMult and ComplEx"),
    "loss_genre": (_set(loss_genre=_lib.LOSS_IDS["Logsigmoid"]), "KGE_LOSS_SOFTMAX"),
    "adv": (_set(adv=1), "adv"),
    "pairwise": (_set(pairwise=1), "pairwise"),
    "width": (_set(d_e=516, d_r=516), "d_e"),
    "ent_norm": (_set(flags=_lib.NORM_FLAGS['ent']['clip']), "NORM"),
    "rel_norm": (_set(flags=_lib.NORM_FLAGS['rel']['unit']), "NORM"),
    "neg_deg": (_set(flags=_lib.FLAG_NEG_DEG_SAMPLE), "NEG_DEG_SAMPLE"),
    "neg_score": (lambda eng, b, out: setattr(out, "neg_score", eng.ent.data_ptr()), "neg_score"),
    "g_neg": (lambda eng, b, out: setattr(out, "g_neg", eng.ent.data_ptr()), "g_neg"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_entry_refuses(what):
    c = V.CASES[0]
    tables, batch = V.inputs(c)
    _, eng, b = run_step(c, tables, batch)
    before = [t.clone() for t in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)]
    out = _lib.KgeStepOut()
    change, text = REFUSALS[what]
    change(eng, b, out)
    ws = eng.workspace_for(b) if what != "width" else eng._ws
    rc = _lib.lib().kge_step_fused(C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), _lib.ptr(ws), eng._ws_bytes,
                                   _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and text in _lib.lib().kge_last_error().decode(), _lib.lib().kge_last_error()
    for t0, t1 in zip(before, (eng.ent, eng.ent_state, eng.rel, eng.rel_state)):
        assert torch.equal(t0, t1)


@pytest.mark.parametrize("what", ["capture", "step_async", "emit", "sample_job", "attach_known"])
def test_engine_refuses(what):
    c = V.CASES[0]
    _, eng, b = run_step(c, *V.inputs(c))
    calls = dict(capture=lambda: eng.capture([b]), step_async=lambda: eng.step_async(b), emit=lambda: eng.step(b, emit=_lib.KgeEmit()),
                 sample_job=lambda: eng.step(b, sample_job=_lib.KgeSamplerJob()), attach_known=lambda: eng.attach_known(None))
    with pytest.raises(_lib.KgeError, match="one_vs_all"):
        calls[what]()
    with pytest.raises(_lib.KgeError, match="one_vs_all.*Adam"):
        StepEngine(c.model, c.n_ent, V.N_REL, c.d, 12.0, V.LR, DEV, loss_genre='Softmax', one_vs_all=True, optimizer='Adam')


def test_cli_trains_on_the_planted_graph(tmp_path, capsys):
    import glob
    import json
    from dglke_amd import train as T
    from test_gpu_cli import _planted
    _planted(str(tmp_path / "kg"))
    T.main(["--model_name", "DistMult", "--format", "udd_hrt", "--dataset", "toy", "--data_path", str(tmp_path / "kg"), "--data_files",
            "e.dict", "r.dict", "train.txt", "valid.txt", "test.txt", "--save_path", str(tmp_path / "ckpts"), "--gpu", "0",
            "--batch_size", "256", "--neg_sample_size", "64", "--hidden_dim", "32", "-g", "8", "--lr", "0.1", "--max_step", "100",
            "--log_interval", "50", "--one_vs_all"])
    out = capsys.readouterr().out
    losses = [float(ln.rsplit(":", 1)[1]) for ln in out.splitlines() if "average loss" in ln]
    assert "--neg_sample_size 64 is ignored" in out and len(losses) == 2 and losses[1] < losses[0], out
    conf = json.load(open(glob.glob(str(tmp_path / "ckpts" / "*" / "config.json"))[0]))
    assert conf["one_vs_all"] is True and conf["loss_genre"] == "Softmax"
