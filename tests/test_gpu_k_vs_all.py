"""The K-vs-all step on the device: StepEngine(k_vs_all=True).step -> kge_step_fused_known on a batch with N == 0
(csrc/kge_kvsall.hip) against the float64 statement of k_vs_all_cases.py.

Tolerance of a compared quantity, the rule of test_gpu_one_vs_all.py: 8 x the error the float32 restatement of the same formulas
makes against the float64 result on that case, with a floor of 4 fp32 ulps of the quantity's largest component.  Every measured
error and its bound go to profiles/k_vs_all_errors.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import k_vs_all_cases as K
from dglke_amd import _lib, plan
from dglke_amd.engine import StepEngine
from dglke_amd.known import KnownIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANT = ("loss", "pos", "g_rel", "ent", "ent_state", "rel", "rel_state")
LINES = {}


def run_step(c, tables, batch, known):
    eng = StepEngine(c.model, c.n_ent, K.N_REL, c.d, 12.0, K.LR, DEV, regularization_coef=c.reg_coef, loss_genre='BCE',
                     k_vs_all=True, label_smoothing=c.smooth)
    eng.load_tables(tables[0], tables[2], tables[1], tables[3])
    eng.attach_known(KnownIndex(known, c.n_ent, K.N_REL, DEV))
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
    with open(os.path.join(ROOT, "profiles", "k_vs_all_errors.txt"), "w") as f:
        f.write("kge_step_fused_known on N == 0 batches against the float64 statement: per case and quantity the largest |error|, its "
                "bound (8 x the float32 restatement's error, floor 4 ulp of the largest component) and their ratio (<= 1 passes)\n")
        for n in sorted(LINES):
            for q, err, bound in LINES[n]:
                f.write("%-52s %-10s err %.3e  bound %.3e  ratio %.3f\n" % (n, q, err, bound, err / bound))


@pytest.mark.parametrize("c", K.CASES, ids=lambda c: c.name)
def test_step_matches_statement(c):
    tables, batch, known = K.inputs(c)
    ref, f32 = K.step(c, tables, batch, known), K.step(c, tables, batch, known, np.float32)
    got, _, _ = run_step(c, tables, batch, known)
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
    c = K.DETERMINISM
    tables, batch, known = K.inputs(c)
    one, two = run_step(c, tables, batch, known)[0], run_step(c, tables, batch, known)[0]
    for q in QUANT:
        assert np.array_equal(one[q], two[q]), q


def _set(**kw):
    return lambda eng, kn, out: [setattr(eng.hp, k, v) for k, v in kw.items()]


REFUSALS = {
    "model": (_set(model=_lib.MODEL_IDS["TransE_l2"]), "DistMult and ComplEx"),
    "softmax": (_set(loss_genre=_lib.LOSS_IDS["Softmax"]), "KGE_LOSS_SOFTMAX with a known index"),
    "loss_genre": (_set(loss_genre=_lib.LOSS_IDS["Logsigmoid"]), "KGE_LOSS_BCE"),
    "adv": (_set(adv=1), "adv"),
    "smoothing": (_set(margin=1.0), "[0, 1)"),
    "width": (_set(d_e=516, d_r=516), "d_e"),
    "ent_norm": (_set(flags=_lib.NORM_FLAGS['ent']['clip']), "NORM"),
    "neg_deg": (_set(flags=_lib.FLAG_NEG_DEG_SAMPLE), "NEG_DEG_SAMPLE"),
    "g_neg": (lambda eng, kn, out: setattr(out, "g_neg", eng.ent.data_ptr()), "g_neg"),
    "n_rel": (lambda eng, kn, out: setattr(kn, "n_rel", 0), "n_rel"),
    "no_arrays": (lambda eng, kn, out: (setattr(kn, "m_tail", 5), setattr(kn, "keys_tail", None)), "kge_known"),
    "job": (None, "sampler job"),
    "null_ws": (None, "null argument"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_entry_refuses(what):
    c = K.CASES[0]
    tables, batch, known = K.inputs(c)
    _, eng, b = run_step(c, tables, batch, known)
    before = [t.clone() for t in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)]
    out, kn = _lib.KgeStepOut(), eng._known[0]
    change, text = REFUSALS[what]
    job = C.byref(_lib.KgeSamplerJob()) if what == "job" else None
    if change:
        change(eng, kn, out)
    ws = None if what == "null_ws" else _lib.ptr(eng._ws)
    rc = _lib.lib().kge_step_fused_known(C.byref(eng.hp), C.byref(eng.tb), C.byref(b.c), C.byref(out), ws, eng._ws_bytes,
                                         job, C.byref(kn), None, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and text in _lib.lib().kge_last_error().decode(), _lib.lib().kge_last_error()
    for t0, t1 in zip(before, (eng.ent, eng.ent_state, eng.rel, eng.rel_state)):
        assert torch.equal(t0, t1)


@pytest.mark.parametrize("what", ["capture", "step_async", "emit", "sample_job", "no_index"])
def test_engine_refuses(what):
    c = K.CASES[0]
    tables, batch, known = K.inputs(c)
    _, eng, b = run_step(c, tables, batch, known)
    calls = dict(capture=lambda: eng.capture([b]), step_async=lambda: eng.step_async(b), emit=lambda: eng.step(b, emit=_lib.KgeEmit()),
                 sample_job=lambda: eng.step(b, sample_job=_lib.KgeSamplerJob()),
                 no_index=lambda: (eng.attach_known(None), eng.step(b)))
    with pytest.raises(_lib.KgeError, match="k_vs_all"):
        calls[what]()
    with pytest.raises(_lib.KgeError, match="k_vs_all.*one_vs_all"):
        StepEngine(c.model, c.n_ent, K.N_REL, c.d, 12.0, K.LR, DEV, loss_genre='BCE', k_vs_all=True, one_vs_all=True)
    with pytest.raises(_lib.KgeError, match="k_vs_all.*BCE"):
        StepEngine(c.model, c.n_ent, K.N_REL, c.d, 12.0, K.LR, DEV, loss_genre='Softmax', k_vs_all=True)


def test_cli_trains_on_the_planted_graph(tmp_path, capsys):
    import glob
    import json
    from dglke_amd import train as T
    from test_gpu_cli import _planted
    _planted(str(tmp_path / "kg"))
    T.main(["--model_name", "DistMult", "--format", "udd_hrt", "--dataset", "toy", "--data_path", str(tmp_path / "kg"), "--data_files",
            "e.dict", "r.dict", "train.txt", "valid.txt", "test.txt", "--save_path", str(tmp_path / "ckpts"), "--gpu", "0",
            "--batch_size", "256", "--neg_sample_size", "64", "--hidden_dim", "32", "-g", "8", "--lr", "0.1", "--max_step", "100",
            "--log_interval", "50", "--k_vs_all", "--label_smoothing", "0.1"])
    out = capsys.readouterr().out
    losses = [float(ln.rsplit(":", 1)[1]) for ln in out.splitlines() if "average loss" in ln]
    assert "[Train] --k_vs_all" in out and len(losses) == 2 and losses[1] < losses[0], out
    conf = json.load(open(glob.glob(str(tmp_path / "ckpts" / "*" / "config.json"))[0]))
    assert conf["k_vs_all"] is True and conf["label_smoothing"] == 0.1 and conf["loss_genre"] == "BCE"
