"""SimplE and QuatE on the all-entity steps (csrc/kge_allent_clamp.hip; QuatE through the strict step's edge kernels):
StepEngine(one_vs_all / k_vs_all).step against the float64 statement of clamp_quate_cases.py, the command line on the planted graph,
and what stays refused.  Tolerance, the rule of test_gpu_one_vs_all.py: 8 x the error of the float32 restatement against the float64
result on that case, floor 4 fp32 ulps of the quantity's largest component.  Errors and bounds go to profiles/clamp_quate_errors.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import clamp_quate_cases as Q
from dglke_amd import _lib, plan
from dglke_amd.engine import StepEngine
from dglke_amd.known import KnownIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANT = ("loss", "pos", "g_rel", "ent", "ent_state", "rel", "rel_state")
LINES = {}


def _kw(crit):
    return dict(loss_genre='Softmax', one_vs_all=True) if crit == 'ova' else dict(loss_genre='BCE', k_vs_all=True, label_smoothing=Q.SMOOTH)


def run_step(c, tables, batch, known):
    eng = StepEngine(c.model, c.n_ent, Q.N_REL, c.d, 12.0, Q.LR, DEV, regularization_coef=c.reg_coef, **_kw(c.crit))
    eng.load_tables(tables[0], tables[2], tables[1], tables[3])
    if c.crit == 'kva':
        eng.attach_known(KnownIndex(known, c.n_ent, Q.N_REL, DEV))
    hi, ri, ti, w = batch
    b = plan.make_batch(hi, ti, ri, np.zeros(0, np.int64), c.B, 0, c.neg_head, DEV, edge_w=w)
    want = dict(pos_score=torch.empty(c.B, device=DEV), g_rel=torch.empty(c.B, c.d, device=DEV))
    eng.step(b, want)
    torch.cuda.synchronize()
    got = dict(loss=np.float32(eng.read_loss()[2]), pos=want["pos_score"], g_rel=want["g_rel"], ent=eng.ent, ent_state=eng.ent_state,
               rel=eng.rel, rel_state=eng.rel_state)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}, eng, b


@pytest.mark.parametrize("c", Q.CASES, ids=lambda c: c.name)
def test_step_matches_statement(c):
    tables, batch, known = Q.inputs(c)
    ref, f32 = Q.step(c, tables, batch, known), Q.step(c, tables, batch, known, np.float32)
    got, _, _ = run_step(c, tables, batch, known)
    rows = []
    for q in QUANT:
        r = np.asarray(ref[q], np.float64)
        assert np.all(np.isfinite(got[q])), q
        err = float(np.abs(got[q] - r).max())
        rows.append((q, err, max(8.0 * float(np.abs(np.asarray(f32[q], np.float64) - r).max()), 4 * 2.0 ** -23 * float(np.abs(r).max()))))
    LINES[c.name] = rows
    with open(os.path.join(ROOT, "profiles", "clamp_quate_errors.txt"), "w") as f:
        f.write("SimplE / QuatE all-entity steps against the float64 statement: largest |error|, bound, ratio\n")
        f.writelines("%-44s %-10s err %.3e  bound %.3e  ratio %.3f\n" % (n, q, e, b, e / b) for n in sorted(LINES) for q, e, b in LINES[n])
    print("\n".join("%s %s err %.3e bound %.3e" % ((c.name,) + x) for x in rows))
    for q, err, bound in rows:
        assert err <= bound, (q, err, bound)
    if c.kind == 'weights':                                      # a second run: bit-identical
        again = run_step(c, tables, batch, known)[0]
        assert all(np.array_equal(got[q], again[q]) for q in QUANT)


@pytest.mark.parametrize("model", ["SimplE", "QuatE"])
def test_cli_trains_and_tests_on_the_planted_graph(model, tmp_path, capsys):
    from dglke_amd import train as TR
    from test_gpu_cli import _planted
    _planted(str(tmp_path / "kg"))
    TR.main(["--model_name", model, "--format", "udd_hrt", "--dataset", "toy", "--data_path", str(tmp_path / "kg"), "--data_files", "e.dict",
             "r.dict", "train.txt", "valid.txt", "test.txt", "--save_path", str(tmp_path / "ckpts"), "--gpu", "0", "--batch_size", "256",
             "--neg_sample_size", "64", "--hidden_dim", "32", "-g", "8", "--lr", "0.1", "--max_step", "100", "--log_interval", "50",
             "--k_vs_all", "--label_smoothing", "0.1", "--test"])
    out = capsys.readouterr().out
    losses = [float(ln.rsplit(":", 1)[1]) for ln in out.splitlines() if "average loss" in ln]
    assert len(losses) == 2 and losses[1] < losses[0], out
    mrr = [float(ln.rsplit(":", 1)[1]) for ln in out.splitlines() if "MRR" in ln]
    assert mrr and all(np.isfinite(x) and 0 < x <= 1 for x in mrr), out


@pytest.mark.parametrize("crit", ["ova", "kva"])
@pytest.mark.parametrize("model,adam", [("TransE_l2", False), ("RotatE", False), ("SimplE", True), ("QuatE", True)])
def test_still_refused_by_the_engine_and_the_c_entry(model, adam, crit):      # (Adam, kge_step_optim: the strict step's batch check)
    with pytest.raises(_lib.KgeError, match="Adam" if adam else "DistMult and ComplEx"):
        StepEngine(model, 63, Q.N_REL, 8, 12.0, Q.LR, DEV, optimizer='Adam' if adam else 'Adagrad', **_kw(crit))
    c = [x for x in Q.CASES if x.crit == crit and x.model == (model if adam else 'SimplE')][0]
    _, eng, b = run_step(c, *Q.inputs(c))
    before = [t.clone() for t in (eng.ent, eng.ent_state, eng.rel, eng.rel_state)]
    h, ws, hp, tb, s = _lib.lib(), eng.workspace_for(b), C.byref(eng.hp), C.byref(eng.tb), _lib.stream_ptr()
    if adam:
        mom = [torch.zeros(n, 2, c.d, device=DEV) for n in (c.n_ent, Q.N_REL)]
        opt = _lib.KgeOptim(_lib.OPT_ADAM, 0.9, 0.999, 1e-8, mom[0].data_ptr(), mom[1].data_ptr())
        rc = h.kge_step_optim(hp, C.byref(opt), tb, C.byref(b.c), None, _lib.ptr(ws), eng._ws_bytes, _lib.PHASE_ALL, None, None, 0, s)
    else:
        eng.hp.model = _lib.MODEL_IDS[model]
        rc = (h.kge_step_fused(hp, tb, C.byref(b.c), None, _lib.ptr(ws), eng._ws_bytes, s) if crit == 'ova' else
              h.kge_step_fused_known(hp, tb, C.byref(b.c), None, _lib.ptr(ws), eng._ws_bytes, None, C.byref(eng._known[0]), None, 0, s))
    torch.cuda.synchronize()
    text = h.kge_last_error().decode()
    assert rc == -1 and (("kge_step: need C*chunk == B" in text) if adam else ("DistMult and ComplEx" in text and model in text)), text
    for t0, t1 in zip(before, (eng.ent, eng.ent_state, eng.rel, eng.rel_state)):
        assert torch.equal(t0, t1)
