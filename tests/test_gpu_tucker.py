"""TuckER on the device (csrc/kge_tucker.hip): StepEngine('TuckER', one_vs_all / k_vs_all).step against the float64 statement of
tucker_cases.py, eval.Ranker against float64 ranks on an integer grid, and the entries that stay closed to the model.

Tolerance of a compared quantity, the rule of test_gpu_one_vs_all.py: 8 x the error the float32 restatement of the same formulas
makes against the float64 result on that case, with a floor of 4 fp32 ulps of the quantity's largest component.  Every measured
error and its bound go to profiles/tucker_errors.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tucker_cases as T
from dglke_amd import _lib, plan
from dglke_amd.engine import StepEngine
from dglke_amd.eval import Ranker
from dglke_amd.known import KnownIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANT = ("loss", "pos", "g_rel", "ent", "ent_state", "rel", "rel_state", "core", "core_state")
LINES = {}


def run_step(c, tables, batch, known):
    kw = dict(loss_genre='Softmax', one_vs_all=True) if c.crit == 'ova' else dict(loss_genre='BCE', k_vs_all=True, label_smoothing=T.SMOOTH)
    eng = StepEngine('TuckER', c.n_ent, T.N_REL, c.d_e, 12.0, T.LR, DEV, regularization_coef=c.reg_coef, relation_dim=c.d_r, **kw)
    eng.load_tables(tables[0], tables[2], tables[1], tables[3])
    eng.proj.copy_(torch.as_tensor(tables[4]).reshape(eng.proj.shape))
    eng.proj_state.copy_(torch.as_tensor(tables[5]))
    if c.crit == 'kva':
        eng.attach_known(KnownIndex(known, c.n_ent, T.N_REL, DEV))
    hi, ri, ti, w = batch
    b = plan.make_batch(hi, ti, ri, np.zeros(0, np.int64), c.B, 0, c.neg_head, DEV, edge_w=w)
    want = dict(pos_score=torch.empty(c.B, device=DEV), g_rel=torch.empty(c.B, c.d_r, device=DEV))
    eng.step(b, want)
    torch.cuda.synchronize()
    got = dict(loss=np.float32(eng.read_loss()[2]), pos=want["pos_score"], g_rel=want["g_rel"], ent=eng.ent, ent_state=eng.ent_state,
               rel=eng.rel, rel_state=eng.rel_state, core=eng.proj, core_state=eng.proj_state)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}, eng, b


def _report(name, rows):
    LINES[name] = rows
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tucker_errors.txt"), "w") as f:
        f.write("TuckER steps against the float64 statement: largest |error|, bound (8 x the float32 restatement's, floor 4 ulp), ratio\n")
        for n in sorted(LINES):
            for q, err, bound in LINES[n]:
                f.write("%-44s %-10s err %.3e  bound %.3e  ratio %.3f\n" % (n, q, err, bound, err / bound))


@pytest.mark.parametrize("c", T.CASES, ids=lambda c: c.name)
def test_step_matches_statement(c):
    tables, batch, known = T.inputs(c)
    ref, f32 = T.step(c, tables, batch, known), T.step(c, tables, batch, known, np.float32)
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
    c = T.DETERMINISM
    tables, batch, known = T.inputs(c)
    one, two = run_step(c, tables, batch, known)[0], run_step(c, tables, batch, known)[0]
    for q in QUANT:
        assert np.array_equal(one[q], two[q]), q


@pytest.mark.parametrize("neg_head", [False, True])
@pytest.mark.parametrize("filtered", [False, True])
def test_ranks_equal_float64_on_an_integer_grid(neg_head, filtered):
    rng = np.random.RandomState(5)
    n_ent, d_e, d_r, E = 129, 8, 4, 40
    ent, rel = rng.randint(-2, 3, (n_ent, d_e)), rng.randint(-2, 3, (T.N_REL, d_r))
    W = rng.randint(-2, 3, (d_r, d_e, d_e))
    h, t, r = rng.randint(0, n_ent, E), rng.randint(0, n_ent, E), rng.randint(0, T.N_REL, E)
    a = T.operand(neg_head, ent[t if neg_head else h].astype(np.float64), rel[r].astype(np.float64), W.astype(np.float64))
    S, own = a @ ent.T, (h if neg_head else t)
    pos = S[np.arange(E), own]
    beats = S >= pos[:, None]                                    # raw: every entity counts, the row's own end too
    filt = None
    if filtered:                                                 # every row leaves out its own end and entities 0, 64 and 128
        lists = [np.unique([0, 64, 128, int(o)]) for o in own]   # (ascending, unique: the layout of eval's filters)
        for i, ids in enumerate(lists):
            beats[i, ids] = False
        ends = np.cumsum([len(x) for x in lists])
        filt = (np.stack([ends - [len(x) for x in lists], ends], 1).astype(np.int64), np.concatenate(lists).astype(np.int64))
    dev = lambda x: torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()
    rk = Ranker('TuckER', dev(ent), dev(rel), 12.0, 1.0, batch=16, proj=dev(W.reshape(-1, d_e)))
    ranks, p = rk.ranks(h, r, t, neg_head, filt=filt, want_pos_score=True)
    assert np.array_equal(p.cpu().numpy().astype(np.float64), pos)
    assert np.array_equal(ranks.cpu().numpy(), 1 + beats.sum(1))


def _engine():
    c = T.CASES[0]
    tables, batch, known = T.inputs(c)
    _, eng, b = run_step(c, tables, batch, known)
    return c, eng, b


CLOSED = ["kge_step_fused", "kge_step_fused_sampling", "kge_step_fused_known", "kge_step_phase", "kge_step_phase_known", "kge_step_optim:adagrad",
          "kge_step_async", "kge_step_grads", "kge_step_sharded", "kge_rank_eval_split", "kge_rank_eval_chunked", "kge_rank_rel_eval",
          "kge_topk_select", "kge_topk_select_filtered", "kge_score_pos", "kge_score_pos_bwd", "kge_score_neg_fwd", "kge_score_neg_bwd"]


@pytest.mark.parametrize("entry", CLOSED)
def test_closed_entries_name_the_model_and_the_entry(entry):
    """the sampled step (N > 0) in its entries, the other rankings, top-K and the per-op entries refuse TuckER in front of any launch: the
    NULL-pointer calls of model_contract_cases, and dummies (never dereferenced) where an entry looks at its pointers first"""
    import model_contract_cases as M
    c, eng, b = _engine()
    before = [x.clone() for x in (eng.ent, eng.ent_state, eng.rel, eng.rel_state, eng.proj, eng.proj_state)]
    h, m, de, dr, ONE, BIG = _lib.lib(), eng.hp.model, eng.hp.d_e, eng.hp.d_r, 1, 1 << 20
    pipe = C.c_void_p()
    assert h.kge_pipe_create(C.byref(pipe)) == 0
    calls = dict(M.null_calls(h, _lib, pipe, m, de, dr))
    topk = lambda f, *tail: f(m, 0, ONE, 5, ONE, 2, ONE, ONE, ONE, 1, de, dr, 0.0, 1.0, None, 5, ONE, 1, 1, 3, ONE, ONE, ONE, BIG, *tail)
    calls.update({
        "kge_topk_select": lambda: topk(h.kge_topk_select, None),
        "kge_topk_select_filtered": lambda: topk(h.kge_topk_select_filtered, None, None, None),
        "kge_score_pos": lambda: h.kge_score_pos(m, ONE, ONE, ONE, 2, de, dr, 1.0, 1.0, ONE, None),
        "kge_score_pos_bwd": lambda: h.kge_score_pos_bwd(m, ONE, ONE, ONE, ONE, 2, de, dr, 1.0, 1.0, ONE, ONE, ONE, None),
        "kge_score_neg_fwd": lambda: h.kge_score_neg_fwd(m, 0, ONE, ONE, ONE, 2, 8, 24, de, dr, 1.0, 1.0, ONE, ONE, BIG, 0, None),
        "kge_score_neg_bwd": lambda: h.kge_score_neg_bwd(m, 0, ONE, ONE, ONE, ONE, ONE, 2, 8, 24, de, dr, 1.0, 1.0, ONE, ONE, ONE, ONE, BIG, 0,
                                                         None)})
    try:
        rc = calls[entry]()
    finally:
        h.kge_pipe_destroy(pipe)
    text = h.kge_last_error().decode()
    torch.cuda.synchronize()
    # (kge_step_optim with Adagrad IS kge_step_fused_known, kge_step_phase_known without an index IS kge_step_phase, and they say so;
    #  the filtered top-K entry is kge_topk_select with a filter)
    named = {"kge_step_optim:adagrad": "kge_step_fused_known", "kge_step_phase_known": "kge_step_phase",
             "kge_topk_select_filtered": "kge_topk_select"}.get(entry, entry)
    assert rc == -1 and "TuckER" in text and named in text, text
    for t0, t1 in zip(before, (eng.ent, eng.ent_state, eng.rel, eng.rel_state, eng.proj, eng.proj_state)):
        assert torch.equal(t0, t1)


def _train_argv(tmp_path, *more):
    return ["--model_name", "TuckER", "--format", "udd_hrt", "--dataset", "toy", "--data_path", str(tmp_path / "kg"), "--data_files", "e.dict",
            "r.dict", "train.txt", "valid.txt", "test.txt", "--save_path", str(tmp_path / "ckpts"), "--gpu", "0", "--batch_size", "256",
            "--neg_sample_size", "64", "--hidden_dim", "32", "-g", "8", "--lr", "0.1", "--max_step", "100", "--log_interval", "50"] + list(more)


CLI_REFUSALS = {
    "no criterion": ("train", [], "--one_vs_all or --k_vs_all"),
    "train --eval_relation": ("train", ["--k_vs_all", "--eval_relation"], "relation ranking"),
    "train --neg_deg_sample_eval": ("train", ["--k_vs_all", "--neg_deg_sample_eval", "--no_eval_filter"], "--neg_deg_sample_eval"),
    "train -adv": ("train", ["--k_vs_all", "-adv"], "--k_vs_all cannot be combined with -adv"),
    "train width": ("train", ["--k_vs_all", "--hidden_dim", "30"], "multiple of 4"),
    "eval --eval_relation": ("eval", ["--eval_relation"], "relation ranking"),
    "eval --eval_candidates": ("eval", ["--eval_candidates", "none", "none"], "--eval_candidates"),
    "eval --neg_deg_sample_eval": ("eval", ["--neg_deg_sample_eval", "--no_eval_filter"], "--neg_deg_sample_eval"),
}


@pytest.mark.parametrize("what", sorted(CLI_REFUSALS))
def test_command_lines_refuse_before_anything_is_loaded(what, tmp_path):
    """(no data and no model directory exist: a check that came after loading would fail differently)"""
    from dglke_amd import eval_cli, train as TR
    cli, more, text = CLI_REFUSALS[what]
    with pytest.raises(_lib.KgeError, match=text) as e:
        if cli == "train":
            TR.main(_train_argv(tmp_path, *more))
        else:
            eval_cli.main(["--model_name", "TuckER", "--hidden_dim", "32", "--gpu", "0", "--model_path", str(tmp_path / "none")] + more)
    assert "TuckER" in str(e.value) or what in ("train -adv", "train width")      # (those two are the criterion's own refusals)


def test_cli_trains_tests_and_refuses_prediction(tmp_path, capsys):
    import glob
    import json
    from dglke_amd import predict_cli, train as TR
    from test_gpu_cli import _planted
    _planted(str(tmp_path / "kg"))
    TR.main(_train_argv(tmp_path, "--k_vs_all", "--label_smoothing", "0.1", "--test"))
    out = capsys.readouterr().out
    losses = [float(ln.rsplit(":", 1)[1]) for ln in out.splitlines() if "average loss" in ln]
    assert "[Train] TuckER: one core tensor of 32 x 32 x 32" in out and len(losses) == 2 and losses[1] < losses[0], out
    mrr = [float(ln.rsplit(":", 1)[1]) for ln in out.splitlines() if "MRR" in ln]
    assert mrr and all(np.isfinite(x) and 0 < x <= 1 for x in mrr), out
    run = glob.glob(str(tmp_path / "ckpts" / "*"))[0]
    conf = json.load(open(os.path.join(run, "config.json")))
    assert conf["model_name"] == "TuckER" and conf["k_vs_all"] is True and conf["loss_genre"] == "BCE"
    assert np.load(os.path.join(run, "toy_TuckERprojection.npy")).shape == (32 * 32, 32)
    with pytest.raises(_lib.KgeError, match="dglke_predict: TuckER"):
        predict_cli.main(["--model_path", run, "--format", "h_r_t", "--data_files", "a", "b", "c", "--gpu", "0"])


def test_the_open_steps_need_the_core_and_the_engine_needs_a_criterion():
    c, eng, b = _engine()
    tb = _lib.KgeTables()
    for f in ("ent", "ent_state", "rel", "rel_state", "n_ent", "n_rel"):
        setattr(tb, f, getattr(eng.tb, f))
    ws = eng.workspace_for(b)
    rc = _lib.lib().kge_step_fused(C.byref(eng.hp), C.byref(tb), C.byref(b.c), None, _lib.ptr(ws), eng._ws_bytes, _lib.stream_ptr())
    assert rc == -1 and "1-vs-all" in _lib.lib().kge_last_error().decode() and "core tensor" in _lib.lib().kge_last_error().decode()
    with pytest.raises(_lib.KgeError, match="TuckER.*one_vs_all=True or k_vs_all=True"):
        StepEngine('TuckER', c.n_ent, T.N_REL, 8, 12.0, T.LR, DEV)
    with pytest.raises(_lib.KgeError, match="TuckER.*relation width.*got 6"):
        StepEngine('TuckER', c.n_ent, T.N_REL, 8, 12.0, T.LR, DEV, loss_genre='Softmax', one_vs_all=True, relation_dim=6)
    with pytest.raises(_lib.KgeError, match="TuckER.*entity width.*got 10"):
        StepEngine('TuckER', c.n_ent, T.N_REL, 10, 12.0, T.LR, DEV, loss_genre='Softmax', one_vs_all=True, relation_dim=8)
