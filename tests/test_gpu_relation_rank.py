"""Relation ranking on the device (kge_rank_rel_eval through dglke_amd.eval) against the rank bounds of relation_rank_cases.py:
every model on every route it has (fp32-MFMA tiles / pairwise score block / the RotatE and TransR kernels), raw and filtered,
7 and 130 relations, a ragged second batch; the own relation never counting; positive scores; batching and workspace budget
invariance; the device filter builder; evaluate_relations and `dglke_eval --eval_relation`.  test_relation_rank_inputs.py guards
that the bounds pin almost every ranking."""
import os
import re

import numpy as np
import pytest
import torch

import relation_rank_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORCE_PAIRWISE = 1
SMALL = [(m, hd, de) for (m, hd, de) in RC.SHAPES[:8]]            # one small width per model
SMALL_IDS = [m for (m, _, _) in SMALL]


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _ranker(c, flags=0, batch=RC.EB, rel=None):
    from dglke_amd import eval as kev
    proj = _dev(c.proj) if c.proj is not None else None
    return kev.Ranker(c.model, _dev(c.ent), _dev(c.rel if rel is None else rel), c.gamma, c.emb_init, batch=batch, flags=flags, proj=proj)


def _lists(n_rel, filtered):
    rng, ids = RC.relation_lists(n_rel, filtered)
    return _dev(rng), _dev(ids)


def _check(got, lo, hi, what):
    print(what, "rank - lo:", np.bincount(np.clip(got - lo, 0, 3), minlength=4), "hi - lo max", int((hi - lo).max()))
    assert np.all((lo <= got) & (got <= hi)), (what, np.nonzero((got < lo) | (got > hi))[0][:8], lo[:8], got[:8], hi[:8])
    exact = lo == hi
    assert np.array_equal(got[exact], lo[exact]), what


@pytest.mark.parametrize("model,hidden,de,n_rel", RC.CASES, ids=RC.CASE_IDS)
def test_ranks_are_inside_the_bounds_and_positive_scores_match(model, hidden, de, n_rel):
    c = RC.inputs(model, hidden, de, n_rel)
    for flags in ((0, FORCE_PAIRWISE) if model in RC.TWO_ROUTES else (0,)):
        rk = _ranker(c, flags)
        for filtered in (False, True):
            got, pos = rk.relation_ranks(c.h, c.r, c.t, _lists(n_rel, filtered), want_pos_score=True)
            lo, hi, p = RC.expected(model, hidden, de, n_rel, filtered)
            err = np.abs(pos.cpu().numpy() - p).max()
            print("flags", flags, "filtered", filtered, "max |p err| %.2e" % err)
            _check(got.cpu().numpy().astype(np.int64), lo, hi, (flags, filtered))
            assert err <= RC.TOL


@pytest.mark.parametrize("model,hidden,de", SMALL, ids=SMALL_IDS)
def test_the_own_relation_never_counts(model, hidden, de):
    """Relation b's row is overwritten with a copy of relation a's (a = the test triples' most frequent relation).  For a triple
    with r = a, column b then scores what the own column a scores - the same kernel on the same bits - so the rank with b counting
    minus the rank with b listed is exactly whether the OWN-form score reaches the positive score in fp32: 0 or 1.  Where it is 1
    and the bounds pin the rank (lo == hi), a kernel that counted the own column would be one above lo; the raw rank must be lo.
    Triples whose list holds b (filtered) keep their rank bit for bit, and every rank stays inside the bounds of the changed
    table."""
    n_rel = 7
    c = RC.inputs(model, hidden, de, n_rel)
    a = int(np.bincount(c.r, minlength=n_rel).argmax())
    b = (a + 1) % n_rel
    rel2 = np.array(c.rel)
    rel2[b] = rel2[a]
    S2 = RC.score_matrix(c, np.float64, rel2)
    p2 = S2[np.arange(RC.E), c.r]
    mine = c.r == a
    for flags in ((0, FORCE_PAIRWISE) if model in RC.TWO_ROUTES else (0,)):
        rk = _ranker(c, flags, rel=rel2)
        for filtered in (False, True):
            frng, fids = RC.relation_lists(n_rel, filtered)
            got = rk.relation_ranks(c.h, c.r, c.t, (_dev(frng), _dev(fids))).cpu().numpy().astype(np.int64)
            lo, hi = RC.bounds(c, S2, p2, filtered)
            _check(got, lo, hi, ("duplicate", flags, filtered))
            # the same lists with b added to the lists of the triples whose relation is a
            lists = [np.union1d(fids[frng[i, 0]:frng[i, 1]], [b] if mine[i] else []).astype(np.int64) for i in range(RC.E)]
            ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
            without = rk.relation_ranks(c.h, c.r, c.t, (_dev(np.stack([ptr[:-1], ptr[1:]], 1)), _dev(np.concatenate(lists)))
                                        ).cpu().numpy().astype(np.int64)
            gain = got - without
            listed = np.array([b in fids[frng[i, 0]:frng[i, 1]] for i in range(RC.E)])
            assert np.all((gain[mine] == 0) | (gain[mine] == 1)) and np.all(gain[~mine] == 0)
            assert np.all(gain[mine & listed] == 0)
            # column b aside, the changed table ranks like the original one: the original bounds, b left out, pin `without`
            p, S = RC.oracle_scores(model, hidden, de, n_rel)
            keep = np.ones(n_rel, bool)
            keep[b] = False
            for i in np.nonzero(mine & ~listed)[0]:
                cnt = keep.copy()
                cnt[fids[frng[i, 0]:frng[i, 1]]] = False
                lo_i = 1 + int((cnt & (S[i] >= p[i] + RC.TOL)).sum())
                hi_i = 1 + int((cnt & (S[i] >= p[i] - RC.TOL)).sum())
                assert lo_i <= without[i] <= hi_i
                if lo_i == hi_i:                           # own column (a) not counted, whatever `gain` says about its rounding
                    assert without[i] == lo_i, (flags, filtered, i, int(gain[i]))
            print("flags", flags, "filtered", filtered, "triples of relation", a, ":", int(mine.sum()), "own-form score >= p for",
                  int(gain[mine].sum()))


@pytest.mark.parametrize("model,hidden,de", SMALL + [("RESCAL", 12, None), ("DistMult", 30, None)],
                         ids=SMALL_IDS + ["RESCAL_h12", "DistMult_h30"])
def test_ranks_do_not_depend_on_the_batch_or_the_budget(model, hidden, de):
    """exact by construction (every (triple, relation) pair goes through the same operations whatever its batch)"""
    from dglke_amd import _lib
    n_rel = 130
    c = RC.inputs(model, hidden, de, n_rel)
    filt = _lists(n_rel, True)
    base_rk = _ranker(c, batch=RC.EB)
    base = base_rk.relation_ranks(c.h, c.r, c.t, filt).cpu().numpy()
    for eb in (1, RC.E):
        assert np.array_equal(_ranker(c, batch=eb).relation_ranks(c.h, c.r, c.t, filt).cpu().numpy(), base), eb
    small = _ranker(c, batch=RC.EB)
    small.rel_ws_budget = 1                                # never below one row
    assert np.array_equal(small.relation_ranks(c.h, c.r, c.t, filt).cpu().numpy(), base)
    assert small._rws.numel() == _lib.lib().kge_rank_rel_workspace_bytes(_lib.model_id(model), 1, n_rel, c.d_e, c.d_r)
    assert small._rws.numel() < base_rk._rws.numel()
    empty = base_rk.relation_ranks(c.h[:0], c.r[:0], c.t[:0], filt)
    assert tuple(empty.shape) == (0,)


def test_filter_builder_and_evaluate_relations():
    from dglke_amd import eval as kev
    model, hidden, n_rel = "ComplEx", 16, 130
    c = RC.inputs(model, hidden, None, n_rel)
    rk = _ranker(c, batch=1024)
    te, tr = _dev(c.ent), _dev(c.rel)
    for filtered in (False, True):
        known = tuple(np.array(x[RC.E:]) for x in (c.kh, c.kr, c.kt)) if filtered else None     # the test triples are appended
        rng, ids = kev.build_relation_filter(known, tuple(np.array(x) for x in (c.h, c.r, c.t)), RC.N_ENT, n_rel, torch.device(DEV))
        assert rng.is_cuda and ids.is_cuda
        wrng, wids = RC.relation_lists(n_rel, filtered)
        rng_h, ids_h = rng.cpu().numpy(), ids.cpu().numpy()
        for i in range(RC.E):
            assert np.array_equal(ids_h[rng_h[i, 0]:rng_h[i, 1]], wids[wrng[i, 0]:wrng[i, 1]]), (filtered, i)
        ranks = rk.relation_ranks(c.h, c.r, c.t, _lists(n_rel, filtered))
        got = kev.evaluate_relations(model, te, tr, c.gamma, c.emb_init, tuple(np.array(x) for x in (c.h, c.r, c.t)), known)
        assert got == kev.metrics_from_ranks(ranks)
        assert set(got) == {"MRR", "MR", "HITS@1", "HITS@3", "HITS@10"}


def test_dglke_eval_prints_the_relation_metrics(tmp_path, capsys):
    """`dglke_eval --eval_relation` prints evaluate_relations' five metrics as REL_* lines after the entity metrics (filtered,
    and raw with --no_eval_filter); without the flag stdout has no REL_ line"""
    from dglke_amd import eval as kev
    from dglke_amd import eval_cli
    model, hidden, n_rel = "DistMult", 32, 7
    c = RC.inputs(model, hidden, None, n_rel)
    data, save = str(tmp_path / "kg"), str(tmp_path / "model")
    os.makedirs(data)
    os.makedirs(save)
    with open(os.path.join(data, "e.dict"), "w") as f:
        f.writelines("%d\te%d\n" % (i, i) for i in range(RC.N_ENT))
    with open(os.path.join(data, "r.dict"), "w") as f:
        f.writelines("%d\tr%d\n" % (i, i) for i in range(n_rel))
    trip = np.stack([c.kh, c.kr, c.kt], 1)
    np.savetxt(os.path.join(data, "train.txt"), trip[RC.E:], fmt="%d", delimiter="\t")
    np.savetxt(os.path.join(data, "test.txt"), trip[:RC.E], fmt="%d", delimiter="\t")
    np.savetxt(os.path.join(data, "valid.txt"), trip[RC.E:RC.E + 10], fmt="%d", delimiter="\t")
    np.save(os.path.join(save, "toy_DistMult_entity.npy"), c.ent)
    np.save(os.path.join(save, "toy_DistMult_relation.npy"), c.rel)
    base = ["--model_name", model, "--format", "udd_hrt", "--dataset", "toy", "--data_path", data, "--data_files", "e.dict",
            "r.dict", "train.txt", "valid.txt", "test.txt", "--model_path", save, "--hidden_dim", str(hidden), "-g", "8", "--gpu", "0"]
    te, tr = _dev(c.ent), _dev(c.rel)
    test = tuple(np.array(x) for x in (c.h, c.r, c.t))
    known = tuple(np.array(x) for x in (c.kh, c.kr, c.kt))
    capsys.readouterr()
    for extra, kn in (([], known), (["--no_eval_filter"], None)):
        eval_cli.main(base + ["--eval_relation"] + extra)
        out = capsys.readouterr().out
        want = kev.evaluate_relations(model, te, tr, c.gamma, c.emb_init, test, kn)
        lines = [l for l in out.split("\n") if re.match(r"^\[0\]Test average ", l)]
        assert len(lines) == 10 and not any("REL_" in l for l in lines[:5]), out
        assert lines[5:] == ['[0]Test average REL_{}: {}'.format(k, want[k]) for k in ("MRR", "MR", "HITS@1", "HITS@3", "HITS@10")], out
    plain = eval_cli.main(base)
    out = capsys.readouterr().out
    assert "REL_" not in out and len([l for l in out.split("\n") if re.match(r"^\[0\]Test average ", l)]) == 5
    assert not any(k.startswith("REL_") for k in plain)
