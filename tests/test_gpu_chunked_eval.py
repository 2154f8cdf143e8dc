"""Chunked-candidate ranking on the device (kge_rank_eval_chunked through dglke_amd.eval) against the oracle's rank bounds of
chunked_eval_cases.py: every model on both routes (fp32-MFMA tiles / score block), both sides, raw and filtered, ragged chunks,
per-triple lists, empty slots, repeats, the chunk's own entities prepended with the zeroed own column; grouping invariance;
evaluate_candidates and the two command lines.  test_chunked_eval_inputs.py guards that the bounds pin almost every ranking."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import chunked_eval_cases as CC
from oracle import kge_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FORCE_PAIRWISE = 1


def _ranker(model, hidden, flags=0):
    from dglke_amd import eval as kev
    c = CC.inputs(model, hidden)
    proj = torch.from_numpy(c.proj).to(DEV) if c.proj is not None else None
    return kev.Ranker(model, torch.from_numpy(c.ent).to(DEV), torch.from_numpy(c.rel).to(DEV), c.gamma, c.emb_init, flags=flags, proj=proj)


def _check(got, lo, hi, free, what):
    assert np.all((lo <= got) & (got <= hi)), (what, np.nonzero((got < lo) | (got > hi))[0][:8], lo[:8], got[:8], hi[:8])
    exact = (lo == hi) & (free == 0)
    assert np.array_equal(got[exact], lo[exact]), what


@pytest.mark.parametrize("flags", [0, FORCE_PAIRWISE])
@pytest.mark.parametrize("model,hidden", CC.CASES, ids=CC.CASE_IDS)
def test_ranks_are_inside_the_oracle_bounds(model, hidden, flags):
    c = CC.inputs(model, hidden)
    rk = _ranker(model, hidden, flags)
    for chunk, n_cand in CC.CONFIGS:
        cand = CC.candidates(chunk, n_cand)
        for neg_head in (False, True):
            for filtered in (False, True):
                filt = CC.filter_lists(model, hidden, neg_head) if filtered else None
                got, pos = rk.chunked_ranks(c.h, c.r, c.t, neg_head, chunk, cand=cand, filt=filt, want_pos_score=True)
                lo, hi, free, p = CC.expected(model, hidden, neg_head, chunk, cand, filtered=filtered)
                _check(got.cpu().numpy(), lo, hi, free, (chunk, n_cand, neg_head, filtered))
                assert np.abs(pos.cpu().numpy() - p).max() <= 1e-4
    # one list shared by all chunks ([n], stride 0) is the same as that list repeated per chunk
    shared = CC.candidates(24, 40)[1]
    a = rk.chunked_ranks(c.h, c.r, c.t, False, 24, cand=shared).cpu().numpy()
    b = rk.chunked_ranks(c.h, c.r, c.t, False, 24, cand=np.tile(shared, (4, 1))).cpu().numpy()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("flags", [0, FORCE_PAIRWISE])
@pytest.mark.parametrize("model,hidden", CC.CASES, ids=CC.CASE_IDS)
def test_own_entities_are_prepended_and_the_own_column_scores_zero(model, hidden, flags):
    """self_cand, raw.  The oracle replaces the own column's score by 0.0.  Over the pinned rankings (lo == hi) of each side the
    ranks differ from those of an own column that always counts for some positive p, and from one that never counts for some
    negative p: the zero is really applied.  (Against all entities every list holds a free column, so the pinned rankings come
    from the sampled configuration: the two are taken together, as in the CPU guard.)"""
    c = CC.inputs(model, hidden)
    rk = _ranker(model, hidden, flags)
    for neg_head in (False, True):
        seen_pos = seen_neg = 0
        for chunk, n_cand in CC.SELF_CONFIGS:
            cand = CC.candidates(chunk, n_cand)
            got = rk.chunked_ranks(c.h, c.r, c.t, neg_head, chunk, cand=cand, self_cand=True).cpu().numpy()
            lo, hi, free, p = CC.expected(model, hidden, neg_head, chunk, cand, self_cand=True)
            assert np.all((lo <= got) & (got <= hi)), (chunk, n_cand, neg_head, np.nonzero((got < lo) | (got > hi))[0][:8])
            exact = lo == hi
            assert np.array_equal(got[exact], lo[exact])
            always = CC.expected(model, hidden, neg_head, chunk, cand, self_cand=True, own="always")[0]
            never = CC.expected(model, hidden, neg_head, chunk, cand, self_cand=True, own="never")[0]
            seen_pos += int((got[exact & (p > 0)] != always[exact & (p > 0)]).sum())
            seen_neg += int((got[exact & (p < 0)] != never[exact & (p < 0)]).sum())
        assert seen_pos > 0 and seen_neg > 0, (neg_head, seen_pos, seen_neg)
    from dglke_amd import _lib
    with pytest.raises(_lib.KgeError):                     # the reference asserts that the two exclude each other
        rk.chunked_ranks(c.h, c.r, c.t, False, 24, filt=CC.filter_lists(model, hidden, False), self_cand=True)


@pytest.mark.parametrize("model,hidden", [("TransE_l2", 32), ("RotatE", 16)])
def test_a_chunk_spanning_several_row_tiles(model, hidden):
    """E = 300 in chunks of 150 against 200 candidates each: three 64-row tiles per chunk, the last one partial"""
    c = CC.inputs(model, hidden)
    n = 300
    h, r, t = c.kh[:n].copy(), c.kr[:n].copy(), c.kt[:n].copy()
    cand = CC.candidates(150, 200, n)
    rk = _ranker(model, hidden)
    for neg_head in (False, True):
        _, p, S = O.rank_eval(model, c.ent64, c.rel64, h, r, t, neg_head, c.gamma, c.emb_init)
        got = rk.chunked_ranks(h, r, t, neg_head, 150, cand=cand).cpu().numpy()
        for i in range(n):
            ids = cand[i // 150]
            s = S[i, ids[ids >= 0]]
            lo, hi = 1 + int((s >= p[i] + CC.TOL).sum()), 1 + int((s >= p[i] - CC.TOL).sum())
            assert lo <= got[i] <= hi, (neg_head, i, lo, got[i], hi)


@pytest.mark.parametrize("model,hidden", [("DistMult", 400), ("TransE_l1", 32)])
def test_ranks_do_not_depend_on_how_the_rows_are_grouped(model, hidden):
    """exact by construction (k runs in table order, every pair goes through the same operations whatever its chunk, tile or
    block): one call = one call per chunk = a call whose workspace holds one chunk at a time"""
    c = CC.inputs(model, hidden)
    chunk, cand = 24, CC.candidates(24, 40)
    for neg_head in (False, True):
        frng, fids = CC.filter_lists(model, hidden, neg_head)
        rk = _ranker(model, hidden)
        one = rk.chunked_ranks(c.h, c.r, c.t, neg_head, chunk, cand=cand, filt=(frng, fids)).cpu().numpy()
        parts = []
        for k, e0 in enumerate(range(0, CC.E, chunk)):
            e1 = min(CC.E, e0 + chunk)
            parts.append(rk.chunked_ranks(c.h[e0:e1], c.r[e0:e1], c.t[e0:e1], neg_head, e1 - e0, cand=cand[k],
                                          filt=(frng[e0:e1], fids)).cpu().numpy())
        assert np.array_equal(one, np.concatenate(parts))
        small = _ranker(model, hidden)
        small.chunk_ws_budget = 1                       # never less than one chunk: four blocks of one chunk
        blocks = small.chunked_ranks(c.h, c.r, c.t, neg_head, chunk, cand=cand, filt=(frng, fids)).cpu().numpy()
        from dglke_amd import _lib
        assert small._cws.numel() == _lib.lib().kge_rank_chunked_workspace_bytes(_lib.model_id(model), chunk, chunk, 40, 0,
                                                                                 c.ent.shape[1], c.rel.shape[1])
        assert small._cws.numel() < rk._cws.numel()
        assert np.array_equal(one, blocks)


def test_evaluate_candidates_gives_the_metrics_of_the_per_triple_ranks():
    from dglke_amd import _lib
    from dglke_amd import eval as kev
    model, hidden = "ComplEx", 16
    c = CC.inputs(model, hidden)
    cand = CC.candidates(1, 130)
    rk = _ranker(model, hidden)
    te, tr = torch.from_numpy(c.ent).to(DEV), torch.from_numpy(c.rel).to(DEV)
    known = (c.kh, c.kr, c.kt)
    for kn in (None, known):
        ranks = {}
        for neg_head in (True, False):
            filt = CC.filter_lists(model, hidden, neg_head) if kn is not None else None
            ranks[neg_head] = rk.chunked_ranks(c.h, c.r, c.t, neg_head, 1, cand=cand, filt=filt)
        both = kev.evaluate_candidates(model, te, tr, c.gamma, c.emb_init, (c.h, c.r, c.t), cand_head=cand, cand_tail=cand, known=kn)
        assert both == kev.metrics_from_ranks(torch.cat([ranks[True], ranks[False]]))
        tail = kev.evaluate_candidates(model, te, tr, c.gamma, c.emb_init, (c.h, c.r, c.t), cand_tail=cand, known=kn)
        assert tail == kev.metrics_from_ranks(ranks[False])
    with pytest.raises(_lib.KgeError):                     # an id outside the table is an argument error
        bad = np.array(cand)
        bad[5, 7] = CC.N_ENT
        kev.evaluate_candidates(model, te, tr, c.gamma, c.emb_init, (c.h, c.r, c.t), cand_tail=bad)
    with pytest.raises(_lib.KgeError):                     # one row per test triple
        kev.evaluate_candidates(model, te, tr, c.gamma, c.emb_init, (c.h, c.r, c.t), cand_head=cand[:50])


def _planted(path, n_ent=400, n_rel=6, n=9000, seed=3):
    from planted_kg import make_planted
    train, test = make_planted(n_ent, n_rel, n, dim=8, seed=seed)
    valid, test = test[:len(test) // 2], test[len(test) // 2:]
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "e.dict"), "w") as f:
        f.writelines("%d\te%d\n" % (i, i) for i in range(n_ent))
    with open(os.path.join(path, "r.dict"), "w") as f:
        f.writelines("%d\tr%d\n" % (i, i) for i in range(n_rel))
    for name, t in (("train.txt", train), ("valid.txt", valid), ("test.txt", test)):
        np.savetxt(os.path.join(path, name), t, fmt="%d", delimiter="\t")
    return train, valid, test


def _run(cmd, timeout=300):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    return out


def _metric_lines(out, tag):
    return [l for l in out.split("\n") if re.match(r"^\[0\]%s average " % tag, l)]


def test_dglke_eval_degree_sampling_and_candidate_files(tmp_path):
    """`dglke_eval --neg_deg_sample_eval` prints evaluate(neg_deg_sample=True)'s metric lines and `--eval_candidates` those of
    evaluate_candidates, as strings"""
    from dglke_amd import eval as kev
    data = str(tmp_path / "kg")
    train, valid, test = _planted(data, n_ent=401)
    rng = np.random.RandomState(2)
    save = str(tmp_path / "model")
    os.makedirs(save)
    ent = ((rng.rand(401, 32) - 0.5) * 0.6).astype(np.float32)
    rel = ((rng.rand(6, 32) - 0.5) * 0.6).astype(np.float32)
    np.save(os.path.join(save, "toy_DistMult_entity.npy"), ent)
    np.save(os.path.join(save, "toy_DistMult_relation.npy"), rel)
    base = [sys.executable, os.path.join(ROOT, "dgl-ke_amd", "dglke_eval"), "--model_name", "DistMult", "--format", "udd_hrt",
            "--dataset", "toy", "--data_path", data, "--data_files", "e.dict", "r.dict", "train.txt", "valid.txt", "test.txt",
            "--model_path", save, "--hidden_dim", "32", "-g", "8", "--gpu", "0"]
    te, tr = torch.from_numpy(ent).to(DEV), torch.from_numpy(rel).to(DEV)
    trip = (test[:, 0], test[:, 1], test[:, 2])
    fmt = lambda m: ['[0]Test average {}: {}'.format(k, v) for k, v in m.items()]

    out = _run(base + ["--no_eval_filter", "--neg_deg_sample_eval", "--neg_sample_size_eval", "40", "--batch_size_eval", "24"])
    want = kev.evaluate("DistMult", te, tr, 8.0, 10.0 / 32, trip, None, n_cand=40, chunk=24, neg_deg_sample=True, seed=0 + 29)
    got = _metric_lines(out, "Test")
    assert len(got) == 5 and got == fmt(want), (got, want)
    uniform = kev.evaluate("DistMult", te, tr, 8.0, 10.0 / 32, trip, None, n_cand=40, chunk=24, seed=0 + 29)
    assert uniform != want                                # the flag is not a no-op

    ch, ct = rng.randint(0, 401, (len(test), 50)), rng.randint(0, 401, (len(test), 50))
    ct[::7, -4:] = -1                                      # ragged rows
    np.save(str(tmp_path / "cand_head.npy"), ch)
    np.save(str(tmp_path / "cand_tail.npy"), ct)
    known = tuple(np.concatenate([train[:, k], valid[:, k], test[:, k]]) for k in range(3))
    out = _run(base + ["--eval_candidates", str(tmp_path / "cand_head.npy"), str(tmp_path / "cand_tail.npy")])
    want = kev.evaluate_candidates("DistMult", te, tr, 8.0, 10.0 / 32, trip, ch, ct, known)
    got = _metric_lines(out, "Test")
    assert len(got) == 5 and got == fmt(want), (got, want)
