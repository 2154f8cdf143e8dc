"""Exact-tie semantics of every fused ranking path, on the integer-grid tables of rank_tie_cases.py: fp32 is exact there, so every
device rank must EQUAL the fp64 rank 1 + #{candidates that count : s >= p} - `np.array_equal`, no band - and candidates that score
exactly the positive score are everywhere (test_rank_tie_inputs.py proves both on the CPU: a `>` in the place of `>=` changes at
least half of the ranks of every case).

Entry points: Ranker.ranks (kge_rank_eval_ex: mask GEMM / score block + rank_count_kernel), SplitRanker.ranks (kge_rank_eval_split,
shards of 128, 1, 128 and 0 rows), Ranker.chunked_ranks (kge_rank_eval_chunked, --neg_deg_sample_eval included),
Ranker.relation_ranks (kge_rank_rel_eval) and kge_topk_select against the ranks.  Every test prints how many rankings it compared."""
import numpy as np
import pytest
import torch

import rank_tie_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORCE_PAIRWISE = 1
K = 128
TOPK_CASES = [c for c in T.CASES if c[0] == "grid" and c[1] != "TransR"]      # TransR has no inference path


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _tables(c):
    return _dev(c.ent), _dev(c.rel), (_dev(c.proj) if c.proj is not None else None)


def _same(got, want, case, entry, p, tied_of):
    """exact equality of integer ranks; on a mismatch: the case, the entry point, the first triple that differs, its positive score
    and the candidate columns that tie with it"""
    got = np.asarray(got).astype(np.int64)
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        print("MISMATCH %s | %s | %d of %d triples differ | first: triple %d got %d want %d | positive score %r | tied columns %s"
              % ("-".join(map(str, case)), entry, len(bad), len(want), i, got[i], want[i], float(p[i]), tied_of(i).tolist()))
    assert np.array_equal(got, want), (case, entry, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    return len(want)


def _pos_same(pos, c, p, case, entry):
    pos = pos.cpu().numpy()
    want = T.pos32(c, p)
    assert pos.dtype == np.float32 and np.array_equal(pos, want), (case, entry, np.nonzero(pos != want)[0][:8].tolist())


@pytest.mark.parametrize("kind,model,d_e", T.CASES, ids=T.CASE_IDS)
def test_full_table_and_list_ranks_equal_the_fp64_ranks(kind, model, d_e):
    """Ranker.ranks: flags 0 (the mask GEMM where it is supported, else a score block + rank_count_kernel) and 1 (the pairwise
    score block), both sides, raw and filtered, all entities and lists of 70 and 257 with repeats; one batch of 130 (row blocks of
    128 + 2) and batches of 48 + 48 + 34"""
    from dglke_amd import eval as kev
    case = (kind, model, d_e)
    c = T.inputs(*case)
    ent, rel, proj = _tables(c)
    n = 0
    for flags in (0, FORCE_PAIRWISE):
        for batch in (T.E, 48):
            rk = kev.Ranker(model, ent, rel, c.gamma, c.emb_init, batch=batch, flags=flags, proj=proj)
            for neg_head in (False, True):
                p, S = T.oracle_scores(*case, neg_head)
                filt = T.filter_lists(*case, neg_head)
                for cand in (None,) + tuple(T.cand_list(m) for m in T.LIST_LENS):
                    for f in (None, filt):
                        cols = f if f is None or cand is None else kev.filter_columns(cand, f, 0, T.E)
                        got, pos = rk.ranks(c.h, c.r, c.t, neg_head, cols, cand=cand, want_pos_score=True)
                        entry = "Ranker.ranks flags=%d batch=%d %s %s %s" % (
                            flags, batch, "head" if neg_head else "tail", "all" if cand is None else "list%d" % len(cand),
                            "filtered" if f else "raw")
                        n += _same(got.cpu().numpy(), T.ranks_of(c, p, S, neg_head, cand, f), case, entry, p,
                                   lambda i: T.tied_columns(p, S, i, cand))
                        _pos_same(pos, c, p, case, entry)
    print("Ranker.ranks %s: %d rankings compared" % ("-".join(map(str, case)), n))


@pytest.mark.parametrize("kind,model,d_e", T.CASES, ids=T.CASE_IDS)
def test_shard_counts_add_up_to_the_fp64_ranks(kind, model, d_e):
    """SplitRanker.ranks on the rows [0, 128), [128, 129), [129, 257) and an empty shard: 1 + sum_k (ranks_k - 1) is the whole-table
    rank, ties included"""
    from dglke_amd import eval as kev
    case = (kind, model, d_e)
    c = T.inputs(*case)
    ent, rel, proj = _tables(c)
    ids, inv = np.unique(np.concatenate([c.h, c.t]), return_inverse=True)
    qent = ent[_dev(ids)].contiguous()
    qh, qt = inv[:T.E].copy(), inv[T.E:].copy()
    known = (c.kh, c.kr, c.kt)
    n = 0
    for flags in (0, FORCE_PAIRWISE):
        for neg_head in (False, True):
            p, S = T.oracle_scores(*case, neg_head)
            for cand in (None, T.cand_list(T.LIST_LENS[-1])):
                for filtered in (False, True):
                    total = np.zeros(T.E, np.int64)
                    for lo, hi in zip(T.SHARD_CUTS[:-1], T.SHARD_CUTS[1:]):
                        rk = kev.SplitRanker(model, ent[lo:hi].contiguous(), rel, c.gamma, c.emb_init, batch=48, flags=flags, proj=proj)
                        f = local = None
                        if filtered:
                            f = kev.build_filter(*kev.shard_known(known, neg_head, lo, hi), c.h, c.r, c.t, neg_head, T.N_REL)
                        if cand is not None:
                            _, local = kev.owned_candidates(cand, lo, hi)
                            if f is not None:
                                f = kev.filter_columns(local, f, 0, T.E)
                        total += rk.ranks(qent, qh, c.r, qt, neg_head, f, cand=local).cpu().numpy().astype(np.int64) - 1
                    entry = "SplitRanker.ranks flags=%d %s %s %s" % (flags, "head" if neg_head else "tail",
                                                                     "all" if cand is None else "list%d" % len(cand),
                                                                     "filtered" if filtered else "raw")
                    want = T.ranks_of(c, p, S, neg_head, cand, T.filter_lists(*case, neg_head) if filtered else None)
                    n += _same(total + 1, want, case, entry, p, lambda i: T.tied_columns(p, S, i, cand))
    print("SplitRanker.ranks %s: %d rankings compared" % ("-".join(map(str, case)), n))


@pytest.mark.parametrize("kind,model,d_e", T.CASES, ids=T.CASE_IDS)
def test_chunked_ranks_equal_the_fp64_ranks(kind, model, d_e):
    """Ranker.chunked_ranks in chunks of 16 (the last one holds 2 triples): all entities and per-chunk lists with pads and repeats,
    raw and filtered by entity id; self_cand (raw), where the triple's own column scores exactly 0.0f and ties with the positive
    scores that are exactly 0 (the grid cases hold several)"""
    from dglke_amd import eval as kev
    case = (kind, model, d_e)
    c = T.inputs(*case)
    ent, rel, proj = _tables(c)
    n = 0
    for flags in (0, FORCE_PAIRWISE):
        rk = kev.Ranker(model, ent, rel, c.gamma, c.emb_init, flags=flags, proj=proj)
        for neg_head in (False, True):
            p, S = T.oracle_scores(*case, neg_head)
            filt = T.filter_lists(*case, neg_head)
            for cand in (None, T.chunk_lists()):
                for f, self_cand in ((None, False), (filt, False), (None, True)):
                    got, pos = rk.chunked_ranks(c.h, c.r, c.t, neg_head, T.CHUNK, cand=cand, filt=f, self_cand=self_cand,
                                                want_pos_score=True)
                    entry = "Ranker.chunked_ranks flags=%d %s %s %s" % (
                        flags, "head" if neg_head else "tail", "all" if cand is None else "lists",
                        "self_cand" if self_cand else "filtered" if f else "raw")
                    want = T.ranks_of(c, p, S, neg_head, cand, f, T.CHUNK, self_cand=self_cand)
                    n += _same(got.cpu().numpy(), want, case, entry, p,
                               lambda i: T.tied_columns(p, S, i, None if cand is None else cand[i // T.CHUNK]))
                    _pos_same(pos, c, p, case, entry)
    print("Ranker.chunked_ranks %s: %d rankings compared" % ("-".join(map(str, case)), n))


@pytest.mark.parametrize("kind,model,d_e,n_rel", T.REL_CASES, ids=T.REL_CASE_IDS)
def test_relation_ranks_equal_the_fp64_ranks(kind, model, d_e, n_rel):
    """Ranker.relation_ranks, raw and filtered, both routes: relations that score exactly the true relation's score count, the own
    relation never does (a collapsed relation table: rank = 1 + n_rel - |list_i|)"""
    from dglke_amd import eval as kev
    case = (kind, model, d_e, n_rel)
    c = T.rel_inputs(*case)
    ent, rel, proj = _tables(c)
    p, S = T.rel_oracle_scores(*case)
    n = 0
    for flags in (0, FORCE_PAIRWISE):
        for batch in (T.E, 48):
            rk = kev.Ranker(model, ent, rel, c.gamma, c.emb_init, batch=batch, flags=flags, proj=proj)
            for filtered in (False, True):
                lists = T.relation_lists(*case, filtered)
                got, pos = rk.relation_ranks(c.h, c.r, c.t, (_dev(lists[0]), _dev(lists[1])), want_pos_score=True)
                entry = "Ranker.relation_ranks flags=%d batch=%d %s" % (flags, batch, "filtered" if filtered else "raw")
                n += _same(got.cpu().numpy(), T.rel_ranks_of(p, S, lists), case, entry, p, lambda i: T.tied_columns(p, S, i))
                _pos_same(pos, c, p, case, entry)
    print("Ranker.relation_ranks %s: %d rankings compared" % ("-".join(map(str, case)), n))


def _topk(c, side, ent, rel, cand):
    from dglke_amd import _lib
    L = _lib.lib()
    h, r, t, cd = _dev(c.h), _dev(c.r), _dev(c.t), _dev(cand)
    res_s = torch.zeros(T.E, K, dtype=torch.float32, device=DEV)
    res_o = torch.full((T.E, K), -1, dtype=torch.int64, device=DEV)
    base = torch.zeros(T.E, dtype=torch.int64, device=DEV)
    ws = torch.empty(L.kge_topk_workspace_bytes(T.E, len(cand), c.d_e, K), dtype=torch.uint8, device=DEV)
    _lib.check(L.kge_topk_select(_lib.MODEL_IDS[c.model], side, _lib.ptr(ent), T.N_ENT, _lib.ptr(rel), T.N_REL, _lib.ptr(h),
                                 _lib.ptr(r), _lib.ptr(t), T.E, c.d_e, c.d_r, c.gamma, c.emb_init, _lib.ptr(cd), len(cand),
                                 _lib.ptr(base), 1, 1, K, _lib.ptr(res_s), _lib.ptr(res_o), _lib.ptr(ws), ws.numel(),
                                 _lib.stream_ptr()))
    return res_s.cpu().numpy(), res_o.cpu().numpy()


@pytest.mark.parametrize("kind,model,d_e", TOPK_CASES, ids=["%s-%s-%d" % c for c in TOPK_CASES])
def test_topk_scores_orders_and_counts_agree_with_the_ranks(kind, model, d_e):
    """kge_topk_select with K = 128 over lists of 70 and 128 candidates (repeats) returns EVERY candidate: the scores equal the fp64
    ones, ties come back in candidate order, and the number of returned scores >= the positive score is the raw rank - 1 of
    Ranker.ranks over the same list (which counts the own column whenever the list holds it).  SimplE: the selection scores are
    unclamped (the reference's infer form), the ranking's are clamped - compared after the clamp.  RESCAL: heads only - the
    ranking's tail side is the reference's (M h) . t', the selection's h . (M t')."""
    from dglke_amd import eval as kev
    case = (kind, model, d_e)
    c = T.inputs(*case)
    ent, rel, proj = _tables(c)
    rk = kev.Ranker(model, ent, rel, c.gamma, c.emb_init, batch=T.E)
    n = 0
    for side in ((1,) if model == "RESCAL" else (0, 1)):
        p, S = T.oracle_scores(*case, bool(side))
        for m in (70, K):
            cand = T.cand_list(257)[:m]
            top_s, top_o = _topk(c, side, ent, rel, cand)
            assert np.all(top_o[:, :m] >= 0) and np.all(top_o[:, m:] == -1)
            Sc = S[:, cand]
            if model == "SimplE":       # undo the clamp: the raw half-integer score
                a64 = T.O.pos_side(model, bool(side), c.ent[c.h if not side else c.t].astype(np.float64), c.rel[c.r].astype(np.float64))
                Sc = 0.5 * a64 @ c.ent[cand].astype(np.float64).T
            if model == "TransE_l2":    # the fp32 value of gamma - sqrt(d^2) on the exact integer d^2 (rank_tie_cases.pos32)
                Sc = (np.float32(c.gamma) - np.sqrt(np.rint((c.gamma - Sc) ** 2).astype(np.float32))).astype(np.float64)
            order = np.argsort(-Sc, axis=1, kind="stable")              # descending score, ties by position
            entry = "kge_topk_select side=%d list%d" % (side, m)
            assert np.array_equal(top_o[:, :m], order), (case, entry, np.nonzero((top_o[:, :m] != order).any(1))[0][:8].tolist())
            assert np.array_equal(top_s[:, :m].astype(np.float64), np.take_along_axis(Sc, order, 1)), (case, entry)
            rank, pos = rk.ranks(c.h, c.r, c.t, bool(side), None, cand=cand, want_pos_score=True)
            pos = pos.cpu().numpy()
            shown = np.clip(top_s[:, :m], -T.O.SIMPLE_CLAMP, T.O.SIMPLE_CLAMP) if model == "SimplE" else top_s[:, :m]
            n += _same((shown >= pos[:, None]).sum(1) + 1, rank.cpu().numpy().astype(np.int64), case, entry, p,
                       lambda i: T.tied_columns(p, S, i, cand))
            _pos_same(torch.from_numpy(pos), c, p, case, entry)
    print("kge_topk_select %s: %d rankings compared" % ("-".join(map(str, case)), n))
