"""Ranking evaluation on the device (libkge_hip `kge_rank_eval`): the filtered MRR / MR / HITS@k
protocol of the reference's `test()` loop (train_pytorch.py:199-253) - every test triple against
ALL entities as corrupted heads and as corrupted tails (EvalSampler, dataloader/sampler.py:514-597,
`--neg_sample_size_eval -1`), triples that exist in the graph masked out when `eval_filter`
(general_models.py:463-475) - without the per-triple Python loop of `forward_test`.

The host part (this file) only builds the filter lists once per dataset; scoring and counting run
in HIP.  There is no CPU path."""
import ctypes as C

import numpy as np
import torch

from . import _lib, models


def build_filter(known_h, known_r, known_t, test_h, test_r, test_t, neg_head, n_relations=None):
    """filter lists for `kge_rank_eval`: for test triple i the entities e such that the triple with
    its head (neg_head) / tail replaced by e is a KNOWN triple (train + valid + test, like the
    graph the reference's EvalSampler draws `false_neg` from).  Triples sharing (r,t) / (h,r) share
    one list.  Returns (rng [E,2] int64, ids [M] int64) numpy arrays."""
    known_h, known_r, known_t = (np.asarray(x, np.int64) for x in (known_h, known_r, known_t))
    test_h, test_r, test_t = (np.asarray(x, np.int64) for x in (test_h, test_r, test_t))
    R = int(n_relations if n_relations is not None else max(known_r.max(initial=0), test_r.max(initial=0)) + 1)
    if neg_head:
        key, val = known_t * R + known_r, known_h
        tkey = test_t * R + test_r
    else:
        key, val = known_h * R + known_r, known_t
        tkey = test_h * R + test_r
    order = np.lexsort((val, key))
    key, val = key[order], val[order]
    if key.shape[0]:
        keep = np.ones(key.shape[0], bool)
        keep[1:] = (key[1:] != key[:-1]) | (val[1:] != val[:-1])      # unique (key, entity) pairs
        key, val = key[keep], val[keep]
    rng = np.stack([np.searchsorted(key, tkey, "left"), np.searchsorted(key, tkey, "right")], 1).astype(np.int64)
    return rng, val.astype(np.int64)


_FORCE_TWO_KEY_SORT = False      # tests: take the large-graph path of build_filter_device on a small graph


def _put_ids(x, dev):
    if isinstance(x, torch.Tensor):
        return x.to(dev, torch.int64)
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.int64))).to(dev)


def sort_known_device(known, neg_head, n_relations, n_entities, dev):
    """the sort half of `build_filter_device`: (key, val) int64 tensors on `dev`, the unique (key, entity) pairs of the known
    triples (h, r, t) sorted by key, then entity - key = t * R + r with heads as values (neg_head) or h * R + r with tails.
    Intermediates are dropped as soon as they are used: for M known triples the peak is 2 x 16 M bytes above what was allocated
    before (measured at M = 597 213 on the device, tools/link_predict_timing.py: the composite key and torch.unique's
    buffers), against the 16 M bytes that remain.  Returns None when `key` itself would overflow int64."""
    R, NE = int(n_relations), int(n_entities)
    if NE * R >= (1 << 62):
        return None
    two_key = NE * R * NE >= (1 << 62) or _FORCE_TWO_KEY_SORT
    kh, kr, kt = known
    if neg_head:
        key, val = _put_ids(kt, dev) * R, _put_ids(kh, dev)
    else:
        key, val = _put_ids(kh, dev) * R, _put_ids(kt, dev)
    key += _put_ids(kr, dev)
    if two_key:
        o = torch.argsort(val, stable=True)
        o = o[torch.argsort(key[o], stable=True)]            # lexicographic (key, entity) order
        key, val = key[o], val[o]
        del o
        if key.shape[0]:
            keep = torch.ones(key.shape[0], dtype=torch.bool, device=key.device)
            keep[1:] = (key[1:] != key[:-1]) | (val[1:] != val[:-1])
            key, val = key[keep], val[keep]
    else:
        key *= NE
        key += val
        del val
        comp = torch.unique(key)                             # sorted unique (key, entity) pairs
        del key
        key = torch.div(comp, NE, rounding_mode='floor')
        val = comp - key * NE
    return key, val


def key_ranges(key, qkey):
    """the lookup half: [n, 2] int64, the [left, right) range of every query key in the sorted `key`"""
    return torch.stack([torch.searchsorted(key, qkey, right=False), torch.searchsorted(key, qkey, right=True)], 1).contiguous()


def build_filter_device(known, test, neg_head, n_relations, n_entities, dev):
    """`build_filter` with the sort on the device: the same lists in the same order (unique (key, entity) pairs sorted by key, then
    entity; per test triple the [left, right) range of its key), as int64 DEVICE tensors ready for `Ranker.ranks`.  One composite
    key `(key * n_entities + entity)` through `torch.unique` instead of a host `np.lexsort` over every known triple - 0.09 s per
    corruption side at FB15k's 592 k known triples, which was 87 % of a validation (tools/eval_timing.py).  When the composite key
    does not fit int64 (Freebase: 86 M entities x 14 824 relations x 86 M) the same order comes from two stable device sorts
    (entity, then key).  Returns None only when even `key` would overflow.  (The sort is `sort_known_device`, which the
    link-prediction index - known.py - keeps; the lookup is `key_ranges`.)"""
    kv = sort_known_device(known, neg_head, n_relations, n_entities, dev)
    if kv is None:
        return None
    key, val = kv
    R = int(n_relations)
    th_, tr_, tt_ = (_put_ids(x, dev) for x in test)
    tkey = (tt_ if neg_head else th_) * R + tr_
    return key_ranges(key, tkey), val.contiguous()


def build_relation_filter(known, test, n_entities, n_relations, dev=None):
    """relation lists for `Ranker.relation_ranks` (kge_rank_rel_eval): for test triple i = (h, r, t) the ascending unique relation
    ids that do NOT count among its candidates - its own relation r, and with `known` ((h, r, t) id arrays, or None for raw
    ranking) every relation j for which (h, j, t) is a known triple.  The test triples are appended to the known ones, so every
    list holds its own relation.  Sorted on `dev` (default: the GPU when there is one) like `build_filter_device`: one composite
    key ((h * n_entities + t) * n_relations + relation) through torch.unique, or two stable sorts when that would not fit int64;
    the ranges come from `key_ranges`.  Returns (ranges [E, 2], ids) int64 tensors on `dev`; triples with the same (h, t) share a
    list.  known=None: ranges[i] = (i, i + 1), ids = r."""
    if dev is None:
        dev = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    th_, tr_, tt_ = (_put_ids(x, dev) for x in test)
    E = int(th_.shape[0])
    if known is None:
        lo = torch.arange(E, dtype=torch.int64, device=dev)
        return torch.stack([lo, lo + 1], 1).contiguous(), tr_.contiguous()
    NE, R = int(n_entities), int(n_relations)
    if NE * NE >= (1 << 62):
        raise _lib.KgeError("build_relation_filter: %d entities are too many for the (head, tail) key" % NE)
    kh, kr, kt = (torch.cat([_put_ids(x, dev), y]) for x, y in zip(known, (th_, tr_, tt_)))
    key = kh * NE
    key += kt
    del kh, kt
    if NE * NE * R >= (1 << 62) or _FORCE_TWO_KEY_SORT:
        o = torch.argsort(kr, stable=True)
        o = o[torch.argsort(key[o], stable=True)]            # lexicographic (key, relation) order
        key, val = key[o], kr[o]
        del o
        keep = torch.ones(key.shape[0], dtype=torch.bool, device=key.device)
        keep[1:] = (key[1:] != key[:-1]) | (val[1:] != val[:-1])
        key, val = key[keep], val[keep]
    else:
        key *= R
        key += kr
        comp = torch.unique(key)                             # sorted unique (key, relation) pairs
        del key
        key = torch.div(comp, R, rounding_mode='floor')
        val = comp - key * R
    return key_ranges(key, th_ * NE + tt_), val.contiguous()


class Ranker(object):
    """device-resident evaluation of one (ent, rel) table pair."""

    def __init__(self, model_name, ent, rel, gamma, emb_init, batch=1024, flags=0, proj=None):
        if not ent.is_cuda:
            raise _lib.KgeError("Ranker needs CUDA (HIP) tensors; there is no CPU path")
        self.model = _lib.model_id(model_name)
        self.ent, self.rel = ent, rel
        self.gamma, self.emb_init = float(gamma), float(emb_init)
        self.batch = int(batch)
        self.flags = int(flags)
        self.proj = proj                   # TransR: projection table [n_rel, d_e * d_r]
        if model_name == 'TransR' and proj is None:
            raise _lib.KgeError("TransR ranking needs the projection table (proj=...)")
        self._ws = None
        self._all = None
        self._cws = None                   # workspace of chunked_ranks
        self.chunk_ws_budget = 512 << 20   # bytes: chunked_ranks asks for at most this (never less than one chunk needs)
        self._rws = None                   # workspace of relation_ranks
        self.rel_ws_budget = 512 << 20     # bytes: relation_ranks asks for at most this (never less than one row needs)

    def relation_ranks(self, h, r, t, filt, want_pos_score=False):
        """int32 [E] ranks of the true RELATIONS among all relations (kge_rank_rel_eval): 1 + the relations outside the triple's
        list that score at least as high as the true one.  filt: the (ranges, relation ids) pair of `build_relation_filter` -
        required, every list holds at least the triple's own relation.  The triples go in batches of `self.batch`, halved until
        the workspace fits `rel_ws_budget` (RESCAL's query rows are d_e^2 wide, TransR keeps a [relations, batch] block)."""
        dev = self.ent.device

        def put(x, dt=torch.int64):
            if isinstance(x, torch.Tensor):
                return x.to(dev, dt).contiguous()
            return torch.as_tensor(np.ascontiguousarray(x)).to(dev, dt)
        if filt is None:
            raise _lib.KgeError("relation_ranks needs the lists of build_relation_filter (raw ranking: known=None)")
        h, r, t = put(h), put(r), put(t)
        frng, fids = put(filt[0].reshape(-1)), put(filt[1])
        E = int(h.shape[0])
        ranks = torch.zeros(E, dtype=torch.int32, device=dev)
        pos = torch.empty(E, dtype=torch.float32, device=dev) if want_pos_score else None
        if E == 0:
            return (ranks, pos) if want_pos_score else ranks
        n_rel, d_e, d_r = int(self.rel.shape[0]), int(self.ent.shape[1]), int(self.rel.shape[1])

        def need_of(eb):
            return _lib.rank_rel_workspace_bytes(self.model, eb, n_rel, d_e, d_r)
        Eb = max(1, min(self.batch, E))
        while Eb > 1 and need_of(Eb) > self.rel_ws_budget:
            Eb = (Eb + 1) // 2
        need = need_of(Eb)
        m = models.BY_ID.get(self.model)
        if need == 0 and m and m.no_relation_ranking_lib:
            raise _lib.KgeError("kge_rank_rel_eval: not available for %s (%s)" % (m.name, m.no_relation_ranking_lib))
        if need == 0:
            raise _lib.KgeError("relation_ranks: the tables are %s / %s, which this model does not take"
                                % (tuple(self.ent.shape), tuple(self.rel.shape)))
        if self._rws is None or self._rws.numel() < need:
            self._rws = None
            self._rws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().kge_rank_rel_eval(
            self.model, _lib.ptr(self.ent), self.ent.shape[0], _lib.ptr(self.rel), n_rel, _lib.ptr(self.proj), _lib.ptr(h),
            _lib.ptr(r), _lib.ptr(t), E, d_e, d_r, self.gamma, self.emb_init, _lib.ptr(frng), _lib.ptr(fids), Eb, _lib.ptr(ranks),
            _lib.ptr(pos), _lib.ptr(self._rws), need, self.flags, _lib.stream_ptr()))
        return (ranks, pos) if want_pos_score else ranks

    def chunked_ranks(self, h, r, t, neg_head, chunk, cand=None, filt=None, self_cand=False, want_pos_score=False):
        """int32 [E] ranks, the triples taken in chunks of `chunk` and every chunk ranked against its own candidates
        (kge_rank_eval_chunked, one call).  cand: None (all entities), [n] (one list for all chunks) or [n_chunks, n] entity ids,
        -1 = empty slot; filt: the (ranges, entity ids) pair of build_filter_device / build_filter - ids, not columns;
        self_cand: prepend every chunk's own corrupted-side entities, the triple's own column scoring 0 (--neg_deg_sample_eval)."""
        dev = self.ent.device

        def put(x, dt=torch.int64):
            if x is None:
                return None
            if isinstance(x, torch.Tensor):
                return x.to(dev, dt).contiguous()
            return torch.as_tensor(np.ascontiguousarray(x)).to(dev, dt)
        h, r, t, cand = put(h), put(r), put(t), put(cand)
        E, chunk = int(h.shape[0]), int(chunk)
        n_ent = int(self.ent.shape[0])
        if chunk <= 0:
            raise _lib.KgeError("chunked_ranks: chunk must be positive")
        if self_cand and filt is not None:
            raise _lib.KgeError("if negative sampling based on degree, we can't filter positive edges.")
        n_chunks = (E + chunk - 1) // chunk
        stride = 0
        if cand is not None:
            if cand.dim() == 2:
                if cand.shape[0] != n_chunks:
                    raise _lib.KgeError("chunked_ranks: %d candidate lists for %d chunks" % (cand.shape[0], n_chunks))
                stride = int(cand.shape[1])
            elif cand.dim() != 1:
                raise _lib.KgeError("chunked_ranks: cand must be [n] or [n_chunks, n]")
            if cand.numel() == 0:
                raise _lib.KgeError("chunked_ranks: empty candidate list")
            if int(cand.max()) >= n_ent:
                raise _lib.KgeError("chunked_ranks: candidate id %d outside the %d entities" % (int(cand.max()), n_ent))
        n_cand = int(cand.shape[-1]) if cand is not None else n_ent
        frng = fids = None
        if filt is not None:
            frng, fids = put(filt[0].reshape(-1)), put(filt[1])
            if fids.shape[0] == 0:
                fids = torch.zeros(1, dtype=torch.int64, device=dev)
        ranks = torch.zeros(E, dtype=torch.int32, device=dev)
        pos = torch.empty(E, dtype=torch.float32, device=dev) if want_pos_score else None
        if E == 0:
            return (ranks, pos) if want_pos_score else ranks
        d_e, d_r = int(self.ent.shape[1]), int(self.rel.shape[1])

        def need_of(nch):
            return _lib.lib().kge_rank_chunked_workspace_bytes(self.model, nch * chunk, chunk, n_cand, int(bool(self_cand)), d_e, d_r)
        nch = n_chunks                      # whole chunks per block: as many as the budget holds, at least one
        while nch > 1 and need_of(nch) > self.chunk_ws_budget:
            nch = (nch + 1) // 2
        need = need_of(nch)
        if self._cws is None or self._cws.numel() < need:
            self._cws = None
            self._cws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().kge_rank_eval_chunked(
            self.model, int(bool(neg_head)), _lib.ptr(self.ent), n_ent, _lib.ptr(self.rel), self.rel.shape[0], _lib.ptr(self.proj),
            _lib.ptr(h), _lib.ptr(r), _lib.ptr(t), E, d_e, d_r, self.gamma, self.emb_init, chunk, _lib.ptr(cand), n_cand, stride,
            int(bool(self_cand)), _lib.ptr(frng), _lib.ptr(fids), _lib.ptr(ranks), _lib.ptr(pos), _lib.ptr(self._cws), need,
            self.flags, _lib.stream_ptr()))
        return (ranks, pos) if want_pos_score else ranks

    def ranks(self, h, r, t, neg_head, filt=None, cand=None, want_pos_score=False):
        """int32 [E] ranks of the true triples among the corruptions of the chosen side."""
        dev = self.ent.device

        def put(x, dt=torch.int64):
            if x is None:
                return None
            if isinstance(x, torch.Tensor):
                return x.to(dev, dt).contiguous()
            return torch.as_tensor(np.ascontiguousarray(x)).to(dev, dt)
        h, r, t, cand = put(h), put(r), put(t), put(cand)
        E = int(h.shape[0])
        if cand is None and self.proj is not None:         # TransR kernels walk an explicit candidate list
            if self._all is None:
                self._all = torch.arange(self.ent.shape[0], dtype=torch.int64, device=dev)
            cand = self._all
        n_cand = int(cand.shape[0]) if cand is not None else int(self.ent.shape[0])
        frng = fids = None
        if filt is not None:
            frng, fids = put(filt[0].reshape(-1)), put(filt[1])
            if fids.shape[0] == 0:
                fids = torch.zeros(1, dtype=torch.int64, device=dev)
        Eb = max(1, min(self.batch, E))
        need = _lib.lib().kge_rank_workspace_bytes(Eb, _lib.rank_ws_cands(self.model, n_cand), self.ent.shape[1])
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need + 4096, dtype=torch.uint8, device=dev)
        ranks = torch.zeros(E, dtype=torch.int32, device=dev)
        pos = torch.empty(E, dtype=torch.float32, device=dev) if want_pos_score else None
        _lib.check(_lib.lib().kge_rank_eval_ex(
            self.model, int(bool(neg_head)), _lib.ptr(self.ent), self.ent.shape[0], _lib.ptr(self.rel),
            self.rel.shape[0], _lib.ptr(self.proj), _lib.ptr(h), _lib.ptr(r), _lib.ptr(t), E, self.ent.shape[1],
            self.rel.shape[1],
            self.gamma, self.emb_init, _lib.ptr(cand), n_cand, _lib.ptr(frng), _lib.ptr(fids), Eb,
            _lib.ptr(ranks), _lib.ptr(pos), _lib.ptr(self._ws), self._ws.numel(), self.flags, _lib.stream_ptr()))
        return (ranks, pos) if want_pos_score else ranks


def metrics_from_ranks(ranks):
    """the averages `test()` prints (train_pytorch.py:236-247): MRR, MR, HITS@1/3/10."""
    rk = ranks.to(torch.float64)
    return {"MRR": float((1.0 / rk).mean()), "MR": float(rk.mean()),
            "HITS@1": float((rk <= 1).double().mean()), "HITS@3": float((rk <= 3).double().mean()),
            "HITS@10": float((rk <= 10).double().mean())}


def print_metrics(mode, metrics):
    """the lines of `test()` (train_pytorch.py:236-247): '[0]Valid average MRR: ...'; mode: 'Valid' or 'Test'"""
    for k, v in metrics.items():
        print('[{}]{} average {}: {}'.format(0, mode, k, v))


def eval_setup(dataset, which, args, cands=None):
    """what dglke_train's validation / test and dglke_eval hand to `evaluate*`, from the split `which` ('valid' / 'test') of
    `dataset` and the flags: (test, known, batch, cands).
    test: the split's (h, r, t), with --eval_percent p < 1 a random share of it (RandomState(seed + 17): the same rows in every
    process and at every validation); cands: the optional (head, tail) candidate matrices, either may be None, cut to the same rows;
    known: train + valid + test concatenated (the splits that exist), or None with --no_eval_filter;
    batch: test triples per kernel call - 4096 (or --batch_size_eval if larger), less where batch x entities x 4 bytes of scores
    would pass 2 GiB; 64 for TransR, which projects every candidate with every test triple's matrix."""
    trip = getattr(dataset, which)
    if trip is None:
        raise _lib.KgeError("the dataset has no %s split" % which)
    test = tuple(np.asarray(x) for x in trip[:3])
    if args.eval_percent < 1:
        n = len(test[0])
        keep = np.random.RandomState(args.seed + 17).permutation(n)[:max(1, int(n * args.eval_percent))]
        test = tuple(x[keep] for x in test)
        if cands is not None:
            cands = [c[keep] if c is not None else None for c in cands]
    known = None
    if args.eval_filter:
        parts = [p for p in (dataset.train, dataset.valid, dataset.test) if p is not None]
        known = tuple(np.concatenate([np.asarray(p[k]) for p in parts]) for k in range(3))
    batch = int(max(1, min(max(args.batch_size_eval, 4096), (1 << 31) // (4 * dataset.n_entities), len(test[0]))))
    if args.model_name == 'TransR':
        batch = min(batch, 64)
    return test, known, batch, cands


def sampled_ranks(rk, h, r, t, neg_head, filt, n_entities, n_cand, chunk, rng, cand_of_chunk=None):
    """`--neg_sample_size_eval n_cand` (EvalSampler with a negative sample size below the entity count,
    dataloader/sampler.py:514-597): every chunk of `chunk` test triples is ranked against ITS OWN n_cand candidates
    drawn uniformly with replacement from all entities; with a filter, candidates that make a known triple do not
    count (the sampler's false-negative bias, general_models.py:463-475).  rank = 1 + #{unfiltered candidates scoring
    >= the true triple}.  cand_of_chunk(k): override of the draw (tests)."""
    h, r, t = (np.asarray(x, np.int64) for x in (h, r, t))
    E = h.shape[0]
    out = []
    for k, e0 in enumerate(range(0, E, chunk)):
        e1 = min(E, e0 + chunk)
        cand = cand_of_chunk(k) if cand_of_chunk is not None else rng.randint(0, n_entities, size=n_cand)
        cand = np.asarray(cand, np.int64)
        f = filter_columns(cand, filt, e0, e1) if filt is not None else None
        out.append(rk.ranks(h[e0:e1], r[e0:e1], t[e0:e1], neg_head, f, cand=cand))
    return torch.cat(out)


def filter_columns(cand, filt, e0, e1):
    """columns of the candidate list `cand` that hold a filtered entity, per test triple e0 .. e1 - 1 (duplicates in the draw
    are separate columns): sorted candidates + two binary searches per filtered id.  Returns (rng [e1 - e0, 2], cols)."""
    order = np.argsort(cand, kind="stable")
    sc = cand[order]
    frng, fids = filt
    ptr, cols = [0], []
    for i in range(e0, e1):
        ids = fids[frng[i, 0]:frng[i, 1]]
        lo, hi = np.searchsorted(sc, ids, "left"), np.searchsorted(sc, ids, "right")
        hit = [order[a:b] for a, b in zip(lo, hi) if b > a]
        c = np.concatenate(hit) if hit else np.zeros(0, np.int64)
        cols.append(c)
        ptr.append(ptr[-1] + c.shape[0])
    ptr = np.asarray(ptr, np.int64)
    return np.stack([ptr[:-1], ptr[1:]], 1), np.concatenate(cols) if cols else np.zeros(0, np.int64)


def evaluate(model_name, ent, rel, gamma, emb_init, test, known=None, batch=1024, modes=("head", "tail"), proj=None,
             n_cand=None, chunk=None, seed=0, cache=None, neg_deg_sample=False):
    """filtered (known given) or raw ranking metrics over both corruption modes, averaged over all
    2E rankings like the reference (logs of the head and the tail sampler are concatenated,
    train_pytorch.py:221-231).  test / known: (h, r, t) triples of int64 arrays.  n_cand, 0 < n_cand < number of entities:
    rank against n_cand sampled candidates per chunk of `chunk` triples instead of all entities (anything else - the flag's -1,
    None, the entity count - ranks against all of them: --neg_sample_size_eval is passed as it is).
    cache: a dict the caller keeps per (split, known set) - the filter lists and the test triples stay on the device between
    calls (a training run validates the SAME split against the SAME known triples every --eval_interval steps).
    neg_deg_sample: --neg_deg_sample_eval (general_models.py:396-432) - every chunk's own corrupted-side entities are prepended
    to its candidates (n_cand sampled ones, or all entities) and the triple's own column scores 0; raw ranking only."""
    if neg_deg_sample and known is not None:
        raise _lib.KgeError("if negative sampling based on degree, we can't filter positive edges.")
    rk = Ranker(model_name, ent, rel, gamma, emb_init, batch, proj=proj)
    th_, tr_, tt_ = test
    n_ent = int(ent.shape[0])
    sampled = n_cand is not None and 0 < n_cand < n_ent
    rng = np.random.RandomState(seed)
    dev = ent.device
    if neg_deg_sample:
        ck = int(chunk or batch)
        n_chunks = (len(th_) + ck - 1) // ck
        tdev = tuple(_put_ids(x, dev) for x in test)
        cands = None
        if sampled:       # sampled_ranks' order: one draw per chunk, every chunk of the first mode before the second
            cands = np.stack([rng.randint(0, n_ent, size=int(n_cand)) for _ in range(len(modes) * n_chunks)]) \
                if n_chunks else np.zeros((0, int(n_cand)), np.int64)
            cands = _put_ids(cands, dev).reshape(len(modes), n_chunks, int(n_cand))
        allr = [rk.chunked_ranks(tdev[0], tdev[1], tdev[2], mode == "head", ck, cand=cands[k] if sampled else None, self_cand=True)
                for k, mode in enumerate(modes)]
        return metrics_from_ranks(torch.cat(allr))
    if cache is not None and not sampled:
        if "test" not in cache:
            cache["test"] = tuple(torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.int64))).to(dev) for x in test)
        th_, tr_, tt_ = cache["test"]
    allr = []
    for mode in modes:
        neg_head = mode == "head"
        filt = None
        if known is not None:
            if cache is not None and ("filt", mode, sampled) in cache:
                filt = cache[("filt", mode, sampled)]
            else:
                # lists built on the device - and kept there, unless candidates are sampled: then the host maps them to columns
                filt = build_filter_device(known, (th_, tr_, tt_), neg_head, rel.shape[0], n_ent, dev)
                if sampled and filt is not None:
                    filt = (filt[0].cpu().numpy(), filt[1].cpu().numpy())
                if filt is None:
                    filt = build_filter(known[0], known[1], known[2], *(x.cpu().numpy() if isinstance(x, torch.Tensor) else x
                                                                        for x in (th_, tr_, tt_)), neg_head, rel.shape[0])
                if cache is not None:
                    cache[("filt", mode, sampled)] = filt
        if sampled:
            allr.append(sampled_ranks(rk, th_, tr_, tt_, neg_head, filt, n_ent, int(n_cand), int(chunk or batch), rng))
        else:
            allr.append(rk.ranks(th_, tr_, tt_, neg_head, filt))
    return metrics_from_ranks(torch.cat(allr))


def evaluate_candidates(model_name, ent, rel, gamma, emb_init, test, cand_head=None, cand_tail=None, known=None, batch=1024,
                        proj=None):
    """ranking against GIVEN candidates, one list per test triple and side - the official ogbl-wikikg2 / ogbl-biokg protocol and
    what the reference's forward_test_wikikg does (general_models.py:487-527).  cand_head / cand_tail: [E, n] integer matrices of
    entity ids (row i: the corrupted heads / tails triple i is ranked against; -1 pads a short row), either may be None; known:
    (h, r, t) triples whose corruptions do not count (filtered on the device by entity id).  The metrics cover the sides given."""
    if cand_head is None and cand_tail is None:
        raise _lib.KgeError("evaluate_candidates needs candidates for at least one side")
    rk = Ranker(model_name, ent, rel, gamma, emb_init, batch, proj=proj)
    dev = ent.device
    tdev = tuple(_put_ids(x, dev) for x in test)
    E = int(tdev[0].shape[0])
    n_ent = int(ent.shape[0])
    allr = []
    for neg_head, cand in ((True, cand_head), (False, cand_tail)):
        if cand is None:
            continue
        cand = _put_ids(cand, dev)
        if cand.dim() != 2 or cand.shape[0] != E:
            raise _lib.KgeError("evaluate_candidates: the %s candidates are %s for %d test triples"
                                % ("head" if neg_head else "tail", tuple(cand.shape), E))
        filt = None
        if known is not None:
            filt = build_filter_device(known, tdev, neg_head, rel.shape[0], n_ent, dev)
            if filt is None:
                filt = build_filter(known[0], known[1], known[2], *(x.cpu().numpy() for x in tdev), neg_head, rel.shape[0])
        allr.append(rk.chunked_ranks(tdev[0], tdev[1], tdev[2], neg_head, 1, cand=cand, filt=filt))
    return metrics_from_ranks(torch.cat(allr))


def evaluate_relations(model_name, ent, rel, gamma, emb_init, test, known=None, batch=1024, proj=None, cache=None):
    """relation ranking: every test triple (h, r, t) against ALL relations as (h, ?, t) - the metrics of `metrics_from_ranks` over
    the E rankings.  rank = 1 + the relations, other than r itself, that score at least as high as r; with `known` ((h, r, t)
    triples) the relations j for which (h, j, t) is a known triple do not count either (filtered), known=None ranks raw.  The
    reference has no such evaluation; the protocol is stated in include/kge_hip.h (kge_rank_rel_eval).  cache: as in `evaluate` -
    the lists and the test ids stay on the device between the validations of a run."""
    rk = Ranker(model_name, ent, rel, gamma, emb_init, batch, proj=proj)
    dev = ent.device
    if cache is not None and "rel_test" in cache:
        tdev, filt = cache["rel_test"], cache["rel_filt"]
    else:
        tdev = tuple(_put_ids(x, dev) for x in test)
        filt = build_relation_filter(known, tdev, ent.shape[0], rel.shape[0], dev)
        if cache is not None:
            cache["rel_test"], cache["rel_filt"] = tdev, filt
    return metrics_from_ranks(rk.relation_ranks(tdev[0], tdev[1], tdev[2], filt))


# ---- range-sharded tables ---------------------------------------------------------------------------------------------------
# The multi-GPU trainers keep the entity table range-sharded: rank k owns rows [lo_k, hi_k).  The evaluation below never assembles
# it: every rank scores ALL test triples against the candidates IT owns (kge_rank_eval_split) and the counts are summed over the
# ranks.  (The reference splits the test triples over its processes instead, each scoring against one shared host table:
# train.py:230-257, 330-350; train_pytorch.py:199-253.)

def shard_known(known, neg_head, lo, hi):
    """the known triples whose corrupted entity (the head when neg_head, else the tail) lies in [lo, hi), that entity shifted
    by -lo: their filter lists (build_filter / build_filter_device) are this rank's share of the full lists, as columns of its
    shard."""
    kh, kr, kt = (np.asarray(x, np.int64) for x in known)
    side = kh if neg_head else kt
    m = (side >= lo) & (side < hi)
    kh, kr, kt = kh[m], kr[m], kt[m]
    if neg_head:
        kh = kh - lo
    else:
        kt = kt - lo
    return kh, kr, kt


def owned_candidates(cand, lo, hi):
    """the positions of a candidate list that a rank owning [lo, hi) scores, and their rows in its shard (duplicates stay
    separate columns)."""
    cand = np.asarray(cand, np.int64)
    pos = np.nonzero((cand >= lo) & (cand < hi))[0]
    return pos, cand[pos] - lo


def allgather_rows(local, lo, bounds, ids, comm):
    """rows `ids` (sorted, unique, global; a device tensor every rank passes alike) of a range-sharded table: every owner
    contributes the rows it holds through ONE equal-split all-gather (`comm`: dist.RcclComm / HostStagedComm / TorchComm) and
    every rank receives all of them - copies, bit for bit (a summing all-reduce would turn -0.0 into +0.0)."""
    world = len(bounds) - 1
    cut = torch.searchsorted(ids, torch.as_tensor(np.asarray(bounds, np.int64), device=ids.device)).cpu().numpy()
    cnt = cut[1:] - cut[:-1]
    cap = int(cnt.max())
    rank = comm.rank
    d = local.shape[1]
    send = torch.zeros(cap, d, dtype=local.dtype, device=local.device)
    if cnt[rank]:
        send[:cnt[rank]] = local[ids[cut[rank]:cut[rank + 1]] - lo]
    recv = torch.empty(world * cap, d, dtype=local.dtype, device=local.device)
    comm.all_gather(recv, send)
    return torch.cat([recv[k * cap:k * cap + cnt[k]] for k in range(world)])


class SplitRanker(object):
    """kge_rank_eval_split on one rank's shard: query rows given per call, candidates = (a subset of) the shard."""

    def __init__(self, model_name, shard, rel, gamma, emb_init, batch=1024, flags=0, proj=None):
        if not rel.is_cuda:
            raise _lib.KgeError("SplitRanker needs CUDA (HIP) tensors; there is no CPU path")
        if model_name == 'TransR' and proj is None:
            raise _lib.KgeError("TransR ranking needs the projection table (proj=...)")
        self.model = _lib.model_id(model_name)
        self.shard, self.rel, self.proj = shard, rel, proj
        self.gamma, self.emb_init = float(gamma), float(emb_init)
        self.batch, self.flags = int(batch), int(flags)
        self._ws = None
        self._all = None

    def ranks(self, qent, h, r, t, neg_head, filt=None, cand=None):
        """int32 [E]: 1 + #{unfiltered candidates of this shard scoring >= the true triple}; h / t index qent."""
        dev = self.rel.device

        def put(x, dt=torch.int64):
            if x is None:
                return None
            if isinstance(x, torch.Tensor):
                return x.to(dev, dt).contiguous()
            return torch.as_tensor(np.ascontiguousarray(x)).to(dev, dt)
        h, r, t, cand = put(h), put(r), put(t), put(cand)
        E = int(h.shape[0])
        n_cent = int(self.shard.shape[0])
        if cand is None and self.proj is not None:         # TransR kernels walk an explicit candidate list
            if self._all is None:
                self._all = torch.arange(n_cent, dtype=torch.int64, device=dev)
            cand = self._all
        n_cand = int(cand.shape[0]) if cand is not None else n_cent
        if cand is not None and n_cand == 0:               # none of a sampled list is ours (an empty list has no pointer)
            cand, n_cent = None, 0
        frng = fids = None
        if filt is not None:
            frng, fids = put(filt[0].reshape(-1)), put(filt[1])
            if fids.shape[0] == 0:
                fids = torch.zeros(1, dtype=torch.int64, device=dev)
        Eb = max(1, min(self.batch, E))
        need = _lib.lib().kge_rank_workspace_bytes(Eb, n_cand, qent.shape[1])
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need + 4096, dtype=torch.uint8, device=dev)
        ranks = torch.zeros(E, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().kge_rank_eval_split(
            self.model, int(bool(neg_head)), _lib.ptr(qent), qent.shape[0], _lib.ptr(self.shard), n_cent, _lib.ptr(self.rel),
            self.rel.shape[0], _lib.ptr(self.proj), _lib.ptr(h), _lib.ptr(r), _lib.ptr(t), E, qent.shape[1], self.rel.shape[1],
            self.gamma, self.emb_init, _lib.ptr(cand), n_cand, _lib.ptr(frng), _lib.ptr(fids), Eb, _lib.ptr(ranks), None,
            _lib.ptr(self._ws), self._ws.numel(), self.flags, _lib.stream_ptr()))
        return ranks


def evaluate_sharded(model_name, shard, lo, n_entities, rel, gamma, emb_init, test, rows_of, known=None, batch=1024,
                     modes=("head", "tail"), proj=None, n_cand=None, chunk=None, seed=0, cache=None, group=None,
                     block_bytes=64 << 20):
    """`evaluate` on a range-sharded entity table, collective over `group` (every rank calls it with the same arguments but its
    own shard = rows [lo, lo + len(shard)) of the table).  rows_of(ids): the rows of the sorted unique global ids `ids` on this
    rank (collective: ShardedTables.gather, or allgather_rows).  rel / proj: the WHOLE relation-side tables on every rank.

    Every rank ranks every test triple against the candidates it owns - the whole shard, or with n_cand the owned positions of
    each chunk's draw, drawn exactly as `sampled_ranks` draws them (same seed, same order) - with the filter lists restricted to
    its entities; 1 + the sum of the ranks' counts is `evaluate`'s rank, and the metrics are computed from the same tensor.
    The query rows (heads and tails of the test triples) are assembled in blocks of at most ~block_bytes."""
    import torch.distributed as dist
    th_, tr_, tt_ = (np.asarray(x, np.int64) for x in test)
    E = th_.shape[0]
    n_ent = int(n_entities)
    hi = lo + int(shard.shape[0])
    sampled = n_cand is not None and 0 < n_cand < n_ent
    chunk = int(chunk or batch)
    rng = np.random.RandomState(seed)
    dev = rel.device
    rk = SplitRanker(model_name, shard, rel, gamma, emb_init, batch, proj=proj)
    if cache is not None and "test" in cache:
        tdev = cache["test"]
    else:
        tdev = tuple(torch.as_tensor(np.ascontiguousarray(x)).to(dev) for x in (th_, tr_, tt_))
        if cache is not None:
            cache["test"] = tdev
    filt = {}
    for mode in modes:
        if known is None:
            filt[mode] = None
            continue
        key = ("filt", mode, sampled, lo, hi)
        if cache is not None and key in cache:
            filt[mode] = cache[key]
            continue
        neg_head = mode == "head"
        kn = shard_known(known, neg_head, lo, hi)
        f = build_filter_device(kn, tdev, neg_head, rel.shape[0], n_ent, dev)
        if sampled and f is not None:
            f = (f[0].cpu().numpy(), f[1].cpu().numpy())
        if f is None:
            f = build_filter(kn[0], kn[1], kn[2], th_, tr_, tt_, neg_head, rel.shape[0])
            if not sampled:
                f = (torch.as_tensor(f[0]).to(dev), torch.as_tensor(f[1]).to(dev))
        if cache is not None:
            cache[key] = f
        filt[mode] = f
    # blocks of test triples: whole evaluation batches (all entities) / whole chunks (sampled), so that every kernel call ranks
    # the same rows as `evaluate` does
    unit = chunk if sampled else max(1, min(int(batch), E))
    per = max(1, int(block_bytes) // max(1, 8 * int(shard.shape[1]) * unit)) * unit
    counts = torch.zeros(len(modes) * E, dtype=torch.int64, device=dev)
    # the sampled protocol draws every chunk of the first mode, then of the second: modes outside the blocks
    for group_modes in ([[m] for m in modes] if sampled else [list(modes)]):
        for b0 in range(0, E, per):
            b1 = min(E, b0 + per)
            ids, inv = torch.unique(torch.cat([tdev[0][b0:b1], tdev[2][b0:b1]]), return_inverse=True)
            qent = rows_of(ids).contiguous()
            qh, qt = inv[:b1 - b0].contiguous(), inv[b1 - b0:].contiguous()
            qr = tdev[1][b0:b1]
            for mode in group_modes:
                neg_head = mode == "head"
                mi = modes.index(mode)
                f = filt[mode]
                if not sampled:
                    fb = (f[0][b0:b1], f[1]) if f is not None else None
                    counts[mi * E + b0:mi * E + b1] = rk.ranks(qent, qh, qr, qt, neg_head, fb).to(torch.int64) - 1
                    continue
                for e0 in range(b0, b1, chunk):
                    e1 = min(b1, e0 + chunk)
                    cand = rng.randint(0, n_ent, size=int(n_cand))
                    pos, local = owned_candidates(cand, lo, hi)
                    fc = None
                    if f is not None:
                        fc = filter_columns(local, f, e0, e1)
                    got = rk.ranks(qent, qh[e0 - b0:e1 - b0], qr[e0 - b0:e1 - b0], qt[e0 - b0:e1 - b0], neg_head, fc,
                                   cand=local)
                    counts[mi * E + e0:mi * E + e1] = got.to(torch.int64) - 1
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        if dist.get_backend(group) == "gloo":
            host = counts.cpu()
            dist.all_reduce(host, group=group)
            counts = host.to(dev)
        else:
            dist.all_reduce(counts, group=group)
    ranks = (counts + 1).to(torch.int32)
    return metrics_from_ranks(ranks)
