"""Inference with trained embeddings: the reference's ScoreInfer and EmbSimInfer (python/dglke/models/infer.py:52-344),
same constructors, same topK() signatures, same result layout (a list of tuples of numpy arrays, one per group).

Every score and every selection runs in libkge_hip (csrc/kge_topk.hip): the query rows T(h, r) / T(t, r) are formed on
the device, scored against the candidate list by a tiled kernel whose epilogue keeps a running top-K per row, and the
per-row lists are merged into per-group results on the device.  No score block is ever materialised: the workspace is
O(rows in flight x (D + segments x K)) + O(N), and this module only builds id lists, sizes row batches and reads back K
results per group.

Deliberate differences from the reference:
  * RotatE's relation phase always uses the trained emb_init = (gamma + 2) / hidden_dim, also under score_func 'none'
    (the reference rebuilds the model with gamma 0 there and so rotates by a phase it never trained);
  * equal scores are ordered by position - (head, relation, tail) or (left, right) - where the reference leaves them unordered;
  * a NaN score ranks below every number;
  * the device is a GPU (no CPU path), TransR is refused (as in the reference) and K is limited to 1 .. TOPK_MAX;
  * the models: TransE_l1 / TransE_l2, DistMult, ComplEx, RotatE, RESCAL as in the reference, and SimplE, QuatE (rows of
    four quaternion quarters, the relation normalised per quaternion: include/kge_hip.h) and PairRE (relation rows [rH | rT] on
    unit-normalised entity rows), TransH (relation rows [d | w], both ends projected onto the hyperplane of normal w) and TransD
    (entity rows [e | e_p], relation rows [r | r_p], both ends through the rank-one map r_p e_p^T + I), which the reference does not
    have;
  * ke_model: attach_graph takes the known triples (head, rel, tail) themselves (there is no DGLGraph here);
  * ke_model: exclude_mode 'exclude' is exact - known combinations are left out inside the selection kernel, where the
    reference takes the 4K best and falls back to a full sort when too few of them survive; results agree wherever
    scores are not tied.
"""
import os

import numpy as np
import torch as th

from . import _lib
from ._lib import KgeError

TOPK_MAX = 128                      # KGE_TOPK_MAX
SIM_IDS = {"cosine": 16, "l2": 17, "l1": 18, "dot": 19, "ext_jaccard": 20}
WORKSPACE_BUDGET = 256 << 20        # bytes of workspace per call: fixes the rows in flight
DEFAULT_INFER_BATCHSIZE = 1024      # accepted by EmbSimInfer for signature parity (batching follows WORKSPACE_BUDGET)


def gpu_device(device):
    if device is None or (isinstance(device, (int, np.integer)) and device < 0) or str(device) == "cpu":
        raise KgeError("inference runs on the GPU only: pass --gpu <id> (there is no CPU path)")
    return th.device("cuda", int(device)) if isinstance(device, (int, np.integer)) else th.device(device)


def check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= TOPK_MAX:
        raise KgeError("--topK %r is outside 1 .. %d (the largest K the top-K kernels keep)" % (k, TOPK_MAX))
    return int(k)


def host_ids(x, n, what):
    """a user id list as int64 numpy (None = all n), every id checked to lie in 0 .. n-1 BEFORE anything reaches the
    device: the kernels read table rows at these ids"""
    if x is None:
        return None
    a = np.asarray(x, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() >= n):
        bad = int(a[(a < 0) | (a >= n)][0])
        raise KgeError("%s id %d is outside 0 .. %d (the table has %d rows)" % (what, bad, n - 1, n))
    return a


def _ids(a, n, dev):
    if a is None:
        return th.arange(n, dtype=th.int64, device=dev)
    return th.as_tensor(a).to(dev)


def on_device(fn):
    """run a method with its object's GPU as the current device: torch's id lists and the library calls (on
    torch's current stream, _lib.stream_ptr) then go to the same device and stream"""
    def wrapped(self, *a, **kw):
        with th.cuda.device(self.dev):
            return fn(self, *a, **kw)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def _workspace(nbytes, dev):
    return th.empty(max(int(nbytes), 1), dtype=th.uint8, device=dev)


def rows_in_flight(n_cand, d, k, budget=WORKSPACE_BUDGET):
    """the most query rows (a power of two, <= 4096) whose kge_topk_select workspace fits `budget`"""
    h = _lib.lib()
    rows = 4096
    while rows > 1 and h.kge_topk_workspace_bytes(rows, n_cand, d, k) > budget:
        rows //= 2
    return rows


def vector_topk(score, k):
    """the k best of a device score vector: (scores, positions) of the min(k, n) results"""
    h = _lib.lib()
    n = score.numel()
    dev = score.device
    res_s = th.zeros(1, k, dtype=th.float32, device=dev)
    res_o = th.full((1, k), -1, dtype=th.int64, device=dev)
    if n:
        ws = _workspace(h.kge_topk_workspace_bytes(0, n, 0, k), dev)
        _lib.check(h.kge_topk_vector(_lib.ptr(score), n, k, _lib.ptr(res_s), _lib.ptr(res_o), _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr()))
    m = min(k, n)
    return res_s[0, :m], res_o[0, :m]


def select_groups(func, side, ent, rel, d_e, d_r, gamma, emb_init, cand, n_rows, group_rows, row_fn, stride, k, max_rows=None,
                  filt_ids=None):
    """top-k per group of `group_rows` consecutive query rows (n_rows of them, rows batched to the workspace budget).
    row_fn(r0, r1) -> (h, r, t, row_base) int64 device tensors of rows [r0, r1).  Returns res_s, res_o [groups, k].
    With filt_ids (the sorted entity lists of known.KnownIndex) row_fn returns a fifth tensor, the rows' [r1 - r0, 2] list
    ranges, and candidates in a row's list are left out (kge_topk_select_filtered); a group may then return fewer than k
    results (ordinal -1 in the rest)."""
    h = _lib.lib()
    dev = cand.device
    G = n_rows // group_rows
    res_s = th.zeros(G, k, dtype=th.float32, device=dev)
    res_o = th.full((G, k), -1, dtype=th.int64, device=dev)
    N = cand.numel()
    if n_rows == 0 or N == 0:
        return res_s, res_o
    d_ws = _lib.topk_row_width(func, d_e)          # PairRE / TransH keep a pair of vectors per query row (include/kge_hip.h)
    if max_rows is None:
        max_rows = rows_in_flight(N, d_ws, k)
    per = (max_rows // group_rows) * group_rows if group_rows <= max_rows else max_rows
    ws = _workspace(_lib.topk_workspace_bytes(func, min(per, n_rows), N, d_e, k), dev)
    relp = _lib.ptr(rel) if rel is not None else None
    n_rel = rel.shape[0] if rel is not None else 0
    r0 = 0
    while r0 < n_rows:
        g0 = r0 // group_rows
        if group_rows <= max_rows:
            r1, grc = min(n_rows, r0 + per), group_rows
        else:                                                  # a group over several calls: the result carries over
            r1 = min((g0 + 1) * group_rows, r0 + per)
            grc = r1 - r0
        if filt_ids is not None:
            hh, rr, tt, base, fptr = row_fn(r0, r1)
            _lib.check(h.kge_topk_select_filtered(func, side, _lib.ptr(ent), ent.shape[0], relp, n_rel, _lib.ptr(hh),
                                                  _lib.ptr(rr), _lib.ptr(tt), r1 - r0, d_e, d_r, float(gamma),
                                                  float(emb_init), _lib.ptr(cand), N, _lib.ptr(base), int(stride), grc, k,
                                                  _lib.ptr(res_s[g0:]), _lib.ptr(res_o[g0:]), _lib.ptr(ws), ws.numel(),
                                                  _lib.ptr(fptr), _lib.ptr(filt_ids), _lib.stream_ptr()))
            r0 = r1
            continue
        hh, rr, tt, base = row_fn(r0, r1)[:4]
        _lib.check(h.kge_topk_select(func, side, _lib.ptr(ent), ent.shape[0], relp, n_rel, _lib.ptr(hh), _lib.ptr(rr),
                                     _lib.ptr(tt), r1 - r0, d_e, d_r, float(gamma), float(emb_init), _lib.ptr(cand), N,
                                     _lib.ptr(base), int(stride), grc, k, _lib.ptr(res_s[g0:]), _lib.ptr(res_o[g0:]),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        r0 = r1
    return res_s, res_o


def _np(x):
    return x.cpu().numpy()


def predict_topk(func, ent, rel_tab, gamma, emb_init, score_out, head, rel, tail, exec_mode, k, max_rows=None, known=None,
                 exclude_mode=None):
    """the top-k triples of one execution mode (ScoreInfer.topK and ke_model link_predict share this): a list of
    (head, rel, tail, score, mask) numpy tuples, one per group.  head / rel / tail: checked host id lists (None = all).
    known (a known.KnownIndex) with exclude_mode 'exclude': combinations that are known triples never enter the selection
    (kge_topk_select_filtered with the lists of the side the kernel scores; triplet_wise: kge_triples_known on the
    inputs), a group returns the unknown ones it has, up to k; 'mask': the unfiltered result plus a bool array per group,
    from one kge_triples_known call over the results of all groups; None: mask is None."""
    dev = ent.device
    num_entity, num_rel = ent.shape[0], rel_tab.shape[0]
    head, rel, tail = _ids(head, num_entity, dev), _ids(rel, num_rel, dev), _ids(tail, num_entity, dev)
    H, R, T = head.numel(), rel.numel(), tail.numel()
    d_e, d_r = ent.shape[1], rel_tab.shape[1]
    exclude = exclude_mode == 'exclude'
    if exec_mode == 'triplet_wise':
        if not H == R == T:
            raise KgeError("For triplet wise execution mode, head, relation and tail lists should have same length")
        if exclude:
            keep = th.nonzero(known.known(head, rel, tail) == 0).reshape(-1)       # the unknown inputs, in input order
            head, rel, tail = head[keep], rel[keep], tail[keep]
            H = head.numel()
        hs, rs, ts = ent[head].contiguous(), rel_tab[rel].contiguous(), ent[tail].contiguous()
        raw = th.empty(H, dtype=th.float32, device=dev)
        if H:
            _lib.check(_lib.lib().kge_score_pos(func, _lib.ptr(hs), _lib.ptr(rs), _lib.ptr(ts), H, d_e, d_r,
                                                gamma, emb_init, _lib.ptr(raw), _lib.stream_ptr()))
        s, o = vector_topk(raw, k)
        mask = _np(known.known(head[o], rel[o], tail[o])).astype(bool) if exclude_mode == 'mask' else None
        return [(_np(head[o]), _np(rel[o]), _np(tail[o]), _np(score_out(s)), mask)]

    def run(side, n_rows, group_rows, split):
        """split(k) -> (a_pos, rpos) of row k; side 0: a = head, candidates = tails; side 1: a = tail, candidates = heads"""
        def row_fn(r0, r1):
            kk = th.arange(r0, r1, dtype=th.int64, device=dev)
            apos, rpos = split(kk)
            if side == 0:
                aid, rid, base = head[apos], rel[rpos], (apos * R + rpos) * T
            else:
                aid, rid, base = tail[apos], rel[rpos], rpos * T + apos
            if exclude:
                return aid, rid, aid, base, known.ranges(side, aid, rid)
            return aid, rid, aid, base
        cand = tail if side == 0 else head
        return select_groups(func, side, ent, rel_tab, d_e, d_r, gamma, emb_init, cand, n_rows, group_rows, row_fn,
                             1 if side == 0 else R * T, k, max_rows, known.filt_ids(side) if exclude else None)

    a_major = lambda kk: (kk // R, kk % R)             # rows (a, r), a-major
    if exec_mode == 'all':
        side = 0 if T >= H else 1
        res_s, res_o = run(side, (H if side == 0 else T) * R, max(1, (H if side == 0 else T) * R), a_major)
    elif exec_mode == 'batch_head':
        res_s, res_o = run(0, H * R, max(R, 1), a_major)
    elif exec_mode == 'batch_tail':
        res_s, res_o = run(1, T * R, max(R, 1), a_major)
    else:                                                # batch_rel: rows (r, a), relation-major
        side = 0 if T >= H else 1
        na = H if side == 0 else T
        res_s, res_o = run(side, R * na, max(na, 1), lambda kk: (kk % na, kk // na))
    groups = {'all': 1, 'batch_head': H, 'batch_rel': R, 'batch_tail': T}[exec_mode]
    combos = {'all': H * R * T, 'batch_head': R * T, 'batch_rel': H * T, 'batch_tail': H * R}[exec_mode]
    m = min(k, combos)
    M = None
    if exclude_mode == 'mask' and m and res_o.shape[0] and H and R and T:
        o = res_o[:, :m].reshape(-1)                     # (unfiltered: the first m slots of every group are results)
        tp, rest = o % T, o // T
        M = _np(known.known(head[rest // R], rel[rest % R], tail[tp])).astype(bool).reshape(-1, m)
    S, O = _np(score_out(res_s[:, :m])), _np(res_o[:, :m])          # one read-back for all groups
    hn, rn, tn = _np(head), _np(rel), _np(tail)
    short = (O < 0).sum(1) if exclude else None                   # fewer unknown combinations than k: empty slots are last
    out = []
    for g in range(groups):
        o = O[g] if g < O.shape[0] else np.zeros(0, np.int64)     # (an empty list on the other axes: no combinations)
        s = S[g] if g < S.shape[0] else np.zeros(0, np.float32)
        if exclude and g < O.shape[0] and short[g]:
            o, s = o[:m - short[g]], s[:m - short[g]]
        tp, rest = (o % T, o // T) if T else (o, o)
        rp, hp = (rest % R, rest // R) if R else (rest, rest)
        mask = None
        if exclude_mode == 'mask':
            mask = M[g] if M is not None and g < M.shape[0] else np.zeros(len(o), bool)
        out.append((hn[hp], rn[rp], tn[tp], s, mask))
    return out


class ScoreInfer(object):
    """models/infer.py:52-214: top-K triples (h, r, t) of a trained model.  score_func 'none': score = x (gamma 0 for
    the distance models, as in the reference); 'logsigmoid': log(sigmoid(x)) with the trained gamma."""

    def __init__(self, device, config, model_path, sfunc='none'):
        if sfunc not in ('none', 'logsigmoid'):
            raise KgeError("score function should be none or logsigmoid (got %r)" % (sfunc,))
        name = config['model_name']
        if name == 'TransR':
            raise KgeError("TransR has no inference path (the reference's InferModel refuses it too)")
        self.func = _lib.model_id(name)
        self.dev = gpu_device(device)
        self.config = config
        self.model_path = model_path
        self.sfunc = sfunc
        self.max_rows = None            # rows in flight per call (None: from WORKSPACE_BUDGET)

    @on_device
    def load_model(self):
        c = self.config
        stem = os.path.join(self.model_path, "%s_%s_" % (c['dataset'], c['model_name']))
        self.ent = th.from_numpy(np.load(stem + "entity.npy").astype(np.float32)).contiguous().to(self.dev)
        self.rel = th.from_numpy(np.load(stem + "relation.npy").astype(np.float32)).contiguous().to(self.dev)
        self.num_entity, self.num_rel = self.ent.shape[0], self.rel.shape[0]
        self.gamma = float(c['gamma']) if self.sfunc == 'logsigmoid' else 0.0
        self.emb_init = (float(c['gamma']) + 2.0) / float(c['hidden_dim'])       # the TRAINED phase scale (RotatE)

    def _score_out(self, s):
        return th.nn.functional.logsigmoid(s) if self.sfunc == 'logsigmoid' else s

    def topK(self, head=None, rel=None, tail=None, exec_mode='all', k=10):
        k = check_k(k)
        if exec_mode not in ('triplet_wise', 'all', 'batch_head', 'batch_rel', 'batch_tail'):
            raise KgeError("unknown execution mode %r" % (exec_mode,))
        head, tail = host_ids(head, self.num_entity, "head"), host_ids(tail, self.num_entity, "tail")
        rel = host_ids(rel, self.num_rel, "relation")
        return self._topk(head, rel, tail, exec_mode, k)

    @on_device
    def _topk(self, head, rel, tail, exec_mode, k):
        return [g[:4] for g in predict_topk(self.func, self.ent, self.rel, self.gamma, self.emb_init, self._score_out, head, rel,
                                            tail, exec_mode, k, self.max_rows)]


class EmbSimInfer(object):
    """models/infer.py:216-344: top-K most similar (left, right) embedding pairs under cosine, l2, l1, dot or
    ext_jaccard (tensor_models.py:59-100)."""

    def __init__(self, device, emb_file, sfunc='cosine', batch_size=DEFAULT_INFER_BATCHSIZE):
        if sfunc not in SIM_IDS:
            raise KgeError("unknown similarity function %r (cosine, l2, l1, dot, ext_jaccard)" % (sfunc,))
        self.dev = gpu_device(device)
        self.emb_file = emb_file
        self.sfunc = sfunc
        self.batch_size = batch_size
        self.max_rows = None

    @classmethod
    def from_tensor(cls, device, emb, sfunc='cosine'):
        """the same machinery on a table that is already loaded (ke_model.embed_sim)"""
        m = cls(device, None, sfunc)
        m.emb = emb.reshape(emb.shape[0], -1).to(m.dev, th.float32).contiguous()
        return m

    @on_device
    def load_emb(self):
        e = np.load(self.emb_file).astype(np.float32)
        self.emb = th.from_numpy(e.reshape(e.shape[0], -1)).contiguous().to(self.dev)

    def topK(self, head=None, tail=None, bcast=False, pair_ws=False, k=10):
        k = check_k(k)
        n = self.emb.shape[0]
        return self._topk(host_ids(head, n, "left"), host_ids(tail, n, "right"), bcast, pair_ws, k)

    @on_device
    def _topk(self, head, tail, bcast, pair_ws, k):
        dev, n, d = self.dev, self.emb.shape[0], self.emb.shape[1]
        head, tail = _ids(head, n, dev), _ids(tail, n, dev)
        L, Rn = head.numel(), tail.numel()
        sim = SIM_IDS[self.sfunc]
        if pair_ws:
            if L != Rn:
                raise KgeError("For pairwise execution mode, the left and right lists should have same length")
            sc = th.empty(L, dtype=th.float32, device=dev)
            if L:
                _lib.check(_lib.lib().kge_sim_pairwise(sim, _lib.ptr(self.emb), n, d, _lib.ptr(head), _lib.ptr(tail), L,
                                                       _lib.ptr(sc), _lib.stream_ptr()))
            s, o = vector_topk(sc, k)
            return [(_np(head[o]), _np(tail[o]), _np(s))]

        def row_fn(r0, r1):
            kk = th.arange(r0, r1, dtype=th.int64, device=dev)
            return head[kk], None, None, kk * Rn
        res_s, res_o = select_groups(sim, 0, self.emb, None, d, 0, 0.0, 0.0, tail, L, 1 if bcast else max(L, 1), row_fn,
                                     1, k, self.max_rows)
        m = min(k, Rn if bcast else L * Rn)
        S, O = _np(res_s[:, :m]), _np(res_o[:, :m])
        hn, tn = _np(head), _np(tail)
        if not bcast:
            s, o = (S[0], O[0]) if L else (np.zeros(0, np.float32), np.zeros(0, np.int64))
            return [(hn[o // Rn], tn[o % Rn], s)] if Rn else [(hn[:0], tn[:0], s[:0])]
        return [(np.full((m,), hn[i]), tn[O[i] % Rn] if Rn else tn[:0], S[i]) for i in range(L)]
