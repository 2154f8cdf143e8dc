"""The K-vs-all step (include/kge_hip.h, kge_step_fused_known on a batch with N == 0) stated in numpy, and the cases the tests run.

`step` is the 1-vs-all statement (one_vs_all_cases.py: operands, per-edge gradients, the order of the three traces) with the criterion
replaced: binary cross-entropy over every entity against smoothed known-answer labels.  float64 by default; with dtype=np.float32
it is the plain float32 restatement whose error sets the tolerance of a case (test_gpu_k_vs_all.py).  It never calls the library."""
from collections import namedtuple

import numpy as np

import one_vs_all_cases as V
from one_vs_all_cases import EPS, LR, N_REL, _adagrad, edge_grads, edge_terms, reg_grad

Case = namedtuple('Case', 'name model neg_head n_ent B d kind smooth reg_coef scores')


def _c(model, neg_head, n_ent, B, d, kind, smooth, reg_coef=0.0, scores='plain'):
    name = '%s-%s-n%d-B%d-d%d-%s-s%g%s' % (model, 'head' if neg_head else 'tail', n_ent, B, d, kind, smooth,
                                          '' if scores == 'plain' else '-' + scores)
    return Case(name, model, neg_head, n_ent, B, d, kind, smooth, reg_coef, scores)


# n_ent: one owner tile and one column tile, each +-1, 300 (ragged last split) and 8200 (two tiles per split); B: below a row tile, one plus a ragged second;
# d: the minimum, a last k-stage with a tail, two full stages, two column groups in the GA kernel, the owner kernel's widest instance.
# Label kinds: none (empty index: the own end alone), edges (a list on both sides of every column-tile and owner boundary), hub (a
# long list shared by rows of two row tiles), dups (the batch's own triples: two rows share a query, one row has h == t)
CASES = [
    _c('DistMult', False, 63, 16, 4, 'none', 0.0), _c('ComplEx', True, 65, 136, 36, 'edges', 0.1),
    _c('DistMult', True, 129, 136, 64, 'edges', 0.0), _c('ComplEx', False, 300, 136, 36, 'hub', 0.1),
    _c('DistMult', False, 300, 16, 64, 'edges', 0.1), _c('ComplEx', True, 129, 16, 4, 'dups', 0.0),
    _c('DistMult', True, 65, 16, 260, 'edges', 0.1), _c('ComplEx', False, 63, 16, 512, 'none', 0.1),
    _c('DistMult', True, 300, 136, 36, 'hub', 0.0), _c('ComplEx', False, 129, 136, 64, 'dups', 0.0),
    _c('ComplEx', True, 65, 136, 36, 'edges', 0.1, 1e-3, 'weights'),      # edge weights, and the regulariser
    _c('DistMult', False, 300, 136, 64, 'edges', 0.1, 0.0, 'big'),        # scores reach +-80
    # 65 column tiles over at most 64 GA parts (two row tiles x two column groups): every split of the GA kernel walks TWO tiles - the
    # cursor, the row sums, the label bits and the G tile all carry over; the hub list has entries in every one of them
    _c('DistMult', True, 8200, 136, 260, 'hub', 0.1),
]
DETERMINISM = CASES[3]


def labels(neg_head, n_ent, hi, ri, ti, known):
    """Y [B, n_ent]: 1 at the row's own true end and at every entity the known triples list for the row's query"""
    kh, kr, kt = known
    kept, own = (ti, hi) if neg_head else (hi, ti)
    kkept, kown = (kt, kh) if neg_head else (kh, kt)
    Y = np.zeros((len(hi), n_ent))
    Y[np.arange(len(hi)), own] = 1
    for i in range(len(hi)):
        Y[i, kown[(kkept == kept[i]) & (kr == ri[i])]] = 1
    return Y


def criterion(S, Y, w, smooth):
    """loss and dL/ds [B, n_ent]; softplus and sigma from one e = exp(-|s|)"""
    t = S.dtype.type
    e = np.exp(-np.abs(S))
    Yp = (t(1) - t(smooth)) * Y.astype(S.dtype) + t(smooth) / t(S.shape[1])
    l = (np.maximum(S, 0) + np.log1p(e) - Yp * S).sum(1)
    sig = np.where(S >= 0, t(1) / (t(1) + e), e / (t(1) + e))
    B = t(S.shape[0])
    return (w * l).sum() / B, (w / B)[:, None] * (sig - Yp)


def step(c, tables, batch, known, dtype=np.float64):
    """one step from (ent, ent_state, rel, rel_state), (h, r, t, w) and the index's triples: dict of loss, pos, g_rel and the four
    arrays after it"""
    ent, es, rel, rs = (np.array(x, dtype) for x in tables)
    hi, ri, ti = batch[:3]
    w = np.asarray(np.ones(len(hi)) if batch[3] is None else batch[3], dtype)
    lr, coef = dtype(LR), dtype(c.reg_coef)
    a, p = edge_terms(c.model, c.neg_head, ent[hi], rel[ri], ent[ti])
    loss, g = criterion(a @ ent.T, labels(c.neg_head, c.n_ent, hi, ri, ti, known), w, c.smooth)
    GA, dp = g @ ent, np.zeros(len(hi), dtype)                                           # the positive is a label like any other
    gh, gt, gr = edge_grads(c.model, c.neg_head, ent[hi], rel[ri], ent[ti], GA, dp)      # from the rows before the dense trace
    gr = gr + reg_grad(rel[ri], coef)
    _adagrad(ent, es, np.arange(ent.shape[0]), g.T @ a, lr)                              # 1. the dense trace
    ids = np.unique(np.concatenate([hi, ti]))                                            # 2. the positive entity trace
    G0 = reg_grad(ent[ids], coef)
    np.add.at(G0, np.searchsorted(ids, hi), gh)
    np.add.at(G0, np.searchsorted(ids, ti), gt)
    _adagrad(ent, es, ids, G0, lr)
    rids = np.unique(ri)                                                                 # 3. the relation trace (per-EDGE mean squares)
    GR = np.zeros((len(rids), rel.shape[1]), dtype)
    np.add.at(GR, np.searchsorted(rids, ri), gr)
    np.add.at(rs, ri, (gr * gr).mean(1))
    rel[rids] -= lr * GR / (np.sqrt(rs[rids]) + dtype(EPS))[:, None]
    return dict(loss=loss, pos=p, g_rel=gr, ent=ent, ent_state=es, rel=rel, rel_state=rs)


def inputs(c):
    """tables and batch as one_vs_all_cases.inputs makes them, and the index's triples (h, r, t) of the case's label kind"""
    tables, (hi, ri, ti, w) = V.inputs(V.Case(c.name, c.model, c.neg_head, c.n_ent, c.B, c.d, c.scores, c.reg_coef))
    kept, own = (ti, hi) if c.neg_head else (hi, ti)

    def query(row, ents):                                        # the triples that make `ents` the answers of the row's query
        ents = np.asarray(ents, np.int64)
        k, r = np.full(len(ents), kept[row]), np.full(len(ents), ri[row])
        return (ents, r, k) if c.neg_head else (k, r, ents)
    known = tuple(np.zeros(0, np.int64) for _ in range(3))
    if c.kind == 'edges':
        want = sorted(set(e for e in (0, 63, 64, 127, 128, c.n_ent - 1) if e < c.n_ent))
        known = query(0, want)
        assert np.flatnonzero(labels(c.neg_head, c.n_ent, hi[:1], ri[:1], ti[:1], known)[0]).tolist() == sorted(set(want + [own[0]]))
    elif c.kind == 'hub':                                        # rows 1 and 130: two row tiles, one list over every tile and split
        kept[130], ri[130] = kept[1], ri[1]
        known = query(1, np.arange(0, c.n_ent, 3))
    elif c.kind == 'dups':
        kept[2], ri[2] = kept[1], ri[1]
        hi[3] = ti[3] = 11
        known = (hi.copy(), ri.copy(), ti.copy())
    return tables, (hi, ri, ti, w), known
