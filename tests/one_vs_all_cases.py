"""The 1-vs-all softmax step (include/kge_hip.h, kge_step_fused on a batch with N == 0) stated in numpy, and the cases the tests run.

`step` is the statement: float64 by default; with dtype=np.float32 it is the plain float32 restatement of the same formulas in the
same order, whose error against the float64 result sets the tolerance of a case (test_gpu_one_vs_all.py).  It never calls the
library."""
import zlib
from collections import namedtuple

import numpy as np

LR, EPS, N_REL = 0.1, 1e-10, 5
Case = namedtuple('Case', 'name model neg_head n_ent B d kind reg_coef')


def _c(model, neg_head, n_ent, B, d, kind='plain', reg_coef=0.0):
    return Case('%s-%s-n%d-B%d-d%d-%s' % (model, 'head' if neg_head else 'tail', n_ent, B, d, kind), model, neg_head, n_ent, B, d, kind,
                reg_coef)


# n_ent: one owner tile (64) and one column tile (128), each +-1, and 300 (ragged last split); B: below a row tile, one, one plus a
# ragged second; d: the minimum, a last k-stage with a tail, two full stages - each value at least once with each model, both sides
CASES = [
    _c('DistMult', False, 63, 16, 4), _c('DistMult', True, 64, 128, 36), _c('DistMult', False, 65, 136, 64),
    _c('DistMult', True, 127, 16, 36), _c('DistMult', False, 129, 128, 64), _c('DistMult', True, 300, 136, 4),
    _c('ComplEx', True, 63, 128, 36), _c('ComplEx', False, 64, 136, 64), _c('ComplEx', True, 65, 16, 4),
    _c('ComplEx', False, 127, 136, 36), _c('ComplEx', True, 129, 16, 64), _c('ComplEx', False, 300, 128, 4),
    # rows wider than 256 floats: two column groups in the GA kernel; the owner kernel's widest instance
    _c('DistMult', True, 65, 16, 260), _c('ComplEx', False, 63, 16, 512),
    _c('DistMult', False, 129, 16, 36, 'dups'),                  # two edges share the true end, one edge has h == t
    _c('ComplEx', True, 65, 136, 36, 'weights', 1e-3),           # edge weights, and the regulariser
    _c('DistMult', True, 300, 128, 64, 'big'),                   # scores reach +-80
]
DETERMINISM = _c('ComplEx', False, 129, 136, 36)


def reg_grad(x, coef):
    return 3 * coef * x * np.abs(x)                              # d/dx coef |x|^3


def edge_terms(model, neg_head, h, r, t):
    """(a, p): the per-edge operand and the positive score"""
    if model == 'DistMult':
        return (t if neg_head else h) * r, (h * r * t).sum(1)
    k = h.shape[1] // 2
    rh, ih, rt, it, c, s = h[:, :k], h[:, k:], t[:, :k], t[:, k:], r[:, :k], r[:, k:]
    p = ((rh * c - ih * s) * rt + (rh * s + ih * c) * it).sum(1)
    if neg_head:                                                 # a = t o conj(r)
        return np.concatenate([rt * c + it * s, it * c - rt * s], 1), p
    return np.concatenate([rh * c - ih * s, rh * s + ih * c], 1), p


def edge_grads(model, neg_head, h, r, t, GA, dp):
    """per-edge gradients of the h, t and r rows from dL/da and dL/dp"""
    dp = dp[:, None]
    if model == 'DistMult':
        gh, gt, gr = dp * r * t, dp * h * r, dp * h * t
        if neg_head:
            return gh, gt + GA * r, gr + GA * t
        return gh + GA * r, gt, gr + GA * h
    k = h.shape[1] // 2
    rh, ih, rt, it, c, s = h[:, :k], h[:, k:], t[:, :k], t[:, k:], r[:, :k], r[:, k:]
    g1, g2 = GA[:, :k], GA[:, k:]
    v_rh, v_ih = dp * (rt * c + it * s), dp * (it * c - rt * s)
    v_rt, v_it = dp * (rh * c - ih * s), dp * (ih * c + rh * s)
    v_rr, v_ir = dp * (rh * rt + ih * it), dp * (rh * it - ih * rt)
    if neg_head:
        v_rt, v_it = v_rt + g1 * c - g2 * s, v_it + g1 * s + g2 * c
        v_rr, v_ir = v_rr + g1 * rt + g2 * it, v_ir + g1 * it - g2 * rt
    else:
        v_rh, v_ih = v_rh + g1 * c + g2 * s, v_ih - g1 * s + g2 * c
        v_rr, v_ir = v_rr + g1 * rh + g2 * ih, v_ir - g1 * ih + g2 * rh
    return np.concatenate([v_rh, v_ih], 1), np.concatenate([v_rt, v_it], 1), np.concatenate([v_rr, v_ir], 1)


def forward(model, neg_head, ent, rel, hi, ri, ti, w):
    """loss, positive scores, operands, dL/ds [B, n_ent]"""
    a, p = edge_terms(model, neg_head, ent[hi], rel[ri], ent[ti])
    S = a @ ent.T
    m = S.max(1)
    lse = m + np.log(np.exp(S - m[:, None]).sum(1))
    B = ent.dtype.type(len(hi))
    loss = (w * (lse - p)).sum() / B
    return loss, p, a, (w / B)[:, None] * np.exp(S - lse[:, None])


def _adagrad(rows, state, ids, G, lr):
    state[ids] += (G * G).mean(1)
    rows[ids] -= lr * G / (np.sqrt(state[ids]) + rows.dtype.type(EPS))[:, None]


def step(c, tables, batch, dtype=np.float64):
    """one step from (ent, ent_state, rel, rel_state) and (h, r, t, w): dict of loss, pos, g_rel and the four arrays after it"""
    ent, es, rel, rs = (np.array(x, dtype) for x in tables)
    hi, ri, ti = batch[:3]
    w = np.asarray(np.ones(len(hi)) if batch[3] is None else batch[3], dtype)
    lr, coef = dtype(LR), dtype(c.reg_coef)
    loss, p, a, g = forward(c.model, c.neg_head, ent, rel, hi, ri, ti, w)
    GA, dp = g @ ent, -w / dtype(len(hi))
    gh, gt, gr = edge_grads(c.model, c.neg_head, ent[hi], rel[ri], ent[ti], GA, dp)      # from the rows before the dense trace
    gr = gr + reg_grad(rel[ri], coef)
    _adagrad(ent, es, np.arange(ent.shape[0]), g.T @ a, lr)                              # 1. the dense trace
    ids = np.unique(np.concatenate([hi, ti]))                                            # 2. the positive entity trace
    G0 = reg_grad(ent[ids], coef)
    np.add.at(G0, np.searchsorted(ids, hi), gh)
    np.add.at(G0, np.searchsorted(ids, ti), gt)
    _adagrad(ent, es, ids, G0, lr)
    rids = np.unique(ri)                                                                 # 3. the relation trace
    GR = np.zeros((len(rids), rel.shape[1]), dtype)                                      # (per-EDGE rows: the state takes every
    np.add.at(GR, np.searchsorted(rids, ri), gr)                                         #  edge's own mean square, as the update
    np.add.at(rs, ri, (gr * gr).mean(1))                                                 #  launch and the reference's trace do)
    rel[rids] -= lr * GR / (np.sqrt(rs[rids]) + dtype(EPS))[:, None]
    return dict(loss=loss, pos=p, g_rel=gr, ent=ent, ent_state=es, rel=rel, rel_state=rs)


def inputs(c):
    """tables (float32, non-zero Adagrad state of the size of the step's mean squares) and the batch (h, r, t, w) of a case"""
    rng = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7fffffff)
    sc = 1.5 / np.sqrt(np.sqrt(c.d))
    ent = rng.uniform(-sc, sc, (c.n_ent, c.d))
    rel = rng.uniform(-sc, sc, (N_REL, c.d))
    hi, ti, ri = rng.randint(0, c.n_ent, c.B), rng.randint(0, c.n_ent, c.B), rng.randint(0, N_REL, c.B)
    if c.kind == 'dups':
        (hi if c.neg_head else ti)[[1, 2]] = 7
        hi[3] = ti[3] = 11
    if c.kind == 'big':                                          # scores are cubic in the rows' scale
        _, _, a, _ = forward(c.model, c.neg_head, ent, rel, hi, ri, ti, np.ones(c.B))
        f = (80.0 / np.abs(a @ ent.T).max()) ** (1.0 / 3.0)
        ent, rel = ent * f, rel * f
    w = rng.uniform(0.5, 2.0, c.B).astype(np.float32) if c.kind == 'weights' else None
    es, rs = rng.uniform(1e-8, 1e-6, c.n_ent), rng.uniform(1e-4, 1e-3, N_REL)
    return tuple(x.astype(np.float32) for x in (ent, es, rel, rs)), (hi, ri, ti, w)
