"""One TuckER step (include/kge_hip.h, KGE_TUCKER) under either all-entity criterion stated in numpy einsum, and the cases the tests run.

`step` is the statement: float64 by default; with dtype=np.float32 the float32 restatement of the same formulas, whose error against
the float64 result sets the tolerance of a case (test_gpu_tucker.py).  The criteria and the three entity-side and relation-side
updates are those of one_vs_all_cases / k_vs_all_cases.  It never calls the library."""
import zlib
from collections import namedtuple

import numpy as np

import k_vs_all_cases as K
import one_vs_all_cases as V
from one_vs_all_cases import EPS, LR, N_REL, _adagrad, reg_grad

Case = namedtuple('Case', 'name crit neg_head n_ent B d_e d_r kind reg_coef')


def _c(crit, neg_head, n_ent, B, d_e, d_r, kind='plain', reg_coef=0.0):
    return Case('%s-%s-n%d-B%d-de%d-dr%d-%s' % (crit, 'head' if neg_head else 'tail', n_ent, B, d_e, d_r, kind), crit, neg_head, n_ent, B,
                d_e, d_r, kind, reg_coef)


# d_e: the minimum, a ragged k-stage, one owner group per l, one plus a ragged one, the owner kernel's 5-block instance and two column
# groups of the operand kernel.  (d_e, d_r) -> parts of the operand kernel = l ranges of the backward kernel (tk_geom: at least
# ceil(256 / d_e) values of l each): (4, *) 1, (36, 12) 2 (8 + 4: ragged), (36, 36) 5 (ragged), (64, 12) 3, (68, 36) 9, (260, 4) 4.
# Every value of d_e, d_r, B and n_ent once per side and per criterion; weights: edge weights and the regulariser; dups: two edges share
# the relation and the kept end; big: core entries scaled so that scores reach +-80
CASES = [
    _c('ova', False, 63, 16, 4, 4), _c('ova', False, 129, 136, 36, 12, 'weights', 1e-3), _c('ova', False, 300, 128, 64, 36, 'big'),
    _c('ova', False, 63, 136, 68, 12), _c('ova', False, 129, 16, 260, 4),
    _c('ova', True, 300, 128, 4, 36), _c('ova', True, 129, 16, 36, 12, 'dups'), _c('ova', True, 63, 16, 64, 4),
    _c('ova', True, 129, 136, 68, 36), _c('ova', True, 300, 128, 260, 12),
    _c('kva', False, 63, 136, 4, 12), _c('kva', False, 129, 16, 36, 12, 'dups'), _c('kva', False, 300, 128, 64, 12, 'big'),
    _c('kva', False, 63, 128, 68, 36), _c('kva', False, 129, 136, 260, 4),
    _c('kva', True, 300, 136, 4, 4), _c('kva', True, 129, 136, 36, 36, 'weights', 1e-3), _c('kva', True, 63, 16, 64, 36),
    _c('kva', True, 129, 128, 68, 4), _c('kva', True, 300, 16, 260, 12),
]
DETERMINISM = CASES[1]
SMOOTH = 0.1


def operand(neg_head, x, r, W):
    return np.einsum('il,ik,lkm->im', r, x, W) if not neg_head else np.einsum('il,im,lkm->ik', r, x, W)


def edge_grads(neg_head, x, r, W, u):
    """GX, GR, GW from u = GA + dp y"""
    if not neg_head:
        return np.einsum('il,lkm,im->ik', r, W, u), np.einsum('ik,lkm,im->il', x, W, u), np.einsum('il,ik,im->lkm', r, x, u)
    return np.einsum('il,lkm,ik->im', r, W, u), np.einsum('ik,lkm,im->il', u, W, x), np.einsum('il,ik,im->lkm', r, u, x)


def loss_and_g(c, a, p, ent, hi, ri, ti, w, known):
    """loss, dL/ds [B, n_ent], dL/dp [B] of the case's criterion"""
    S = a @ ent.T
    B = ent.dtype.type(len(hi))
    if c.crit == 'ova':
        m = S.max(1)
        lse = m + np.log(np.exp(S - m[:, None]).sum(1))
        return (w * (lse - p)).sum() / B, (w / B)[:, None] * np.exp(S - lse[:, None]), -w / B
    loss, g = K.criterion(S, K.labels(c.neg_head, c.n_ent, hi, ri, ti, known), w, SMOOTH)
    return loss, g, np.zeros(len(hi), ent.dtype)


def step(c, tables, batch, known, dtype=np.float64):
    """one step from (ent, ent_state, rel, rel_state, core [d_r, d_e, d_e], core_state [d_r d_e]), (h, r, t, w) and the index's triples"""
    ent, es, rel, rs, W, ws = (np.array(x, dtype) for x in tables)
    hi, ri, ti = batch[:3]
    w = np.asarray(np.ones(len(hi)) if batch[3] is None else batch[3], dtype)
    lr, coef = dtype(LR), dtype(c.reg_coef)
    xi, yi = (ti, hi) if c.neg_head else (hi, ti)
    x, y, r = ent[xi], ent[yi], rel[ri]
    a = operand(c.neg_head, x, r, W)
    p = (a * y).sum(1)
    loss, g, dp = loss_and_g(c, a, p, ent, hi, ri, ti, w, known)
    u = g @ ent + dp[:, None] * y
    gx, gr, gw = edge_grads(c.neg_head, x, r, W, u)                                      # from the values before the step
    gy = dp[:, None] * a
    gh, gt = (gy, gx) if c.neg_head else (gx, gy)
    gr = gr + reg_grad(r, coef)
    W2, gw2 = W.reshape(-1, c.d_e), gw.reshape(-1, c.d_e)                                # 1. the dense core update
    _adagrad(W2, ws, np.arange(W2.shape[0]), gw2, lr)
    _adagrad(ent, es, np.arange(ent.shape[0]), g.T @ a, lr)                              # 2. the dense entity trace
    ids = np.unique(np.concatenate([hi, ti]))                                            # 3. the positive entity trace
    G0 = reg_grad(ent[ids], coef)
    np.add.at(G0, np.searchsorted(ids, hi), gh)
    np.add.at(G0, np.searchsorted(ids, ti), gt)
    _adagrad(ent, es, ids, G0, lr)
    rids = np.unique(ri)                                                                 # 4. the relation trace (per-EDGE mean squares)
    GR = np.zeros((len(rids), rel.shape[1]), dtype)
    np.add.at(GR, np.searchsorted(rids, ri), gr)
    np.add.at(rs, ri, (gr * gr).mean(1))
    rel[rids] -= lr * GR / (np.sqrt(rs[rids]) + dtype(EPS))[:, None]
    return dict(loss=loss, pos=p, g_rel=gr, ent=ent, ent_state=es, rel=rel, rel_state=rs, core=W2, core_state=ws)


def inputs(c):
    """tables (float32; non-zero Adagrad states), the batch (h, r, t, w) and the K-vs-all index's triples of a case"""
    rng = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7fffffff)
    se, sr = 1.5 / np.sqrt(np.sqrt(c.d_e)), 1.5 / np.sqrt(np.sqrt(c.d_r))
    ent, rel = rng.uniform(-se, se, (c.n_ent, c.d_e)), rng.uniform(-sr, sr, (N_REL, c.d_r))
    W = rng.uniform(-1, 1, (c.d_r, c.d_e, c.d_e)) / np.sqrt(c.d_r * c.d_e)
    hi, ti, ri = rng.randint(0, c.n_ent, c.B), rng.randint(0, c.n_ent, c.B), rng.randint(0, N_REL, c.B)
    kept = ti if c.neg_head else hi
    if c.kind == 'dups':
        kept[2], ri[2] = kept[1], ri[1]
        hi[3] = ti[3] = 11
    if c.kind == 'big':
        W *= 80.0 / np.abs(operand(c.neg_head, ent[kept], rel[ri], W) @ ent.T).max()
    w = rng.uniform(0.5, 2.0, c.B).astype(np.float32) if c.kind == 'weights' else None
    es, rs = rng.uniform(1e-8, 1e-6, c.n_ent), rng.uniform(1e-4, 1e-3, N_REL)
    ws = rng.uniform(1e-8, 1e-6, c.d_r * c.d_e)
    known = tuple(np.zeros(0, np.int64) for _ in range(3))
    if c.crit == 'kva':                                          # row 0's query lists entities on both sides of every tile boundary
        ents = np.array(sorted(set(e for e in (0, 63, 64, 127, 128, c.n_ent - 1) if e < c.n_ent)), np.int64)
        k, r = np.full(len(ents), kept[0]), np.full(len(ents), ri[0])
        known = (ents, r, k) if c.neg_head else (k, r, ents)
    return tuple(v.astype(np.float32) for v in (ent, es, rel, rs, W, ws)), (hi, ri, ti, w), known
