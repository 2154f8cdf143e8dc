"""One SimplE / QuatE step under either all-entity criterion (kge_step_fused / kge_step_fused_known with N == 0) stated in numpy, and
the cases the tests run.  `step` is float64 by default; with dtype=np.float32 it is the float32 restatement whose error sets a case's
tolerance (test_gpu_clamp_quate.py).  Criteria and traces are those of one_vs_all_cases / k_vs_all_cases.  SimplE: rows [x_i | x_j],
relation rows [r | r_inv], raw = 1/2 sum(h_i r t_j + t_i r_inv h_j), s = clamp(raw, -20, 20), no gradient where |raw| >= 20.
QuatE: rows of four quarters, s = <x (x) r^, y> with r^ = r / |r| per quaternion.  It never calls the library."""
from collections import namedtuple

import numpy as np

import k_vs_all_cases as K
from one_vs_all_cases import EPS, LR, N_REL, _adagrad, reg_grad      # (N_REL: read by the tests)

CLAMP, MARGIN, SMOOTH = 20.0, 1e-3, 0.1
Case = namedtuple('Case', 'name model crit neg_head n_ent B d kind reg_coef')


def _c(model, crit, neg_head, n_ent, B, d, kind='plain', reg_coef=0.0):
    return Case('-'.join(map(str, (model, crit, 'head' if neg_head else 'tail', n_ent, B, d, kind))), model, crit, neg_head, n_ent, B, d, kind, reg_coef)


# d: one MFMA k-step, a ragged 32-k stage, past one 64-column group, a second column group of the GA kernel; B: inside a row tile, a
# ragged second one; n_ent: inside the owner's 64 rows, one past a column tile, several tiles with a ragged last one - each value per
# model, criterion and side.  dups: two edges share the true end, one has h == t; weights: edge weights and the regulariser
_SHAPES = {('ova', False): [(63, 16, 4), (129, 136, 36, 'weights', 1e-3), (300, 16, 68), (129, 136, 260)],
           ('ova', True): [(300, 136, 4), (63, 16, 36, 'dups'), (129, 136, 68), (300, 16, 260)],
           ('kva', False): [(129, 136, 4), (300, 16, 36, 'dups'), (63, 136, 68), (300, 16, 260)],
           ('kva', True): [(63, 16, 4), (300, 136, 36, 'weights', 1e-3), (129, 16, 68), (63, 136, 260)]}
CASES = [_c(m, crit, side, *shape) for m in ('SimplE', 'QuatE') for (crit, side), shapes in _SHAPES.items() for shape in shapes]


def qmul(x, y):
    (a, b, c, d), (e, f, g, h) = ([v[..., i, :] for i in range(4)] for v in (x, y))
    return np.stack([a * e - b * f - c * g - d * h, a * f + b * e + c * h - d * g, a * g - b * h + c * e + d * f,
                     a * h + b * g - c * f + d * e], -2)


def qconj(x):
    return x * np.array([1, -1, -1, -1], x.dtype)[:, None]


def edge(model, neg_head, h, r, t, u=None):
    """the operand a [B, d]; with u = dL/da + dL/d(raw p) y also the gradients (gx, gr) of the kept end's row and the relation row"""
    x, k, half = (t if neg_head else h), h.shape[1] // 2, h.dtype.type(0.5)
    if model == 'SimplE':                                        # a = 1/2 [r_inv x_j | r x_i] (tails), 1/2 [r x_j | r_inv x_i] (heads)
        xi, xj, c, s = x[:, :k], x[:, k:], r[:, :k], r[:, k:]
        c1, c2 = (c, s) if neg_head else (s, c)
        a = half * np.concatenate([c1 * xj, c2 * xi], 1)
        if u is None:
            return a
        g1, g2 = half * u[:, :k] * xj, half * u[:, k:] * xi      # dL/dc1, dL/dc2
        return a, half * np.concatenate([u[:, k:] * c2, u[:, :k] * c1], 1), np.concatenate([g1, g2] if neg_head else [g2, g1], 1)
    q = r.reshape(len(r), 4, -1)
    n = np.sqrt((q * q).sum(1, keepdims=True))
    ru, xq = q / n, x.reshape(q.shape)
    a = qmul(xq, qconj(ru) if neg_head else ru).reshape(h.shape)
    if u is None:
        return a
    uq = u.reshape(q.shape)
    g = qmul(qconj(xq), uq)                                      # dL/d(the second factor): r^ (tails) or conj(r^) (heads)
    g = qconj(g) if neg_head else g
    return a, qmul(uq, ru if neg_head else qconj(ru)).reshape(h.shape), ((g - ru * (ru * g).sum(1, keepdims=True)) / n).reshape(r.shape)


def forward(c, ent, rel, hi, ri, ti, w, known):
    """loss, clamped positive scores, operands, dL/d(raw scores) [B, n_ent], dL/d(raw p) [B], raw scores, raw p"""
    t, y = ent.dtype.type, ent[hi if c.neg_head else ti]
    a = edge(c.model, c.neg_head, ent[hi], rel[ri], ent[ti])
    R, rp = a @ ent.T, (a * y).sum(1)
    lim, B = t(CLAMP if c.model == 'SimplE' else np.inf), t(len(hi))
    S, p = np.clip(R, -lim, lim), np.clip(rp, -lim, lim)
    if c.crit == 'ova':
        m = S.max(1)
        lse = m + np.log(np.exp(S - m[:, None]).sum(1))
        loss, g, dp = (w * (lse - p)).sum() / B, (w / B)[:, None] * np.exp(S - lse[:, None]), -w / B
    else:
        loss, g = K.criterion(S, K.labels(c.neg_head, c.n_ent, hi, ri, ti, known), w, SMOOTH)
        dp = np.zeros(len(hi), ent.dtype)
    return loss, p, a, g * (np.abs(R) < lim), dp * (np.abs(rp) < lim), R, rp


def step(c, tables, batch, known, dtype=np.float64):
    """one step from (ent, ent_state, rel, rel_state), (h, r, t, w) and the index's triples"""
    ent, es, rel, rs = (np.array(x, dtype) for x in tables)
    hi, ri, ti = batch[:3]
    w = np.asarray(np.ones(len(hi)) if batch[3] is None else batch[3], dtype)
    lr, coef = dtype(LR), dtype(c.reg_coef)
    loss, p, a, g, dp, _, _ = forward(c, ent, rel, hi, ri, ti, w, known)
    y = ent[hi if c.neg_head else ti]
    _, gx, gr = edge(c.model, c.neg_head, ent[hi], rel[ri], ent[ti], g @ ent + dp[:, None] * y)      # from the rows before the dense trace
    gh, gt = (dp[:, None] * a, gx) if c.neg_head else (gx, dp[:, None] * a)
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
    """k_vs_all_cases.inputs: float32 tables with non-zero Adagrad states, the batch (h, r, t, w), and an index whose row 0 lists
    entities on both sides of every tile boundary.  SimplE: the tables are scaled (scores are cubic in the scale) until the raw scores
    reach +-60 and none lies within 2 MARGIN of the bound"""
    (ent, es, rel, rs), (hi, ri, ti, w), known = K.inputs(K.Case(c.name, c.model, c.neg_head, c.n_ent, c.B, c.d, 'edges', SMOOTH, c.reg_coef,
                                                                 c.kind))
    if c.model == 'SimplE':
        def scaled(f):                                           # as float32 holds them
            return (ent * np.float64(f)).astype(np.float32), (rel * np.float64(f)).astype(np.float32)

        def raw(f):
            e, r = (x.astype(np.float64) for x in scaled(f))
            return edge(c.model, c.neg_head, e[hi], r[ri], e[ti]) @ e.T
        f = (60.0 / np.abs(raw(1.0)).max()) ** (1.0 / 3.0)
        while np.abs(np.abs(raw(f)) - CLAMP).min() < 2 * MARGIN:
            f *= 1.001
        ent, rel = scaled(f)
    return (ent, es, rel, rs), (hi, ri, ti, w), known
