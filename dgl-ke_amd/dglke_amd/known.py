"""The known-triple index of link prediction with edge exclusion (ke_model.link_predict, exclude_mode 'mask' / 'exclude').

The reference asks its DGLGraph, result by result, whether an edge exists (models/ke_model.py:205-455, g.edge_ids in a Python
loop).  Here the attached graph becomes, once per corruption side and only when that side is first needed, what the ranking
evaluation already feeds its kernels (eval.sort_known_device): the unique (key, entity) pairs sorted by key, then entity -
key = h * R + r with tails as values (tail side), key = t * R + r with heads as values (head side).  16 bytes per known
triple and side stay on the device; a call then costs two searchsorted over its query rows (`ranges`: the per-row lists of
kge_topk_select_filtered) or one launch of kge_triples_known (`known`)."""
import numpy as np
import torch as th

from . import _lib
from . import eval as kge_eval
from ._lib import KgeError


def _host_col(x, n, what):
    a = np.ascontiguousarray(np.asarray(x.cpu() if isinstance(x, th.Tensor) else x).reshape(-1))
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise KgeError("attach_graph: %s ids must be integers (got %s)" % (what, a.dtype))
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= n):
        bad = int(a[(a < 0) | (a >= n)][0])
        raise KgeError("attach_graph: %s id %d is outside 0 .. %d" % (what, bad, n - 1))
    return a


class KnownIndex(object):
    """triples = (head, rel, tail) equal-length integer arrays / tensors; every id is range-checked on the host before
    anything reaches the device.  `dev` may be a CPU device for `side` and `ranges` (torch only); `known` is a kernel."""

    def __init__(self, triples, n_entities, n_relations, dev):
        if len(triples) != 3:
            raise KgeError("attach_graph: the graph is a triple (head, rel, tail) of id arrays")
        self.n_ent, self.n_rel, self.dev = int(n_entities), int(n_relations), th.device(dev)
        h, r, t = triples
        self.triples = (_host_col(h, self.n_ent, "head"), _host_col(r, self.n_rel, "relation"), _host_col(t, self.n_ent, "tail"))
        if not self.triples[0].shape == self.triples[1].shape == self.triples[2].shape:
            raise KgeError("attach_graph: head, rel and tail must have the same length")
        self._sides = {}

    def __len__(self):
        return int(self.triples[0].shape[0])

    def side(self, neg_head):
        """(keys, vals) of one corruption side, sorted on the device at the first use"""
        neg_head = bool(neg_head)
        if neg_head not in self._sides:
            kv = kge_eval.sort_known_device(self.triples, neg_head, self.n_rel, self.n_ent, self.dev)
            if kv is None:
                raise KgeError("the known-triple index needs entities x relations below 2^62")
            self._sides[neg_head] = (kv[0].contiguous(), kv[1].contiguous())
        return self._sides[neg_head]

    def ranges(self, neg_head, a_ids, r_ids):
        """[n, 2] int64: row i's list is vals[ranges[i, 0] : ranges[i, 1]] - the known tails of (a_i, r_i), or its known
        heads (neg_head).  a_ids, r_ids: int64 tensors on the index's device."""
        keys, _ = self.side(neg_head)
        return kge_eval.key_ranges(keys, a_ids * self.n_rel + r_ids)

    def filt_ids(self, neg_head):
        vals = self.side(neg_head)[1]
        return vals if vals.numel() else th.zeros(1, dtype=th.int64, device=self.dev)      # (never NULL for the library)

    def known(self, h, r, t):
        """uint8 [n]: 1 where (h_i, r_i, t_i) is a known triple (kge_triples_known on the tail side's index)"""
        keys, vals = self.side(False)
        n = h.numel()
        out = th.zeros(n, dtype=th.uint8, device=self.dev)
        if n and keys.numel():
            h, r, t = h.contiguous(), r.contiguous(), t.contiguous()
            _lib.check(_lib.lib().kge_triples_known(_lib.ptr(keys), _lib.ptr(vals), keys.numel(), self.n_rel, _lib.ptr(h),
                                                    _lib.ptr(r), _lib.ptr(t), n, _lib.ptr(out), _lib.stream_ptr()))
        return out
