"""The reference's second-generation inference API (python/dglke/models/ke_model.py:56-118, 457-641, 855-979): model classes
with load(), attach_graph(), link_predict() and embed_sim(), on the HIP score + top-K kernels of infer.py.

    m = TransE_l2Model(0, 12.0); m.load(path); m.attach_graph((head, rel, tail))
    m.link_predict(head=[..], rel=[..], exec_mode='batch_head', exclude_mode='exclude', topk=10)

link_predict returns a list of 5-tuples (head, rel, tail, score, mask) of numpy arrays - one for 'triplet_wise' and 'all', one
per head / relation / tail for the batch modes; mask is None unless exclude_mode == 'mask'.  'exclude' leaves the triples of
the attached graph out INSIDE the selection (kge_topk_select_filtered: no score block, no over-long candidate list, no host
loop over results), 'mask' flags them (kge_triples_known, one call for all groups).

The one signature difference: attach_graph takes the known triples - (head, rel, tail) id arrays of equal length, or an
object with `.train` of that shape (kgdataset.KGDataset) - where the reference takes a DGLGraph; etid_field / ntid_filed
are accepted and ignored.  The model classes score with the gamma they were constructed with under both sfunc values
(ke_model.py:868-893); everything else follows infer.py's stated differences (ties by position, NaN last, K <= 128, GPU
only, TransR refused, 'exclude' exact).  fit / save / eval are not supported, as in the reference.  The classes: TransE, TransE_l1,
TransE_l2, TransR (loads, refuses link_predict), DistMult, ComplEx, RotatE, RESCAL as in the reference, and SimplE, QuatE,
PairRE, TransH and TransD, which the reference does not have."""
import json
import os

import numpy as np
import torch as th

from . import _lib
from . import infer
from . import models
from ._lib import KgeError
from .infer import DEFAULT_INFER_BATCHSIZE
from .known import KnownIndex

EMB_INIT_EPS = 2.0
EXEC_MODES = ('triplet_wise', 'all', 'batch_head', 'batch_rel', 'batch_tail')


class BasicGEModel(object):
    """ke_model.py:56-853"""

    def __init__(self, device, model_name, score_func=None):
        self._g = None
        self._known = None
        self._model_name = model_name
        self.dev = self._device = infer.gpu_device(device)
        self._entity_emb = None
        self._relation_emb = None
        self._score_func = score_func            # (kept for signature parity: scoring is the library's)
        self._gamma = getattr(self, '_gamma', 0.0)
        self._emb_init = 1.0
        self.max_rows = None                     # rows in flight per call (None: from infer.WORKSPACE_BUDGET)

    def attach_graph(self, g, etid_field='tid', ntid_filed='ntid'):
        """g: (head, rel, tail) integer arrays / tensors of equal length, or an object with `.train` of that shape"""
        if self._entity_emb is None:
            raise KgeError("attach_graph needs the loaded model (the ids are checked against its tables): call load() first")
        trip = getattr(g, 'train', g)
        try:
            trip = tuple(trip)
        except TypeError:
            raise KgeError("attach_graph: the graph is a triple (head, rel, tail) of id arrays, or an object with .train")
        self._known = KnownIndex(trip, self.num_entity, self.num_rel, self.dev)
        self._g = g

    def _files(self, model_path):
        ef, rf = os.path.join(model_path, 'entity.npy'), os.path.join(model_path, 'relation.npy')
        cfg = os.path.join(model_path, 'config.json')
        if not (os.path.exists(ef) and os.path.exists(rf)) and os.path.exists(cfg):      # the trainer's own names
            with open(cfg) as f:
                c = json.load(f)
            stem = os.path.join(model_path, "%s_%s_" % (c['dataset'], c['model_name']))
            ef, rf = stem + 'entity.npy', stem + 'relation.npy'
        return ef, rf

    @infer.on_device
    def load(self, model_path):
        """entity.npy and relation.npy in model_path (ke_model.py:861-866)"""
        ef, rf = self._files(model_path)
        put = lambda f: th.from_numpy(np.load(f).astype(np.float32)).contiguous().to(self.dev)
        ent, rel = put(ef), put(rf)
        self._entity_emb, self._relation_emb = ent, rel.reshape(rel.shape[0], -1)
        self._known = self._g = None
        self._after_load()

    def _after_load(self):
        pass

    def save(self, model_path):
        raise KgeError("Not support training now")

    def fit(self):
        raise KgeError("Not support training now")

    def eval(self):
        raise KgeError("Not support evaluation now")

    def link_predict(self, head=None, rel=None, tail=None, exec_mode='all', sfunc='none', topk=10, exclude_mode=None,
                     batch_size=DEFAULT_INFER_BATCHSIZE):
        """ke_model.py:457-641.  Returns a list of (head, rel, tail, score, mask) numpy tuples."""
        if self._model_name == 'TransR':
            raise KgeError("TransR has no inference path (the reference's TransRScore.infer is empty too)")
        if sfunc not in ('none', 'logsigmoid'):
            raise KgeError("score function should be none or logsigmoid (got %r)" % (sfunc,))
        if exec_mode not in EXEC_MODES:
            raise KgeError("unknown execution mode %r" % (exec_mode,))
        if exclude_mode not in (None, 'mask', 'exclude'):
            raise KgeError("exclude_mode should be None, 'mask' or 'exclude' (got %r)" % (exclude_mode,))
        if exclude_mode is not None and self._known is None:
            raise KgeError("exclude_mode %r needs the known triples: call attach_graph() first" % (exclude_mode,))
        if self._entity_emb is None:
            raise KgeError("link_predict needs a loaded model: call load() first")
        k = infer.check_k(topk)
        head, tail = infer.host_ids(head, self.num_entity, "head"), infer.host_ids(tail, self.num_entity, "tail")
        rel = infer.host_ids(rel, self.num_rel, "relation")
        return self._predict(head, rel, tail, exec_mode, sfunc, k, exclude_mode)

    @infer.on_device
    def _predict(self, head, rel, tail, exec_mode, sfunc, k, exclude_mode):
        out = th.nn.functional.logsigmoid if sfunc == 'logsigmoid' else (lambda s: s)
        return infer.predict_topk(_lib.model_id(self._model_name), self._entity_emb, self._relation_emb, float(self._gamma),
                                  float(self._emb_init), out, head, rel, tail, exec_mode, k, self.max_rows, self._known,
                                  exclude_mode)

    def embed_sim(self, left=None, right=None, embed_type='entity', sfunc='cosine', bcast=False, pair_ws=False, topk=10):
        """ke_model.py:754-829: top-K similar (left, right) pairs of the entity or the relation table"""
        if embed_type not in ('entity', 'relation'):
            raise KgeError("emb should entity or relation (got %r)" % (embed_type,))
        emb = self.entity_embed if embed_type == 'entity' else self.relation_embed
        if emb is None:
            raise KgeError("embed_sim needs a loaded model: call load() first")
        return infer.EmbSimInfer.from_tensor(self.dev, emb, sfunc).topK(left, right, bcast=bcast, pair_ws=pair_ws, k=topk)

    @property
    def model_name(self):
        return self._model_name

    @property
    def entity_embed(self):
        return self._entity_emb

    @property
    def relation_embed(self):
        return self._relation_emb

    @property
    def num_entity(self):
        return -1 if self.entity_embed is None else self.entity_embed.shape[0]

    @property
    def num_rel(self):
        return -1 if self.relation_embed is None else self.relation_embed.shape[0]

    @property
    def graph(self):
        return self._g


def _check_loaded_widths(self):
    """the loaded tables against the width rule of the model's record (models.py)"""
    m, d_e, d_r = models.MODELS[self._model_name], self._entity_emb.shape[1], self._relation_emb.shape[1]
    if not models.widths_ok(m, d_e, d_r):
        raise KgeError(m.loaded_text % (d_e, d_r))


class KGEModel(BasicGEModel):
    """ke_model.py:855-866"""

    def __init__(self, device, model_name, score_func=None):
        super(KGEModel, self).__init__(device, model_name, score_func)


class TransEModel(KGEModel):
    def __init__(self, device, gamma):
        self._gamma = gamma
        super(TransEModel, self).__init__(device, 'TransE')


class TransE_l2Model(KGEModel):
    def __init__(self, device, gamma):
        self._gamma = gamma
        super(TransE_l2Model, self).__init__(device, 'TransE_l2')


class TransE_l1Model(KGEModel):
    def __init__(self, device, gamma):
        self._gamma = gamma
        super(TransE_l1Model, self).__init__(device, 'TransE_l1')


class TransRModel(KGEModel):
    """loads like the others; link_predict refuses (the reference's TransRScore.infer is `pass`)"""

    def __init__(self, device, gamma):
        self._gamma = gamma
        super(TransRModel, self).__init__(device, 'TransR')


class DistMultModel(KGEModel):
    def __init__(self, device):
        super(DistMultModel, self).__init__(device, 'DistMult')


class ComplExModel(KGEModel):
    def __init__(self, device):
        super(ComplExModel, self).__init__(device, 'ComplEx')


class SimplEModel(KGEModel):
    """(not among the reference's classes; the kernels have the score)"""

    def __init__(self, device):
        super(SimplEModel, self).__init__(device, 'SimplE')


class QuatEModel(KGEModel):
    """(not among the reference's classes) QuatE: rows are four quarters of quaternion components, the relation row as wide as
    the entity row and normalised per quaternion inside the kernels (include/kge_hip.h, enum kge_model)"""

    def __init__(self, device):
        super(QuatEModel, self).__init__(device, 'QuatE')

    _after_load = _check_loaded_widths


class PairREModel(KGEModel):
    """(not among the reference's classes) PairRE: relation rows [rH | rT], twice as wide as the entity rows, which the kernels
    normalise to unit length; score = gamma - |h^ o rH - t^ o rT|_1 (include/kge_hip.h, enum kge_model)"""

    def __init__(self, device, gamma):
        self._gamma = gamma
        super(PairREModel, self).__init__(device, 'PairRE')

    _after_load = _check_loaded_widths


class TransHModel(KGEModel):
    """(not among the reference's classes) TransH: relation rows [d | w], twice as wide as the entity rows; both ends are projected
    onto the hyperplane of normal w and score = gamma - |h_perp + d - t_perp|_2 (include/kge_hip.h, enum kge_model)"""

    def __init__(self, device, gamma):
        self._gamma = gamma
        super(TransHModel, self).__init__(device, 'TransH')

    _after_load = _check_loaded_widths


class TransDModel(KGEModel):
    """(not among the reference's classes) TransD: entity rows [e | e_p] and relation rows [r | r_p] of the same width; both ends go
    through the relation's rank-one map x + (x_p . x) r_p and score = gamma - |h_perp + r - t_perp|_2 (include/kge_hip.h, enum
    kge_model)"""

    def __init__(self, device, gamma):
        self._gamma = gamma
        super(TransDModel, self).__init__(device, 'TransD')

    _after_load = _check_loaded_widths


class RESCALModel(KGEModel):
    """relation rows are entity_dim x entity_dim matrices (ke_model.py:935-938)"""

    def __init__(self, device):
        super(RESCALModel, self).__init__(device, 'RESCAL')

    def _after_load(self):
        d = self._entity_emb.shape[1]
        if self._relation_emb.shape[1] != d * d:
            raise KgeError("RESCAL: relation rows of %d values do not fit entity_dim %d" % (self._relation_emb.shape[1], d))


class RotatEModel(KGEModel):
    def __init__(self, device, gamma):
        self._gamma = gamma
        super(RotatEModel, self).__init__(device, 'RotatE')

    def _after_load(self):
        self._emb_init = (self._gamma + EMB_INIT_EPS) / (self._entity_emb.shape[1] // 2)      # ke_model.py:949-955


class GNNModel(BasicGEModel):
    """ke_model.py:957-978: a general-purpose score over externally produced embeddings"""

    def __init__(self, device, model_name, gamma=0):
        if model_name not in ('TransE', 'TransE_l2', 'TransE_l1', 'DistMult'):
            raise KgeError("For general purpose Scoring function for GNN, we only support TransE_l1, TransE_l2 "
                           "DistMult, but {} is given.".format(model_name))
        self._gamma = gamma
        super(GNNModel, self).__init__(device, model_name)
