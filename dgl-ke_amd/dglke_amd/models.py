"""The model table: one record per --model_name value, every fact the Python side knows about a model.  The C side keeps the
same facts in csrc/kge_models.hpp; the kernels and the semantics are described in include/kge_hip.h (enum kge_model).

Nothing here touches a device or imports the library: _lib, the command lines, the engine and the model classes read it."""
from collections import OrderedDict, namedtuple

Model = namedtuple('Model', [
    'name', 'id',
    'score', 'score_args',         # the class of score_fun.py and its arguments ('gamma' / 'emb_init': KEModel's values; else literal)
    'ent_multiple', 'rel_width',   # the width rule: d_e a positive multiple of ent_multiple, d_r == rel_width(d_e) (None: no rule here)
    'de', 'dr',                    # -de / -dr on the command lines: True required, False forbidden, 'tied' both or neither, None free
    'flags_text',                  # ... the text for breaking that: %(de)s " -de" / " no -de", %(dr)s " -dr" / ", no -dr", %(cdr)s ", -dr" / ", no -dr"
    'cli_multiple', 'cli_of',      # 'hidden_dim': --hidden_dim >= and a multiple of cli_multiple; 'width': the entity width a multiple of it
    'multiple_text',               # ... the text: %(x2)s " x 2 with -de" or "", %(width)d, %(hidden)d
    'multiple_first',              # the multiple is checked in front of the flags
    'kemodel_text', 'engine_text', 'loaded_text',     # the width rule's text in general_models.KEModel, engine.StepEngine, ke_model (d_e, d_r)
    'single_gpu_only',             # strict step on local tables: no --gpu list, no sharded tables
    'no_stale_pipeline',           # not in --async_update_pipeline / --async_update_rel
    'no_relation_ranking',         # None, or why --eval_relation does not apply
    'no_relation_ranking_lib',     # ... in the words of eval.relation_ranks
    'rank_cands', 'topk_row',      # workspace facts: candidates a rank / top-K workspace is sized for per candidate; floats per top-K query row
    'rank_rel_as',                 # relation ranking takes this model's workspace layout followed by the normalised relation table
    'norm_ent', 'norm_rel',        # --ent_norm / --rel_norm: equal slices of an entity / relation row, each projected on its own (norm_rel 0: refused)
    'norm_rel_unit',               # ... bit k: relation slice k is normalised to length 1 under either relation mode (TransH's w)
    'no_rel_norm',                 # ... None, or why --rel_norm does not apply
    'projection', 'relation_matrix', 'alias_of'])     # TransR's third table; RESCAL's relation rows are matrices; TransE is TransE_l2


def _model(name, id, score, score_args=(), **kw):
    d = dict.fromkeys(Model._fields)
    d.update(name=name, id=id, score=score, score_args=score_args, rank_cands=1, topk_row=lambda d_e: d_e, multiple_first=False,
             single_gpu_only=False, no_stale_pipeline=False, projection=False, relation_matrix=False, norm_ent=1, norm_rel=1,
             norm_rel_unit=0)
    d.update(kw)
    return Model(**d)


_LOCAL = dict(single_gpu_only=True, no_stale_pipeline=True)
_OWN_REL = dict(norm_rel=0, no_rel_norm="its relation-side tables are updated by kernels of their own")
_TWO_PROJECTIONS = dict(no_relation_ranking="the relation row enters through two projections",
                        no_relation_ranking_lib="the relation row enters through two projections: no relation ranking")

MODELS = OrderedDict((m.name, m) for m in (       # in the order of the --model_name choices
    _model('TransE', 1, 'TransEScore', ('gamma', 'l2'), alias_of='TransE_l2'),
    _model('TransE_l1', 0, 'TransEScore', ('gamma', 'l1')),
    _model('TransE_l2', 1, 'TransEScore', ('gamma', 'l2')),
    _model('TransR', 7, 'TransRScore', projection=True, **_OWN_REL),
    _model('RESCAL', 6, 'RESCALScore', relation_matrix=True, **_OWN_REL),
    _model('DistMult', 2, 'DistMultScore'),
    _model('ComplEx', 3, 'ComplExScore'),
    _model('RotatE', 4, 'RotatEScore', ('gamma', 'emb_init'), norm_rel=0, no_rel_norm="the row holds phases"),
    _model('SimplE', 5, 'SimplEScore'),
    _model('QuatE', 8, 'QuatEScore', ent_multiple=4, rel_width=lambda d_e: d_e, de='tied', dr='tied',
           flags_text="QuatE: the relation width must equal the entity width: pass -dr together with -de (and neither alone)",
           cli_multiple=4, cli_of='width', multiple_first=True,
           multiple_text="QuatE: the entity width (--hidden_dim%(x2)s = %(width)d) must be a multiple of 4 (four quarters [a | b | c | d])",
           kemodel_text="QuatE needs an entity width that is a multiple of 4 and relation_dim == entity_dim (got %d, %d)",
           engine_text="QuatE needs an entity width that is a multiple of 4 and relation width == entity width (got %d, %d)",
           loaded_text="QuatE: rows of %d (entity) and %d (relation) values: the width must be a multiple of 4 and the same for both",
           rank_rel_as='DistMult', **_LOCAL),
    _model('PairRE', 10, 'PairREScore', ('gamma',), ent_multiple=1, rel_width=lambda d_e: 2 * d_e, de=False, dr=True,
           flags_text="PairRE: the relation row [rH | rT] is twice as wide as the entity row: pass -dr without -de (got%(de)s%(dr)s)",
           kemodel_text="PairRE needs relation_dim == 2 * entity_dim, r = [rH | rT] (got %d, %d)",
           engine_text="PairRE needs relation width == 2 * entity width (-dr without -de; got %d, %d)",
           loaded_text="PairRE: rows of %d (entity) and %d (relation) values: the relation row must be twice as wide",
           no_relation_ranking="the score is not a product with the relation row",
           no_relation_ranking_lib="the score is not a product of a query row and the relation row: no relation ranking",
           topk_row=lambda d_e: 2 * d_e, norm_rel=2, **_LOCAL),                           # [rH | rT]
    _model('TransH', 12, 'TransHScore', ('gamma',), ent_multiple=4, rel_width=lambda d_e: 2 * d_e, de=False, dr=True,
           flags_text="TransH: the relation row [d | w] is twice as wide as the entity row: pass -dr without -de (got%(de)s%(dr)s)",
           cli_multiple=4, cli_of='hidden_dim', multiple_text="TransH: --hidden_dim must be a multiple of 4 (got %(hidden)d)",
           kemodel_text="TransH needs an entity width that is a multiple of 4 and relation_dim == 2 * entity_dim, r = [d | w] (got %d, %d)",
           engine_text="TransH needs an entity width that is a multiple of 4 and relation width == 2 * entity width "
                       "(-dr without -de; got %d, %d)",
           loaded_text="TransH: rows of %d (entity) and %d (relation) values: the entity width must be a multiple of 4 and the "
                       "relation row twice as wide",
           topk_row=lambda d_e: 2 * d_e + 1, norm_rel=2, norm_rel_unit=2,                 # [d | w], |w| = 1
           **dict(_LOCAL, **_TWO_PROJECTIONS)),
    _model('TransD', 14, 'TransDScore', ('gamma',), ent_multiple=8, rel_width=lambda d_e: d_e, de=True, dr=True,
           flags_text="TransD: entity rows [e | e_p] and relation rows [r | r_p] are both twice --hidden_dim: pass -de and -dr "
                      "(got%(de)s%(cdr)s)",
           cli_multiple=4, cli_of='hidden_dim', multiple_text="TransD: --hidden_dim must be a multiple of 4 (got %(hidden)d)",
           kemodel_text="TransD needs entity_dim == relation_dim, rows [x | x_p] of two halves that are multiples of 4 (got %d, %d)",
           engine_text="TransD needs entity and relation rows of the same width, two halves of a multiple of 4 each "
                       "(-de and -dr, --hidden_dim %% 4 == 0; got %d, %d)",
           loaded_text="TransD: rows of %d (entity) and %d (relation) values: both must be [x | x_p], the same width and a multiple of 8",
           rank_cands=2, topk_row=lambda d_e: d_e + 2, norm_ent=2, norm_rel=2,            # [e | e_p], [r | r_p]
           **dict(_LOCAL, **_TWO_PROJECTIONS)),
))
NAMES = list(MODELS)                                                 # the --model_name choices
DEFAULT = 'TransE'                                                   # ... and its default
MODEL_IDS = dict((m.name, m.id) for m in MODELS.values())            # (ids 9, 11 and 13 are not models)
BY_ID = dict((m.id, m) for m in MODELS.values() if not m.alias_of)


def widths_ok(m, d_e, d_r):
    """the width rule of a record (True where it has none: the older models' rules live in the library and in KEModel)"""
    return m.rel_width is None or (d_e >= m.ent_multiple and d_e % m.ent_multiple == 0 and d_r == m.rel_width(d_e))


def own_relation_update(m):
    """TransR and RESCAL update their relation-side tables (projection matrices, relation matrices) with kernels of their own: no
    update pipeline, no Adam, and on several GPUs those tables stay with the trainer that holds the relation's edges"""
    return m.projection or m.relation_matrix


NORM_MODES = ('none', 'clip', 'unit')                                # the --ent_norm / --rel_norm choices


def norm_slices(m, table, mode):
    """the slices of a row of `table` ('ent' / 'rel') under --ent_norm / --rel_norm `mode` as a list of modes, one per slice
    ('clip' / 'unit'); [] where the mode is none.  A model whose relation row has no slices (norm_rel 0) raises ValueError."""
    if mode in (None, 'none'):
        return []
    if mode not in ('clip', 'unit'):
        raise ValueError("norm mode %r: none, clip or unit" % (mode,))
    parts = m.norm_ent if table == 'ent' else m.norm_rel
    if parts == 0:
        raise ValueError("%s: --rel_norm does not apply (%s)" % (m.name, m.no_rel_norm))
    forced = 0 if table == 'ent' else m.norm_rel_unit
    return ['unit' if (forced >> k) & 1 else mode for k in range(parts)]
