"""Fused-step driver: one C-ABI call (`kge_step_fused`) = KEModel.forward + loss.backward() +
KEModel.update of the reference (train_pytorch.py:141-152) for one batch, enqueued on the current
HIP stream with no host synchronisation.  `StepEngine.capture()` records a sequence of steps over
pre-staged batches into a HIP graph so that the launch-bound inner loop is replayed without host
work (one step is only a few microseconds of HBM traffic, SURVEY.md 7 'hard parts')."""
import ctypes as C
import math

import torch

from . import _lib, models
from ._lib import check, lib, model_id, ptr, stream_ptr


class StepEngine(object):
    def __init__(self, model_name, n_entities, n_relations, hidden_dim, gamma, lr, device,
                 double_entity_emb=False, double_relation_emb=False, neg_adversarial_sampling=False,
                 adversarial_temperature=1.0, regularization_coef=0.0, regularization_norm=3,
                 loss_genre='Logsigmoid', pairwise=False, margin=1.0, flags=0,
                 tables=None, shards=None, optimizer='Adagrad', adam_betas=(0.9, 0.999), adam_eps=1e-8, moments=None,
                 ent_norm=None, rel_norm=None):
        """optimizer 'Adam': lazy row-sparse Adam with a per-row step count (include/kge_hip.h, kge_step_optim) - the state
        tables hold the counts, the engine owns the moment tables ent_mom [n_ent, 2, d_e] / rel_mom [n_rel, 2, d_r] (`moments`:
        a pair the caller shares between engines, as `tables` shares the rows and the state).
        ent_norm / rel_norm None | 'clip' | 'unit': the norm constraints of radius 1 on the rows every strict step has updated
        (include/kge_hip.h, KGE_FLAG_ENT_NORM_* / KGE_FLAG_REL_NORM_*; the slices of a row: models.py).  Tables the engine creates
        are projected whole once (`project_tables`); tables handed in are the caller's to project."""
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.KgeError("StepEngine needs a CUDA (HIP) device; there is no CPU fallback")
        self.model_name = model_name
        self.n_entities, self.n_relations = n_entities, n_relations
        self.hidden_dim = hidden_dim
        self.gamma = gamma
        self.emb_init = (gamma + 2.0) / hidden_dim          # general_models.py:217-218
        self.d_e = 2 * hidden_dim if double_entity_emb else hidden_dim
        self.d_r = 2 * hidden_dim if double_relation_emb else hidden_dim
        if model_name == 'RESCAL':                          # relation row = [rel_dim x ent_dim] matrix, general_models.py:232-236
            self.d_r = self.d_r * self.d_e
        m = models.MODELS.get(model_name)                   # (unknown names: model_id below)
        if m and not models.widths_ok(m, self.d_e, self.d_r):
            raise _lib.KgeError(m.engine_text % (self.d_e, self.d_r))
        if m and m.single_gpu_only and shards is not None:
            raise _lib.KgeError("%s runs the strict step on local tables only (no sharded tables)" % m.name)
        for table, mode in (('ent', ent_norm), ('rel', rel_norm)):
            if mode not in _lib.NORM_FLAGS[table]:
                raise _lib.KgeError("%s_norm %r: None, 'clip' or 'unit'" % (table, mode))
        self.ent_norm = None if ent_norm == 'none' else ent_norm
        self.rel_norm = None if rel_norm == 'none' else rel_norm
        if self.ent_norm or self.rel_norm:
            if shards is not None:
                raise _lib.KgeError("the norm constraints run on the strict step of local tables only (no sharded tables)")
            if self.rel_norm and m and m.norm_rel == 0:
                raise _lib.KgeError("rel_norm is not available for %s (%s)" % (m.name, m.no_rel_norm))
        flags = int(flags) | _lib.NORM_FLAGS['ent'][self.ent_norm] | _lib.NORM_FLAGS['rel'][self.rel_norm]
        hp = _lib.KgeHParams()
        hp.model = model_id(model_name)
        hp.d_e, hp.d_r = self.d_e, self.d_r
        hp.loss_genre = _lib.LOSS_IDS[loss_genre]
        hp.adv = int(bool(neg_adversarial_sampling))
        hp.pairwise = int(bool(pairwise))
        hp.reg_norm = int(regularization_norm)
        hp.flags = int(flags)
        hp.gamma = float(gamma)
        hp.emb_init = float(self.emb_init)
        hp.lr = float(lr)
        hp.adv_temp = float(adversarial_temperature)
        hp.margin = float(margin if margin is not None else 1.0)
        hp.reg_coef = float(regularization_coef)
        hp.eps = 1e-10
        self.hp = hp
        import os
        if (shards is not None and shards.n_shards == 1 and not shards.emulate and tables is None and
                os.environ.get("KGE_P2P_LOCAL_SHORTCUT", "1") != "0"):
            # ONE shard (world 1): every row is a row of this process's own arena - the plain single-table step on it (round 6:
            # no shard-map division per row, no dense copy of the negative rows; the emulated-shard tests keep the map)
            if (shards.d_e, shards.d_r) != (self.d_e, self.d_r):
                raise _lib.KgeError("sharded tables have row widths (%d, %d), model needs (%d, %d)"
                                    % (shards.d_e, shards.d_r, self.d_e, self.d_r))
            tables = (shards.ent(0), shards.ent_state(0), shards.rel(0), shards.rel_state(0))
            self.shards_local = shards     # (keeps the arena alive)
            shards = None
        self.shards = shards           # p2p.ShardedTables: the tables live in the peers' HBM
        if shards is not None:
            if (shards.d_e, shards.d_r) != (self.d_e, self.d_r):
                raise _lib.KgeError("sharded tables have row widths (%d, %d), model needs (%d, %d)"
                                    % (shards.d_e, shards.d_r, self.d_e, self.d_r))
            self.ent, self.ent_state = shards.ent(0), shards.ent_state(0)
            self.rel, self.rel_state = shards.rel(0), shards.rel_state(0)
        self.proj = self.proj_state = None      # TransR: projection_emb of the score function (score_fun.py:114-118)
        if shards is not None:
            if model_name in ('TransR', 'RESCAL') and not getattr(shards, 'rel_local', False):
                raise _lib.KgeError("%s on sharded tables needs ShardedTables(rel_local=True%s): relation-side tables local to the rank"
                                    % (model_name, ", proj_dim=d_e*d_r" if model_name == 'TransR' else ""))
            if model_name == 'TransR':
                if shards.proj_tab is None or shards.proj_tab.shape[1] != self.d_e * self.d_r:
                    raise _lib.KgeError("TransR on sharded tables needs ShardedTables(proj_dim=%d)" % (self.d_e * self.d_r))
                self.proj, self.proj_state = shards.proj_tab, shards.proj_state_tab
        elif tables is None:
            if model_name == 'TransR':
                self.proj = torch.empty(n_relations, self.d_e * self.d_r, dtype=torch.float32, device=self.device)
                self.proj_state = torch.zeros(n_relations, dtype=torch.float32, device=self.device)
            self.ent = torch.empty(n_entities, self.d_e, dtype=torch.float32, device=self.device)
            self.ent_state = torch.zeros(n_entities, dtype=torch.float32, device=self.device)
            self.rel = torch.empty(n_relations, self.d_r, dtype=torch.float32, device=self.device)
            self.rel_state = torch.zeros(n_relations, dtype=torch.float32, device=self.device)
            self.reset_parameters()
        else:
            self.ent, self.ent_state, self.rel, self.rel_state = tables[:4]
            if model_name == 'TransR':
                if len(tables) < 6:
                    raise _lib.KgeError("TransR needs tables = (ent, ent_state, rel, rel_state, proj, proj_state)")
                self.proj, self.proj_state = tables[4], tables[5]
        self.optimizer = optimizer
        self.opt = None
        self.ent_mom = self.rel_mom = None
        if optimizer not in _lib.OPT_IDS:
            raise _lib.KgeError("optimizer %r: Adagrad or Adam" % (optimizer,))
        if optimizer == 'Adam':
            self._init_adam(adam_betas, adam_eps, moments)
        self._bind_tables()
        self.loss4 = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.loss_accum = torch.zeros(4 * _lib.ACC_SLOTS, dtype=torch.float32, device=self.device)
        self._sum4 = torch.zeros(4, dtype=torch.float32, device=self.device)
        # hand-off words of the strict step's first launch (kge_step_out.tickets): zero now, every step returns them to zero
        self.tickets = torch.zeros(_lib.TICKET_INTS, dtype=torch.int32, device=self.device)
        self._ws = None
        self._ws_bytes = 0
        self._graphs = 0               # graphs captured with this engine's workspace baked in (the workspace may not move then)
        self._pipe = None              # kge_pipe of the --async_update pipeline (side stream + events)
        self._aws = None
        self._aws_bytes = 0
        self._known = None             # (KgeKnown, KnownIndex) of attach_known: known triples left out of the negatives
        self._kmask = None
        self._kmask_bytes = 0

    @classmethod
    def from_args(cls, args, model_name, n_entities, n_relations, device, tables=None, shards=None, moments=None, **given):
        """the engine of an argument namespace (dglke_train's, or a hand-made one: what is missing or None takes the reference's
        default).  `given`: constructor arguments the caller holds itself (KEModel: hidden_dim, gamma, the double_* flags).  The
        step flags are decided here and nowhere else: degree-sampled negatives with --neg_deg_sample for every model, the
        relation trace deferred too when both --async_update and --async_update_rel are set (only the async step reads it)."""
        def arg(name, default=None):
            return getattr(args, name, None) or default
        flags = _lib.FLAG_NEG_DEG_SAMPLE if arg('neg_deg_sample') else 0
        if arg('async_update') and arg('async_update_rel'):
            flags |= _lib.FLAG_ASYNC_REL
        kw = dict(hidden_dim=getattr(args, 'hidden_dim', None), gamma=getattr(args, 'gamma', None),
                  double_entity_emb=bool(arg('double_ent')), double_relation_emb=bool(arg('double_rel')))
        kw.update(given)
        return cls(model_name, n_entities, n_relations, kw['hidden_dim'], kw['gamma'], args.lr, device,
                   kw['double_entity_emb'], kw['double_relation_emb'], bool(arg('neg_adversarial_sampling')),
                   arg('adversarial_temperature', 1.0), arg('regularization_coef', 0.0),
                   getattr(args, 'regularization_norm', 3) or 0, arg('loss_genre', 'Logsigmoid'), bool(arg('pairwise')),
                   getattr(args, 'margin', 1.0), flags=flags, tables=tables, shards=shards,
                   optimizer=arg('optimizer', 'Adagrad'), moments=moments,
                   adam_betas=(getattr(args, 'adam_beta1', None) if getattr(args, 'adam_beta1', None) is not None else 0.9,
                               getattr(args, 'adam_beta2', None) if getattr(args, 'adam_beta2', None) is not None else 0.999),
                   adam_eps=arg('adam_eps', 1e-8), ent_norm=arg('ent_norm'), rel_norm=arg('rel_norm'))

    def _init_adam(self, betas, eps, moments):
        if self.model_name in ('RESCAL', 'TransR'):
            raise _lib.KgeError("Adam is not available for RESCAL / TransR (their relation-side tables are updated by kernels of "
                                "their own)")
        if self.shards is not None:
            raise _lib.KgeError("Adam runs the strict step on local tables only (no sharded tables)")
        if self.d_e % 4 or self.d_r % 4 or max(self.d_e, self.d_r) > _lib.ADAM_MAX_DIM:
            raise _lib.KgeError("Adam needs row widths that are multiples of 4 and at most %d floats (got %d, %d)"
                                % (_lib.ADAM_MAX_DIM, self.d_e, self.d_r))
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise _lib.KgeError("Adam needs beta1 and beta2 in [0, 1) (got %g, %g)" % (b1, b2))
        if not float(eps) > 0.0:
            raise _lib.KgeError("Adam needs eps > 0 (got %g)" % float(eps))
        if moments is not None:
            self.ent_mom, self.rel_mom = moments
        else:
            need = 4 * 2 * (self.ent.shape[0] * self.d_e + self.rel.shape[0] * self.d_r)
            try:
                self.ent_mom = torch.zeros(self.ent.shape[0], 2, self.d_e, dtype=torch.float32, device=self.device)
                self.rel_mom = torch.zeros(self.rel.shape[0], 2, self.d_r, dtype=torch.float32, device=self.device)
            except RuntimeError as e:
                raise _lib.KgeError("Adam: the moment tables need %d bytes (twice the embedding tables) and could not be "
                                    "allocated: %s" % (need, e))
        if tuple(self.ent_mom.shape) != (self.ent.shape[0], 2, self.d_e) or tuple(self.rel_mom.shape) != (self.rel.shape[0], 2, self.d_r):
            raise _lib.KgeError("Adam: moment tables must be [n_ent, 2, d_e] and [n_rel, 2, d_r]")
        o = _lib.KgeOptim()
        o.kind, o.beta1, o.beta2, o.eps = _lib.OPT_ADAM, b1, b2, float(eps)
        o.ent_mom, o.rel_mom = ptr(self.ent_mom), ptr(self.rel_mom)
        self.opt = o

    def _step_optim(self, batch, out, ws, phases):
        """kge_step_optim: the strict step (or some of its phase groups) with this engine's optimizer"""
        km, kn, kb = None, None, 0
        if self._known is not None:
            km, kn, kb = self.known_mask_for(batch), C.byref(self._known[0]), self._kmask_bytes
        check(lib().kge_step_optim(C.byref(self.hp), C.byref(self.opt), C.byref(self.tb), C.byref(batch.c), C.byref(out), ptr(ws),
                                   self._ws_bytes, phases, kn, ptr(km), kb, stream_ptr()))

    def attach_known(self, index):
        """leave the triples of `index` (known.KnownIndex on this engine's device; None detaches) out of every step's negatives:
        a (positive, negative) pair whose corrupted triple is in the index takes the score KGE_KNOWN_SCORE in the loss - loss term,
        gradient and self-adversarial weight 0 (include/kge_hip.h, kge_step_fused_known).  The index is only read: engines of
        several `--num_proc` lanes share one; the pair mask of a step lives in a buffer of this engine's.  Strict single-table
        step (`step`, `step_timed`, `capture`); not with KGE_FLAG_NEG_DEG_SAMPLE / FUSED_LOSS / LOSS_IN_FWD."""
        if index is None:
            self._known = None
            return
        if self.shards is not None:
            raise _lib.KgeError("attach_known: known-triple exclusion runs on the strict single-table step only")
        if (index.n_ent, index.n_rel) != (self.n_entities, self.n_relations):
            raise _lib.KgeError("attach_known: the index describes %d entities x %d relations, the engine %d x %d"
                                % (index.n_ent, index.n_rel, self.n_entities, self.n_relations))
        if torch.device(index.dev) != self.device:
            raise _lib.KgeError("attach_known: the index lives on %s, the engine on %s" % (index.dev, self.device))
        (kt, vt), (kh, vh) = index.side(False), index.side(True)
        k = _lib.KgeKnown()
        k.keys_tail, k.vals_tail, k.m_tail = ptr(kt), ptr(vt), kt.numel()
        k.keys_head, k.vals_head, k.m_head = ptr(kh), ptr(vh), kh.numel()
        k.n_rel = index.n_rel
        self._known = (k, index)       # (the index keeps the sorted arrays alive)

    def known_mask_for(self, b):
        need = int(lib().kge_known_mask_bytes(b.B, b.N))
        if need > self._kmask_bytes:
            if self._graphs:
                raise _lib.KgeError("the known-pair mask would be re-allocated after graph capture")
            self._kmask = torch.zeros(need, dtype=torch.uint8, device=self.device)
            self._kmask_bytes = need
        return self._kmask

    def _bind_tables(self):
        tb = _lib.KgeTables()
        tb.ent, tb.ent_state = ptr(self.ent), ptr(self.ent_state)
        tb.rel, tb.rel_state = ptr(self.rel), ptr(self.rel_state)
        tb.n_ent, tb.n_rel = self.ent.shape[0], self.rel.shape[0]
        tb.proj, tb.proj_state = ptr(self.proj), ptr(self.proj_state)
        self.tb = tb

    def reset_parameters(self):
        torch.nn.init.uniform_(self.ent, -self.emb_init, self.emb_init)
        torch.nn.init.uniform_(self.rel, -self.emb_init, self.emb_init)
        self.ent_state.zero_()
        self.rel_state.zero_()
        if getattr(self, 'ent_mom', None) is not None:
            self.ent_mom.zero_()
            self.rel_mom.zero_()
        if self.proj is not None:                 # TransRScore.reset_parameters: projection_emb.init(1.0)
            torch.nn.init.uniform_(self.proj, -1.0, 1.0)
            self.proj_state.zero_()
        self.project_tables()

    def project_tables(self):
        """the projection of the norm constraints on EVERY row of the constrained tables, in place (torch on the device: not a hot
        path).  Fresh tables are projected once, so that rows no step has touched yet satisfy the constraint too; a step projects
        the rows it updates itself.  Nothing to do without ent_norm / rel_norm."""
        m = models.MODELS[self.model_name]
        for table, mode, t in (('ent', getattr(self, 'ent_norm', None), self.ent), ('rel', getattr(self, 'rel_norm', None), self.rel)):
            modes = models.norm_slices(m, table, mode)
            if not modes:
                continue
            x = t.view(t.shape[0], len(modes), -1)
            for k, md in enumerate(modes):
                n = x[:, k].norm(dim=1, keepdim=True)
                scale = (n > 0) & (n != 1) if md == 'unit' else n > 1
                x[:, k] = torch.where(scale, x[:, k] / n, x[:, k])

    def load_tables(self, ent, rel, ent_state=None, rel_state=None, ent_mom=None, rel_mom=None):
        """rows, state (Adagrad: running mean squares; Adam: per-row counts) and, under Adam, the moment tables [n, 2, d];
        what is not given is zeroed"""
        self.ent.copy_(torch.as_tensor(ent))
        self.rel.copy_(torch.as_tensor(rel))
        if self.opt is None and (ent_mom is not None or rel_mom is not None):
            raise _lib.KgeError("load_tables: moment tables belong to an engine with optimizer='Adam'")
        if self.opt is not None:
            for dst, src in ((self.ent_mom, ent_mom), (self.rel_mom, rel_mom)):
                if src is None:
                    dst.zero_()
                else:
                    dst.copy_(torch.as_tensor(src).reshape(dst.shape))
        if ent_state is None:
            self.ent_state.zero_()
        else:
            self.ent_state.copy_(torch.as_tensor(ent_state))
        if rel_state is None:
            self.rel_state.zero_()
        else:
            self.rel_state.copy_(torch.as_tensor(rel_state))

    def named_tensors(self):
        """the live tensors a restart needs, by name: 'entity', 'relation' (rows), '..._state' (Adagrad: running mean squares;
        Adam: per-row counts), TransR's 'projection' / 'projection_state', Adam's 'entity_mom' / 'relation_mom' [n, 2, d].  The
        tensors themselves, not copies: engines that share tables name the same ones."""
        t = {'entity': self.ent, 'relation': self.rel, 'entity_state': self.ent_state, 'relation_state': self.rel_state}
        if self.proj is not None:
            t['projection'], t['projection_state'] = self.proj, self.proj_state
        if self.opt is not None:
            t['entity_mom'], t['relation_mom'] = self.ent_mom, self.rel_mom
        return t

    def load_named(self, src, block_bytes=64 << 20):
        """overwrite every tensor of named_tensors() IN PLACE from `src` (name -> array or tensor of the same shape and dtype; a
        memory-mapped file is read row block by row block, at most block_bytes at a time): the table pointers of `tb`, engines
        that share the tables and graphs captured on them stay valid.  Unlike load_tables nothing is zeroed by default: a name
        that is missing, or one this engine does not have, is refused."""
        dst = self.named_tensors()
        if set(src) != set(dst):
            raise _lib.KgeError("load_named: the engine has %s, given %s" % (sorted(dst), sorted(src)))
        for name, d in dst.items():
            s = src[name]
            if tuple(s.shape) != tuple(d.shape):
                raise _lib.KgeError("load_named: %s is %s, the engine's is %s" % (name, tuple(s.shape), tuple(d.shape)))
            n = int(d.shape[0])
            row_bytes = max(1, d[0].numel() * d.element_size()) if n else 1
            per = max(1, int(block_bytes) // row_bytes)
            for a in range(0, n, per):
                blk = s[a:a + per]
                if not isinstance(blk, torch.Tensor):
                    import numpy as np
                    blk = torch.from_numpy(np.array(blk))         # (one block in host memory)
                if blk.dtype != d.dtype:
                    raise _lib.KgeError("load_named: %s is %s, the engine's is %s" % (name, blk.dtype, d.dtype))
                d[a:a + per].copy_(blk)

    def workspace_for(self, b):
        need = lib().kge_step_workspace_bytes(C.byref(self.hp), b.B, b.C, b.chunk, b.N, b.UE, b.UR)
        if need > self._ws_bytes:
            if self._graphs:
                raise _lib.KgeError("workspace would be re-allocated after graph capture")
            self._ws = torch.empty(int(need * 1.25) + 4096, dtype=torch.uint8, device=self.device)
            self._ws_bytes = self._ws.numel()
        return self._ws

    def step(self, batch, want=None, emit=None, per_step_loss=False, sample_job=None):
        """enqueue one fused step.  `want`: dict of optional output tensors (pos_score, neg_score,
        g_pos_ent, g_neg, g_rel).  `emit`: KgeEmit for the sharded path.  `sample_job` (KgeSamplerJob, DeviceSampler.tail_jobs):
        the step's launches also BUILD that batch of the next group (kge_step_fused_sampling; strict step on local tables)."""
        ws = self.workspace_for(batch)
        out = _lib.KgeStepOut()
        if want is not None or per_step_loss:
            out.loss4 = ptr(self.loss4)
        out.loss_accum = ptr(self.loss_accum)
        out.tickets = ptr(self.tickets)
        if want:
            for k, t in want.items():
                setattr(out, k, ptr(t))
        if sample_job is not None and (self.shards is not None or emit is not None):
            raise _lib.KgeError("the sampler tail rides on the strict single-table step only")
        if self.opt is not None:
            if sample_job is not None or emit is not None:
                raise _lib.KgeError("Adam: the sampler-tail step and the gradient-emitting step have no Adam form "
                                    "(sample_job / emit must be None)")
            self._step_optim(batch, out, ws, _lib.PHASE_ALL)
            return
        if self._known is not None:
            if self.shards is not None or emit is not None:
                raise _lib.KgeError("known-triple exclusion runs on the strict single-table step only")
            km = self.known_mask_for(batch)
            check(lib().kge_step_fused_known(C.byref(self.hp), C.byref(self.tb), C.byref(batch.c), C.byref(out), ptr(ws),
                                             self._ws_bytes, C.byref(sample_job) if sample_job is not None else None,
                                             C.byref(self._known[0]), ptr(km), self._kmask_bytes, stream_ptr()))
            return
        if self.shards is not None:
            if emit is not None:
                raise _lib.KgeError("gradient emission and peer-to-peer sharding are different multi-GPU modes")
            check(lib().kge_step_sharded(C.byref(self.hp), C.byref(self.shards.c), C.byref(batch.c),
                                         C.byref(out), ptr(ws), self._ws_bytes, stream_ptr()))
        elif emit is None and sample_job is not None:
            check(lib().kge_step_fused_sampling(C.byref(self.hp), C.byref(self.tb), C.byref(batch.c),
                                                C.byref(out), ptr(ws), self._ws_bytes, C.byref(sample_job), stream_ptr()))
        elif emit is None:
            check(lib().kge_step_fused(C.byref(self.hp), C.byref(self.tb), C.byref(batch.c),
                                       C.byref(out), ptr(ws), self._ws_bytes, stream_ptr()))
        else:
            check(lib().kge_step_grads(C.byref(self.hp), C.byref(self.tb), C.byref(batch.c),
                                       C.byref(out), C.byref(emit), ptr(ws), self._ws_bytes,
                                       stream_ptr()))

    def step_timed(self, batch):
        """ONE strict step issued as its four phase groups (kge_step_phase: gather+positive / negative scores+loss /
        gradients / Adagrad - together exactly kge_step_fused) with HIP events in between; returns the four durations in
        seconds (forward = gather + scores + loss, like the reference's timer around model.forward).  Synchronises."""
        if self.shards is not None:
            self.step(batch)
            return None
        ws = self.workspace_for(batch)
        out = _lib.KgeStepOut()
        out.loss_accum = ptr(self.loss_accum)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        for k, ph in enumerate((_lib.PHASE_GATHER, _lib.PHASE_FORWARD, _lib.PHASE_BACKWARD, _lib.PHASE_UPDATE)):
            if self.opt is not None:
                self._step_optim(batch, out, ws, ph)
            elif self._known is not None:
                km = self.known_mask_for(batch)
                check(lib().kge_step_phase_known(C.byref(self.hp), C.byref(self.tb), C.byref(batch.c), C.byref(out), ptr(ws),
                                                 self._ws_bytes, ph, C.byref(self._known[0]), ptr(km), self._kmask_bytes,
                                                 stream_ptr()))
            else:
                check(lib().kge_step_phase(C.byref(self.hp), C.byref(self.tb), C.byref(batch.c), C.byref(out), ptr(ws),
                                           self._ws_bytes, ph, stream_ptr()))
            ev[k + 1].record()
        ev[4].synchronize()
        t = [ev[k].elapsed_time(ev[k + 1]) * 1e-3 for k in range(4)]
        return dict(forward=t[0] + t[1], backward=t[2], update=t[3])

    # ---- --async_update: UPDATE(s-1) in the same launch as backward(s) (include/kge_hip.h, kge_step_async) ----
    def async_workspace_for(self, b):
        need = lib().kge_step_async_workspace_bytes(C.byref(self.hp), b.B, b.C, b.chunk, b.N, b.UE, b.UR)
        if need > self._aws_bytes:
            if self._graphs:
                raise _lib.KgeError("workspace would be re-allocated after graph capture")
            self._aws = torch.empty(int(need * 1.25) + 8192, dtype=torch.uint8, device=self.device)
            self._aws_bytes = self._aws.numel()
        return self._aws

    def step_async(self, batch, want=None, per_step_loss=False, next_batch=None):
        """enqueue one step of the --async_update pipeline: gathers rows that contain every update up to step s-2's
        (inside one flush-to-flush group), applies step s-1's update in the same launch as this step's forward tiles.
        `next_batch`: the batch of the following step_async call (optional): with KGE_FLAG_ASYNC_REL its PREP shares
        this step's backward launch.  `flush_async()` must follow the last step (before the tables are read / before a
        stream capture ends)."""
        if self.shards is not None:
            raise _lib.KgeError("--async_update is not available on peer-to-peer sharded tables")
        if self.opt is not None:
            raise _lib.KgeError("Adam: the --async_update pipeline has no Adam form")
        if self._known is not None:
            raise _lib.KgeError("known-triple exclusion is not available in the --async_update pipeline")
        if self._pipe is None:
            h = C.c_void_p()
            check(lib().kge_pipe_create(C.byref(h)))
            self._pipe = h
        ws = self.async_workspace_for(batch)
        out = _lib.KgeStepOut()
        if want is not None or per_step_loss:
            out.loss4 = ptr(self.loss4)
        out.loss_accum = ptr(self.loss_accum)
        if want:
            for k, t in want.items():
                setattr(out, k, ptr(t))
        check(lib().kge_step_async(self._pipe, C.byref(self.hp), C.byref(self.tb), C.byref(batch.c),
                                   C.byref(next_batch.c) if next_batch is not None else None, C.byref(out),
                                   ptr(ws), self._aws_bytes, stream_ptr()))
        self._async_keep = (batch, next_batch)       # the pending update / the prefetched PREP read their plan arrays

    def steps_async(self, batches):
        """a group of steps of the pipeline, every step naming its successor, flushed at the end"""
        for k, b in enumerate(batches):
            self.step_async(b, next_batch=batches[k + 1] if k + 1 < len(batches) else None)
        self.flush_async()

    def flush_async(self):
        if self._pipe is not None:
            check(lib().kge_step_async_flush(self._pipe, stream_ptr()))

    def __del__(self):
        try:
            if self._pipe is not None:
                lib().kge_pipe_destroy(self._pipe)
                self._pipe = None
        except Exception:
            pass

    def alloc_outputs(self, batch):
        dev = self.device
        # neg_deg_sample: every chunk is scored against its own positives too (N' = chunk + N rows)
        Np = batch.N + (batch.chunk if self.hp.flags & _lib.FLAG_NEG_DEG_SAMPLE else 0)
        return dict(pos_score=torch.empty(batch.B, device=dev),
                    neg_score=torch.empty(batch.C, batch.chunk, Np, device=dev),
                    g_pos_ent=torch.empty(batch.UE, self.d_e, device=dev),
                    g_neg=torch.empty(batch.C * Np, self.d_e, device=dev),
                    g_rel=torch.empty(batch.B, self.d_r, device=dev))

    def capture(self, batches, stream=None, async_update=False, sampler=None):
        """record `len(batches)` consecutive steps into one HIP graph (on `stream` if given);
        returns the graph.  async_update: the --async_update pipeline, flushed at the end of the group.
        sampler (dataloader.DeviceSampler; `batches` is then the NUMBER of steps, at most its slots): the graph is [one sampler
        launch + that many steps over its slots] - every replay trains on the next batches of the sampler's sequence, whose host
        step counter the caller advances by the group size per replay (an even size keeps the corruption sides in place)."""
        if sampler is not None:
            if async_update:
                raise _lib.KgeError("capture: the sampler form records strict steps")
            n = int(batches)
            probe = sampler._batches.get((0, sampler.host_step % 2 == 0))
            if probe is None:
                from .dataloader import DeviceBatch
                probe = DeviceBatch(sampler, 0, sampler.host_step % 2 == 0)
            self.workspace_for(probe)
            if self._known is not None:
                self.known_mask_for(probe)
            g = torch.cuda.CUDAGraph()
            with _lib.graph_capture(g, stream=stream):
                batches = sampler.sample(n)
                for b in batches:
                    self.step(b)
            sampler.host_step -= n         # the capture itself did not run the steps
            g._kge_batches = batches
            self._graphs += 1
            return g
        for b in batches:
            (self.async_workspace_for if async_update else self.workspace_for)(b)
            if self._known is not None:
                self.known_mask_for(b)
        # warm-up on a side stream is not needed: the library allocates nothing
        g = torch.cuda.CUDAGraph()
        with _lib.graph_capture(g, stream=stream):
            if async_update:
                self.steps_async(batches)
            else:
                for b in batches:
                    self.step(b)
        g._kge_batches = batches       # the graph reads the batches' arrays: they live as long as the graph does
        self._graphs += 1
        return g

    def read_loss(self):
        """[pos_loss, neg_loss, loss, regularization] of the last step run with `want` or
        `per_step_loss` (one 16-byte D2H copy)."""
        return self.loss4.tolist()

    def read_loss_sums(self, zero=True):
        """sums of the four loss terms over all steps since the last reset (one reduction
        kernel + one 16-byte D2H copy); the caller divides by its step count."""
        check(lib().kge_reduce_loss(ptr(self.loss_accum), ptr(self._sum4), int(zero), stream_ptr()))
        return self._sum4.tolist()
