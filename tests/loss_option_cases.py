"""Case table and input builders of the loss-option tests (test infrastructure; a plain module, not a conftest).

Every oracle-based GPU test outside this family runs Logsigmoid, point-wise, adv_temp 1, reg_norm 3.  The cases below walk the
other values of --loss_genre / -pw / -m / -a / -rn at the shapes where the kernels change instance.  They are shared by
  tests/test_loss_option_inputs.py   (CPU): the inputs exercise the criteria (hinge straddles its kink, the sigmoid sees both
                                     tails) and fp32 against fp64 oracle stays inside the hinge-flip caps;
  tests/test_gpu_loss_options.py     (GPU): the fused step under every case against the fp64 oracle.

Tables are the default init U(-emb_init, emb_init) times `scale`; gamma and scale are chosen per shape so that the scores have
mean ~0 and a standard deviation of 1.5 - 2 (the recipes' own gamma / init put every score on one side of every criterion - the
five toy goldens this family replaces as the only genre coverage never crossed the hinge's kink).  The distance models need a
larger gamma than the recipes' for that: the spread of an L1 / L2 distance over 400 columns is ~3.5 % of its mean.
"""
import numpy as np

from oracle import kge_oracle as O

FUSED_LOSS, SPLIT_FWD, LOSS_IN_FWD, NEG_DEG, NO_TRANSE_FAST = 8, 128, 1024, 32, 2       # include/kge_hip.h KGE_FLAG_*
GEMM_FLAGS = (0, FUSED_LOSS, SPLIT_FWD, LOSS_IN_FWD)
GEMM_MODELS = ("TransE_l2", "DistMult", "ComplEx", "SimplE")

SCORE_RTOL = SCORE_ATOL = 1e-4          # the suite's score tolerance; a hinge flip is legitimate only inside it
FLIP_CAP = 1e-4                         # flipped pairs / pairs, per case and step
ROW_CAP = 0.02                          # excluded rows / rows of any compared array

# name -> model, n_ent, n_rel, hidden, de, dr, B, N, chunk, gamma, lr, scale
SHAPES = {
    # the recipes' shapes (tests/test_gpu_parity.py SHAPES), gamma / scale as explained above
    "cfgT": ("TransE_l2", 14951, 1345, 400, False, False, 1000, 200, 200, 48.0, 0.25, 19.2),
    "cfgD": ("DistMult", 14951, 1345, 400, False, False, 1000, 200, 200, 143.0, 0.08, 2.1),
    "complex": ("ComplEx", 50000, 535, 200, True, True, 1024, 256, 256, 143.0, 0.1, 1.0),
    "rotate": ("RotatE", 14951, 1345, 200, True, False, 1024, 256, 256, 48.0, 0.009, 0.92),
    "l1": ("TransE_l1", 14951, 1345, 400, False, False, 400, 200, 200, 48.0, 0.01, 1.18),
    "simple": ("SimplE", 5000, 50, 200, True, True, 512, 128, 128, 143.0, 0.1, 1.3),
    # tests/test_gpu_rescal.py CASES[0] and tests/test_gpu_transr.py TILE_SHAPES[0]
    "rescal": ("RESCAL", 2000, 300, 500, False, False, 256, 64, 64, 6.0, 0.05, 16.0),
    "transr": ("TransR", 500, 9, 72, False, True, 70, 70, 35, 20.0, 0.05, 0.142),
    # the loss kernel's instances above 256 and above 512 negatives per row
    "n288": ("DistMult", 5000, 50, 64, False, False, 128, 288, 64, 143.0, 0.08, 0.45),
    "n600": ("DistMult", 5000, 50, 64, False, False, 128, 600, 64, 143.0, 0.08, 0.45),
    "t600": ("TransE_l2", 5000, 50, 64, False, False, 128, 600, 64, 24.0, 0.1, 7.45),
    # mid widths (D >= 64) for edge importance / --neg_deg_sample
    "midT": ("TransE_l2", 5000, 50, 64, False, False, 96, 48, 48, 24.0, 0.1, 7.45),
    "midR": ("RotatE", 2000, 20, 32, True, False, 128, 32, 32, 24.0, 0.05, 0.89),
    "midD": ("DistMult", 5000, 50, 64, False, False, 96, 48, 48, 143.0, 0.08, 0.45),
    # update kernel: four 16-byte packs per lane (D_e = 800) and a width that is no multiple of 4 (scalar path)
    "d800": ("TransE_l2", 3000, 11, 400, True, True, 256, 64, 64, 48.0, 0.1, 13.6),
    "odd": ("TransE_l2", 300, 10, 30, False, False, 48, 10, 12, 12.0, 0.1, 4.8),
    "oddD": ("DistMult", 300, 10, 18, False, False, 48, 10, 12, 12.0, 0.1, 1.6),
}
_FIELDS = ("model", "n_ent", "n_rel", "hidden", "de", "dr", "B", "N", "chunk", "gamma", "lr", "scale")


def case(cid, shape, genre="Logsigmoid", pairwise=False, margin=1.0, adv=True, adv_temp=1.0, reg_coef=0.0, reg_norm=3, impts=False,
         neg_deg=False, flags=(0,), rows=1e-3, seed=0, **over):
    """rows: bound on post-update rows in units of lr (1e-3 at the recipes' shapes, 5e-3 at the small ones: the suite's two
    existing bounds).  flags: the kernel-path flags the GPU test runs the case under (--neg_deg_sample is added to each)."""
    c = dict(zip(_FIELDS, SHAPES[shape]))
    c.update(id=cid, shape=shape, genre=genre, pairwise=pairwise, margin=margin, adv=bool(adv and not pairwise), adv_temp=adv_temp,
             reg_coef=reg_coef, reg_norm=reg_norm, impts=impts, neg_deg=neg_deg, flags=tuple(flags), rows=rows, seed=seed)
    c.update(over)
    return c


def _genre_block():
    """the four genre settings at the six recipe shapes; the matrix-core models under every forward / loss launch variant"""
    out = []
    for sh in ("cfgT", "cfgD", "complex", "rotate", "l1", "simple"):
        fl = GEMM_FLAGS if SHAPES[sh][0] in GEMM_MODELS else (0,)
        out.append(case(sh + "-hinge-adv", sh, "Hinge", adv=True, adv_temp=0.5, flags=fl))
        out.append(case(sh + "-bce-adv", sh, "BCE", adv=True, flags=fl))
        out.append(case(sh + "-logistic", sh, "Logistic", adv=False, flags=fl))
        out.append(case(sh + "-hinge-pairwise", sh, "Hinge", pairwise=True, flags=fl))
    return out


# regulariser coefficients: chosen so that the regulariser is >= 1 % of the largest gradient component (asserted from the oracle
# by both test files); the loss gradient is O(1 / B) per element, d/dx coef |x|^q = coef q |x|^(q-1)
CASES = _genre_block() + [
    # ---- remaining genre coverage
    case("n288-hinge-adv", "n288", "Hinge", adv_temp=0.5, rows=5e-3),
    case("n600-hinge-adv", "n600", "Hinge", adv_temp=0.5, rows=5e-3),
    case("rescal-hinge", "rescal", "Hinge"),
    case("rescal-bce", "rescal", "BCE"),
    case("transr-hinge", "transr", "Hinge", rows=5e-3),
    case("transr-bce", "transr", "BCE", rows=5e-3),
    case("midT-nd-hinge", "midT", "Hinge", neg_deg=True, rows=5e-3),
    case("midT-nd-bce", "midT", "BCE", neg_deg=True, rows=5e-3),
    case("midR-nd-hinge", "midR", "Hinge", neg_deg=True, rows=5e-3),
    case("midR-nd-bce", "midR", "BCE", neg_deg=True, rows=5e-3),
    case("midT-impts-hinge-pairwise", "midT", "Hinge", pairwise=True, impts=True, rows=5e-3),
    case("midR-impts-hinge-pairwise", "midR", "Hinge", pairwise=True, impts=True, rows=5e-3),
    case("midD-impts-bce-adv", "midD", "BCE", impts=True, flags=(0, FUSED_LOSS), rows=5e-3),
    # ---- adversarial temperature: the three softmax implementations (loss_row_regs: flags 0 / SPLIT_FWD / LOSS_IN_FWD; the forward
    #      tiles' partial softmax: FUSED_LOSS; the generic loss_kernel: N > 512)
    case("cfgT-advtemp0.5", "cfgT", adv_temp=0.5, flags=GEMM_FLAGS, reg_coef=1e-9),
    case("cfgT-advtemp2", "cfgT", adv_temp=2.0, flags=GEMM_FLAGS, reg_coef=1e-9),
    case("rotate-advtemp0.5", "rotate", adv_temp=0.5, reg_coef=1e-7),
    case("rotate-advtemp2", "rotate", adv_temp=2.0, reg_coef=1e-7),
    case("t600-advtemp2", "t600", adv_temp=2.0, flags=(0, FUSED_LOSS), rows=5e-3),
    case("n600-advtemp0.5-bce", "n600", "BCE", adv_temp=0.5, rows=5e-3),
    # ---- regulariser norm != 3.  launch_update (kge_rowwise.hip) sends every in-place update with the regulariser on and
    #      reg_norm != 3 to update_kernel_reg<NIT, false, 0> - the only register-resident instance with a run-time norm - as long as
    #      the row widths are multiples of 4 and <= 1024.  That holds for every case of this block except odd-reg2 / oddD-reg4,
    #      which take the scalar update_kernel<1>: cfgT / cfgD / l1 / complex / rotate run <1 or 2, false, 0>, d800 runs <4, false, 0>,
    #      the --neg_deg_sample cases run it with the sampled rows' regulariser added inside (a.nd_chunk), and RESCAL / TransR
    #      reach it for the entity table (their relation-side tables are updated by kge_rescal.hip / kge_transr.hip, whose
    #      reg_grad calls take the same run-time norm).
    case("cfgT-reg2", "cfgT", reg_norm=2, reg_coef=2e-6, flags=(0, NO_TRANSE_FAST)),
    case("cfgT-reg1", "cfgT", reg_norm=1, reg_coef=5e-6, flags=(0, NO_TRANSE_FAST)),
    case("cfgT-reg4", "cfgT", reg_norm=4, reg_coef=3e-7, flags=(0, NO_TRANSE_FAST)),
    case("cfgD-reg2", "cfgD", reg_norm=2, reg_coef=2e-5),
    case("cfgD-reg1", "cfgD", reg_norm=1, reg_coef=2e-5),
    case("complex-reg4", "complex", reg_norm=4, reg_coef=2e-5),
    case("complex-reg2", "complex", reg_norm=2, reg_coef=2e-5),
    case("rotate-reg2", "rotate", reg_norm=2, reg_coef=3e-4),      # kge_api.hip: the shared-pair path's folded regulariser is norm 3 only
    case("rotate-reg1", "rotate", reg_norm=1, reg_coef=1e-4),
    case("l1-reg2", "l1", reg_norm=2, reg_coef=8e-4),
    case("l1-reg4", "l1", reg_norm=4, reg_coef=2e-2),
    case("rescal-reg2", "rescal", reg_norm=2, reg_coef=5e-4),
    case("transr-reg1", "transr", reg_norm=1, reg_coef=2e-2, rows=5e-3),
    case("transr-reg2", "transr", reg_norm=2, reg_coef=0.2, rows=5e-3),
    case("midT-nd-reg2", "midT", reg_norm=2, reg_coef=5e-5, neg_deg=True, rows=5e-3),      # the update kernel adds the sampled rows' regulariser
    case("midR-nd-reg4", "midR", reg_norm=4, reg_coef=5e-4, neg_deg=True, rows=5e-3),
    case("d800-reg2", "d800", reg_norm=2, reg_coef=8e-6),
    case("d800-reg1", "d800", reg_norm=1, reg_coef=1e-5),
    case("odd-reg2", "odd", reg_norm=2, reg_coef=3e-4, rows=5e-3),
    case("oddD-reg4", "oddD", reg_norm=4, reg_coef=1e-3, rows=5e-3),
]


def fuzz_case(seed):
    """one random small configuration over the loss-option axes (its own seeded generator: the 48 cases of
    tests/test_gpu_parity.py::_random_step_case are defined by theirs)"""
    rng = np.random.RandomState(31000 + seed)
    model = ["TransE_l1", "TransE_l2", "DistMult", "ComplEx", "RotatE", "SimplE"][seed % 6]
    de = model in ("ComplEx", "RotatE", "SimplE")
    dr = model in ("ComplEx", "SimplE")
    genre = ["Hinge", "BCE", "Logistic", "Logsigmoid"][(seed // 6) % 4]
    pairwise = genre in ("Hinge", "Logistic") and bool(rng.randint(2))
    hidden = int(rng.choice([8, 12, 16, 18, 20, 32, 48, 64]))
    chunk = int(rng.choice([1, 3, 4, 8, 16, 17, 32]))
    Cn = int(rng.randint(1, 5))
    N = int(rng.choice([1, 2, 5, 8, 16, 20, 36, 64, 65, 130]))
    flags = int(rng.choice([0, 0, 1, 2, 8, 16, 32, 128, 512, 1024]))
    reg_norm = int(rng.choice([1, 2, 3, 4]))
    distance = model in ("TransE_l1", "TransE_l2", "RotatE")
    c = dict(id="fuzz%d" % seed, shape="fuzz", model=model, n_ent=int(rng.choice([30, 200, 2000])), n_rel=int(rng.choice([3, 17])),
             hidden=hidden, de=de, dr=dr, B=Cn * chunk, N=N, chunk=chunk, gamma=float(rng.choice([6.0, 12.0])),
             lr=float(rng.choice([0.05, 0.2])), genre=genre, pairwise=pairwise, margin=float(rng.choice([0.5, 1.0, 2.0])),
             adv=bool(rng.randint(2)) and not pairwise, adv_temp=float(rng.choice([0.5, 1.0, 2.0])),
             reg_coef=float(rng.choice([0.0, 1e-3])), reg_norm=reg_norm, impts=bool(rng.randint(3) == 0), neg_deg=bool(flags & NEG_DEG),
             flags=(flags & ~NEG_DEG,), rows=5e-3, seed=500 + seed)
    # scale: the distance models around score 0 (mean distance ~ gamma: scale ~ 1 / mean |u| per column), the product models wide
    c["scale"] = float(rng.choice([0.8, 1.0, 1.2])) if distance else float(rng.choice([1.0, 2.0, 3.0]))
    return c


# --------------------------------------------------------------------------------------------------------------------------
def config(c):
    return O.Config(c["model"], c["gamma"], c["hidden"], c["lr"], adv=c["adv"], adv_temp=c["adv_temp"], reg_coef=c["reg_coef"],
                    reg_norm=c["reg_norm"], loss_genre=c["genre"], pairwise=c["pairwise"], margin=c["margin"], double_ent=c["de"],
                    double_rel=c["dr"], neg_deg=c["neg_deg"])


def tables(c):
    """float32 entity / relation tables (TransR: and the projection table, U(-1, 1) like the reference's, unscaled)"""
    cfg = config(c)
    rng = np.random.RandomState(4321 + c["seed"])
    rel_w = cfg.rel_dim * cfg.ent_dim if c["model"] == "RESCAL" else cfg.rel_dim           # general_models.py:232-236
    s = cfg.emb_init * c["scale"]
    ent = rng.uniform(-s, s, size=(c["n_ent"], cfg.ent_dim)).astype(np.float32)
    rel = rng.uniform(-s, s, size=(c["n_rel"], rel_w)).astype(np.float32)
    proj = None
    if c["model"] == "TransR":
        proj = rng.uniform(-1.0, 1.0, size=(c["n_rel"], cfg.ent_dim * cfg.rel_dim)).astype(np.float32)
    return ent, rel, proj


def batches(c, steps=2):
    """tail then head corruption; `w`: edge importance or None.  TransR: no edge with h == t (its entity gradient is (h - t) P = 0
    in exact arithmetic and rounding residue in fp32 - Adagrad's first step turns that residue into a move of lr: no digits to
    compare, see tests/test_gpu_transr.py)"""
    rng = np.random.RandomState(8765 + c["seed"])
    out = []
    for step in range(1, steps + 1):
        bt = O.synth_batch(rng, c["n_ent"], c["n_rel"], c["B"], c["N"], c["chunk"], step)
        if c["model"] == "TransR":
            same = bt["h"] == bt["t"]
            bt["t"][same] = (bt["t"][same] + 1) % c["n_ent"]
            nid, inv = np.unique(np.concatenate([bt["h"], bt["t"]]), return_inverse=True)
            bt.update(nid=nid.astype(np.int64), h_local=inv[:c["B"]].astype(np.int64), t_local=inv[c["B"]:].astype(np.int64))
        bt["w"] = rng.uniform(0.5, 1.5, size=c["B"]).astype(np.float32) if c["impts"] else None
        out.append(bt)
    return out


def oracle_forward_backward(c, ent, rel, proj, bt):
    cfg = config(c)
    w = None if bt["w"] is None else bt["w"].astype(ent.dtype)
    a = (bt["nid"], bt["h_local"], bt["t_local"], bt["r"], bt["neg"], bt["neg_head"], c["chunk"], c["N"], w)
    if c["model"] == "TransR":
        return O.transr_forward_backward(cfg, ent, rel, proj, *a)
    return O.forward_backward(cfg, ent, rel, *a)


def oracle_step(c, ent, es, rel, rs, proj, ps, bt):
    """one oracle train step in the dtype of the tables, in place"""
    cfg = config(c)
    w = None if bt["w"] is None else bt["w"].astype(ent.dtype)
    a = (bt["nid"], bt["h_local"], bt["t_local"], bt["r"], bt["neg"], bt["neg_head"], c["chunk"], c["N"], w)
    if c["model"] == "TransR":
        return O.transr_train_step(cfg, ent, es, rel, rs, proj, ps, *a)
    return O.train_step(cfg, ent, es, rel, rs, *a)


def oracle_scores(c, ent, rel, proj, bt):
    """(pos [B], neg [B, N']) only - what the input guard needs, without the backward (--neg_deg_sample: N' = chunk + N, the
    masked diagonal at score 0 like the reference's)"""
    cfg = config(c)
    if c["model"] == "TransR" or c["neg_deg"]:
        o = oracle_forward_backward(c, ent, rel, proj, bt)
        return o["pos_score"], o["neg_score"].reshape(c["B"], -1)
    dt = ent.dtype
    h, t, r = ent[bt["h"]], ent[bt["t"]], rel[bt["r"]]
    gamma = dt.type(cfg.gamma)
    p = O.score_pos(cfg.model, h, r, t, gamma, cfg.emb_init)
    a = O.pos_side(cfg.model, bt["neg_head"], t if bt["neg_head"] else h, r, cfg.emb_init)
    n = O.score_neg(cfg.model, a, ent[bt["neg"]], c["B"] // c["chunk"], c["chunk"], c["N"], gamma)
    return p, n.reshape(c["B"], -1)


# --------------------------------------------------------------------------------------------------------------------------
# hinge activity and flips
# --------------------------------------------------------------------------------------------------------------------------
def hinge_v(c, pos, neg):
    """the hinge's argument v = margin - label * score in the dtype of the scores (loss.py: only v < 0 is zeroed, v == 0 keeps
    its gradient).  Returns (v_pos [B] or None when pairwise, v_neg [B, N'])."""
    dt = np.asarray(pos).dtype
    m = dt.type(c["margin"])
    pos, neg = np.asarray(pos), np.asarray(neg).reshape(len(pos), -1)
    if c["pairwise"]:
        return None, m - (pos[:, None] - neg)
    return m - pos, m + neg


def activity(c, pos, neg):
    """what the criterion sees: Hinge -> (share of active positives or None, share of active negatives / pairs);
    BCE / Logistic -> (lowest, highest) argument of the sigmoid"""
    pos, neg = np.asarray(pos, np.float64), np.asarray(neg, np.float64).reshape(len(pos), -1)
    if c["genre"] == "Hinge":
        vp, vn = hinge_v(c, pos, neg)
        return (None if vp is None else float((vp >= 0).mean())), float((vn >= 0).mean())
    x = (pos[:, None] - neg).ravel() if c["pairwise"] else np.concatenate([pos, neg.ravel()])
    return float(x.min()), float(x.max())


def activity_ok(c, pos, neg):
    a = activity(c, pos, neg)
    if c["genre"] == "Hinge":
        return all(0.2 <= s <= 0.8 for s in a if s is not None)
    if c["genre"] in ("BCE", "Logistic"):
        return a[0] <= -3.0 and a[1] >= 3.0
    return True


def hinge_flips(c, bt, pos_a, neg_a, pos64, neg64):
    """pairs whose hinge is active in one set of scores (`_a`: float32, the kernel's or the fp32 oracle's) and not in the float64
    oracle's: the XOR of the two activity masks.  Returns None for the other genres, else a dict:
      n_flips, n_pairs, worst_v   (largest float64 |v| / its tolerance among the flipped pairs: must be <= 1)
      slots / edges / pos_local / ent / rel : the gradient rows (g_neg, g_rel, g_pos_ent by index into bt['nid']) and table rows
      the flipped pairs feed - whole rows, because Adagrad scales a row by the mean of its squared gradient."""
    if c["genre"] != "Hinge":
        return None
    B, chunk, N = c["B"], c["chunk"], c["N"]
    pos_a, pos64 = np.asarray(pos_a, np.float32), np.asarray(pos64, np.float64)
    neg_a, neg64 = np.asarray(neg_a, np.float32).reshape(B, -1), np.asarray(neg64, np.float64).reshape(B, -1)
    Np = neg64.shape[1]
    vpa, vna = hinge_v(c, pos_a, neg_a)
    vp64, vn64 = hinge_v(c, pos64, neg64)
    fn = (vna >= 0) != (vn64 >= 0)
    fp = np.zeros(B, bool) if vpa is None else (vpa >= 0) != (vp64 >= 0)
    n_pairs = fn.size + (0 if vpa is None else B)
    # a legitimate flip sits inside the score tolerance of the kink (pairwise: of two scores)
    tol_n = SCORE_ATOL + SCORE_RTOL * np.abs(neg64)
    if c["pairwise"]:
        tol_n = tol_n + SCORE_ATOL + SCORE_RTOL * np.abs(pos64)[:, None]
    worst = 0.0
    if fn.any():
        worst = max(worst, float((np.abs(vn64) / tol_n)[fn].max()))
    if fp.any():
        worst = max(worst, float((np.abs(vp64) / (SCORE_ATOL + SCORE_RTOL * np.abs(pos64)))[fp].max()))
    ii, jj = np.nonzero(fn)
    edges = set(ii.tolist()) | set(np.nonzero(fp)[0].tolist())
    ents, slots = set(), set()
    own = bt["h"] if bt["neg_head"] else bt["t"]              # --neg_deg_sample: columns < chunk are the chunk's own corrupted-side rows
    for i, j in zip(ii.tolist(), jj.tolist()):
        ch = i // chunk
        if Np != N and j < chunk:
            ents.add(int(own[ch * chunk + j]))
        else:
            s = ch * N + (j - (Np - N))
            slots.add(s)
            ents.add(int(bt["neg"][s]))
    for i in edges:
        ents.update((int(bt["h"][i]), int(bt["t"][i])))
    rels = set(int(bt["r"][i]) for i in edges)
    nid = bt["nid"]
    in_pos = sorted(e for e in ents if nid[min(np.searchsorted(nid, e), len(nid) - 1)] == e)
    return dict(n_flips=int(fn.sum() + fp.sum()), n_pairs=int(n_pairs), worst_v=worst, slots=sorted(slots), edges=sorted(edges),
                pos_local=np.searchsorted(nid, in_pos).tolist() if in_pos else [], ent=sorted(ents), rel=sorted(rels))


def check_flip_caps(c, bt, fl, tag):
    """section 'conditions, not measurements': flips <= 1e-4 of the pairs, every flip inside the score tolerance, excluded rows
    <= 2 % of the rows of every compared array"""
    if fl is None:
        return
    assert fl["n_flips"] <= FLIP_CAP * fl["n_pairs"], "%s: %d hinge flips among %d pairs" % (tag, fl["n_flips"], fl["n_pairs"])
    assert fl["worst_v"] <= 1.0, "%s: a flipped pair sits %.2f score tolerances from the kink" % (tag, fl["worst_v"])
    C = c["B"] // c["chunk"]
    for what, rows, total in (("g_neg", fl["slots"], C * c["N"]), ("g_rel", fl["edges"], c["B"]),
                              ("g_pos_ent", fl["pos_local"], len(bt["nid"])), ("entity table", fl["ent"], c["n_ent"]),
                              ("relation table", fl["rel"], c["n_rel"])):
        assert len(rows) <= ROW_CAP * total, "%s: %d of %d rows of %s excluded" % (tag, len(rows), total, what)


def reg_share(c, out, ent, rel, bt):
    """largest regulariser gradient component / largest gradient component, from an oracle step's output (ent / rel: the tables
    the step started from)"""
    if not (c["reg_coef"] > 0):
        return 0.0
    q = c["reg_norm"]
    rg = max(np.abs(O.reg_grad(ent[bt["nid"]].astype(np.float64), c["reg_coef"], q)).max(),
             np.abs(O.reg_grad(ent[bt["neg"]].astype(np.float64), c["reg_coef"], q)).max(),
             np.abs(O.reg_grad(rel[bt["r"]].astype(np.float64), c["reg_coef"], q)).max())
    g = max(np.abs(out["g_pos_ent"]).max(), np.abs(out["g_neg"]).max(), np.abs(out["g_rel"]).max())
    return float(rg / g)
