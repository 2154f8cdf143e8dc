"""Float64 statement, oracle hook, case tables and input builders of the Softmax loss genre (--loss_genre Softmax,
include/kge_hip.h KGE_LOSS_SOFTMAX).  Test infrastructure; a plain module, not a conftest.  Shared by
  tests/test_softmax_loss_inputs.py   (CPU): the statement against torch's cross_entropy and autograd, every case does what it is
                                      listed for, the refusals;
  tests/test_gpu_softmax_loss.py      (GPU): the loss op, the fused step, --exclude_positive, the gradient-emitting step, the CLI.

The oracle has no Softmax genre.  oracle.kge_oracle.forward_backward / transr_forward_backward (and tests/known_negative_cases.py)
look `loss_fwd_bwd` up in the oracle module when they are called: `hook(monkeypatch)` installs a wrapper there that sends the
genre "Softmax" to `softmax_fwd_bwd` below and every other genre to the original function.

The definition (row i: positive score p_i, row scores n_ij exactly as the loss kernel sees them - the masked diagonal column of
--neg_deg_sample at score 0, a known pair at -1e6 -, weight w_i = edge importance of edge i or 1):
    m_i = max(p_i, max_j n_ij);  e_p = exp(p_i - m_i), e_j = exp(n_ij - m_i), Z_i = e_p + sum_j e_j
    l_i = m_i + log Z_i - p_i;   loss = (1/B) sum_i w_i l_i
    dL/dn_ij = (w_i / B) e_j / Z_i;   dL/dp_i = -(w_i / B) (sum_j e_j) / Z_i
(the gradient of a masked column is zeroed by the callers of loss_fwd_bwd, as for every other genre: forward_backward multiplies
dneg by its mask, and exp(-1e6 - m) is 0.0 in float64).
"""
import numpy as np

import loss_option_cases as L
from oracle import kge_oracle as O

GENRE = "Softmax"
GENRE_ID = 4                # include/kge_hip.h KGE_LOSS_SOFTMAX


def softmax_fwd_bwd(pos, neg, w=None):
    """the statement, in the dtype of `pos`.  Returns ((nan, nan, loss), dL/dpos [B], dL/dneg [B, N]) like O.loss_fwd_bwd"""
    dt = pos.dtype
    B, N = neg.shape
    wv = np.ones(B, dt) if w is None else np.asarray(w).reshape(B).astype(dt)
    m = np.maximum(pos, neg.max(1))
    ep, en = np.exp(pos - m), np.exp(neg - m[:, None])
    s = en.sum(1)
    Z = ep + s
    l = m + np.log(Z) - pos
    # (a dominating positive: log Z = log1p(s) keeps the digits that 1 + s drops)
    dom = ep == 1
    l = np.where(dom, np.log1p(s), l)
    loss = (wv * l).sum() / dt.type(B)
    dneg = (wv / dt.type(B) / Z)[:, None] * en
    dpos = -(wv / dt.type(B)) * s / Z
    return (np.nan, np.nan, loss), dpos.astype(dt), dneg.astype(dt)


_ORIGINAL = O.loss_fwd_bwd


def hooked_loss_fwd_bwd(pos, neg, w=None, genre="Logsigmoid", adv=False, adv_temp=1.0, pairwise=False, margin=1.0):
    if genre == GENRE:
        assert not adv and not pairwise, "Softmax has no -adv and no -pw form"
        return softmax_fwd_bwd(pos, neg, w)
    return _ORIGINAL(pos, neg, w, genre, adv, adv_temp, pairwise, margin)


def hook(monkeypatch):
    monkeypatch.setattr(O, "loss_fwd_bwd", hooked_loss_fwd_bwd)


# --------------------------------------------------------------------------------------------------------------------------
# 1. the loss op: one N per instance of the loss kernel (launch_loss, csrc/kge_rowwise.hip)
# --------------------------------------------------------------------------------------------------------------------------
def loss_instance(N, aligned):
    """the kernel instance launch_loss takes for N columns; aligned: the score / gradient arrays start on 16-byte boundaries (the
    packed layout needs that and N % 4 == 0)"""
    pk = aligned and N % 4 == 0
    if pk and N <= 256:
        return "one pack"
    if pk and N <= 512:
        return "two packs"
    for nper in (1, 2, 4, 8):
        if N <= 64 * nper:
            return "strided NPER %d" % nper
    return "streaming"


# N, aligned (False: the test hands the op a score array that starts 4 bytes behind a 16-byte boundary), the instance it must take
OP_SHAPES = [
    (1, True, "strided NPER 1"), (5, True, "strided NPER 1"), (64, False, "strided NPER 1"), (65, True, "strided NPER 2"),
    (128, False, "strided NPER 2"), (130, True, "strided NPER 4"), (200, True, "one pack"), (256, True, "one pack"),
    (257, True, "strided NPER 8"), (260, True, "two packs"), (512, True, "two packs"), (513, True, "streaming"),
    (600, True, "streaming"),
]
OP_B = (1, 7, 130)
HARD = ("all-equal", "positive+60", "negative+60", "around+80", "around-80", "negative+60-at+80")


def _hard_row(kind, N, rng):
    """(p, n [N]): rows a softmax without the max subtraction, or dL/dp as 1 - e_p / Z, gets wrong"""
    noise = rng.normal(0.0, 1.0, N)
    if kind == "all-equal":
        return 3.25, np.full(N, 3.25)
    if kind == "positive+60":
        return float(noise.max() + 60.0), noise
    if kind == "negative+60":
        n = noise.copy()
        n[N // 2] = noise.max() + 60.0
        return float(rng.normal()), n
    if kind == "around+80":
        return float(80.0 + rng.normal()), 80.0 + noise
    if kind == "around-80":
        return float(-80.0 + rng.normal()), -80.0 + noise
    n = 80.0 + noise
    n[N - 1] = n.max() + 60.0
    return float(80.0 + rng.normal()), n


def op_inputs(B, N, weights):
    """float32 (pos [B], neg [B, N], w [B] or None): scores N(0, 2), the first rows replaced by the HARD rows (B = 1: one of them,
    chosen by N, so that the thirteen shapes walk all six)"""
    rng = np.random.RandomState(1000 * B + N)
    pos = rng.normal(0.0, 2.0, B)
    neg = rng.normal(0.0, 2.0, (B, N))
    kinds = HARD if B >= len(HARD) else (HARD[[s[0] for s in OP_SHAPES].index(N) % len(HARD)],)
    for i, kind in enumerate(kinds):
        pos[i], neg[i] = _hard_row(kind, N, rng)
    w = rng.uniform(0.5, 1.5, B).astype(np.float32) if weights else None
    return pos.astype(np.float32), neg.astype(np.float32), w


# --------------------------------------------------------------------------------------------------------------------------
# 2. the fused step.  Shapes, gamma and scale are those of tests/loss_option_cases.py: scores of mean ~0 and standard deviation
#    1.5 - 2 on both sides, so that with 10 .. 600 negatives per row a negative carries the largest softmax weight in most rows
#    and no row's gradient vanishes (asserted from the float64 statement by tests/test_softmax_loss_inputs.py)
# --------------------------------------------------------------------------------------------------------------------------
def case(cid, shape, **kw):
    return L.case(cid, shape, GENRE, adv=False, **kw)


def _flags(shape):
    return L.GEMM_FLAGS if L.SHAPES[shape][0] in L.GEMM_MODELS else (0,)


# regulariser: the coefficient of loss_option_cases' cfgD-reg2 (>= 1 % of the largest gradient component: asserted)
STEP_CASES = [case(sh + "-softmax", sh, flags=_flags(sh)) for sh in ("cfgT", "cfgD", "complex", "rotate", "l1", "simple")] + [
    case("rescal-softmax", "rescal"),
    case("transr-softmax", "transr", rows=5e-3),
    case("n288-softmax", "n288", rows=5e-3),
    case("n600-softmax", "n600", rows=5e-3),
    case("t600-softmax", "t600", rows=5e-3),
    case("odd-softmax", "odd", rows=5e-3),
    case("oddD-softmax", "oddD", rows=5e-3),
    case("midT-nd-softmax", "midT", neg_deg=True, rows=5e-3),
    case("midR-nd-softmax", "midR", neg_deg=True, rows=5e-3),
    case("midT-impts-softmax", "midT", impts=True, rows=5e-3),
    case("midD-impts-softmax", "midD", impts=True, flags=(0, L.FUSED_LOSS), rows=5e-3),
    case("cfgD-reg2-softmax", "cfgD", reg_norm=2, reg_coef=2e-5),
]
# the instance of the loss kernel a step case must reach (the step's score block is 256-byte aligned: packed where N % 4 == 0)
STEP_INSTANCE = {"cfgT": "one pack", "cfgD": "one pack", "complex": "one pack", "rotate": "one pack", "l1": "one pack",
                 "simple": "one pack", "rescal": "one pack", "transr": "strided NPER 2", "n288": "two packs", "n600": "streaming",
                 "t600": "streaming", "odd": "strided NPER 1", "oddD": "strided NPER 1", "midT": "one pack", "midR": "one pack",
                 "midD": "one pack"}


def step_N(c):
    """columns of a row as the loss kernel sees it"""
    return c["chunk"] + c["N"] if c["neg_deg"] else c["N"]


def row_stats(pos, neg, w=None):
    """from the float64 statement: (share of rows in which a negative carries the largest softmax weight, largest |dL/dn| * B / w)"""
    pos, neg = np.asarray(pos, np.float64), np.asarray(neg, np.float64).reshape(len(pos), -1)
    _, _, dneg = softmax_fwd_bwd(pos, neg, None)
    return float((neg.max(1) > pos).mean()), float(dneg.max() * len(pos))


# 3. --exclude_positive: tests/known_negative_cases.py's TransE_l2 (400 wide, 200 negatives: one pack) and RotatE cases, genre Softmax
def known_case(cid):
    import known_negative_cases as KN
    c = [x for x in KN.CASES if x["id"] == cid][0]
    return dict(c, id=cid + "-softmax", genre=GENRE, adv=False, pairwise=False)


KNOWN_IDS = ("l2-d400-n200-adv", "rotate-d32-n40-adv")
