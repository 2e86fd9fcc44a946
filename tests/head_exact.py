"""Inputs, models and conditions that hold the Linear head + cross entropy family (csrc/head_common.h and the kernels written on it:
head_gs_sgd.hip, concat_head.hip, qmf_head.hip, feature_step.hip) to a reference at every regime of its loops.
test_head_exact_cpu.py proves the conditions, test_head_exact_gpu.py runs the kernels.  Not product code.

The families share head_row_dot, head_softmax2, head_ce_grad and head_col_sum, so comparing them with each other
(test_head_family_gpu.py) cannot see an error in a helper.  Four input classes compare them with something else:

  LIN    X, W nonzero multiples of 1/4 with |v| <= 3/4, bias a multiple of 1/4, a given dlogits of nonzero multiples of 2^-6 with
         |g| <= 7/64, scale 1 or 0.5.  Every product of a sum is a multiple of one unit and sum |terms| < 2^24 units
         (exact.assert_sum_budget), so logits, dW, db and dX are the mathematically exact values bit for bit in ANY summation order.
  SAT    LIN plus seven feature columns that carry an amplitude-32 +-1 code: in X the code of the row's winner class, in W the code of
         each class.  The winner's logit beats every other by 2 * 32^2 minus the noise of the other columns, asserted >= 128.  Then
         expf(l - max) is exactly 0 off the winner (exp(-128) = 2.6e-56 is far below half the smallest fp32 subnormal), s = 1,
         lse = max, p is one-hot, the row loss is (max - l[label]) * inv and dlogits is 0 or +-inv.  With inv = 2^-7 the whole fused
         call -- loss, dlogits, dW, db, dX, and the feature phase's momentum and updated head at lr = 2^-3 -- is exact bit for bit.
         (Assumes logf(1.0f) == 0 and a correctly rounded 1.0f / 1.0f on the device.)
  UNI    W = 0 and a constant bias: every logit of a row is equal, e = 1 for every class, s = C exactly, p = fl(1 / C) is one
         correctly rounded division, dlogits = (fl(1 / C) - onehot) * 2^-7 one more rounding: bit-equal to the float32 restatement.
         A softmax slot or a 64-trip missing from s makes it 64 or 128 instead of C.
  DENSE  the numerics: exact_tokens.softmax_scores' five families for the standalone cross entropy, head-like random inputs for the
         fused calls, against fp64 on the same fp32 inputs at the tolerances the suite already uses (cited where they are applied).

The models take `fault=`: the errors these inputs exist for, restated in plain Python.  FAULTS names, for each, where it is reached
and which class and entry point prove it; the CPU test asserts that the faulty model differs there on EVERY table shape."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import qmf_model as Q
from exact import assert_sum_budget, case_seed, rand_ints
from exact_tokens import softmax_scores
from oracle import mla_oracle as O

INV = 2.0 ** -7          # inv_batch of the exact classes: the API takes any value, and a power of two keeps loss and dlogits exact
LR = 2.0 ** -3           # feature phase, SAT: p - lr * buf is exact
AMP = 32.0               # amplitude of the SAT code
NBITS = 7                # code bits: 2^7 = MLA_HEAD_MAXC classes
MARGIN = 128.0           # SAT condition: top logit - runner-up
F64, F32 = torch.float64, torch.float32

# (B, D, C).  B: 1, 3, 5 (four rows per workgroup of ce_fwd_bwd / head_logits), 64, 65, 130 (first, second, third trip of
# head_col_sum).  D: 8, 63, 64, 65, 70 (lane tail of head_row_dot), 256, 257, 320 (full / one-element / partial second 256-column
# block).  C: 1, 2, 3 (fewer classes than waves), 17 (more than the 16 waves of the feature phase), 63, 64, 65 (slot boundary),
# 127, 128 (limit).  Every value at least twice; B = 130, D = 257 and C = 128 meet each other (test_head_exact_cpu.py).
TABLE = [(1, 8, 1), (1, 70, 128), (3, 63, 2), (3, 257, 17), (5, 64, 3), (5, 65, 63), (5, 257, 128), (64, 70, 64),
         (64, 256, 65), (64, 8, 127), (65, 65, 65), (65, 320, 3), (65, 63, 128), (65, 256, 17), (130, 257, 65), (130, 70, 128),
         (130, 320, 64), (130, 64, 1), (130, 8, 2), (3, 320, 127), (64, 257, 63), (1, 256, 2), (3, 70, 1), (5, 63, 17)]
# C past MLA_HEAD_MAXC, for the entry points that accept any C (ce_fwd_bwd, head_bwd, head_logits): third and fifth 64-trip
WIDE = [(5, 70, 129), (65, 257, 200), (3, 64, 257), (130, 8, 257), (64, 65, 129), (1, 320, 200)]
# modalities of the concat / QMF cases, by position in TABLE: M * D = 3 * 70 (one partial block, boundaries inside), 2 * 320 and
# 3 * 257 (boundaries spread over blocks) are among them
MODS = [2 + i % 2 for i in range(len(TABLE))]
# (M, B, D, C, n_data) of qmf_head_fwd_bwd, DENSE
QMF_DENSE = [(2, 65, 70, 65, 200), (3, 130, 64, 3, 131), (2, 5, 257, 128, 7)]
SCALES = (1.0, 0.5)
CE_FAMILIES = ("normal", "wide", "equal", "spike", "low")

# fault -> (reached(B, D, C, M, scale), class, entry point that proves it)
FAULTS = {
    "colsum_64": (lambda B, D, C, M, s: B > 64, "LIN", "head_bwd db"),                 # head_col_sum stops after 64 rows
    "colsum_stride63": (lambda B, D, C, M, s: B >= 64, "LIN", "head_bwd db"),          # head_col_sum strides 63 rows
    "lane_tail": (lambda B, D, C, M, s: D % 64 != 0, "LIN", "head_logits"),            # head_row_dot drops d >= D - D % 64
    "slot2_sum": (lambda B, D, C, M, s: C > 64, "UNI", "ce_fwd_bwd dlogits"),          # second softmax slot missing from s
    "slot2_max": (lambda B, D, C, M, s: C > 64, "SAT", "head_ce_fwd_bwd"),             # second slot missing from the maximum
    "partial_block": (lambda B, D, C, M, s: (M * D) % 256 != 0, "LIN", "head_bwd / concat_head_bwd dW, dX"),
    "ce_trip3": (lambda B, D, C, M, s: C > 128, "UNI", "ce_fwd_bwd dlogits"),          # ce_fwd_bwd drops classes [128, 192)
    "concat_mod256": (lambda B, D, C, M, s: M > 1 and D != 256, "LIN", "concat_head_bwd dW, dx"),   # column j -> modality j // 256
    "no_scale": (lambda B, D, C, M, s: s != 1.0, "LIN", "head_bwd / concat_head_bwd"),
}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _quarters(shape, seed):
    return (rand_ints(shape, -3, 3, seed, nonzero=True).double() / 4).float()


def _units(t, unit):
    """|t| / unit as int64; t must lie on the grid."""
    q = t.double().abs() / unit
    assert torch.equal(q, q.round()), "operand off its grid"
    return q.long()


@functools.lru_cache(maxsize=None)
def lin_case(B, D, C, M=1, salt=0):
    """xs[m] (B, D), W (C, M * D), b (C), dl (B, C); never written to.  M = 3: zero bias, so out_m = s_m + b * fl(1 / 3) needs no
    restatement of that rounding; M = 2: b / 2 is exact.
    dl is arranged so that the head_col_sum faults change db in EVERY column: the sum over the rows from 64 on is non-zero, and so is
    dl[63] + dl[126], the rows a stride of 63 counts twice."""
    seed = case_seed(B, D, C, M, salt) * 16
    xs = [_quarters((B, D), seed + 1 + m) for m in range(M)]
    W = _quarters((C, M * D), seed + 5)
    b = torch.zeros(C) if M == 3 else _quarters((C,), seed + 6)
    dli = rand_ints((B, C), -7, 7, seed + 7, nonzero=True)
    if B > 126:
        dli[126] = dli[126].abs() * torch.sign(dli[63])
    if B > 64:
        dli[64] = torch.where(dli[64:].sum(0) == 0, -dli[64], dli[64])
        assert (dli[64:].sum(0) != 0).all()
    dl = (dli.double() / 64).float()
    X, Xu, Wu = torch.cat(xs, 1), _units(torch.cat(xs, 1), 0.25), _units(W, 0.25)
    budget = {"logits": assert_sum_budget(Xu @ Wu.T + _units(b, 1.0 / 16), f"LIN logits {B, D, C, M}"),      # units of 1/16
              "dW": assert_sum_budget(dli.abs().T @ Xu, f"LIN dW {B, D, C, M}"),                               # units of 2^-8
              "dX": assert_sum_budget(dli.abs() @ Wu, f"LIN dX {B, D, C, M}"),
              "db": assert_sum_budget(dli.abs().sum(0), f"LIN db {B, D, C, M}")}                               # units of 2^-6
    return SimpleNamespace(B=B, D=D, C=C, M=M, xs=xs, X=X, W=W, b=b, dl=dl, budget=budget)


def code_cols(D):
    """Seven columns of [0, D): the first and last, both sides of 63|64 and 255|256 where D has them, then inwards from the ends."""
    cand = [0, D - 1, 63, 64, 255, 256] + [v for k in range(1, 8) for v in (k, D - 1 - k)]
    cols = []
    for c in cand:
        if 0 <= c < D and c not in cols:
            cols.append(c)
    assert len(cols) >= NBITS, "SAT needs D >= 7"
    return cols[:NBITS]


def code_of(classes):
    """(n,) class indices -> (n, 7) code: bit k set -> +AMP, clear -> -AMP."""
    bits = (torch.as_tensor(classes).long().reshape(-1, 1) >> torch.arange(NBITS)) & 1
    return (bits.double() * 2 - 1).float() * AMP


def sat_hit(r):
    """Rows whose label is the winner (zero gradient row, zero loss); both kinds occur among rows 0, 63, 64 and B - 1."""
    return r % 3 == 0 if r < 63 else (r + 1) % 3 == 0


@functools.lru_cache(maxsize=None)
def sat_case(B, D, C, M=1, salt=0):
    """LIN with the code in modality 0's columns.  Winners: pseudo-random, row 0's is C - 1 (the second softmax slot when C > 64).
    Labels: the winner (sat_hit rows, and everywhere when C = 1), else the winner with one SET code bit cleared -- a smaller index, so
    below C -- or class 1 for winner 0: the runner-up, 2 * 32^2 below the winner."""
    lin = lin_case(B, D, C, M, salt)
    seed = case_seed(B, D, C, M, salt) * 16
    win = rand_ints((B,), 0, C - 1, seed + 8)
    win[0] = C - 1
    labels = win.clone()
    for r in range(B):
        if C == 1 or sat_hit(r):
            continue
        w = int(win[r])
        setbits = [k for k in range(NBITS) if w >> k & 1]
        labels[r] = w ^ (1 << setbits[r % len(setbits)]) if setbits else 1
    assert int(labels.min()) >= 0 and int(labels.max()) < C
    cols = code_cols(D)
    xs = [x.clone() for x in lin.xs]
    W = lin.W.clone()
    xs[0][:, cols] = code_of(win)
    W[:, cols] = code_of(torch.arange(C))
    X = torch.cat(xs, 1)
    out64 = X.double() @ W.double().T + lin.b.double()
    top = out64.topk(min(2, C), dim=1).values
    margin = (top[:, 0] - top[:, 1]).min().item() if C > 1 else float("inf")
    rowloss_u = ((top[:, 0] - out64[torch.arange(B), labels]) * 16).long()               # units of 2^-4 * INV
    budget = {"logits": assert_sum_budget(_units(X, 0.25) @ _units(W, 0.25).T + _units(lin.b, 1.0 / 16), f"SAT logits {B, D, C, M}"),
              "loss": assert_sum_budget(rowloss_u.abs().sum(), f"SAT loss {B, D, C, M}"),
              # dlogits is 0 or +-INV: one unit of INV / 4 per quarter of X or W
              "dW": assert_sum_budget(_units(X, 0.25).sum(0).max(), f"SAT dW {B, D, C, M}"),
              "dX": assert_sum_budget(2 * _units(W, 0.25).max(), f"SAT dX {B, D, C, M}")}
    return SimpleNamespace(B=B, D=D, C=C, M=M, xs=xs, X=X, W=W, b=lin.b, labels=labels, win=win, margin=margin, budget=budget)


@functools.lru_cache(maxsize=None)
def uni_case(B, D, C):
    lin = lin_case(B, D, C)
    return SimpleNamespace(B=B, D=D, C=C, M=1, xs=lin.xs, X=lin.X, W=torch.zeros_like(lin.W), b=torch.full((C,), 0.75),
                           logits=torch.full((B, C), 0.75), labels=O.portable_labels(case_seed(B, D, C), B, C))


@functools.lru_cache(maxsize=None)
def dense_case(B, D, C, M=1):
    """Head-like random inputs, scaled so that softmax rows are neither flat nor saturated."""
    seed = case_seed(B, D, C, M) + 7000
    xs = [O.portable_normal(seed + m, (B, D), stream=31, mean=0.3, std=0.7) for m in range(M)]
    hd = O.make_head_params(M * D, C, seed + 10)
    return SimpleNamespace(B=B, D=D, C=C, M=M, xs=xs, X=torch.cat(xs, 1), W=hd["weight"] * 8, b=hd["bias"] * 8,
                           labels=O.portable_labels(seed, B, C))


@functools.lru_cache(maxsize=None)
def dense_ce_case(B, C, family):
    """(B, C) logits of one of exact_tokens.softmax_scores' families (one row of a C x C score matrix per sample) and labels that
    alternate between the row's largest class (the spike) and the next one."""
    logits = softmax_scores(C, family, case_seed(B, C, CE_FAMILIES.index(family)), B=1, H=B)[0, :, 0, :].contiguous()
    top = logits.argmax(1)
    labels = torch.where(torch.arange(B) % 2 == 0, top, (top + 1) % C)
    return SimpleNamespace(B=B, C=C, logits=logits, labels=labels, top=top)


def with_bad_labels(labels, C):
    """-1 at row 0 and C at row B - 1 (one row: -1)."""
    bad = labels.clone()
    bad[-1] = C
    bad[0] = -1
    return bad


# ---- models: plain torch in `dt` (fp64; fp32 for the restatements), every sum in whatever order torch likes ---------------------------
def col_sum(v, fault=None):
    """head_col_sum over the rows of v."""
    n = v.shape[0]
    if fault == "colsum_64":
        return v[:64].sum(0)
    if fault == "colsum_stride63":
        return v[[r for t in range(64) for r in range(t, n, 63)]].sum(0)
    return v.sum(0)


def row_dot(X, W, fault=None):
    """head_row_dot for every (row, class)."""
    if fault == "lane_tail":
        k = X.shape[1] - X.shape[1] % 64
        return X[:, :k] @ W[:, :k].T
    return X @ W.T


def logits_model(X, W, b, fault=None, dt=F64):
    return row_dot(X.to(dt), W.to(dt), fault) + b.to(dt)


def ce_model(logits, labels, inv, fault=None, dt=F64):
    """Mean-reduced cross entropy as the kernels form it: rowloss (B), dlogits (B, C), loss.  A label outside [0, C): NaN row loss,
    zero dlogits row."""
    l = logits.to(dt)
    B, C = l.shape
    in_max = torch.ones(C, dtype=torch.bool)
    in_sum = torch.ones(C, dtype=torch.bool)
    if fault == "slot2_max":
        in_max[64:] = False
    if fault == "slot2_sum":
        in_sum[64:] = False
    if fault == "ce_trip3":
        in_max[128:192] = False
        in_sum[128:192] = False
    m = l[:, in_max].max(1).values
    e = torch.exp(l - m[:, None])
    s = e[:, in_sum].sum(1)
    labels = torch.as_tensor(labels).long()
    ok = (labels >= 0) & (labels < C)
    lab = labels.clamp(0, C - 1)
    onehot = torch.zeros((B, C), dtype=dt)
    onehot[torch.arange(B), lab] = 1
    nan = torch.full((B,), float("nan"), dtype=dt)
    rowloss = torch.where(ok, (torch.log(s) - (l[torch.arange(B), lab] - m)) * inv, nan)
    dl = torch.where(ok[:, None], (e / s[:, None] - onehot) * inv, torch.zeros((), dtype=dt))
    if fault == "ce_trip3":
        dl[:, 128:192] = float("nan")                                   # never written
    return rowloss, dl, col_sum(rowloss, fault)


def bwd_model(xs, W, dl, scale=1.0, fault=None, dt=F64):
    """autograd of the (concatenated) Linear for a given dlogits: dW (C, M * D), db (C), [dx_m (B, D)]."""
    M, D = len(xs), xs[0].shape[1]
    X, W, dl = torch.cat(xs, 1).to(dt), W.to(dt), dl.to(dt)
    MD = M * D
    dcat = dl @ W
    if fault == "concat_mod256":                                        # column j read from / written to modality j // 256
        j = torch.arange(MD)
        m_bad = (j // 256).clamp(max=M - 1)
        col = (j - m_bad * D) % D
        X = X[:, m_bad * D + col]
        moved = torch.full_like(dcat, float("nan"))
        moved[:, m_bad * D + col] = dcat
        dcat = moved
    dW, db = dl.T @ X, col_sum(dl, fault)
    if fault != "no_scale":
        dW, db, dcat = dW * scale, db * scale, dcat * scale
    if fault == "partial_block" and MD % 256:
        k = MD - MD % 256
        dW[:, k:] = float("nan")
        dcat[:, k:] = float("nan")
    return dW, db, [dcat[:, m * D:(m + 1) * D] for m in range(M)]


def head_model(X, W, b, labels, inv, fault=None, dt=F64):
    """mla_head_ce_fwd_bwd."""
    logits = logits_model(X, W, b, fault, dt)
    rowloss, dl, loss = ce_model(logits, labels, inv, fault, dt)
    dW, db, (dX,) = bwd_model([X], W, dl, 1.0, fault, dt)
    return SimpleNamespace(logits=logits, rowloss=rowloss, dl=dl, loss=loss, dW=dW, db=db, dX=dX)


def concat_fwd_model(xs, W, b, fault=None, dt=F64):
    """out (B, C), out_m (M, B, C) = s_m + b * (1 / M)."""
    M, D = len(xs), xs[0].shape[1]
    s = [row_dot(xs[m].to(dt), W[:, m * D:(m + 1) * D].to(dt), fault) for m in range(M)]
    b = b.to(dt)
    return sum(s) + b, torch.stack([t + b * torch.tensor(1.0 / M, dtype=torch.float32).to(dt) for t in s])


def concat_model(xs, W, b, labels, inv, fault=None, dt=F64):
    """mla_concat_head_ce_fwd_bwd."""
    out, out_m = concat_fwd_model(xs, W, b, fault, dt)
    rowloss, dl, loss = ce_model(out, labels, inv, fault, dt)
    loss_m = torch.stack([ce_model(o, labels, inv, fault, dt)[2] for o in out_m])
    dW, db, dxs = bwd_model(xs, W, dl, 1.0, fault, dt)
    return SimpleNamespace(out=out, out_m=out_m, dl=dl, loss=loss, loss_m=loss_m, dW=dW, db=db, dxs=dxs)


def feature_model(X, W, b, labels, inv, lr, fault=None, dt=F64):
    """mla_feature_phase with project = 0, first = 1, wd = 0: buf is the raw gradient of [W | b], the head moves by -lr * buf."""
    h = head_model(X, W, b, labels, inv, fault, dt)
    return SimpleNamespace(logits=h.logits, loss=h.loss, dl=h.dl, buf=torch.cat([h.dW.reshape(-1), h.db]),
                           W=W.to(dt) - lr * h.dW, b=b.to(dt) - lr * h.db)


def exact32(t):
    """fp64 -> fp32; nothing may round on the way (NaN stays NaN)."""
    f = t.float()
    assert torch.equal(f.double().nan_to_num(nan=12345.0), t.double().nan_to_num(nan=12345.0)), "an exact value is not representable in fp32"
    return f


def differs(a, b, unit):
    """The largest |a - b| is at least one unit, or one side is NaN where the other is not."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    if (torch.isnan(a) != torch.isnan(b)).any():
        return True
    d = (a - b).nan_to_num().abs().max().item()
    return d >= unit


# ---- qmf_head_fwd_bwd, DENSE --------------------------------------------------------------------------------------------------------
QMF_STEPS = 2
QMF_DECISION = 1e-4        # test_qmf_cpu.py::test_fixture_input_conditions: every ranking decision this far from its threshold


def _qmf_inputs(M, B, D, C, n_data, seed):
    """qmf_model.head_inputs with the heads times 8: the confidences E / 10 then differ by tenths, as the normalised History margins do,
    so the hinge is active for many pairs and the ranking loss is of the size of its terms.  (At the fixture's scale the confidences
    differ by hundredths, nearly every hinge is inactive, and what is left of the ranking loss is below the fp32 rounding of one
    confidence: 2e-5 of it is no bound a correct kernel can keep.)"""
    _, Ws, bs = Q.head_inputs(O, seed, M, B, D, C)
    Ws, bs = [W * 8 for W in Ws], [b * 8 for b in bs]
    steps = []
    for s in range(QMF_STEPS):
        xs = Q.head_inputs(O, seed + 1 + s, M, B, D, C)[0]
        idx = rand_ints((B,), 0, n_data - 1, seed * 8 + s)
        idx[B - 1] = idx[B // 2]                                        # an index twice in one batch: the last occurrence writes
        steps.append(SimpleNamespace(xs=xs, labels=O.portable_labels(seed + s, B, C), idx=idx))
    return Ws, bs, steps


def qmf_decisions(r):
    """(margin, hinge argument t (c_i - r_i), target) of one model step, all (M, B), fp64."""
    t, mg, conf = r["target"], r["margin"].float().double(), r["conf"]
    ha = t * (conf - (torch.roll(conf, -1, 1) + mg / torch.where(t == 0, torch.ones_like(t), t)))
    return r["margin"], ha, t


@functools.lru_cache(maxsize=None)
def qmf_dense_case(M, B, D, C, n_data, form="av"):
    """Two consecutive steps whose every ranking decision in the fp64 model is more than QMF_DECISION from its threshold (the first
    seed of 64 that holds), with the model's results."""
    w_cml, w_crl = Q.FORMS[form]
    for seed in range(100 * M + B, 100 * M + B + 64):
        Ws, bs, steps = _qmf_inputs(M, B, D, C, n_data, seed)
        hists = [Q.History(n_data) for _ in range(M)]
        good = True
        for st in steps:
            st.ref = Q.qmf_step(st.xs, Ws, bs, st.labels, st.idx, hists, w_cml, w_crl)
            st.hist = (np.stack([h.correctness for h in hists]).copy(), np.stack([h.confidence for h in hists]).copy())
            mg, ha, t = qmf_decisions(st.ref)
            good = good and bool(torch.isfinite(mg).all() and (mg[mg != 0] > QMF_DECISION).all() and (ha[t != 0].abs() > QMF_DECISION).all())
        if good:
            return SimpleNamespace(M=M, B=B, D=D, C=C, n_data=n_data, seed=seed, Ws=Ws, bs=bs, steps=steps, w_cml=w_cml, w_crl=w_crl)
    raise AssertionError(f"qmf_dense_case {M, B, D, C, n_data}: no seed keeps every ranking decision {QMF_DECISION} from its threshold")
