"""The per-sample evaluation rule of mla_eval_head (csrc/eval_head.hip), restated on the CPU: gating, presence, fusion, first-maximum
arg-max and counters, one row at a time.  numpy; fp64 by default, fp32 on request (the arithmetic of the kernel, for the conditions
that only exist in fp32: an exp that underflows to exactly 0).

tests/test_eval_head_cpu.py holds this restatement to the reference's own expressions applied to a 1-D row
(oracle.mla_oracle.gating_weights: on a vector, softmax(dim=0) IS the sample's class distribution);
tests/test_eval_head_gpu.py holds the kernel to it."""
from types import SimpleNamespace

import numpy as np

import tail_model as T
from oracle import mla_oracle as O

F32, F64 = np.float32, np.float64

# (M, B, C) of the dense sample-mode cases: a partial workgroup, one row, the second softmax slot (65), the cap (128), M = 2 and 3
SAMPLE_DENSE = [(2, 32, 6), (3, 7, 8), (2, 1, 3), (3, 65, 101), (2, 5, 65), (3, 130, 128), (2, 3, 2), (3, 64, 4)]
WEIGHT_TOL = 1e-5                   # the project's tolerance on fusion weights (tests/test_eval_gpu.py, tests/test_tail_gpu.py)
SATURATED = 200.0                   # one logit this far above the rest: exp(-200) is exactly 0 in fp32


def identity_head(C):
    """W = I (C, C), b = 0: with features equal to the wanted logits every dot has one non-zero term, so the kernel's logits ARE
    those values and every logits-level design of tail_model can be fed through the fused kernel."""
    return np.eye(C, dtype=F32), np.zeros(C, dtype=F32)


def row_entropy(l, dtype=F64):
    """H = - sum_c p_c lp_c of one row as the kernel forms it: lp = (l - max) - log sum exp(l - max), p = e / s; a class whose
    exp is exactly 0 contributes 0, its limit."""
    l = np.asarray(l, dtype=dtype)
    sh = l - l.max()
    e = np.exp(sh)
    s = e.sum(dtype=dtype)
    lp = sh - np.log(s)
    t = np.where(e != 0, (e / s) * lp, dtype(0))
    return dtype(0) - t.sum(dtype=dtype)


def row_weights(logits, mode, alphas, eligible, dtype=F64):
    """The fusion weights of one row: logits = [l_0 .. l_{M-1}] (C,), eligible (M,) bool.  mode 1: g_m = exp(max_k H_k - H_m) over the
    eligible modalities, w = g / sum g; mode 0: alpha_m, renormalised over the eligible ones when one is absent.  Absent: +0.0."""
    M = len(logits)
    el = np.asarray(eligible, dtype=bool)
    w = np.zeros(M, dtype=dtype)
    if mode == 1:
        H = np.array([row_entropy(l, dtype) for l in logits], dtype=dtype)
        g = np.where(el, np.exp(H[el].max() - H), dtype(0)).astype(dtype)
        w[el] = g[el] / g.sum(dtype=dtype)
    elif el.all():
        w[:] = np.asarray(alphas[:M], dtype=dtype)
    else:
        a = np.asarray(alphas[:M], dtype=dtype)
        w[el] = a[el] / a[el].sum(dtype=dtype)
    return w


def eval_rows(outs, label, mode, alphas, present=None, dtype=F64):
    """outs: M arrays (B, C); label (B,); present (B, M) or None.  -> weights (B, M), fused (B, C), pred (B, 1 + M) int64,
    counts (2 + M, C) int64, bad (B,) bool.  A row whose label lies outside [0, C), that has no present modality or (mode 0, a
    modality absent) whose eligible alphas do not sum above 0 is counted nowhere: NaN weights and fused row, pred -1."""
    outs = [np.asarray(o, dtype=dtype) for o in outs]
    M, (B, C) = len(outs), outs[0].shape
    label = np.asarray(label)
    have = np.ones((B, M), dtype=bool) if present is None else np.asarray(present) != 0
    weights = np.full((B, M), np.nan, dtype=dtype)
    fused = np.full((B, C), np.nan, dtype=dtype)
    pred = np.full((B, 1 + M), -1, dtype=np.int64)
    counts = np.zeros((2 + M, C), dtype=np.int64)
    bad = np.zeros(B, dtype=bool)
    for r in range(B):
        no_share = mode == 0 and not have[r].all() and not np.asarray(alphas[:M], dtype=F64)[have[r]].sum() > 0
        if not 0 <= label[r] < C or not have[r].any() or no_share:
            bad[r] = True
            continue
        rows = [o[r] for o in outs]
        w = row_weights(rows, mode, alphas, have[r], dtype)
        v = np.zeros(C, dtype=dtype)
        for m in range(M):                                   # modalities in order
            v = v + w[m] * rows[m]
        weights[r], fused[r] = w, v
        pred[r] = [int(np.argmax(v))] + [int(np.argmax(x)) for x in rows]          # numpy.argmax: the first maximum
        counts[0, label[r]] += 1
        for k in range(1 + M):
            counts[1 + k, label[r]] += int(pred[r, k] == label[r])
    return SimpleNamespace(weights=weights, fused=fused, pred=pred, counts=counts, bad=bad)


def top2_margin(fused):
    """Smallest gap between the largest and the second largest fused logit over the (good) rows."""
    f = np.asarray(fused, dtype=F64)
    f = f[~np.isnan(f).any(axis=1)]
    if f.shape[1] < 2 or f.shape[0] == 0:
        return float("inf")
    top = np.sort(f, axis=1)
    return float((top[:, -1] - top[:, -2]).min())


def sample_dense_case(M, B, C):
    """Dense normal logits (std 1.5) per modality and labels: a pure function of (M, B, C)."""
    outs = [O.portable_normal(9500 + 10 * B + C + m, (B, C), stream=63, std=1.5).numpy() for m in range(M)]
    return outs, O.portable_labels(9500 + B + C, B, C).numpy()


def saturated_row(C, at):
    """One logit SATURATED above the rest: entropy exactly 0 in fp32."""
    l = np.zeros(C, dtype=F32)
    l[at] = SATURATED
    return l


def every_pattern(B, M=3):
    """(B, M) uint8 cycling through every non-empty presence pattern, all-present first."""
    pats = [[(p >> m) & 1 for m in range(M)] for p in range(2 ** M - 1, 0, -1)]
    return np.array([pats[r % len(pats)] for r in range(B)], dtype=np.uint8)


def fused_tol(M, outs):
    """The weight tolerance carried through the sum: M * 1e-5 * max |logit| (rounding of the sum itself is far below it)."""
    return M * WEIGHT_TOL * max(float(np.abs(o).max()) for o in outs)


EVAL_MARGIN = T.EVAL_MARGIN
