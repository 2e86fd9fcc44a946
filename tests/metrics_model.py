"""Restatement of csrc/metrics.hip in numpy, fp64: average precision in the kernel's exact order (`ap_ordered`), the textbook
threshold sweep it must agree with (`ap_by_thresholds`), confusion counts, the fp64 softmax the stored scores are measured against,
and the inputs the CPU and GPU tests share.

Scores are class-major, (H, C, cap) fp32, as the store keeps them; labels (cap) integers; the first N rows count."""
import numpy as np

F32, F64 = np.float32, np.float64
_LANES = np.arange(64)


def ap_terms(scores, labels, N):
    """(H, N) fp64: row r's term TP(>= s) / CNT(>= s) at its own score s = scores[h][c][r] in its own class c = labels[r], both counts
    over the rows below N; 0.0 where the label is no class or where no score is >= s (s is NaN)."""
    H, C, _cap = scores.shape
    lab = np.asarray(labels)[:N].astype(np.int64)
    terms = np.zeros((H, N), dtype=F64)
    with np.errstate(invalid="ignore"):
        for h in range(H):
            for c in range(C):
                rows = np.flatnonzero(lab == c)
                if rows.size == 0:
                    continue
                col = scores[h, c, :N]
                ge = col[None, :] >= col[rows][:, None]                       # (P, N); a NaN is >= nothing, nothing is >= it
                cnt = ge.sum(axis=1).astype(np.int64)
                tp = (ge & (lab == c)[None, :]).sum(axis=1).astype(np.int64)
                terms[h, rows] = np.where(cnt > 0, tp.astype(F64) / np.maximum(cnt, 1).astype(F64), 0.0)
    return terms


def wave_sum(lanes):
    """The xor butterfly of wave_sum_d over 64 lane values: offsets 32, 16, .., 1; every lane ends with the same sum."""
    v = np.array(lanes, dtype=F64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[_LANES ^ o]
    return v[0]


def ap_ordered(scores, labels, N):
    """-> (ap (H, C) fp64, npos (C) int64, terms (H, N) fp64) in the kernel's order: lane l adds the terms of its rows l, l + 64, ..
    that belong to the class in increasing row order from +0.0, the lanes are added by the butterfly, one division by npos.  A class
    without a positive: NaN."""
    H, C, _cap = scores.shape
    lab = np.asarray(labels)[:N].astype(np.int64)
    terms = ap_terms(scores, labels, N)
    ap = np.full((H, C), np.nan, dtype=F64)
    npos = np.array([(lab == c).sum() for c in range(C)], dtype=np.int64)
    for h in range(H):
        for c in range(C):
            if npos[c] == 0:
                continue
            lanes = np.zeros(64, dtype=F64)
            for n in np.flatnonzero(lab == c):                                # increasing n: each lane's own rows in order
                lanes[n % 64] = lanes[n % 64] + terms[h, n]
            ap[h, c] = wave_sum(lanes) / F64(npos[c])
    return ap, npos, terms


def ap_by_thresholds(col, positive):
    """The textbook sweep for one class: sum over the distinct thresholds, from the highest down, of (R_n - R_{n-1}) P_n with
    P_n = TP(>= t) / CNT(>= t) and R_n = TP(>= t) / P (sklearn.metrics.average_precision_score).  Finite scores, at least one positive."""
    col, positive = np.asarray(col, dtype=F64), np.asarray(positive, dtype=bool)
    P = int(positive.sum())
    ap, r_prev = 0.0, 0.0
    for t in np.unique(col)[::-1]:
        ge = col >= t
        tp = int((ge & positive).sum())
        ap += (tp / P - r_prev) * (tp / int(ge.sum()))
        r_prev = tp / P
    return ap


def confusion(pred, labels, N, C):
    """(H, C, C) int64 [true][predicted] over the rows below N; a row whose label or prediction is no class is skipped."""
    pred, lab = np.asarray(pred)[:, :N], np.asarray(labels)[:N]
    conf = np.zeros((pred.shape[0], C, C), dtype=np.int64)
    for h in range(pred.shape[0]):
        for n in range(N):
            if 0 <= lab[n] < C and 0 <= pred[h, n] < C:
                conf[h, lab[n], pred[h, n]] += 1
    return conf


def softmax64(logits):
    """Row softmax of (B, C) logits in fp64."""
    x = np.asarray(logits, dtype=F64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def first_argmax(logits):
    return np.argmax(np.asarray(logits), axis=1)                              # numpy: the first maximum


def f1_scores(conf, average):
    """sklearn's f1_score(average=..., zero_division=0) from one head's confusion counts (C, C)."""
    c = np.asarray(conf, dtype=F64)
    tp, true, predicted = np.diag(c), c.sum(axis=1), c.sum(axis=0)
    f = np.array([2 * tp[k] / (true[k] + predicted[k]) if true[k] + predicted[k] > 0 else 0.0 for k in range(c.shape[0])])
    if average == "macro":
        seen = (true + predicted) > 0
        return float(f[seen].mean())
    return float((f * true).sum() / true.sum())


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
AP_N = (1, 63, 64, 65, 130)
AP_C = (1, 2, 6, 64, 65, 128)
AP_H = (1, 3, 4)
AP_FAMILIES = ("quarters", "random", "special")
TAIL = 7                                                                      # poisoned rows past N: cap = N + TAIL


def ap_case(N, C, H, family):
    """-> (scores (H, C, N + TAIL) fp32, labels (N + TAIL) int32).  Rows >= N are poison: NaN scores under valid labels.
    quarters  scores from {0, 1/4, 1/2, 3/4}: ties everywhere
    random    uniform floats
    special   random with NaN, +inf and -inf entries, and the labels -1 and C among the rows
    Where C >= 3 and N >= 2, class 1 has no positive; where C == 1 every row is a positive of class 0 (a class that is all positives)."""
    rng = np.random.default_rng(1000 * N + 10 * C + H + 7 * AP_FAMILIES.index(family))
    cap = N + TAIL
    if family == "quarters":
        scores = (rng.integers(0, 4, size=(H, C, cap)) / 4).astype(F32)
    else:
        scores = rng.random((H, C, cap), dtype=F32)
    labels = rng.integers(0, C, size=cap).astype(np.int32)
    if C >= 3 and N >= 2:
        labels[labels == 1] = 2                                               # class 1: no positive
    if family == "special":
        flat = scores.reshape(-1)
        k = max(3, flat.size // 10)
        at = rng.choice(flat.size, size=k, replace=False)
        flat[at[: k // 3]] = np.nan
        flat[at[k // 3: 2 * k // 3]] = np.inf
        flat[at[2 * k // 3:]] = -np.inf
        if N >= 2:
            labels[0], labels[N - 1] = -1, C
        if N >= 65:
            labels[64] = C + 5
    scores[:, :, N:] = np.nan                                                 # never read
    return scores, labels


# (batch sizes appended in order): offsets 0, 1, 6, 70 -- unaligned -- and a short last batch
APPEND_BATCHES = (1, 5, 64, 3)
APPEND_CAP = 75


def near_tie_case(M, B, C, alphas, seed=0):
    """M logit matrices (B, C), labels and the fp32 weights: in every row two classes c0, c1 stand far above the others and their
    fused values sum_m w_m l_m lie within two ulps of each other (the last modality's l[c1] is solved for in fp64, rounded, and moved
    by r % 5 - 2 ulps), so which of them wins depends on how the sum is rounded -- `fuse32` with and without fused multiply-add
    disagrees on a tenth of the rows.  The label is c0 in even rows, c1 in odd rows: every flipped arg-max changes a counter."""
    rng = np.random.default_rng(seed + M)
    w = np.array(alphas, dtype=F32)
    outs = [np.full((B, C), -10.0, dtype=F32) for _ in range(M)]
    labels = np.zeros(B, dtype=np.int64)
    for r in range(B):
        c0 = r % C
        c1 = (c0 + 1 + (r // C) % (C - 1)) % C
        for m in range(M):
            outs[m][r, c0], outs[m][r, c1] = F32(rng.uniform(-2, 2)), F32(rng.uniform(-2, 2))
        target = sum(F64(w[m]) * F64(outs[m][r, c0]) for m in range(M)) - sum(F64(w[m]) * F64(outs[m][r, c1]) for m in range(M - 1))
        x, k = F32(target / F64(w[M - 1])), r % 5 - 2
        for _ in range(abs(k)):
            x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf), dtype=F32)
        outs[M - 1][r, c1] = x
        labels[r] = c0 if r % 2 == 0 else c1
    return outs, labels, w


def fuse32(outs, w, fma):
    """v = 0; v += w_m * l_m in modality order, in fp32: each step one rounding (fma) or two."""
    v = np.zeros_like(outs[0])
    for m, o in enumerate(outs):
        if fma:
            v = (F64(w[m]) * o.astype(F64) + v.astype(F64)).astype(F32)
        else:
            v = (v + (w[m] * o).astype(F32)).astype(F32)
    return v
