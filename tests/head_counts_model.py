"""Inputs and numpy expectation for HeadCounts (mla_hip/evaluators.py), shared by test_head_counts_cpu.py and test_head_counts_gpu.py.

Logits are integer-valued fp32, |v| <= 9 -- far below 2^20 -- so the fused value 1 * out + 0 * out_a + 0 * out_v of the kernel is exact
and equals `out`; the expected counters are numpy.argmax with no tolerance.  Every case has
  row 0      tied: in `out` and in every out_m the maximum stands in two slots (FIRST and a later one); the label is FIRST, so
             the row is a hit exactly when the first maximum wins;
  rows 1, 2  (B >= 3) labels -1 and C: counted nowhere;
  row B - 1  (B >= 4) labelled with its own arg-max of `out`: at B = 257 that is row 256, the row the kernel's thread 0 takes on its
             second trip (256-thread row stride), and it must be counted as a hit.
B = 1 holds the tied row alone (there is no room for the bad rows; bad_row_case covers a batch that is nothing but a bad row)."""
import numpy as np

SHAPES = [(M, C, B) for M in (2, 3) for C in (2, 6) for B in (1, 5, 257)]
FIRST = {2: 0, 6: 2}           # the tied row's first maximum, per C
LATER = {2: 1, 6: 4}           # ... and its second


def case(M, C, B):
    """-> out (B, C), out_m (M, B, C) fp32, label int64 (B), bad (B) bool."""
    rng = np.random.default_rng(1000 * M + 10 * C + B)
    heads = rng.integers(-8, 9, size=(1 + M, B, C)).astype(np.float32)
    label = rng.integers(0, C, size=B).astype(np.int64)
    heads[:, 0, :] = np.minimum(heads[:, 0, :], 8.0)
    heads[:, 0, FIRST[C]] = heads[:, 0, LATER[C]] = 9.0
    label[0] = FIRST[C]
    bad = np.zeros(B, dtype=bool)
    if B >= 3:
        label[1], label[2] = -1, C
        bad[1] = bad[2] = True
    if B >= 4:
        label[B - 1] = heads[0, B - 1].argmax()
    return heads[0], heads[1:], label, bad


def bad_row_case(M, C, bad_label):
    """One row, labelled -1 or C: nothing may be counted."""
    out, out_m, label, _ = case(M, C, 1)
    label[0] = bad_label
    return out, out_m, label, np.ones(1, dtype=bool)


def hits(logits, label, ok, C):
    """Per class: rows (with a label inside [0, C)) whose first maximum is their label."""
    hit = ok & (logits.argmax(axis=1) == label)
    return np.bincount(label[hit], minlength=C)


def expected(out, out_m, label, C):
    """-> counts (5, C) = [num, argmax(out), argmax(out), argmax(out_a), argmax(out_v)], counts_t (4, C) = [num, out_t x 3]
    (zeros with two modalities: nothing is launched on it)."""
    ok = (label >= 0) & (label < C)
    num = np.bincount(label[ok], minlength=C)
    h_out = hits(out, label, ok, C)
    counts = np.stack([num, h_out, h_out, hits(out_m[0], label, ok, C), hits(out_m[1], label, ok, C)])
    counts_t = np.zeros((4, C), dtype=np.int64)
    if len(out_m) == 3:
        h_t = hits(out_m[2], label, ok, C)
        counts_t = np.stack([num, h_t, h_t, h_t])
    return counts, counts_t


def ratios(counts, counts_t, M):
    """result(): (acc, acc_a, acc_v[, acc_t]) = sum(correct) / max(sum(num), 1)."""
    num = max(int(counts[0].sum()), 1)
    res = [counts[1].sum() / num, counts[3].sum() / num, counts[4].sum() / num]
    if M == 3:
        res.append(counts_t[1].sum() / num)
    return tuple(float(v) for v in res)
