"""CPU: the inputs test_head_counts_gpu.py feeds HeadCounts and their numpy expectation are what head_counts_model.py says they are."""
import numpy as np
import pytest

import head_counts_model as H


@pytest.mark.parametrize("M,C,B", H.SHAPES)
def test_inputs_are_exact_tied_and_hold_the_bad_rows(M, C, B):
    out, out_m, label, bad = H.case(M, C, B)
    heads = np.concatenate([out[None], out_m])
    assert heads.dtype == np.float32 and heads.shape == (1 + M, B, C) and label.dtype == np.int64
    assert (heads == np.rint(heads)).all() and np.abs(heads).max() < 2 ** 20       # integers: 1 * out + 0 * a + 0 * v is exact
    for h in heads:                                                                 # row 0: the maximum twice, the label on the first
        top = np.flatnonzero(h[0] == h[0].max())
        assert top.tolist() == [H.FIRST[C], H.LATER[C]] and h[0].argmax() == H.FIRST[C] == label[0]
    assert bad.sum() == (2 if B >= 3 else 0)
    if B >= 3:
        assert label[1] == -1 and label[2] == C and bad[1] and bad[2]
    assert (((label < 0) | (label >= C)) == bad).all()
    if B >= 4:
        assert not bad[B - 1] and label[B - 1] == out[B - 1].argmax()


@pytest.mark.parametrize("M,C,B", H.SHAPES)
def test_expectation_is_the_argmax_count_of_the_good_rows(M, C, B):
    out, out_m, label, bad = H.case(M, C, B)
    counts, counts_t = H.expected(out, out_m, label, C)
    assert counts.shape == (5, C) and counts_t.shape == (4, C)
    assert counts[0].sum() == B - bad.sum() and (counts[1] == counts[2]).all()
    # by hand, one row at a time
    want = np.zeros((5, C), dtype=np.int64)
    want_t = np.zeros((4, C), dtype=np.int64)
    for r in range(B):
        if bad[r]:
            continue
        l = label[r]
        want[0, l] += 1
        for k, h in ((1, out), (2, out), (3, out_m[0]), (4, out_m[1])):
            first = min(c for c in range(C) if h[r, c] == h[r].max())
            want[k, l] += first == l
        if M == 3:
            want_t[0, l] += 1
            first = min(c for c in range(C) if out_m[2][r, c] == out_m[2][r].max())
            want_t[1:, l] += first == l
    assert (counts == want).all() and (counts_t == want_t).all()
    # the tied row is a hit of every head; a last-maximum rule would miss it
    assert all(counts[k, H.FIRST[C]] >= 1 for k in (1, 3, 4)) and (M == 2 or counts_t[1, H.FIRST[C]] >= 1)
    # without the bad rows the other rows count the same
    alone = H.expected(out[~bad], out_m[:, ~bad], label[~bad], C)
    assert (alone[0] == counts).all() and (alone[1] == counts_t).all()
    res = H.ratios(counts, counts_t, M)
    assert len(res) == 1 + M and all(0.0 <= v <= 1.0 for v in res) and res[0] == counts[1].sum() / max(B - bad.sum(), 1)


@pytest.mark.parametrize("bad_label", [-1, "C"])
def test_a_batch_of_one_bad_row_expects_nothing(bad_label):
    for M, C in ((2, 2), (3, 6)):
        out, out_m, label, bad = H.bad_row_case(M, C, C if bad_label == "C" else -1)
        counts, counts_t = H.expected(out, out_m, label, C)
        assert bad.all() and counts.sum() == 0 and counts_t.sum() == 0 and H.ratios(counts, counts_t, M) == (0.0,) * (1 + M)


def test_the_evaluators_count_with_it():
    from mla_hip import JointEvaluator, QMFEvaluator
    from mla_hip.evaluators import HeadCounts
    assert issubclass(JointEvaluator, HeadCounts) and issubclass(QMFEvaluator, HeadCounts)
