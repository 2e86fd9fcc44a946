"""GPU: HeadCounts (mla_hip/evaluators.py) alone, on plain tensors: the counters JointEvaluator and QMFEvaluator keep.

Inputs are head_counts_model.py's: integer-valued fp32 logits, so the kernel's fused value 1 * out + 0 * out_a + 0 * out_v is exact and
every expected counter is numpy.argmax with NO tolerance.  Each case holds a tied row (the first maximum wins), a row labelled -1 and
one labelled C (counted nowhere; B >= 3), and at B = 257 a row past eval_fuse_kernel's 256-thread row stride.  The counters are also
compared with the two mla_eval_fuse calls the evaluators made before HeadCounts existed -- (out, out_a, out_v) with weights (1, 0, 0),
(out_t, out_t) with (1, 0) -- made here by hand."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_counts_model as H  # noqa: E402


def dev(out, out_m, label):
    return torch.from_numpy(out).cuda(), [torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in out_m], torch.from_numpy(label).cuda()


def by_hand(out, out_m, label, C):
    """The parent's arithmetic: the two eval_fuse calls with the trick weights, into fresh buffers."""
    from mla_hip import ops
    counts = torch.zeros(C * 5, device="cuda", dtype=torch.int32)
    counts_t = torch.zeros(C * 4, device="cuda", dtype=torch.int32)
    w = torch.zeros(3, device="cuda")
    ops.eval_fuse([out, out_m[0], out_m[1]], label, counts, w, False, [1.0, 0.0, 0.0])
    if len(out_m) == 3:
        ops.eval_fuse([out_m[2], out_m[2]], label, counts_t, w, False, [1.0, 0.0])
    return counts.view(5, C).cpu().numpy(), counts_t.view(4, C).cpu().numpy()


@pytest.mark.parametrize("M,C,B", H.SHAPES)
def test_counters_are_numpy_argmax_exactly(M, C, B):
    from mla_hip.evaluators import HeadCounts
    out, out_m, label, bad = H.case(M, C, B)
    want, want_t = H.expected(out, out_m, label, C)
    d_out, d_m, d_label = dev(out, out_m, label)
    hc = HeadCounts(M, C, "cuda")
    assert hc.counts.shape == (5 * C,) and hc.counts_t.shape == (4 * C,) and hc.weights.shape == (3,)
    assert hc.counts.dtype == torch.int32 and hc.counts_t.dtype == torch.int32 and hc.result() == (0.0,) * (1 + M)

    hc.count(d_out, d_m, d_label)
    got, got_t = hc.counts.view(5, C).cpu().numpy(), hc.counts_t.view(4, C).cpu().numpy()
    assert (got == want).all(), (got, want)                          # [num, argmax(out), argmax(out), argmax(out_a), argmax(out_v)]
    assert (got_t == want_t).all(), (got_t, want_t)                  # M = 3: the out_t row at index 1 (and 2, 3); M = 2: untouched
    assert got[0].sum() == B - bad.sum()                             # the rows labelled -1 and C are counted nowhere
    hand, hand_t = by_hand(d_out, d_m, d_label, C)
    assert (got == hand).all() and (got_t == hand_t).all()
    assert hc.result() == H.ratios(want, want_t, M)
    assert hc.result(per_modality=False) == H.ratios(want, want_t, M)[:1]

    hc.count(d_out, d_m, d_label)                                    # the counters accumulate
    assert (hc.counts.view(5, C).cpu().numpy() == 2 * want).all() and (hc.counts_t.view(4, C).cpu().numpy() == 2 * want_t).all()
    assert hc.result() == H.ratios(want, want_t, M)
    hc.reset()
    assert int(hc.counts.abs().sum()) == 0 and int(hc.counts_t.abs().sum()) == 0

    if bad.any():                                                    # the good rows alone count what they counted among the bad ones
        keep = ~bad
        hc.count(*dev(out[keep], out_m[:, keep], label[keep]))
        assert (hc.counts.view(5, C).cpu().numpy() == want).all() and (hc.counts_t.view(4, C).cpu().numpy() == want_t).all()


@pytest.mark.parametrize("bad_label", [-1, "C"])
def test_a_batch_of_one_bad_row_counts_nothing(bad_label):
    from mla_hip.evaluators import HeadCounts
    for M, C in ((2, 2), (3, 6)):
        out, out_m, label, _ = H.bad_row_case(M, C, C if bad_label == "C" else -1)
        hc = HeadCounts(M, C, "cuda")
        hc.count(*dev(out, out_m, label))
        assert int(hc.counts.abs().sum()) == 0 and int(hc.counts_t.abs().sum()) == 0 and hc.result() == (0.0,) * (1 + M)

