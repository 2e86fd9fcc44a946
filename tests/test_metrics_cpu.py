"""CPU: the average-precision restatement of tests/metrics_model.py in the kernel's order against the textbook threshold sweep (and
sklearn where it imports), the policies the GPU tests rest on, the refusals of the three additive ABI entries (nothing is
dereferenced before validation), the evaluators' metrics= / capacity= argument rules, and `make host-check`."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import metrics_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64

try:
    from sklearn.metrics import average_precision_score, f1_score
except ImportError:                                          # the sweep stands alone then
    average_precision_score = f1_score = None


def _against_the_sweep(scores, labels, N, name):
    """ap_ordered of every (head, class) with a positive against ap_by_thresholds within 1e-12 (and sklearn's)."""
    ap, npos, _terms = MM.ap_ordered(scores, labels, N)
    H, C, _ = scores.shape
    worst = 0.0
    for h in range(H):
        for c in range(C):
            pos = np.asarray(labels)[:N] == c
            assert npos[c] == pos.sum()
            if not pos.any():
                assert np.isnan(ap[h, c])
                continue
            want = MM.ap_by_thresholds(scores[h, c, :N], pos)
            worst = max(worst, abs(ap[h, c] - want))
            if average_precision_score is not None:
                worst = max(worst, abs(ap[h, c] - average_precision_score(pos, scores[h, c, :N].astype(F64))))
    print(f"{name}: ap_ordered off the sweep by {worst:.3g}")
    assert worst <= 1e-12
    return ap


@pytest.mark.parametrize("N,C,H", [(1, 1, 1), (63, 2, 3), (64, 6, 4), (65, 65, 1), (130, 6, 3), (130, 128, 1), (744, 6, 3)])
@pytest.mark.parametrize("family", ["quarters", "random"])
def test_ordered_sum_equals_the_threshold_sweep(N, C, H, family):
    if N in MM.AP_N:
        scores, labels = MM.ap_case(N, C, H, family)
    else:                                                    # CREMA-D's test set size: more than one row per lane, eleven trips
        rng = np.random.default_rng(N)
        scores = (rng.integers(0, 4, size=(H, C, N)) / 4).astype(F32) if family == "quarters" else rng.random((H, C, N), dtype=F32)
        labels = rng.integers(0, C, size=N).astype(np.int32)
    _against_the_sweep(scores, labels, N, f"{family} N={N} C={C} H={H}")


def test_closed_forms():
    """All scores equal: AP = P / N.  Perfectly separated: AP = 1.  One positive ranked k-th (no ties): AP = 1 / k."""
    N = 70
    labels = (np.arange(N) % 3 == 0).astype(np.int32)        # class 1: 24 positives; class 0 the rest
    P = int(labels.sum())
    flat = np.full((1, 2, N), 0.25, dtype=F32)
    ap = _against_the_sweep(flat, labels, N, "all equal")
    assert abs(ap[0, 1] - P / N) <= 1e-15 and abs(ap[0, 0] - (N - P) / N) <= 1e-15     # P equal terms P / N, added and divided by P
    sep = np.stack([np.where(labels == c, 0.9, 0.1) + np.arange(N) * 1e-3 for c in range(2)])[None].astype(F32)
    ap = _against_the_sweep(sep, labels, N, "separated")
    assert abs(ap[0, 1] - 1) <= 1e-15 and abs(ap[0, 0] - 1) <= 1e-15
    for k in (1, 2, 17, N):
        one = np.zeros(N, dtype=np.int32)
        one[5] = 1
        col = np.insert(np.arange(N - 1, dtype=F32), 5, N - k - 0.5)        # the others are 0 .. N - 2: k - 1 of them lie above it
        s = np.stack([-col, col])[None].astype(F32)
        ap = _against_the_sweep(s, one, N, f"single positive at rank {k}")
        assert abs(ap[0, 1] - 1.0 / k) <= 1e-15


def test_policies_of_the_restatement():
    """NaN scores, labels that are no class, classes without a positive, rows past N."""
    scores = np.array([[[0.5, np.nan, 0.25, 0.5, 0.75, np.nan], [0.1, 0.2, np.nan, 0.4, 0.5, np.nan]]], dtype=F32)   # (1, 2, 6), N = 5
    labels = np.array([0, 0, 1, 7, -1, 0], dtype=np.int32)
    ap, npos, terms = MM.ap_ordered(scores, labels, 5)
    # class 0, rows 0 and 1: row 0 (0.5): >= are rows 0, 3, 4 -> tp 1 of 3; row 1 is NaN: term 0.  Rows 3, 4 are negatives of class 0.
    assert terms[0].tolist() == [1 / 3, 0.0, 0.0, 0.0, 0.0] and npos.tolist() == [2, 1]
    assert ap[0, 0] == (1 / 3 + 0.0) / 2 and ap[0, 1] == 0.0          # class 1's one positive is NaN-scored: term 0
    # the poisoned row 5 (label 0, NaN) was not read: with N = 6 it is a third positive of class 0
    assert MM.ap_ordered(scores, labels, 6)[1].tolist() == [3, 1]
    ap, npos, _ = MM.ap_ordered(scores, np.array([1, 1, 1, 1, 1, 1], dtype=np.int32), 5)
    assert np.isnan(ap[0, 0]) and npos.tolist() == [0, 5]
    # +-inf order like numbers; the butterfly adds what a plain sum adds when every term is exact
    s = np.array([[[np.inf, -np.inf, 0.0, np.inf]]], dtype=F32)
    ap, _, terms = MM.ap_ordered(s, np.array([0, 0, 0, 0], dtype=np.int32), 4)
    assert terms[0].tolist() == [1.0, 1.0, 1.0, 1.0] and ap[0, 0] == 1.0
    assert MM.wave_sum(np.arange(64)) == 64 * 63 / 2


def test_confusion_and_f1_of_the_model():
    from mla_hip.metrics import f1_from_confusion
    rng = np.random.default_rng(3)
    N, C = 200, 5
    labels = rng.integers(0, C - 1, size=N)                  # class 4 never a label ...
    pred = np.stack([rng.integers(0, C - 1, size=N), rng.integers(0, C, size=N)])   # ... head 0 never predicts it, head 1 does
    conf = MM.confusion(pred, labels, N, C)
    assert conf.sum(axis=(1, 2)).tolist() == [N, N] and (conf.sum(axis=2) == np.bincount(labels, minlength=C)).all()
    bad = labels.copy()
    bad[0], bad[1] = -1, C
    assert MM.confusion(pred, bad, N, C).sum(axis=(1, 2)).tolist() == [N - 2, N - 2]
    for average in ("macro", "weighted"):
        got = f1_from_confusion(conf, average)
        for h in range(2):
            assert abs(got[h] - MM.f1_scores(conf[h], average)) <= 1e-15
            if f1_score is not None:
                assert abs(got[h] - f1_score(labels, pred[h], average=average, zero_division=0)) <= 1e-12
    with pytest.raises(ValueError, match="macro"):
        f1_from_confusion(conf, "micro")
    assert f1_from_confusion(np.zeros((1, 3, 3)), "macro") == (0.0,) and f1_from_confusion(np.zeros((1, 3, 3)), "weighted") == (0.0,)


def test_softmax_model_and_the_exact_rows():
    """What the append tests assert bit for bit: a saturated row's fp32 softmax is exactly one-hot (exp(-128) underflows to 0), an
    equal row's is fl(1 / C) everywhere (e = 1 in every slot, s = C exactly)."""
    assert np.exp(F32(-128.0)) == 0
    for C in (1, 2, 65, 128):
        assert F32(C) == C and abs(float(F32(1) / F32(C)) - 1 / C) <= 2.0 ** -24 / C * 2
    p = MM.softmax64(np.array([[0.0, 1.0, 2.0], [5.0, 5.0, 5.0]]))
    assert np.abs(p.sum(axis=1) - 1).max() <= 1e-15 and np.abs(p[1] - 1 / 3).max() <= 1e-16
    assert MM.first_argmax(np.array([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0]])).tolist() == [1, 0]


# ---- the C entries -------------------------------------------------------------------------------------------------------------------
def test_abi_entries_are_additive_and_refuse_before_any_launch():
    from mla_hip import _lib, torch_ops
    lib = _lib.load()
    for name, nargs in (("mla_scores_append", 15), ("mla_average_precision", 10), ("mla_confusion_count", 8), ("mla_metrics_ws_bytes", 2)):
        assert hasattr(lib, name) and len(_lib.PROTOTYPES[name][1]) == nargs
    assert lib.mla_abi_version() == 3                        # additive
    assert {"average_precision", "confusion_count"} <= set(torch_ops.op_names())
    assert lib.mla_metrics_ws_bytes(744, 3) == 744 * 3 * 8 and lib.mla_metrics_ws_bytes(0, 3) == 0
    fake = 0x1000                                            # non-null, aligned, never dereferenced: validation fails first
    err = lib.mla_last_error

    def append(l0=fake, l1=fake, l2=fake, l3=None, weights=None, labels=fake, scores=fake, pred=fake, out=fake, H=3, B=4, C=6, pos=0, cap=8):
        return lib.mla_scores_append(l0, l1, l2, l3, weights, labels, scores, pred, out, H, B, C, pos, cap, None)
    assert append(C=129) == -1 and b"mla_scores_append: need 0 < C <= 128 (got 129)" in err()
    assert append(H=0) == -1 and b"mla_scores_append: need 1 <= H <= 4 heads (got 0)" in err()
    assert append(H=5) == -1 and b"need 1 <= H <= 4 heads (got 5)" in err()
    assert append(pos=5) == -1 and b"rows 5 .. 8 do not fit a store of cap = 8 rows" in err()
    assert append(pos=-1) == -1 and b"do not fit" in err()
    assert append(B=0) == -1 and b"need B > 0" in err()
    assert append(cap=0) == -1 and b"need 0 < cap" in err()
    for null in ("l0", "l2", "labels", "scores", "pred", "out"):
        assert append(**{null: None}) == -1 and b"mla_scores_append: null pointer" in err(), null
    assert append(H=4) == -1 and b"null pointer" in err()                              # four heads need l3
    assert append(weights=fake) == -1 and b"pass no fused matrix" in err()             # weights: head 0 is formed, not passed
    assert append(weights=fake, l0=None, H=1) == -1 and b"pass no fused matrix" in err()
    assert append(labels=fake + 4) == -1 and b"8-byte" in err()
    assert append(scores=fake + 2) == -1 and b"4-byte" in err()

    def ap(scores=fake, labels=fake, N=4, cap=8, H=3, C=6, out=fake, npos=fake, ws=fake):
        return lib.mla_average_precision(scores, labels, N, cap, H, C, out, npos, ws, None)
    assert ap(C=129) == -1 and b"mla_average_precision: need 0 < C <= 128 (got 129)" in err()
    assert ap(H=0) == -1 and b"mla_average_precision: need 1 <= H <= 4 heads (got 0)" in err()
    assert ap(H=5) == -1 and b"need 1 <= H <= 4 heads (got 5)" in err()
    assert ap(N=9) == -1 and b"need 0 < N <= cap rows (got N = 9, cap = 8)" in err()
    assert ap(N=0) == -1 and b"need 0 < N <= cap" in err()
    for null in ("scores", "labels", "out", "npos", "ws"):
        assert ap(**{null: None}) == -1 and b"mla_average_precision: null pointer" in err(), null
    assert ap(ws=fake + 4) == -1 and b"8-byte" in err()

    def conf(pred=fake, labels=fake, N=4, cap=8, H=3, C=6, out=fake):
        return lib.mla_confusion_count(pred, labels, N, cap, H, C, out, None)
    assert conf(C=129) == -1 and b"mla_confusion_count: need 0 < C <= 128 (got 129)" in err()
    assert conf(H=0) == -1 and b"mla_confusion_count: need 1 <= H <= 4 heads (got 0)" in err()
    assert conf(H=5) == -1 and conf(N=9) == -1 and b"need 0 < N <= cap rows" in err()
    for null in ("pred", "labels", "out"):
        assert conf(**{null: None}) == -1 and b"mla_confusion_count: null pointer" in err(), null
    assert conf(out=fake + 2) == -1 and b"4-byte" in err()
    with pytest.raises(Exception):                           # no CPU implementation: torch's "no kernel" error
        torch.ops.mla_hip.average_precision(torch.zeros(1, 2, 4), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(Exception):
        torch.ops.mla_hip.confusion_count(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), 2)


def test_host_check_builds_and_runs_the_metrics_program():
    csrc = os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "host-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "metrics host check ok" in r.stdout and "metrics_host_check.cpp" in r.stdout and "-fsanitize=address,undefined" in r.stdout


# ---- the evaluators' argument rules --------------------------------------------------------------------------------------------------
class ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "CREMAD", True, "Normal", True


def test_evaluators_take_metrics_and_capacity_and_default_to_nothing():
    from mla_hip import CLIPClassifier, Evaluator, JointEvaluator, QMFEvaluator
    from mla_hip._lib import MLAHipError
    from mla_hip.metrics import MetricsMixin, ScoreStore
    for cls in (Evaluator, JointEvaluator, QMFEvaluator):
        params = inspect.signature(cls.__init__).parameters
        assert params["metrics"].default is False and params["capacity"].default is None and issubclass(cls, MetricsMixin)
    model = CLIPClassifier(ClipArgs(), device="cpu", seed=0, feat_dim=64)
    ev = Evaluator(model)
    assert ev._store is None and ev._fixed_weights is None
    for call in (ev.average_precision, ev.mean_average_precision, ev.confusion, ev.f1, lambda: ev.scores):
        with pytest.raises(MLAHipError, match="metrics=False"):
            call()
    with pytest.raises(ValueError, match="capacity="):
        Evaluator(model, metrics=True)
    with pytest.raises(ValueError, match="capacity"):
        Evaluator(model, metrics=True, capacity=0)
    ev = Evaluator(model, metrics=True, capacity=10)        # host tensors: nothing is launched before the first update
    st = ev._store
    assert isinstance(st, ScoreStore) and (st.H, st.C, st.capacity, st.n) == (3, 6, 10, 0)
    assert st.scores.shape == (3, 6, 10) and st.pred.shape == (3, 10) and st.labels.shape == (10,)
    assert st.pred.dtype == torch.int32 and st.labels.dtype == torch.int32 and ev._fixed_weights.tolist() == [0.5, 0.5]
    # an empty store answers without a launch: NaN everywhere, zero counts
    assert np.isnan(ev.average_precision()).all() and ev.average_precision().shape == (3, 6)
    assert all(np.isnan(v) for v in ev.mean_average_precision()) and ev.confusion().sum() == 0 and ev.f1() == (0.0, 0.0, 0.0)
    scores, pred, labels, n = ev.scores
    assert n == 0 and scores.shape == (3, 6, 0) and pred.shape == (3, 0) and labels.shape == (0,)
    # a batch past the capacity is refused before anything is launched (here: before anything could be)
    st.n = 8
    with pytest.raises(MLAHipError, match="capacity=10"):
        st.append([None, torch.zeros(3, 6), torch.zeros(3, 6)], torch.zeros(3, dtype=torch.int64), ev._fixed_weights)
    assert st.n == 8
    ev.reset()
    assert st.n == 0

    class Active:                                            # a communicator with more than one rank
        active = True
    with pytest.raises(NotImplementedError, match="across ranks"):
        Evaluator(model, comm=Active(), metrics=True, capacity=10)
    Evaluator(model, comm=Active())                          # without metrics an active comm is what it was
