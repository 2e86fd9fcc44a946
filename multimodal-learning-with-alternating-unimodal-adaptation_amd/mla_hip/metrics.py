"""Evaluation metrics beyond accuracy, kept on the device: mean average precision, confusion counts and F1.

valid() of the reference forms prediction = softmax(out), pred_a and pred_v (main.py:653-657) and takes only their arg-max.  With
metrics=True an evaluator keeps them: one launch per batch appends the batch's class scores, arg-max predictions and labels to a
`ScoreStore`; average precision and the confusion counts are formed from the store at result time (csrc/metrics.hip).  The row
count lives on the host, so an update() synchronises nothing; every result call costs one host sync, as result() does.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from . import ops
from ._lib import MLAHipError


class ScoreStore:
    """`capacity` rows of H heads (fused first, then each modality) and C classes: scores fp32 (H, C, capacity), class-major so that
    one class is a contiguous column; pred int32 (H, capacity); labels int32 (capacity); `n` rows filled."""

    def __init__(self, H: int, C: int, capacity: int, device):
        if int(capacity) <= 0:
            raise ValueError(f"ScoreStore: capacity must be the number of samples to hold (got {capacity!r})")
        self.H, self.C, self.capacity, self.n = H, C, int(capacity), 0
        self.scores = torch.zeros((H, C, self.capacity), device=device, dtype=torch.float32)
        self.pred = torch.zeros((H, self.capacity), device=device, dtype=torch.int32)
        self.labels = torch.zeros(self.capacity, device=device, dtype=torch.int32)

    def reset(self) -> None:
        self.n = 0

    def append(self, logits: List[Optional[torch.Tensor]], labels: torch.Tensor, weights: Optional[torch.Tensor] = None) -> None:
        """One batch: the H (B, C) logit matrices, or [None] + the modality matrices with the device weight vector eval_fuse wrote."""
        B = labels.shape[0]
        if self.n + B > self.capacity:                      # the C entry refuses too; this message names the remedy
            raise MLAHipError(f"metrics: {self.n} rows stored, a batch of {B} does not fit capacity={self.capacity}; construct the "
                              f"evaluator with capacity=len(dataset)")
        ops.scores_append(logits, labels, self.scores, self.pred, self.labels, self.n, weights=weights)
        self.n += B

    def views(self):
        """(scores (H, C, n), pred (H, n), labels (n), n): device views of the filled rows."""
        n = self.n
        return self.scores[:, :, :n], self.pred[:, :n], self.labels[:n], n

    def average_precision(self) -> np.ndarray:
        if self.n == 0:
            return np.full((self.H, self.C), np.nan)
        dev = self.scores.device
        ap = torch.empty((self.H, self.C), device=dev, dtype=torch.float64)
        npos = torch.empty(self.C, device=dev, dtype=torch.int32)
        ws = torch.empty((self.H, self.capacity), device=dev, dtype=torch.float64)
        ops.average_precision(self.scores, self.labels, self.n, ap, npos, ws)
        return ap.cpu().numpy()

    def confusion(self) -> np.ndarray:
        conf = torch.zeros((self.H, self.C, self.C), device=self.scores.device, dtype=torch.int32)
        if self.n:
            ops.confusion_count(self.pred, self.labels, self.n, conf)
        return conf.cpu().numpy().astype("int64")


def f1_from_counts(tp, true, predicted, average: str) -> float:
    """F1 of one head from its per-class counts (C) each -- correct, true samples, predictions -- with the averaging policy
    f1_from_confusion documents; fp64 from the integers."""
    if average not in ("macro", "weighted"):
        raise ValueError(f"f1: average must be 'macro' or 'weighted', got {average!r}")
    tp, true, predicted = (np.asarray(v, dtype=np.float64) for v in (tp, true, predicted))
    den = true + predicted
    f = np.divide(2 * tp, den, out=np.zeros_like(tp), where=den > 0)
    if average == "macro":
        seen = den > 0
        return float(f[seen].mean()) if seen.any() else 0.0
    return float((f * true).sum() / true.sum()) if true.sum() > 0 else 0.0


def f1_from_confusion(conf: np.ndarray, average: str) -> tuple:
    """Per-head F1 from confusion counts (H, C, C) [true][predicted], sklearn's f1_score(average=...) with zero_division=0: a class
    with no true and no predicted sample has F1 0; "macro" averages the classes that occur as a label or as a prediction, "weighted"
    weights each class by its number of true samples."""
    return tuple(f1_from_counts(np.diag(c), c.sum(axis=1), c.sum(axis=0), average) for c in np.asarray(conf, dtype=np.float64))


class MetricsMixin:
    """metrics= / capacity= of Evaluator, JointEvaluator and QMFEvaluator.  The evaluator calls `_metrics_init` once, `_metrics_append`
    after each batch's counters and `_metrics_reset` from reset(); with metrics=False nothing is allocated and nothing is launched."""

    _store: Optional[ScoreStore] = None

    def _metrics_init(self, metrics: bool, capacity: Optional[int], H: int, C: int, device, comm=None) -> None:
        self._store = None
        if not metrics:
            return
        if comm is not None and comm.active:
            raise NotImplementedError(f"{type(self).__name__}: metrics=True keeps each rank's own rows; gathering stores of different "
                                      f"lengths across ranks is not implemented -- evaluate the metrics in one process")
        if capacity is None:
            raise ValueError(f"{type(self).__name__}: metrics=True needs capacity=, the number of samples to hold (len(test_set))")
        self._store = ScoreStore(H, C, capacity, device)

    def _metrics_reset(self) -> None:
        if self._store is not None:
            self._store.reset()

    def _metrics_append(self, logits, labels, weights=None) -> None:
        if self._store is not None:
            self._store.append(list(logits), labels, weights)

    def _need_store(self) -> ScoreStore:
        if self._store is None:
            raise MLAHipError(f"{type(self).__name__}: constructed with metrics=False; pass metrics=True, capacity=len(test_set)")
        return self._store

    @property
    def scores(self):
        """The store: (scores (H, C, n) class-major softmax scores, pred (H, n), labels (n), n) as device views of the filled rows;
        head 0 is the fused output, then each modality."""
        return self._need_store().views()

    def average_precision(self) -> np.ndarray:
        """Host float64 (H, C): average precision per head and class, NaN where a class has no positive (one host sync)."""
        return self._need_store().average_precision()

    def mean_average_precision(self) -> tuple:
        """(mAP, mAP_a, mAP_v[, mAP_t]): the mean over the classes that have a positive (NaN when none has)."""
        ap = self.average_precision()
        return tuple(float(np.mean(row[~np.isnan(row)])) if not np.isnan(row).all() else float("nan") for row in ap)

    def confusion(self) -> np.ndarray:
        """Host int64 (H, C, C), [true][predicted]; rows with a label outside [0, C) are counted nowhere, as in the counters."""
        return self._need_store().confusion()

    def f1(self, average: str = "macro") -> tuple:
        """Per-head F1 from confusion(), on the host (C * C numbers): "macro" or "weighted"."""
        return f1_from_confusion(self.confusion(), average)
