"""Present-row plans: how a classifier whose encoders treat every sample on its own (transformers: no BatchNorm, no dropout) runs an
encoder on the samples that HAVE its modality (Modal3Classifier(..., present=); csrc/rows.hip).

All absent samples of a modality have the same input -- zeros -- hence the same feature f(0), and their feature gradients reach the
parameters only through their sum.  So the encoder runs on the P present rows plus ONE zero row:

    inputs    rows_gather       (B, ...) -> (P + 1, ...)   present rows, then the zero row
    features  rows_expand       (P + 1, D) -> (B, D)       an absent sample's row is f(0)
    d feature rows_compact_sum  (B, D) -> (P + 1, D)       present rows, then the sum over the absent rows

which, in exact arithmetic, is the step on all B rows; the two differ in the order of floating-point sums.  The index tables are made
on the host from the `present` column and reach the device with one asynchronous copy from pinned memory: no synchronisation.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import MLAHipError


def check_present(present, B: int, M: int) -> torch.Tensor:
    """`present` as a host bool (B, M) tensor.  Refused: anything but a host bool / uint8 tensor (a device tensor would have to be
    read back, which synchronises), another shape, and a sample with no modality at all (the batcher refuses such a mask too)."""
    if not isinstance(present, torch.Tensor):
        raise MLAHipError(f"present: expected a host bool / uint8 tensor ({B}, {M}), got {type(present).__name__}")
    if present.device.type != "cpu":
        raise MLAHipError(f"present: expected a HOST tensor, got one on {present.device} (reading it back would synchronise the device)")
    if present.dtype not in (torch.bool, torch.uint8):
        raise MLAHipError(f"present: expected dtype bool or uint8, got {present.dtype}")
    if tuple(present.shape) != (B, M):
        raise MLAHipError(f"present: expected shape ({B}, {M}) (one column per modality), got {tuple(present.shape)}")
    have = present != 0
    if not bool(have.any(dim=1).all()):
        raise MLAHipError(f"present: sample {int(have.any(dim=1).int().argmin())} has no modality left")
    return have


class RowPlan:
    """One modality's rows of one batch: `idx` the P present rows, `absent` the A = B - P others, `map` rows_expand's source row of
    every sample (its compact row, or P: the zero row); each on the host and, after upload(), in `dev` (int64 (2 B), owned by the
    caller and reused every step: the copy is ordered behind the kernels that read the previous step's tables by the stream)."""

    def __init__(self, have: torch.Tensor):
        B = have.numel()
        self.B = B
        self.idx_host = torch.nonzero(have).reshape(-1)
        self.absent_host = torch.nonzero(~have).reshape(-1)
        self.P, self.A = self.idx_host.numel(), self.absent_host.numel()
        self.map_host = ops.rows_expand_map(self.idx_host, self.P, B, self.P + 1)
        self.idx = self.absent = self.map = None

    @property
    def rows(self) -> int:
        return self.P + 1

    def upload(self, dev: torch.Tensor) -> "RowPlan":
        B, P = self.B, self.P
        host = torch.empty(2 * B, dtype=torch.int64, pin_memory=dev.is_cuda)
        torch.cat([self.idx_host, self.absent_host, self.map_host], out=host)
        dev.copy_(host, non_blocking=True)
        self.idx, self.absent, self.map = dev[:P], dev[P:B], dev[B:]
        return self


def compact_feature_grad(enc, dfeat: torch.Tensor) -> torch.Tensor:
    """The feature gradient as `enc`'s last forward needs it: (B, D) itself after a forward on all rows, else the (P + 1, D)
    compaction the classifier left on the encoder (`enc._row_grad`, a callable) for that forward."""
    compact = getattr(enc, "_row_grad", None)
    return dfeat if compact is None else compact(dfeat)
