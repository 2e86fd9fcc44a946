"""Fusion-weight search: the accuracy / F1 surface over a grid of test-time fusion weights, as a by-product of one evaluation pass.

valid() of the reference fuses with weights found by hand per dataset (av_alpha = 0.55, main.py:968; 0.35 / 0.25 / 0.4,
main.py:56-58).  The per-modality logits do not depend on those weights, and an Evaluator holds them on the device in every
update(): with sweep=grid one more launch per batch (csrc/fusion_sweep.hip) scores every row of the grid, into integer tables.
Nothing is synchronised per batch; sweep_result() costs one host sync and forms everything else in fp64 from the integers.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .metrics import f1_from_counts

SWEEP_MAXG = 4096          # csrc/sweep_args.h


def fusion_grid(M: int, steps: int = 100) -> torch.Tensor:
    """Host float32 grid of fusion weights that sum to 1.  M = 2: (steps + 1, 2), row k = (k / steps, 1.0 - k / steps) -- the pair
    Evaluator(av_alpha=k / steps) hands the kernels.  M = 3: the lattice (i / steps, j / steps, (steps - i - j) / steps), i outer
    and j inner, (steps + 1)(steps + 2) / 2 rows.  Python floats, cast to float32 once."""
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"fusion_grid: steps must be at least 1 (got {steps})")
    if M == 2:
        rows = [(k / steps, 1.0 - k / steps) for k in range(steps + 1)]
    elif M == 3:
        rows = [(i / steps, j / steps, (steps - i - j) / steps) for i in range(steps + 1) for j in range(steps + 1 - i)]
    else:
        raise ValueError(f"fusion_grid: M must be 2 or 3 modalities (got {M!r})")
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


def check_grid(grid, M: int) -> torch.Tensor:
    """The user's grid as a host float32 (G, M) tensor, validated before anything is uploaded."""
    g = torch.as_tensor(grid)
    if g.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"sweep: the grid must be float32 or float64 (got {g.dtype})")
    if g.dim() != 2 or g.shape[1] != M:
        raise ValueError(f"sweep: the grid must be (G, {M}), one weight per modality (got {tuple(g.shape)})")
    if not 1 <= g.shape[0] <= SWEEP_MAXG:
        raise ValueError(f"sweep: the grid must have 1 <= G <= {SWEEP_MAXG} rows (got {g.shape[0]})")
    g = g.detach().cpu()
    if not bool(torch.isfinite(g).all()) or bool((g < 0).any()):
        raise ValueError("sweep: every fusion weight must be finite and non-negative")
    return g.to(torch.float32).contiguous()


class SweepResult(NamedTuple):
    """weights (G, M) float32; tp, pp (G, C) int64: correct / predicted per grid row and class; num (C) int64: samples per class."""
    weights: np.ndarray
    tp: np.ndarray
    pp: np.ndarray
    num: np.ndarray

    @property
    def acc(self) -> np.ndarray:
        """(G,) float64: tp[g].sum() / num.sum().  A (row, g) pair the kernel left out (no weight on anything the row has) is an
        error of g, so a grid row is not rewarded for skipping the samples it cannot classify."""
        return self.tp.sum(axis=1) / np.float64(max(int(self.num.sum()), 1))

    @property
    def counted(self) -> np.ndarray:
        """(G,) int64: the rows grid row g made a prediction for; num.sum() - counted[g] pairs were left out."""
        return self.pp.sum(axis=1)

    def f1(self, average: str = "macro") -> np.ndarray:
        """(G,) float64: F1 = 2 tp / (pp + num) per class, averaged as Evaluator.f1 averages ("macro" | "weighted")."""
        return np.array([f1_from_counts(self.tp[g], self.num, self.pp[g], average) for g in range(self.tp.shape[0])], dtype=np.float64)

    def best(self, metric: str = "acc"):
        """(weights (M,), value, g) of the FIRST maximum in grid order; metric: "acc" | "f1_macro" | "f1_weighted"."""
        if metric not in ("acc", "f1_macro", "f1_weighted"):
            raise ValueError(f"sweep: metric must be 'acc', 'f1_macro' or 'f1_weighted', got {metric!r}")
        v = self.acc if metric == "acc" else self.f1(metric[3:])
        g = int(np.argmax(v))
        return self.weights[g], float(v[g]), g


class FusionSweep:
    """The device side of Evaluator(sweep=): the uploaded grid and the three integer tables."""

    def __init__(self, grid, M: int, C: int, device):
        self.grid_host = check_grid(grid, M)
        self.M, self.C, self.G = M, C, self.grid_host.shape[0]
        self.grid = self.grid_host.to(device)
        self.tp = torch.zeros((self.G, C), device=device, dtype=torch.int32)
        self.pp = torch.zeros((self.G, C), device=device, dtype=torch.int32)
        self.num = torch.zeros(C, device=device, dtype=torch.int32)

    def reset(self) -> None:
        self.tp.zero_()
        self.pp.zero_()
        self.num.zero_()

    def update(self, outs: List[torch.Tensor], labels: torch.Tensor, present: Optional[torch.Tensor] = None) -> None:
        """One batch: the M (B, C) logit matrices, in ONE launch."""
        ops.fusion_sweep(list(outs), labels, self.grid, self.tp, self.pp, num=self.num, present=present)

    def result(self) -> SweepResult:
        """One host sync: the three tables in one copy."""
        flat = torch.cat([self.tp.reshape(-1), self.pp.reshape(-1), self.num]).cpu().numpy().astype("int64")
        n = self.G * self.C
        return SweepResult(self.grid_host.numpy().copy(), flat[:n].reshape(self.G, self.C), flat[n:2 * n].reshape(self.G, self.C),
                           flat[2 * n:])
