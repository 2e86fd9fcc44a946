"""Gate search: the gated fusion family w_m ~ a_m exp(-beta H_m) scored on a grid of gates, as a by-product of one evaluation pass.

The entropy gating of the evaluators (dynamic=True) is one point of that family, a = 1 and beta = 1; the fixed-weight fusion is its
beta = 0 edge.  A gate is (a_0 .. a_{M-1}, beta): a non-negative prior per modality and an inverse temperature on each sample's
entropies (include/mla_hip.h states the rule).  The per-modality logits and entropies do not depend on the gate, and an Evaluator
holds the logits on the device in every update(): with gate_sweep=grid one more launch per batch (csrc/gate_sweep.hip) scores every
gate of the grid, into the integer tables of the fusion-weight search (mla_hip.sweep).  Evaluator(gate_prior=, gate_beta=) then
evaluates with the gate the search found -- found on a validation split, not on the split it is reported on.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import ops
from .sweep import SWEEP_MAXG, SweepResult, fusion_grid

GATE_MAX_PRIOR = 1024.0    # csrc/gate_args.h: with these caps no intermediate of the rule can overflow in fp32
GATE_MAX_BETA = 16.0


def gate_grid(M: int, betas: Sequence[float] = (0, 0.5, 1, 2, 4, 8), steps: int = 20) -> torch.Tensor:
    """Host float32 (G, M + 1) grid of gates, row = (a_0 .. a_{M-1}, beta): beta outer (in the order given), the priors of
    fusion_grid(M, steps) inner, G = len(betas) * len(fusion_grid(M, steps))."""
    betas = [float(b) for b in betas]
    if not betas:
        raise ValueError("gate_grid: betas must hold at least one inverse temperature")
    priors = fusion_grid(M, steps)
    rows = [torch.cat([priors, torch.full((priors.shape[0], 1), b, dtype=torch.float64).to(torch.float32)], dim=1) for b in betas]
    return torch.cat(rows, dim=0).contiguous()


def check_gate_grid(grid, M: int) -> torch.Tensor:
    """The user's grid as a host float32 (G, M + 1) tensor inside the contract on a gate, validated before anything is uploaded."""
    g = torch.as_tensor(grid)
    if g.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"gate_sweep: the grid must be float32 or float64 (got {g.dtype})")
    if g.dim() != 2 or g.shape[1] != M + 1:
        raise ValueError(f"gate_sweep: the grid must be (G, {M + 1}), one prior per modality and beta (got {tuple(g.shape)})")
    if not 1 <= g.shape[0] <= SWEEP_MAXG:
        raise ValueError(f"gate_sweep: the grid must have 1 <= G <= {SWEEP_MAXG} rows (got {g.shape[0]})")
    g = g.detach().cpu().to(torch.float32).contiguous()           # the contract is on what the kernel reads
    if not bool(torch.isfinite(g).all()) or bool((g < 0).any()):
        raise ValueError("gate_sweep: every prior and every beta must be finite and non-negative")
    if bool((g[:, :M] > GATE_MAX_PRIOR).any()) or bool((g[:, M] > GATE_MAX_BETA).any()):
        raise ValueError(f"gate_sweep: every prior must be at most {GATE_MAX_PRIOR:g} and every beta at most {GATE_MAX_BETA:g}")
    return g


def check_gate(prior, beta, M: int):
    """(prior: M floats, beta: float) of Evaluator(gate_prior=, gate_beta=); None means 1.  Inside the contract on a gate."""
    prior = [1.0] * M if prior is None else [float(v) for v in np.asarray(prior, dtype=np.float64).reshape(-1)]
    beta = 1.0 if beta is None else float(beta)
    if len(prior) != M:
        raise ValueError(f"Evaluator: gate_prior must hold {M} priors, one per modality (got {len(prior)})")
    if not all(math.isfinite(v) and 0.0 <= v <= GATE_MAX_PRIOR for v in prior):
        raise ValueError(f"Evaluator: every gate_prior must be finite and in [0, {GATE_MAX_PRIOR:g}] (got {prior})")
    if not (math.isfinite(beta) and 0.0 <= beta <= GATE_MAX_BETA):
        raise ValueError(f"Evaluator: gate_beta must be finite and in [0, {GATE_MAX_BETA:g}] (got {beta})")
    return prior, beta


class GateSweepResult(NamedTuple):
    """priors (G, M) float32, beta (G,) float32; tp, pp (G, C) int64: correct / predicted per gate and class; num (C) int64: samples
    per class.  acc, counted and f1 are SweepResult's, on the same tables."""
    priors: np.ndarray
    beta: np.ndarray
    tp: np.ndarray
    pp: np.ndarray
    num: np.ndarray

    @property
    def counts(self) -> SweepResult:
        return SweepResult(self.priors, self.tp, self.pp, self.num)

    @property
    def acc(self) -> np.ndarray:
        """(G,) float64: tp[g].sum() / num.sum(); a pair the kernel left out is an error of gate g."""
        return self.counts.acc

    @property
    def counted(self) -> np.ndarray:
        """(G,) int64: the rows gate g made a prediction for."""
        return self.counts.counted

    def f1(self, average: str = "macro") -> np.ndarray:
        """(G,) float64, averaged as Evaluator.f1 averages ("macro" | "weighted")."""
        return self.counts.f1(average)

    def best(self, metric: str = "acc"):
        """(prior (M,), beta, value, g) of the FIRST maximum in grid order; metric: "acc" | "f1_macro" | "f1_weighted"."""
        prior, value, g = self.counts.best(metric)
        return prior, float(self.beta[g]), value, g


class GateSweep:
    """The device side of Evaluator(gate_sweep=): the uploaded grid and the three integer tables."""

    def __init__(self, grid, M: int, C: int, device):
        self.grid_host = check_gate_grid(grid, M)
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
        ops.gate_sweep(list(outs), labels, self.grid, self.tp, self.pp, num=self.num, present=present)

    def result(self) -> GateSweepResult:
        """One host sync: the three tables in one copy."""
        flat = torch.cat([self.tp.reshape(-1), self.pp.reshape(-1), self.num]).cpu().numpy().astype("int64")
        n = self.G * self.C
        grid = self.grid_host.numpy()
        return GateSweepResult(grid[:, :self.M].copy(), grid[:, self.M].copy(), flat[:n].reshape(self.G, self.C),
                               flat[n:2 * n].reshape(self.G, self.C), flat[2 * n:])
