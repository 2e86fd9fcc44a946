"""The evaluators: `valid()` of the reference for the MLA model (Evaluator), the joint model (JointEvaluator) and QMF (QMFEvaluator),
with their per-class counters kept on the device.  All three take metrics= / capacity= (mla_hip.metrics); Evaluator also takes sweep=
(mla_hip.sweep) and gate_sweep= / gate_prior= / gate_beta= (mla_hip.gate).  `HeadCounts` is the counting of a fused output and its
per-modality logits the joint and the QMF evaluator share.

Orchestration only: every arithmetic step is a libmla_hip.so kernel (csrc/eval_head.hip, metrics.hip, fusion_sweep.hip, gate_sweep.hip).
"""
from __future__ import annotations

import inspect
from typing import Optional

import torch

from . import ops
from ._lib import MLAHipError
from .dist import Comm
from .gate import GateSweep, GateSweepResult, check_gate
from .metrics import MetricsMixin
from .module import _attached, _joint_fusion
from .rows import check_present
from .sweep import FusionSweep, SweepResult


PRESENT_COLUMNS = ("a", "v", "t")       # the columns of a `present` matrix: (audio, image, text), Modal3Batcher.present / Modal3Classifier._calls


def takes_present(model) -> bool:
    """Whether the model's forward takes present= (Modal3Classifier): asked of `_calls`, which forward_raw hands its options to."""
    fn = getattr(model, "_calls", None) or model.forward_raw
    return "present" in inspect.signature(fn).parameters


def check_eval_mode(model, dynamic: bool, dynamic_mode: str, gate_absent: bool) -> None:
    """Evaluator's argument rules, before anything is allocated."""
    if dynamic_mode not in ("batch", "sample"):
        raise ValueError(f"Evaluator: dynamic_mode must be 'batch' (the published batch-level gating) or 'sample' (per-sample "
                         f"gating), got {dynamic_mode!r}")
    if gate_absent and not takes_present(model):
        raise MLAHipError(f"Evaluator: gate_absent needs a model whose forward takes present= (Modal3Classifier); "
                          f"{type(model).__name__} has no missing-modality masks")
    if gate_absent and dynamic and dynamic_mode != "sample":
        raise ValueError("Evaluator: gate_absent leaves a modality out of single samples' fusion; with dynamic=True that needs "
                         "dynamic_mode='sample' (the batch-level gating has one weight per modality for the whole batch)")


def present_in_encoder_order(model, present, B: int) -> torch.Tensor:
    """The user's host (B, 3) `present` matrix, columns PRESENT_COLUMNS, as uint8 (B, M) with one column per mla_encoders() entry
    in that order -- the pairing Modal3Classifier._calls makes between the columns and its encoders."""
    have = check_present(present, B, len(PRESENT_COLUMNS))
    cols = [PRESENT_COLUMNS.index(tag) for tag, _g, _e in model.mla_encoders()]
    return have[:, cols].to(torch.uint8).contiguous()


class Evaluator(MetricsMixin):
    """`valid()` of the reference under --gs_flag (main.py:486-679): eval-mode encoders, shared head applied to every
    modality, fixed (av_alpha | a/v/t_alpha) or entropy-gated (--dynamic, main.py:65-106) fusion, per-class accuracy
    counters -- kept on the device (one fusion/arg-max kernel per batch instead of the per-sample .cpu() loop of
    main.py:659-676).  Data parallel: the dynamic weights are ONE scalar per modality computed over the whole
    batch (softmax over dim 0), so they depend on the batch composition; the reference evaluates the global batch on GPU 0
    (DataParallel gathers the features, main.py:624-639).  With an active `comm` every rank all-gathers the (B_local, C)
    logits and labels of all ranks (rank order = the order DataParallel scatters / gathers in) on the head communicator
    and runs the fusion kernel on the global batch: every rank holds the same counters and weights as a single process
    evaluating the concatenated batch."""

    def __init__(self, model, dynamic: bool = False, av_alpha: float = 0.5, a_alpha: float = 0.35, v_alpha: float = 0.25,
                 t_alpha: float = 0.4, comm: Optional[Comm] = None, dynamic_mode: str = "batch", gate_absent: bool = False,
                 metrics: bool = False, capacity: Optional[int] = None, sweep=None, gate_sweep=None, gate_prior=None,
                 gate_beta=None):
        """dynamic_mode (with dynamic=True): "batch", the published rule above, or "sample": every sample is gated by the entropy of
        its OWN class distribution (the reference's commented-out softmax(dim=1)), one weight vector per sample.
        gate_absent (models whose update takes present=, i.e. Modal3Classifier): a modality a sample does not have is left out of
        that sample's fusion, weight +0.0, and the others are renormalised -- with the fixed alphas or with dynamic_mode="sample".
        Either one takes the per-sample path: features to counters in ONE launch (ops.eval_head) instead of M head launches and
        the fusion kernel; independent of the batch a sample arrives in, so under data parallel each rank counts its own rows, no
        all-gather, and result() / per_class() sum the counters over the ranks.  That path sets `sample_weights` (B, M), `pred`
        (B, 1 + M: fused arg-max, then each modality's) and `fused` (B, C) of the last batch, in reused buffers; `weights` stays
        the batch-level vector of the default path.
        metrics=True, capacity=len(test_set): every update() also appends the batch's class scores (softmax of the fused and of each
        modality's logits), arg-max predictions and labels to a device store, one more launch per batch; average_precision(),
        mean_average_precision(), confusion() and f1() are formed from it (mla_hip.metrics).  Not with an active `comm`.
        sweep=grid (a host (G, M) tensor of finite, non-negative fusion weights, e.g. fusion_grid(M, steps)): every update() also
        scores the FIXED-weight fusion of the batch at every grid row, one more launch per batch on the logits the update holds
        anyway; sweep_result() answers the accuracy / F1 surface (mla_hip.sweep).  Whatever the evaluator's own mode: with
        dynamic=True it tells whether any fixed weighting beats the gating.  With gate_absent the sweep leaves out what the
        evaluator's fusion leaves out.  Not with an active `comm`.
        gate_sweep=grid (a host (G, M + 1) tensor of gates (a_0 .. a_{M-1}, beta), e.g. gate_grid(M, betas, steps)): every update()
        also scores the gated fusion w_m ~ a_m exp(-beta H_m) of the batch at every gate, one more launch per batch on the same
        logits; gate_sweep_result() answers the surface (mla_hip.gate).  Whatever the evaluator's own mode, under the masks its own
        fusion took (gate_absent + present=).  Not with an active `comm`.
        gate_prior (M floats) / gate_beta (with dynamic=True, dynamic_mode="sample"): the per-sample path gates with that gate
        (ops.eval_head_gated) instead of a = 1, beta = 1; giving one alone leaves the other at 1.  Search it on a validation split."""
        check_eval_mode(model, dynamic, dynamic_mode, gate_absent)
        if (gate_prior is not None or gate_beta is not None) and not (dynamic and dynamic_mode == "sample"):
            raise ValueError("Evaluator: gate_prior / gate_beta shape the per-sample entropy gating; they need dynamic=True, "
                             "dynamic_mode='sample'")
        self.model = model
        self.comm = comm if comm is not None else Comm()
        self.head = model.fusion_module.fc_out
        self.M = len(model.mla_encoders())
        self.C = self.head.out_features
        self.dynamic = dynamic
        self.dynamic_mode, self.gate_absent = dynamic_mode, bool(gate_absent)
        self.per_sample = bool(gate_absent) or (bool(dynamic) and dynamic_mode == "sample")
        self.alphas = [av_alpha, 1.0 - av_alpha] if self.M == 2 else [a_alpha, v_alpha, t_alpha]      # main.py:647-651
        self.counts = torch.zeros(self.C * (2 + self.M), device=model.device, dtype=torch.int32)
        self.weights = torch.zeros(3, device=model.device, dtype=torch.float32)
        self._sample: dict = {}
        self._metrics_init(metrics, capacity, 1 + self.M, self.C, model.device, self.comm)
        # the batch-level path never materialises the fused logits: the store forms them from the weights the fusion kernel used
        self._fixed_weights = torch.tensor(self.alphas, device=model.device, dtype=torch.float32) if self._store is not None else None
        self._sweep = None
        if sweep is not None:
            if self.comm.active:
                raise NotImplementedError("Evaluator: sweep= counts each rank's own rows; summing the tables across ranks is not "
                                          "implemented -- run the fusion-weight search in one process")
            self._sweep = FusionSweep(sweep, self.M, self.C, model.device)
        self._gate = None if gate_prior is None and gate_beta is None else check_gate(gate_prior, gate_beta, self.M)
        self._gate_sweep = None
        if gate_sweep is not None:
            if self.comm.active:
                raise NotImplementedError("Evaluator: gate_sweep= counts each rank's own rows; summing the tables across ranks is "
                                          "not implemented -- run the gate search in one process")
            self._gate_sweep = GateSweep(gate_sweep, self.M, self.C, model.device)
        model.eval()                                                                                   # main.py:519

    def reset(self) -> None:
        self.counts.zero_()
        self._metrics_reset()
        if self._sweep is not None:
            self._sweep.reset()
        if self._gate_sweep is not None:
            self._gate_sweep.reset()

    def _sample_bufs(self, B: int) -> dict:
        if B not in self._sample:
            dev, M, C = self.model.device, self.M, self.C
            self._sample[B] = {"logits": torch.empty((M, B, C), device=dev, dtype=torch.float32),
                               "fused": torch.empty((B, C), device=dev, dtype=torch.float32),
                               "weights": torch.empty((B, M), device=dev, dtype=torch.float32),
                               "pred": torch.empty((B, 1 + M), device=dev, dtype=torch.int32),
                               "present": torch.empty((B, M), device=dev, dtype=torch.uint8)}
        return self._sample[B]

    def _update_per_sample(self, feats, label, present):
        B = label.shape[0]
        buf = self._sample_bufs(B)
        have = None
        if self.gate_absent and present is not None:
            buf["present"].copy_(present_in_encoder_order(self.model, present, B))
            have = buf["present"]
        if self._gate is not None:
            ops.eval_head_gated(list(feats), self.head.weight.detach(), self.head.bias.detach(), label, self.counts, buf["logits"],
                                prior=self._gate[0], beta=self._gate[1], present=have, fused_out=buf["fused"],
                                weights_out=buf["weights"], pred_out=buf["pred"])
        else:
            ops.eval_head(list(feats), self.head.weight.detach(), self.head.bias.detach(), label, self.counts, buf["logits"],
                          mode=1 if self.dynamic else 0, alphas=self.alphas, present=have, fused_out=buf["fused"],
                          weights_out=buf["weights"], pred_out=buf["pred"])
        self.sample_weights, self.pred, self.fused = buf["weights"], buf["pred"], buf["fused"]
        outs = [buf["logits"][m] for m in range(self.M)]
        if self._store is not None:
            at = self._store.n
            self._metrics_append([buf["fused"]] + outs, label)
            if self.gate_absent:                     # a row the kernel counted nowhere (pred -1) is stored as a row without a class
                self._store.labels[at:at + B].masked_fill_(buf["pred"][:, 0] < 0, -1)
        if self._sweep is not None:
            self._sweep.update(outs, label, have)
        if self._gate_sweep is not None:
            self._gate_sweep.update(outs, label, have)
        return outs

    def update(self, *batch, present=None):
        """update(spec, image, label) | update(token, padding_mask, image, label) | update(token, pm, image, spec, label, present=None).
        present (Modal3Classifier only): host bool / uint8 (B, 3) as in MLATrainer.train_step; with gate_absent it also takes the
        absent modalities out of each sample's fusion.  Returns the per-modality logits."""
        *inputs, label = batch
        feats = self.model.forward_raw(*inputs, **({} if present is None else {"present": present}))
        if self.per_sample:
            return self._update_per_sample(feats, label, present)
        outs = [self.head.logits(f, slot="eval_" + str(k)) for k, f in enumerate(feats)]
        if self.comm.active:                                         # global batch (Q9): (world * B_local, C) in rank order
            g_outs = [self.comm.allgather_rows(o) for o in outs]
            g_label = self.comm.allgather_rows(label.contiguous())
            ops.eval_fuse(g_outs, g_label, self.counts, self.weights, self.dynamic, self.alphas)
        else:
            ops.eval_fuse(outs, label, self.counts, self.weights, self.dynamic, self.alphas)
        if self._store is not None:
            self._metrics_append([None] + outs, label, self.weights if self.dynamic else self._fixed_weights)
        if self._sweep is not None:
            self._sweep.update(outs, label)
        if self._gate_sweep is not None:
            self._gate_sweep.update(outs, label)
        return outs

    def _global_counts(self) -> torch.Tensor:
        """The counters of all ranks as (2 + M, C).  The batch-level path evaluates the global batch on every rank already; the
        per-sample path sums a COPY over the ranks on the head communicator, the local counters stay local."""
        c = self.counts
        if self.per_sample and self.comm.active:
            c = c.clone()
            self.comm.allreduce_small(c)
        return c.view(2 + self.M, self.C)

    def result(self):
        """(acc, acc_a, acc_v[, acc_t]) = sum(acc)/sum(num) as in main.py:677-679 (one host sync)."""
        c = self._global_counts().sum(dim=1).cpu().tolist()
        num = max(c[0], 1)
        return tuple(x / num for x in c[1:])

    def per_class(self):
        """The counters as a host int64 array (2 + M, C): samples per class, fused-correct per class, then each modality's
        correct per class (the acc / num lists of main.py:659-676; one host sync)."""
        return self._global_counts().cpu().numpy().astype("int64")

    def sweep_result(self) -> SweepResult:
        """The tables of sweep=grid as a SweepResult: weights, tp, pp, num, acc, counted, f1(average), best(metric) (one host sync)."""
        if self._sweep is None:
            raise MLAHipError("Evaluator: constructed with sweep=None; pass sweep=fusion_grid(M, steps) or a (G, M) tensor of weights")
        return self._sweep.result()

    def gate_sweep_result(self) -> GateSweepResult:
        """The tables of gate_sweep=grid as a GateSweepResult: priors, beta, tp, pp, num, acc, counted, f1(average), best(metric) (one
        host sync)."""
        if self._gate_sweep is None:
            raise MLAHipError("Evaluator: constructed with gate_sweep=None; pass gate_sweep=gate_grid(M, betas, steps) or a (G, M + 1) "
                              "tensor of gates")
        return self._gate_sweep.result()


class HeadCounts:
    """Arg-max counters (first maximum, like np.argmax) of a fused output `out` and its M = 2 or 3 per-modality logits, all (B, C),
    from plain tensors.  They come from the fusion / accuracy kernel (mla_eval_fuse) fed with (out, out_a, out_v) and the fixed
    weights (1, 0, 0): its fused prediction is then exactly arg-max(out); with three modalities a second call counts out_t.
    counts int32 (5 * C): [num, argmax(out), argmax(out), argmax(out_a), argmax(out_v)] per class; counts_t int32 (4 * C):
    [num, argmax(out_t) three times]; weights: the kernel's weight output, scratch.  A row whose label is outside [0, C) is counted
    nowhere."""

    def __init__(self, M: int, C: int, device):
        self.M, self.C = M, C
        self.counts = torch.zeros(C * 5, device=device, dtype=torch.int32)
        self.counts_t = torch.zeros(C * 4, device=device, dtype=torch.int32)
        self.weights = torch.zeros(3, device=device, dtype=torch.float32)

    def reset(self) -> None:
        self.counts.zero_()
        self.counts_t.zero_()

    def count(self, out, out_m, label) -> None:
        ops.eval_fuse([out, out_m[0], out_m[1]], label, self.counts, self.weights, False, [1.0, 0.0, 0.0])
        if self.M == 3:
            ops.eval_fuse([out_m[2], out_m[2]], label, self.counts_t, self.weights, False, [1.0, 0.0])

    def result(self, per_modality: bool = True):
        """(acc, acc_a, acc_v[, acc_t]) = sum(acc) / sum(num) (main.py:677-679; one host sync); per_modality=False: (acc,)."""
        c = self.counts.view(5, self.C).sum(dim=1).cpu().tolist()
        num = max(c[0], 1)
        if not per_modality:
            return (c[1] / num,)
        res = [c[1] / num, c[3] / num, c[4] / num]
        if self.M == 3:
            res.append(self.counts_t.view(4, self.C).sum(dim=1)[1].item() / num)
        return tuple(res)


class JointEvaluator(HeadCounts, MetricsMixin):
    """`valid()` of the joint model (main.py:539-619, 653-679): eval-mode encoders, out = fc_out(cat(...)) and the half /
    third-head logits out_m, arg-max predictions and per-class counters kept on the device (HeadCounts).
    Data parallel: every rank all-gathers out / out_m / labels of all ranks in rank order and counts the global batch, as
    `Evaluator` does.

    metrics=True, capacity=len(test_set): every update() also appends softmax(out) and softmax(out_m), their arg-max and the labels
    to a device store (mla_hip.metrics: average_precision(), mean_average_precision(), confusion(), f1()); film / gated fusion
    stores `out` alone, the reference defines no out_a there.  Not with an active `comm`."""

    def __init__(self, model, comm: Optional[Comm] = None, metrics: bool = False, capacity: Optional[int] = None):
        self.fusion = _attached(_joint_fusion(model), comm)
        self.model = model
        self.comm = comm if comm is not None else Comm()
        self.head = self.fusion if self.fusion is not None else model.fusion_module.fc_out
        HeadCounts.__init__(self, len(model.mla_encoders()), self.head.out_features, model.device)
        self.per_modality = self.fusion is None or self.fusion.per_modality    # film / gated: the reference defines no out_a / out_v
        self._metrics_init(metrics, capacity, 1 + self.M if self.per_modality else 1, self.C, model.device, self.comm)
        model.eval()                                                                # main.py:519

    def reset(self) -> None:
        HeadCounts.reset(self)
        self._metrics_reset()

    def update(self, *batch):
        """update(spec, image, label) | update(token, padding_mask, image, label) | update(token, pm, image, spec, label).
        Returns (out, out_m) of the local batch."""
        *inputs, label = batch
        feats = self.model.forward_raw(*inputs)
        if self.fusion is not None:                           # sum: out_m with HALF the bias (main.py:610-614); film / gated: none
            out, out_m = self.fusion.logits(list(feats), bias_scale=0.5, slot="eval")
        else:
            out, out_m = self.head.concat_logits(list(feats), slot="eval")
        outs = [out] + [out_m[k] if out_m is not None else out for k in range(self.M)]
        if self._store is not None:
            self._metrics_append(outs[:self._store.H], label)
        if self.comm.active:
            outs = [self.comm.allgather_rows(o) for o in outs]
            label = self.comm.allgather_rows(label.contiguous())
        self.count(outs[0], outs[1:], label)
        return out, out_m

    def result(self):
        return HeadCounts.result(self, self.per_modality)


class QMFEvaluator(HeadCounts, MetricsMixin):
    """`valid()` under QMF (main.py:576-586, 653-679): eval-mode encoders, out = sum_m conf_m out_m, arg-max counters of `out`
    and of every out_m, kept on the device (HeadCounts).
    metrics=True, capacity=len(test_set): every update() also appends softmax(out) and softmax(out_m), their arg-max and the labels
    to a device store (mla_hip.metrics: average_precision(), mean_average_precision(), confusion(), f1())."""

    def __init__(self, model, metrics: bool = False, capacity: Optional[int] = None):
        if model.qmf_heads is None:
            raise MLAHipError("QMFEvaluator needs a model with attached QMF heads (attach_qmf_heads / QMFTrainer)")
        self.model, self.heads = model, model.qmf_heads
        HeadCounts.__init__(self, len(self.heads), self.heads[0].out_features, model.device)
        self._bufs: dict = {}
        self._metrics_init(metrics, capacity, 1 + self.M, self.C, model.device)
        model.eval()                                                                # main.py:519

    def reset(self) -> None:
        HeadCounts.reset(self)
        self._metrics_reset()

    def update(self, *batch):
        """update(spec, image, label) | update(token, padding_mask, image, label) | update(token, pm, image, spec, label).
        Returns (out, out_m (M, B, C))."""
        *inputs, label = batch
        feats = self.model.forward_raw(*inputs)
        B = label.shape[0]
        if B not in self._bufs:
            f32 = dict(device=self.model.device, dtype=torch.float32)
            self._bufs[B] = (torch.empty((self.M, B, self.C), **f32), torch.empty((B, self.C), **f32), torch.empty((self.M, B), **f32))
        z, out, conf = self._bufs[B]
        ops.qmf_head_fwd(list(feats), [h.weight.detach() for h in self.heads], [h.bias.detach() for h in self.heads], z, out, conf)
        outs = [z[m] for m in range(self.M)]
        self._metrics_append([out] + outs, label)
        self.count(out, outs, label)
        return out, z
