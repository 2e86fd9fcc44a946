"""The joint concat-fusion training step (gs_flag false) that MLA is measured against, fused driver, and its evaluator.

    optimizer.zero_grad()                                            main.py:164
    a, v[, t], out = model(...)  /  fusion_module(a, v[, t])         :164-168, 232-237, 273
    out_a, out_v[, out_t] = half / third-head logits                 :283-302
    loss = CE(out, label); loss_m = CE(out_m, label) (reported)      :305-309
    loss.backward()                                                  :310
    OGM / OGM-GE: coefficients from out_m, conv-gradient modulation  :312-410
    optimizer.step()                                                 :416

Orchestration only: every arithmetic step is a libmla_hip.so kernel.  Order of work per step:

  1. every encoder's forward on its own stream (as in MLATrainer: no forward depends on another encoder or on the head);
  2. the concatenated head (mla_concat_head_ce_fwd_bwd: out, out_m, losses, dW, db, every dX_m) once, on the calling stream;
     data parallel: (dW|db|losses) packed into one all-reduce;
  3. OGM / OGM-GE: the coefficients (mla_ogm_coeff) from out_m -- of the GLOBAL batch under data parallelism (the rows of
     every rank gathered in rank order, as torch.nn.DataParallel computes them on the gathered outputs);
  4. each encoder's chain on its own stream: backward from dX_m -> gradient all-reduce -> modulation (inside
     [modulation_starts, modulation_ends]; after the all-reduce, so OGM-GE's std is that of the reduced gradient, as the
     reference reads it after DataParallel's reduction) -> its SGD step;
  5. the head's SGD step on the calling stream.

Unlike MLA no modality waits for another's head update: the M encoder backwards run concurrently.  `set_overlap(False)`
puts every kernel on the calling stream in program order (A/B runs).
"""
from __future__ import annotations

from typing import Optional

import torch

from .dist import Comm
from .evaluators import JointEvaluator  # noqa: F401  (its old home)
from .module import _attached, _joint_fusion
from .modulation import OGM
from .trainer import StreamTrainer

MODULATIONS = ("Normal", "OGM", "OGM_GE")


class JointTrainer(StreamTrainer):
    def __init__(self, model, lr: float = 1e-3, momentum: float = 0.9, weight_decay: float = 1e-4, modulation: str = "Normal",
                 alpha: float = 0.3, modulation_starts: int = 0, modulation_ends: int = 50, seed: int = 0,
                 comm: Optional[Comm] = None):
        """`model`: AVClassifier / M3AEClassifier / Modal3Classifier built with gs_flag false.  `modulation`, `alpha`,
        `modulation_starts`, `modulation_ends`: args.* of main.py:312-410; `seed` keys OGM-GE's noise."""
        if modulation not in MODULATIONS:
            raise NotImplementedError(f"JointTrainer implements --modulation {' | '.join(MODULATIONS)}, not {modulation!r}")
        self.fusion = _attached(_joint_fusion(model), comm, modulation)
        super().__init__(model, lr, momentum, weight_decay, False, comm)
        if self.fusion is not None and not self.fusion.per_modality:          # film / gated: no out_a / out_v, no loss_a / loss_v
            self.losses = {"loss": self.losses["loss"]}
        self.M = len(self.encoders)
        self.modulation = modulation
        self.modulation_starts, self.modulation_ends = modulation_starts, modulation_ends
        dev = model.device
        self.ogm = OGM(alpha, modulation, seed, dev) if modulation != "Normal" else None
        self._msg = torch.empty(self.head.numel + 1 + self.M, device=dev, dtype=torch.float32)

    def _modulating(self, epoch: int) -> bool:
        return self.ogm is not None and self.modulation_starts <= epoch <= self.modulation_ends

    def train_step(self, *batch):
        """AVClassifier:     train_step(spec, image, label, epoch)
        M3AEClassifier:   train_step(token, padding_mask, image, label, epoch)
        Modal3Classifier: train_step(token, padding_mask, image, spec, label, epoch)
        Returns device scalars {'loss', 'loss_a', 'loss_v'[, 'loss_t']} (no host sync).  `self.last`: features, `out`,
        `out_m` (M, B, C) and, with OGM / OGM-GE, `coeff`, `scores`, `ratios` (device tensors)."""
        *inputs, label, epoch = batch
        m, opt = self.model, self.optimizer
        if not getattr(m, "training", True):
            m.train()
        B = label.shape[0]
        inv_batch = 1.0 / (B * self.comm.world)
        opt.zero_grad()                                                                   # main.py:164
        main = torch.cuda.current_stream() if self.overlap_forward else None
        # 1. forwards (main.py:273), one stream per encoder; the concatenated head needs them all
        feats, done = self._forwards(inputs)
        for ev in done or ():
            main.wait_event(ev)
        for (tag, _g, _e), f in zip(self.encoders, feats):
            self.last[tag] = f
        # 2. the concatenated head (main.py:273-310)
        if self.fusion is not None:                           # attached sum / film / gated (out_m None and one loss for film / gated)
            out, out_m, L, dX = self.fusion.forward_backward(list(feats), label, inv_batch, self.last)
        else:
            out, out_m, L, dX = self.head.concat_forward_backward(list(feats), label, inv_batch)
        if self.comm.active:                                  # (dW|db) and the rank-local losses: one message
            n = self.head.numel
            self._msg[:n].copy_(self.head.grad)
            self._msg[n:].copy_(L)
            self.comm.allreduce_small(self._msg)
            self.head.grad.copy_(self._msg[:n])
            L.copy_(self._msg[n:])
        self.last["out"], self.last["out_m"] = out, out_m
        self.losses["loss"].copy_(L[:1])
        for k, (tag, _g, _e) in enumerate(self.encoders if out_m is not None else ()):
            self.losses["loss_" + tag].copy_(L[1 + k:2 + k])
        # 3. OGM coefficients (main.py:314-337 / 373-384), from the global batch
        modulate = self._modulating(epoch)
        if self.ogm is not None:
            outs = [out_m[k] for k in range(self.M)]
            if self.comm.active:
                outs = [self.comm.allgather_rows(o) for o in outs]
                lab = self.comm.allgather_rows(label.contiguous())
            else:
                lab = label
            coeff = self.ogm.coefficients(outs, lab)
            self.last["coeff"] = coeff
            self.last["scores"], self.last["ratios"] = self.ogm.info[:self.M], self.ogm.info[3:3 + self.M]
        # 4. encoder chains: backward (loss.backward()) -> all-reduce -> modulation (main.py:392-408) -> SGD (main.py:416)
        for k, (_tag, grp, enc) in enumerate(self.encoders):
            if enc is None:                                   # stored features (CLIPClassifier): no conv gradient to modulate, dX unused
                continue
            es = self._estreams[k] if self.overlap_forward else None
            if es is not None:
                es.wait_stream(main)                          # dX_m (and the coefficients) are ready
            with self._on(es):
                enc.backward_from_pooled(dX[k], enc._pa)
                self.comm.wait(self.comm.allreduce_flat_async(enc.grad))
                if modulate:
                    self.ogm.modulate_one(enc, k)
                opt.mark_ready(grp)
                opt.step_group(grp)
        if modulate:
            self.ogm.step += 1
        # 5. the head's SGD step
        opt.mark_ready("head")
        opt.step_group("head")
        opt.drop_grads()
        return self.losses
