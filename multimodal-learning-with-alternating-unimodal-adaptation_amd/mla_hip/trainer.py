"""The MLA alternating-unimodal training step (main.py:419-476), fused driver.

    joint forward of both encoders                                   main.py:431
    for modality in (audio, visual):                                 main.py:432-454
        head forward + CE + head/feature gradients                   :432-435 / :444-447
        encoder backward
        GSPlugin.before_update on the head gradient                  :437 / :449
        optimizer.step(); optimizer.zero_grad(); exp_count += 1      :439-442 / :451-454
    drop gradients, accumulate the reported losses                   :468-476

Orchestration only: every arithmetic step is a libmla_hip.so kernel.  Quirks reproduced:
Q5 (exp_count / alpha), Q6 (`legacy_zero_grad`), Q7 (visual logits use the head already updated by the
audio step), Q8 (av_alpha fixed at 0.55 in the reported loss).
"""
from __future__ import annotations

import contextlib
import os
from typing import Optional

import torch

from .streams import distinct_streams

from . import ops
from .dist import Comm
from .evaluators import PRESENT_COLUMNS, Evaluator, check_eval_mode, present_in_encoder_order, takes_present  # noqa: F401  (their old home)
from .module import is_attached_fusion
from .optim import FusedAdam, FusedSGD
from .plugin import GSPlugin
from .rows import compact_feature_grad


class StreamTrainer:
    """What MLATrainer and JointTrainer share: model / head / encoders / one optimiser group per encoder and one for the head /
    `comm` / the reported `losses` / `last`, and the per-encoder stream pipeline.

    One HIP stream per encoder carries that encoder's whole chain -- forward, backward, gradient all-reduce, SGD -- and a
    second one its weight-gradient GEMMs; the stream train_step is called on carries only the head path and hands features /
    feature gradients over with events.  No encoder forward depends on the head or on another encoder (Q7), and the next
    STEP's first forward only needs that encoder's own SGD, so the encoder chains run beside each other and across step
    boundaries and fill each other's kernel tails."""

    def __init__(self, model, lr, momentum: float, weight_decay: float, legacy_zero_grad: bool, comm: Optional[Comm],
                 extra_groups: Optional[dict] = None, optimizer: str = "sgd", adam: Optional[dict] = None):
        """extra_groups: further optimiser groups (name -> flat-buffer object) after the encoders' and the head's.
        optimizer: "sgd" (FusedSGD(lr, momentum, weight_decay)) or "adam" (FusedAdam(lr, weight_decay, **adam); `lr` may then be a
        mapping group name -> lr, and `adam` holds betas / eps / param_groups, e.g. param_groups=cav_param_groups(model, lr))."""
        self.model = model
        fusion = model.fusion_module                            # an attached sum / film / gated fusion (mla_hip.fusion) owns its Linears
        self.head = fusion if is_attached_fusion(fusion) else fusion.fc_out
        self.encoders = model.mla_encoders()                    # [(tag, group, encoder)], alternation / concatenation order
        self.feature_only = bool(getattr(model, "feature_only", False))       # stored features: no encoder, no encoder group
        groups = {grp: enc for _t, grp, enc in self.encoders if enc is not None}
        groups["head"] = self.head
        groups.update(extra_groups or {})
        if optimizer == "sgd":
            self.optimizer = FusedSGD(groups, lr, momentum, weight_decay, legacy_zero_grad)
        elif optimizer == "adam":
            if comm is not None and comm.world > 1:
                raise NotImplementedError("optimizer='adam' is not implemented for data-parallel training (comm.world > 1)")
            self.optimizer = FusedAdam(groups, lr=lr, weight_decay=weight_decay, legacy_zero_grad=legacy_zero_grad, **(adam or {}))
        else:
            raise ValueError(f"optimizer must be 'sgd' or 'adam', got {optimizer!r}")
        self.comm = comm if comm is not None else Comm()
        dev = model.device
        self.losses = {k: torch.zeros(1, device=dev, dtype=torch.float32) for k in ["loss"] + ["loss_" + t for t, _g, _e in self.encoders]}
        self.last = {}
        self._can_overlap = dev.type == "cuda" and hasattr(model, "forward_split") and not self.feature_only
        # encoder chains first (they must not share a hardware queue with each other or with the caller's stream), then the
        # weight-gradient side streams, which may double up when the queues run out (streams.py)
        ne = len(self.encoders)
        pool = distinct_streams(2 * ne, dev) if self._can_overlap else []
        self._estreams, self._wstreams = pool[:ne], pool[ne:]
        self.overlap_forward = False
        self.set_overlap(self._can_overlap)

    def join(self) -> None:
        """Make the current stream wait for every encoder chain (parameters, momentum, gradients, BN buffers final).
        Encoders do this themselves when they are used from another stream (forward, state_dict, ...); call it before
        touching optimizer state or raw buffers on the current stream without a device synchronize."""
        if self._estreams and torch.cuda.is_available():
            cur = torch.cuda.current_stream()
            for es in self._estreams:
                cur.wait_stream(es)

    def set_overlap(self, on: bool) -> None:
        """Per-encoder stream pipeline on / off (off: every kernel of the step on the current stream, in program order)."""
        self.join()
        self.overlap_forward = bool(on) and self._can_overlap
        for k, (_t, _g, enc) in enumerate(self.encoders):
            if enc is None:
                continue
            if enc.side_wgrad:
                enc.wgrad_stream = self._wstreams[k] if self.overlap_forward else None
            enc.tail_stream = self._estreams[k] if self.overlap_forward else None

    def _on(self, stream):
        return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()

    def _forwards(self, inputs, **options):
        """The joint forward (main.py:424-431, 273): (features, their completion events).  Under the pipeline each encoder's
        forward is enqueued on its own stream and the caller decides when to wait for which event; else the events are None.
        `options`: the model's forward keywords (Modal3Classifier: present=)."""
        if not self.overlap_forward:
            return self.model.forward_raw(*inputs, **options), None
        main = torch.cuda.current_stream()
        feats, done = [], []
        for es, f in zip(self._estreams, self.model.forward_split(*inputs, **options)):
            es.wait_stream(main)       # inputs are ready; the previous step's head has read this encoder's features
            with torch.cuda.stream(es):
                feats.append(f())      # stream order on `es`: after this encoder's SGD of the previous step
                ev = torch.cuda.Event()
                ev.record()
                done.append(ev)
        return feats, done


class MLATrainer(StreamTrainer):
    def __init__(self, model, lr: float = 1e-3, momentum: float = 0.9, weight_decay: float = 1e-4,
                 gs_mode: str = "as_intended", legacy_zero_grad: bool = False, av_alpha: float = 0.55,
                 comm: Optional[Comm] = None, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8,
                 param_groups: Optional[list] = None):
        """`model`: AVClassifier (ResNet-18 audio+visual), M3AEClassifier (text+image), Modal3Classifier, CAVClassifier or
        CLIPClassifier (stored features: train_step(token_feat, image_feat, label, batch_step, len_dataloader)).  The calling
        stream carries head forward/backward, the packed head exchange, GSPlugin and the head's SGD; the next modality only
        needs the updated head, so the last modality's backward overlaps the next step's first forward.
        gs_mode: GSPlugin's mode -- "as_intended" (the literal utils/utils.py:34-41), "as_published" (never fires) or "owm" (the
        scalar-denominator rule without renormalisation; the fused feature phase then runs mla_feature_phase_owm).
        optimizer="adam" (main.py:736-747): torch.optim.Adam semantics with `betas`, `eps`, `weight_decay`; `lr` a float, a mapping
        {"audio" | ...: lr, "head": lr}, or per-parameter `param_groups` such as `cav_param_groups(model, lr)`; `momentum` is unused."""
        adam = dict(betas=betas, eps=eps, param_groups=param_groups) if optimizer == "adam" else None
        super().__init__(model, lr, momentum, weight_decay, legacy_zero_grad, comm, optimizer=optimizer, adam=adam)
        self.gs_plugin = GSPlugin(dim=self.head.in_features, device=model.device, mode=gs_mode)
        self.av_alpha = av_alpha
        dev = model.device
        self._colsum = torch.empty(self.head.in_features, device=dev, dtype=torch.float32)
        self._msg = torch.empty(self.head.numel + self.head.in_features + 1, device=dev, dtype=torch.float32)
        # Optional HIP-event brackets around the two data-parallel waits of a step (bench.py --gpus N): the packed head exchange
        # (critical path, calling stream) and the wait for an encoder's gradient all-reduce in front of its SGD launch (that
        # encoder's stream).  {"head_exchange": [(start, end)...], "grad_wait": [...]} or None (off: nothing is recorded).
        self.dist_events: Optional[dict] = None
        # Feature-only model (CLIPClassifier): a phase is one mla_feature_phase call.  $MLA_FEATURE_FUSED=0 (read here) or
        # `fused_feature_phase = False` runs the same step on the general chain instead (A/B measurements).
        self.fused_feature_phase = self.feature_only and os.environ.get("MLA_FEATURE_FUSED", "1") != "0"
        self._fbufs: dict = {}
        if self.feature_only and self.comm.world > 1:
            raise NotImplementedError("data-parallel training (comm.world > 1) is not implemented for a feature-only model")

    keep_debug = False

    def _fused_phase(self, name: str, feat: torch.Tensor, label: torch.Tensor, inv_batch: float, batch_step: int,
                     len_dataloader: int) -> None:
        """One modality phase (main.py:432-442) of a feature-only model as ONE mla_feature_phase call: head forward, CE, head
        gradients, GSPlugin.before_update and the head's SGD on the optimiser's own momentum buffer; no dX, and the projected
        gradient never reaches memory (so `keep_debug` takes the chain)."""
        head, opt, gs = self.head, self.optimizer, self.gs_plugin
        B, D, C = feat.shape[0], head.in_features, head.out_features
        if (B, name) not in self._fbufs:
            f32 = dict(device=feat.device, dtype=torch.float32)
            self._fbufs[(B, name)] = (torch.empty((B, C), **f32), torch.empty(1, **f32), torch.empty(ops.feature_ws_elems(B, D, C), **f32))
        logits, loss, ws = self._fbufs[(B, name)]
        fires = gs.mode != "as_published" and gs.exp_count != 0                                # utils/utils.py:29-32 (Q1, Q5)
        if fires and gs.Pl.shape[0] != D:
            gs._resize(D)
        lr, mom, wd = opt._hyper("head")
        n = head.weight.numel()
        ops.feature_phase(feat, label, head.flat[:n].view(C, D), head.flat[n:], opt.buf["head"], gs.Pl if fires else None, logits, loss,
                          ws, inv_batch, fires, gs.alpha(batch_step, len_dataloader), lr, mom, wd, first=not opt.initialized["head"],
                          owm=gs.mode == "owm")
        opt.initialized["head"] = True
        gs._fired = gs._fired or fires
        gs.exp_count += 1                                                                     # :442
        self.last["out_" + name] = logits
        self.losses["loss_" + name].copy_(loss)

    def _fused_ok(self) -> bool:
        opt = self.optimizer
        return (self.fused_feature_phase and not self.keep_debug and isinstance(opt, FusedSGD)
                and opt.seg_initialized["head"] is None)

    def _phase(self, name: str, enc, feat: torch.Tensor, label: torch.Tensor, inv_batch: float,
               batch_step: int, len_dataloader: int, bstream):
        """One modality phase (main.py:432-442).  Critical path on the current stream: head forward/backward ->
        (data parallel: packed head exchange) -> GSPlugin -> head SGD.  The encoder backward (and its gradient
        all-reduce) is NOT on that path -- the next modality only needs the updated head -- so when `bstream` (the
        encoder's own stream) is given it is enqueued there and runs beside the following phases and the next step's
        forwards.  Returns the all-reduce work handles."""
        logits, loss, dX = self.head.forward_backward(feat, label, inv_batch, slot=name)               # :432-435
        self.last["out_" + name] = logits
        self.losses["loss_" + name].copy_(loss)
        if enc is None:
            works = []                                                                        # stored features: nothing behind dX
        elif bstream is None:
            enc.backward_from_pooled(compact_feature_grad(enc, dX), enc._pa)                  # loss.backward()
            works = self.comm.allreduce_flat_async(enc.grad)                                 # overlaps what follows
        else:
            bstream.wait_stream(torch.cuda.current_stream())                                  # dX (and the forward) are ready
            with torch.cuda.stream(bstream):
                enc.backward_from_pooled(compact_feature_grad(enc, dX), enc._pa)
                works = self.comm.allreduce_flat_async(enc.grad)
        fires = self.gs_plugin.mode != "as_published" and self.gs_plugin.exp_count != 0
        r_mean = None
        if self.comm.active:
            ops.colsum(feat, self._colsum, inv_batch)
            ev0 = self._ev_begin()
            self.comm.exchange_head(self.head.grad, self._colsum, self.losses["loss_" + name], self._msg)
            self._ev_end("head_exchange", ev0)
            r_mean = self._colsum
        if self.keep_debug:      # test hooks: inputs of the projection (it is ill-conditioned, tests re-evaluate it in fp64)
            self.last[f"head_grad_{name}_raw"] = self.head.weight_grad.clone()
            self.last[f"Pl_before_{name}"] = self.gs_plugin.Pl.clone()
            self.last[f"r_mean_{name}"] = None if r_mean is None else r_mean.clone()
        if fires:
            self.gs_plugin.before_update(self.head, feat, batch_step, len_dataloader, self.gs_plugin.exp_count,
                                         r_mean=r_mean, grad=self.head.weight_grad)           # :437-438
        if self.keep_debug:
            self.last[f"head_grad_{name}"] = self.head.weight_grad.clone()
        opt = self.optimizer
        opt.mark_ready("head")
        opt.step_group("head")                                                                # optimizer.step(): head
        self.gs_plugin.exp_count += 1                                                         # :442
        return works

    def _ev_begin(self):
        if self.dist_events is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()                                   # on the current stream = the stream the bracketed work is enqueued on
        return e

    def _ev_end(self, kind: str, start) -> None:
        if start is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.dist_events.setdefault(kind, []).append((start, e))

    def dist_event_ms(self) -> dict:
        """kind -> (count, mean ms) of the recorded brackets (call after a device synchronize); clears them."""
        out = {}
        for kind, pairs in (self.dist_events or {}).items():
            ts = [s.elapsed_time(e) for s, e in pairs]
            out[kind] = (len(ts), sum(ts) / max(len(ts), 1))
        if self.dist_events is not None:
            self.dist_events = {}
        return out

    def train_step(self, *batch, present=None):
        """AVClassifier:     train_step(spec, image, label, batch_step, len_dataloader)
        M3AEClassifier:   train_step(token, padding_mask, image, label, batch_step, len_dataloader)
        Modal3Classifier: train_step(token, padding_mask, image, spec, label, batch_step, len_dataloader, present=None)
        spec (B,H,W) or (B,1,H,W); image (B,3,T,H,W) / (B,3,256,256); label int64 (B,).  Returns device scalars
        {'loss','loss_a','loss_v'[,'loss_t']} (no host sync; call .item() when needed, main.py:472-476).
        present (Modal3Classifier only): host bool / uint8 (B, 3), columns (audio, image, text) -- Modal3Batcher.present(step): each
        encoder runs forward and backward on the rows that have its modality plus one zero row; the head, the loss, the projection
        and the optimiser see all B features, as without it."""
        *inputs, label, batch_step, len_dataloader = batch
        options = {} if present is None else {"present": present}
        m, opt = self.model, self.optimizer
        if not getattr(m, "training", True):
            m.train()                                                                         # main.py:135 model.train()
        B = label.shape[0]
        inv_batch = 1.0 / (B * self.comm.world)
        opt.zero_grad()                                                                       # main.py:164
        feats, fwd_done = self._forwards(inputs, **options)                                   # main.py:424-431 (joint forward, Q7)
        if self.feature_only:                                                                 # main.py:428-429, 432-454: head phases only
            for (tag, _g, _e), feat in zip(self.encoders, feats):
                self.last[tag] = feat
                if self._fused_ok():
                    self._fused_phase(tag, feat, label, inv_batch, batch_step, len_dataloader)
                else:
                    self._phase(tag, None, feat, label, inv_batch, batch_step, len_dataloader, None)
            feats = ()
        for k, ((tag, grp, enc), feat) in enumerate(zip(self.encoders, feats)):
            bs = self._estreams[k] if self.overlap_forward else None
            if bs is not None:
                torch.cuda.current_stream().wait_event(fwd_done[k])                           # this encoder's features have landed
            self.last[tag] = feat
            works = self._phase(tag, enc, feat, label, inv_batch, batch_step, len_dataloader, bs)
            opt.mark_ready(grp)
            with self._on(bs):
                ev0 = self._ev_begin() if works else None
                self.comm.wait(works)                                                         # encoder gradients reduced (data parallel)
                self._ev_end("grad_wait", ev0)
                opt.step_group(grp)                                                           # optimizer.step(): this encoder
            if opt.legacy_zero_grad:              # torch 1.8.1: earlier encoders hold zero (not None) grads in later steps (Q6)
                for j in range(k):
                    g2 = self.encoders[j][1]
                    opt.grad_state[g2] = "zero"
                    with self._on(self._estreams[j] if self.overlap_forward else None):
                        opt.step_group(g2)
        opt.drop_grads()                                                                      # main.py:468-470
        t0, t1 = self.encoders[0][0], self.encoders[1][0]
        torch.add(self.losses["loss_" + t0] * self.av_alpha, self.losses["loss_" + t1], alpha=1 - self.av_alpha,
                  out=self.losses["loss"])                                                    # main.py:472 (Q8)
        return self.losses
