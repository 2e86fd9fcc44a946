"""The QMF joint baseline (--modulation QMF): per-modality heads, the History ranking loss, fused driver and evaluator.

    optimizer.zero_grad()                                                     main.py:164
    out_a, out_v[, out_t] = model(...)           audio_fc / visual_fc / txtual_fc   :172, 205, 240; basic_model.py:67-71
    conf_m = log sum exp out_m / 10;  out = sum_m out_m * conf_m.detach()     :173-183, 206-213, 242-249
    clf = sum_m CE(out_m);  history_m.correctness_update(idx, CE_i(out_m), conf_m)   :185-196, 215-223, 251-259
    crl = sum_m rank_loss(conf_m, idx, history_m)                             :198-202, 225-228, 261-264; :108-125
    loss = CE(out) + clf + 0.1 crl  (AVClassifier)  |  clf + crl  (M3AE / Modal3)     :265-268 | :203, 229
    loss.backward(); optimizer.step()                                         :310, 412

`args.modulation == "QMF"` keeps raising in the classifiers' constructors and in JointTrainer; QMF comes in through this module:
build the model with gs_flag false and modulation "Normal", then `QMFTrainer(model, n_data)` (or `attach_qmf_heads(model)` for the
protocol path: `model(...)` then returns the per-modality logits).  `fusion_module.fc_out` exists, as in the reference, and is never
used: it receives no gradient and SGD leaves it untouched.

Orchestration only: every arithmetic step is a libmla_hip.so kernel (csrc/qmf_head.hip).
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import ops
from ._lib import MLAHipError
from .dist import Comm
from .evaluators import QMFEvaluator  # noqa: F401  (its old home)
from .model import SharedHead
from .module import is_attached_fusion
from .trainer import StreamTrainer

HEAD_NAMES = ("audio_fc", "visual_fc", "txtual_fc")          # basic_model.py:45-47, 175-177, 244-247


def attach_qmf_heads(model, seed: Optional[int] = None) -> List[SharedHead]:
    """Give `model` (built with gs_flag false) the reference's per-modality heads nn.Linear(D, C) under its names and in its
    registration order (after the encoders), one per encoder in `mla_encoders()` order.  From then on `model(...)` returns
    (audio_fc(a), visual_fc(v)[, txtual_fc(t)]) and state_dict() carries their keys.  Returns the heads; attaching twice is a no-op."""
    if model.qmf_heads is not None:
        return model.qmf_heads
    if getattr(model, "gs_flag", False):
        raise MLAHipError("QMF needs a classifier built with gs_flag false")
    if is_attached_fusion(model.fusion_module):
        raise MLAHipError("QMF heads cannot be attached to a model with an attached sum / film / gated fusion (mla_hip.fusion)")
    C = model.fusion_module.fc_out.out_features
    heads = []
    for k in range(len(model.mla_encoders())):
        head = SharedHead(model.feat_dim, C, model.device, None if seed is None else seed + k)
        model.add_module(HEAD_NAMES[k], head)
        heads.append(head)
    model.qmf_heads = heads
    return heads


class QMFHistory:
    """utils/utils.py:44-95 for every modality: `correctness` / `confidence` (M, n_data) fp64 on the device, zero-initialised.
    Plain tensors: save and restore them with torch.save / copy_."""

    def __init__(self, n_data: int, M: int, device="cuda"):
        if n_data <= 0:
            raise MLAHipError(f"QMFHistory: n_data must be positive, got {n_data}")
        self.n_data, self.M = int(n_data), int(M)
        self.correctness = torch.zeros((M, n_data), device=device, dtype=torch.float64)
        self.confidence = torch.zeros((M, n_data), device=device, dtype=torch.float64)

    def reset(self) -> None:
        self.correctness.zero_()
        self.confidence.zero_()


def _weights(heads):
    return [h.weight.detach() for h in heads], [h.bias.detach() for h in heads]


class QMFTrainer(StreamTrainer):
    def __init__(self, model, n_data: int, lr: float = 1e-3, momentum: float = 0.9, weight_decay: float = 1e-4,
                 comm: Optional[Comm] = None, seed: Optional[int] = None):
        """`model`: AVClassifier / M3AEClassifier / Modal3Classifier built with gs_flag false; the heads are attached if absent.
        `n_data`: length of the training set (the History is indexed by dataset position, dataset.py:161, 480)."""
        if comm is not None and comm.world > 1:
            raise NotImplementedError("QMFTrainer is single-process: the History is indexed by dataset position and the ranking "
                                      "loss pairs neighbours of the gathered batch; data parallel QMF is not implemented")
        self.heads = attach_qmf_heads(model, seed)
        super().__init__(model, lr, momentum, weight_decay, False, comm,
                         extra_groups={name: h for name, h in zip(HEAD_NAMES, self.heads)})
        self.M = len(self.encoders)
        self.history = QMFHistory(n_data, self.M, model.device)
        # (w_cml, w_crl): main.py:265-268 (AVClassifier) | :203, 229 (--lorb m3ae)
        self.w_cml, self.w_crl = (1.0, 0.1) if type(model).__name__ == "AVClassifier" else (0.0, 1.0)
        self._bufs: dict = {}

    def _buffers(self, B: int) -> dict:
        if B not in self._bufs:
            f32 = dict(device=self.model.device, dtype=torch.float32)
            M, C, D = self.M, self.heads[0].out_features, self.heads[0].in_features
            self._bufs[B] = {"z": torch.empty((M, B, C), **f32), "out": torch.empty((B, C), **f32),
                             "losses": torch.empty(2 * M + 2, **f32), "dX": [torch.empty((B, D), **f32) for _ in range(M)],
                             "ws": torch.empty(ops.qmf_head_ws_elems(B, C, M), **f32),
                             **{k: torch.empty((M, B), **f32) for k in ("conf", "ell", "target", "margin")}}
        return self._bufs[B]

    def train_step(self, *batch):
        """AVClassifier:     train_step(spec, image, label, idx, epoch)
        M3AEClassifier:   train_step(token, padding_mask, image, label, idx, epoch)
        Modal3Classifier: train_step(token, padding_mask, image, spec, label, idx, epoch)
        idx: int64 dataset positions, (B,) or (B, 1).  Returns device scalars {'loss', 'loss_a', 'loss_v'[, 'loss_t']} (no host
        sync).  `self.last`: features, `out`, `out_m` (M, B, C), `conf` (M, B), `rank` (M), `target` (M, B), `margin`, `ell`."""
        *inputs, label, idx, _epoch = batch
        m, opt = self.model, self.optimizer
        if not getattr(m, "training", True):
            m.train()
        B = label.shape[0]
        idx = idx.reshape(-1).contiguous()
        opt.zero_grad()                                                                   # main.py:164
        main = torch.cuda.current_stream() if self.overlap_forward else None
        # 1. forwards, one stream per encoder; the QMF head needs them all
        feats, done = self._forwards(inputs)
        for ev in done or ():
            main.wait_event(ev)
        for (tag, _g, _e), f in zip(self.encoders, feats):
            self.last[tag] = f
        # 2. the QMF head: logits, confidences, History update, ranking loss, every head / feature gradient
        buf = self._buffers(B)
        Ws, bs = _weights(self.heads)
        hist = self.history
        ops.qmf_head_fwd_bwd(list(feats), Ws, bs, label, idx, hist.correctness, hist.confidence, buf["z"], buf["out"], buf["conf"],
                             buf["ell"], buf["target"], buf["margin"], buf["losses"], [h.weight_grad for h in self.heads],
                             [h.bias_grad for h in self.heads], buf["dX"], buf["ws"], self.w_cml, self.w_crl, 1.0 / B)
        L, M = buf["losses"], self.M
        self.last.update(out=buf["out"], out_m=buf["z"], conf=buf["conf"], rank=L[1 + M:1 + 2 * M], target=buf["target"],
                         margin=buf["margin"], ell=buf["ell"])
        self.losses["loss"].copy_(L[:1])
        for k, (tag, _g, _e) in enumerate(self.encoders):
            self.losses["loss_" + tag].copy_(L[1 + k:2 + k])                              # main.py:306-309
        # 3. encoder chains on their own streams: backward (loss.backward()) -> SGD (main.py:412)
        for k, (_tag, grp, enc) in enumerate(self.encoders):
            es = self._estreams[k] if self.overlap_forward else None
            if es is not None:
                es.wait_stream(main)                                                      # dX_m is ready
            with self._on(es):
                enc.backward_from_pooled(buf["dX"][k], enc._pa)
                opt.mark_ready(grp)
                opt.step_group(grp)
        # 4. the heads' SGD steps; "head" (fusion_module.fc_out) has no gradient and is skipped, as torch.optim.SGD skips it
        for name in HEAD_NAMES[:M]:
            opt.mark_ready(name)
            opt.step_group(name)
        opt.drop_grads()
        return self.losses
