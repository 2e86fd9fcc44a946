"""CLIPClassifier (models/basic_model.py:278-319): the `--clip` model of the reference, a classifier on stored CLIP features.

There is no encoder: `forward(token, visual)` squeezes two (B, 1, D) feature tensors (dataset/dataset.py:864-872 stores one
(1, 512) array per sample and modality) and hands them to `fusion_module`.  The only parameters are
`fusion_module.fc_out.weight` / `.bias`.  Under --gs_flag the training step (main.py:428-454) is two head phases and nothing
else -- `MLATrainer` runs each as one `mla_feature_phase` call (csrc/feature_step.hip; `mla_feature_phase_owm` under gs_mode="owm"); with gs_flag false the model goes
through `JointTrainer` / `JointEvaluator` on the concatenated-head kernels like the other classifiers.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import MLAHipError
from .model import ConcatFusion, _Classifier


class CLIPClassifier(_Classifier):
    """`CLIPClassifier(args)` of the reference.  args: dataset Food101 (default, 101 classes) | MVSA (3) | CREMAD (6);
    fusion_method concat; gs_flag (Linear(D, C) shared by both modalities) or not (Linear(2 D, C) on cat(token, visual));
    `feat_dim` (default 512, basic_model.py:300-302; 768 for ViT-L features).  `modulation == "QMF"` raises: the reference's
    CLIPClassifier has no audio_fc / visual_fc heads."""
    feature_only = True
    side_streams = False

    def __init__(self, args, device="cuda", seed: Optional[int] = None, feat_dim: Optional[int] = None):
        if getattr(args, "modulation", "Normal") == "QMF":
            raise NotImplementedError("CLIPClassifier has no per-modality heads (basic_model.py:278-319): --modulation QMF is not "
                                      "implemented for --clip")
        D = int(feat_dim if feat_dim is not None else getattr(args, "feat_dim", 512))
        if D <= 0:
            raise MLAHipError(f"CLIPClassifier: feat_dim must be positive, got {D}")
        super().__init__(args, device, seed, ("Food101", "MVSA", "CREMAD"), ConcatFusion, D, 2)     # basic_model.py:282-308

    def mla_encoders(self):
        """(phase tag, optimiser group name, encoder) in alternation order; the tags are the reference's loss names
        (loss_a = the token phase, loss_v = the image phase, main.py:432-454).  No encoder stands behind a stored feature."""
        return [("a", "token", None), ("v", "visual", None)]

    def _check(self, x: torch.Tensor, what: str) -> torch.Tensor:
        ok = (torch.is_tensor(x) and x.dtype == torch.float32 and x.device.type == self.device.type
              and ((x.dim() == 3 and x.shape[1] == 1) or x.dim() == 2) and x.shape[-1] == self.feat_dim and x.shape[0] > 0)
        if not ok:   # the reference casts nothing (main.py:429): anything but fp32 features on the model's device is refused
            desc = f"{tuple(x.shape)} {x.dtype} on {x.device}" if torch.is_tensor(x) else type(x).__name__
            raise MLAHipError(f"CLIPClassifier: {what} features must be float32 (B, 1, {self.feat_dim}) on {self.device.type}, got {desc}")
        x = x.detach() if not (torch.is_grad_enabled() and x.requires_grad) else x
        return x.squeeze(1).contiguous() if x.dim() == 3 else x.contiguous()               # basic_model.py:314-315

    def _calls(self, token: torch.Tensor, visual: torch.Tensor):
        a, v = self._check(token, "token"), self._check(visual, "visual")
        if a.shape[0] != v.shape[0]:
            raise MLAHipError(f"CLIPClassifier: token / visual batch mismatch ({a.shape[0]} vs {v.shape[0]})")

        def give(x):
            def run(out=None):
                return x if out is None else out.copy_(x)
            return run
        return a.shape[0], [give(a), give(v)]

    def forward(self, token: torch.Tensor, visual: torch.Tensor):
        """basic_model.py:313-319: (token, visual) under gs_flag, else (a, v, out) = fusion_module(token, visual)."""
        a, v = self.forward_raw(token, visual)
        return (a, v) if self.gs_flag else self.fusion_module(a, v)
