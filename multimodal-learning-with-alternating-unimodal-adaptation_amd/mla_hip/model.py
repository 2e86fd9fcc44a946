"""Drop-in model objects for the --gs_flag path of the reference and for the joint concat-fusion step it is measured
against (gs_flag false, main.py:164-168, 232-237, 273-417).

  AVClassifier   models/basic_model.py:14-77   (attribute paths audio_net / visual_net / fusion_module.fc_out)
  ConcatFusion   models/fusion_modules.py:16-24 (--gs_flag: only fc_out is used, main.py:432, 444; joint: forward(x, y)
                 returns (x, y, fc_out(cat(x, y))) on the concatenated-head kernels)
  SharedHead     the nn.Linear(D, C) (joint: nn.Linear(M*D, C)) behind fc_out

state_dict()/load_state_dict() speak the reference's keys and layouts (OIHW conv weights,
`audio_net.conv1.weight`, `fusion_module.fc_out.weight`, optional `module.` prefix,
main.py:724-727, 921); internally everything is flat HWIO buffers (see encoder.py).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from .streams import distinct_streams
import torch.nn as nn

from . import ops
from ._lib import MLAHipError
from .autograd import ConcatHeadLinear, EncoderFeature, HeadLinear, make_anchor
from .encoder import ResNet18Encoder
from .module import FlatModule

N_CLASSES = {"CREMAD": 6, "MVSA": 3, "Food101": 101, "IEMOCAP": 4}   # main.py:491-507


class SharedHead(FlatModule, nn.Linear):
    """fc_out = nn.Linear(in_features, out_features): weight (C,D) and bias (C) in one flat buffer.

    Protocol face: `fc_out(x)` is a differentiable Linear on the HIP kernels (autograd.HeadLinear), `.weight` / `.bias`
    are nn.Parameters viewing the flat buffer, after `loss.backward()` `.weight.grad` / `.bias.grad` alias the flat
    gradient buffer, `named_parameters()` yields 'weight', 'bias' (what utils/utils.py:30 iterates)."""

    def __init__(self, in_features: int, out_features: int, device="cuda", seed: Optional[int] = None):
        FlatModule.__init__(self)
        self.in_features, self.out_features = in_features, out_features
        self.device = torch.device(device)
        self._alloc_flat([("weight", (out_features, in_features)), ("bias", (out_features,))])
        self.weight_grad, self.bias_grad = self.g["weight"], self.g["bias"]
        self.weight = self._param_view(self.p["weight"], self.weight_grad, lambda t: t, "weight")
        self.bias = self._param_view(self.p["bias"], self.bias_grad, lambda t: t, "bias")
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed) if seed is not None else gen.seed()
        std = math.sqrt(2.0 / (in_features + out_features))           # xavier_normal_, utils/utils.py:107-109
        with torch.no_grad():
            self.weight.copy_(torch.randn((out_features, in_features), generator=gen) * std)
        self._ws: dict = {}
        self._anchor = make_anchor(self.device)

    def _bufs(self, B: int, slot: str = "") -> dict:
        if (B, slot) not in self._ws:
            f32 = dict(device=self.device, dtype=torch.float32)
            self._ws[(B, slot)] = {"logits": torch.empty((B, self.out_features), **f32), "loss": torch.empty(1, **f32),
                           "dX": torch.empty((B, self.in_features), **f32),
                           "ws": torch.empty(ops.head_ws_elems(B, self.out_features), **f32)}
        return self._ws[(B, slot)]

    def forward_backward(self, X: torch.Tensor, labels: torch.Tensor, inv_batch: Optional[float] = None, slot: str = ""):
        """Fused trainer path: logits, CE loss and all gradients (main.py:432-435).  Gradients land in
        self.weight_grad / self.bias_grad; returns (logits, loss[1], dX).  inv_batch = 1/global batch."""
        B = X.shape[0]
        buf = self._bufs(B, slot)
        ops.head_ce_fwd_bwd(X, self.weight.detach(), self.bias.detach(), labels, buf["logits"], buf["loss"], self.weight_grad,
                            self.bias_grad, buf["dX"], buf["ws"], (1.0 / B) if inv_batch is None else inv_batch)
        return buf["logits"], buf["loss"], buf["dX"]

    def logits(self, X: torch.Tensor, slot: str = "eval") -> torch.Tensor:
        """out = fc_out(x) without loss/gradients into a reused buffer (Evaluator, main.py:636-639)."""
        buf = self._bufs(X.shape[0], slot)
        ops.head_logits(X, self.weight.detach(), self.bias.detach(), buf["logits"])
        return buf["logits"]

    def _joint_bufs(self, B: int, M: int, slot: str) -> dict:
        key = (B, "joint", M, slot)
        if key not in self._ws:
            f32 = dict(device=self.device, dtype=torch.float32)
            D = self.in_features // M
            self._ws[key] = {"out": torch.empty((B, self.out_features), **f32),
                             "out_m": torch.empty((M, B, self.out_features), **f32),
                             "loss": torch.empty(1 + M, **f32),
                             "dX": [torch.empty((B, D), **f32) for _ in range(M)],
                             "ws": torch.empty(ops.concat_head_ws_elems(B, self.out_features, M), **f32)}
        return self._ws[key]

    def concat_forward_backward(self, xs, labels: torch.Tensor, inv_batch: Optional[float] = None, slot: str = ""):
        """Fused joint-step head (main.py:273-310): out = fc_out(cat(xs)), out_m (the half / third-head logits), the CE
        loss and the reported per-modality losses, and every gradient, in two launches.  Gradients land in
        self.weight_grad / self.bias_grad; returns (out, out_m (M, B, C), losses [loss, loss_m...], [dX_m])."""
        B, M = xs[0].shape[0], len(xs)
        buf = self._joint_bufs(B, M, slot)
        L = buf["loss"]
        ops.concat_head_ce_fwd_bwd(xs, self.weight.detach(), self.bias.detach(), labels, buf["out"], buf["out_m"], L[:1], L[1:],
                                   self.weight_grad, self.bias_grad, buf["dX"], buf["ws"],
                                   (1.0 / B) if inv_batch is None else inv_batch)
        return buf["out"], buf["out_m"], L, buf["dX"]

    def concat_logits(self, xs, slot: str = "eval"):
        """(out, out_m) of the concatenated head into reused buffers, no gradients (JointEvaluator, main.py:539-619)."""
        buf = self._joint_bufs(xs[0].shape[0], len(xs), slot)
        ops.concat_head_fwd(xs, self.weight.detach(), self.bias.detach(), buf["out"], buf["out_m"])
        return buf["out"], buf["out_m"]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """out = fc_out(x)  (main.py:432, 444, 456, 636-639): differentiable when x carries history."""
        if x.dim() != 2 or x.shape[1] != self.in_features:
            raise MLAHipError(f"fc_out expects (B, {self.in_features}), got {tuple(x.shape)}")
        return HeadLinear.apply(self._anchor, self, x)


def concat_fusion_forward(fusion, xs):
    """`output = fc_out(torch.cat(xs, dim=1))` (fusion_modules.py:22-23, 32-34) on the concatenated-head kernels; returns
    (*xs, output).  Differentiable when the features carry history (ConcatHeadLinear)."""
    if not fusion.joint:
        raise NotImplementedError("this fusion module was built for the --gs_flag (MLA) path, where fc_out is applied per "
                                  "modality; construct it with joint=True (gs_flag false) for the concatenated head")
    head = fusion.fc_out
    if len({tuple(x.shape) for x in xs}) != 1 or xs[0].dim() != 2 or xs[0].shape[1] * len(xs) != head.in_features:
        raise MLAHipError(f"{type(fusion).__name__}: expects {len(xs)} x (B, {head.in_features // len(xs)}), "
                          f"got {[tuple(x.shape) for x in xs]}")
    if any(x.requires_grad for x in xs) and torch.is_grad_enabled():
        out = ConcatHeadLinear.apply(head._anchor, head, *xs)
    else:
        out = torch.empty((xs[0].shape[0], head.out_features), device=head.device, dtype=torch.float32)
        out_m = torch.empty((len(xs), xs[0].shape[0], head.out_features), device=head.device, dtype=torch.float32)
        ops.concat_head_fwd([x.detach().contiguous() for x in xs], head.weight.detach(), head.bias.detach(), out, out_m)
    return tuple(xs) + (out,)


class ConcatFusion(nn.Module):
    """models/fusion_modules.py:16-24.  Under --gs_flag (joint=False) only `fc_out` is touched and forward raises; the joint
    step (gs_flag false, joint=True) calls forward(x, y) -> (x, y, fc_out(cat(x, y)))."""

    def __init__(self, input_dim: int = 512, output_dim: int = 100, device="cuda", seed: Optional[int] = None,
                 joint: bool = False):
        super().__init__()
        self.joint = bool(joint)
        self.fc_out = SharedHead(input_dim, output_dim, device, seed)

    def forward(self, x, y):
        return concat_fusion_forward(self, (x, y))


def check_joint_args(args, large_ok: bool = False, clip_ok: bool = False) -> None:
    """What the joint (gs_flag false) classifiers support through `args`: `--modulation Normal | OGM | OGM_GE` with concat fusion.
    `--modulation QMF` (main.py:170-268) lives in `mla_hip.qmf`: build the model with gs_flag false and modulation "Normal", then
    `attach_qmf_heads(model)` / `QMFTrainer(model, n_data)` add the per-modality audio_fc / visual_fc / txtual_fc heads and the
    History ranking loss.  `args.modulation == "QMF"` itself still raises here."""
    mod = getattr(args, "modulation", "Normal")
    if mod == "QMF":
        raise NotImplementedError("mla_hip does not implement --modulation QMF (main.py:170-268): it needs the per-modality "
                                  "audio_fc / visual_fc heads and the History ranking loss")
    if mod not in ("Normal", "OGM", "OGM_GE"):
        raise NotImplementedError(f"Incorrect modulation: {mod}")
    if getattr(args, "lorb", "base") == "large" and not large_ok:
        raise NotImplementedError("mla_hip does not implement --lorb large")
    if getattr(args, "clip", False) and not clip_ok:
        raise NotImplementedError("--clip (stored CLIP features) is mla_hip.CLIPClassifier; this classifier has encoders and does not "
                                  "take args.clip")


class _Classifier(nn.Module):
    """Shared protocol behaviour of AVClassifier / M3AEClassifier / Modal3Classifier.  A subclass builds its encoders and
    states ONCE how its inputs reach them: `_calls(*inputs) -> (batch, [run(out=None) -> (B, D) feature])`, one callable per
    encoder in `mla_encoders()` order; the kernel-level and the autograd forwards below are derived from that list."""
    side_streams = True
    lorb_large = False          # True on the `--lorb large` family (CAVClassifier)
    feature_only = False        # True on CLIPClassifier: stored features, no encoder behind them (mla_encoders() carries None)
    qmf_heads = None            # mla_hip.qmf.attach_qmf_heads: the per-modality heads, in mla_encoders() order

    def __init__(self, args, device, seed: Optional[int], datasets, fusion_cls, feat_dim: int, n_enc: int):
        """datasets: the names the reference's constructor accepts, its default first.  Builds the fusion module (the
        head draws its seed after the encoders': seed + n_enc); the subclass then builds encoder k with `_seed(k)`."""
        super().__init__()
        fusion = getattr(args, "fusion_method", "concat")
        dataset = getattr(args, "dataset", datasets[0])
        if dataset not in datasets:
            raise NotImplementedError("Incorrect dataset name {}".format(dataset))
        if fusion != "concat":
            raise NotImplementedError("Incorrect fusion method: {}!".format(fusion))
        self.gs_flag = bool(getattr(args, "gs_flag", False))
        if not self.gs_flag:
            check_joint_args(args, self.lorb_large, self.feature_only)
        self.args, self.device, self.feat_dim, self._seed0 = args, torch.device(device), feat_dim, seed
        self.fusion_module = fusion_cls(feat_dim if self.gs_flag else n_enc * feat_dim, N_CLASSES[dataset], device,
                                        self._seed(n_enc), joint=not self.gs_flag)

    def _seed(self, k: int) -> Optional[int]:
        return None if self._seed0 is None else self._seed0 + k

    @property
    def module(self):
        """`model.module.fusion_module.fc_out` (main.py:432) also works on the bare model (no DataParallel wrapper)."""
        return self

    def _side_stream(self) -> torch.cuda.Stream:
        """One weight-gradient side stream for all encoders of this model on the protocol path, on a hardware queue of its own
        (streams.py): the encoders' backwards run one after the other there, so one stream serves them all."""
        if getattr(self, "_wgrad_side", None) is None:
            self._wgrad_side = distinct_streams(1, self.device)[0]
        return self._wgrad_side

    def _feature(self, enc, run, B: int) -> torch.Tensor:
        if torch.is_grad_enabled() and self.training:
            if not hasattr(enc, "_anchor"):
                enc._anchor = make_anchor(self.device)
                # protocol path: the weight-gradient GEMMs of a backward run on a side stream beside the dgrad -> BN-backward
                # chain (joined before the gradients are published), like in MLATrainer's pipeline
                if self.side_streams and enc.side_wgrad and enc.wgrad_stream is None and self.device.type == "cuda":
                    enc.wgrad_stream = self._side_stream()
            return EncoderFeature.apply(enc._anchor, enc, run, B, self.feat_dim)
        out = torch.empty((B, self.feat_dim), device=self.device, dtype=torch.float32)
        run(out)
        return out

    def forward_split(self, *inputs, **options):
        """Per-encoder forward closures in alternation order, so the trainer may run each encoder's forward on a stream of
        its own: no encoder forward depends on the head or on another encoder.  `options`: what the subclass's
        `_calls` takes by keyword beside its inputs (Modal3Classifier: present=)."""
        return self._calls(*inputs, **options)[1]

    def forward_raw(self, *inputs, **options):
        """Kernel-level joint forward into the reused feature buffers (trainers / evaluators; no autograd)."""
        return tuple(run() for run in self._calls(*inputs, **options)[1])

    def forward(self, *inputs, **options):
        """The features as fresh (B, D) tensors that carry autograd history to their encoder when grad mode is on and the
        model is training."""
        B, runs = self._calls(*inputs, **options)
        feats = tuple(self._feature(enc, run, B) for (_t, _g, enc), run in zip(self.mla_encoders(), runs))
        if self.qmf_heads is not None:      # QMF: (audio_fc(a), visual_fc(v)[, txtual_fc(t)]), basic_model.py:67-71, 196-200, 269-273
            return tuple(head(f) for head, f in zip(self.qmf_heads, feats))
        return feats

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts DataParallel-style `module.`-prefixed keys as well (main.py:724 strips them by hand)."""
        if any(k.startswith("module.") for k in state_dict):
            state_dict = {k[len("module."):] if k.startswith("module.") else k: v for k, v in state_dict.items()}
        return super().load_state_dict(state_dict, strict=strict, **kw)


class AVClassifier(_Classifier):
    """Two ResNet-18 encoders + ConcatFusion (models/basic_model.py:14-77): Linear(512, C) shared by both modalities
    (--gs_flag) or Linear(1024, C) on cat(a, v) (:31-34)."""

    def __init__(self, args, device="cuda", seed: Optional[int] = None, conv_math: Optional[str] = None):
        """conv_math: "f32" (exact fp32 MFMA), "split" (exact bf16 operand split, fp32-equivalent) or "bf16" (operands
        rounded once to bf16, one product: reduced precision, opt-in); see encoder.py; default from $MLA_CONV_MATH."""
        super().__init__(args, device, seed, ("CREMAD",), ConcatFusion, 512, 2)     # basic_model.py:19-40
        self.audio_net = ResNet18Encoder("audio", device, self._seed(0), conv_math)     # basic_model.py:42
        self.visual_net = ResNet18Encoder("visual", device, self._seed(1), conv_math)   # basic_model.py:43
        self._feat: Dict[int, dict] = {}

    def mla_encoders(self):
        """(phase tag, optimiser group name, encoder) in the order main.py:432-454 alternates over them."""
        return [("a", "audio", self.audio_net), ("v", "visual", self.visual_net)]

    def _feat_buffers(self, B: int) -> dict:
        if B not in self._feat:
            f32 = dict(device=self.device, dtype=torch.float32)
            self._feat[B] = {"a": torch.empty((B, 512), **f32), "v": torch.empty((B, 512), **f32)}
        return self._feat[B]

    def _pooled(self, tag: str, enc, x: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
        """Encoder forward + global average pool: adaptive_avg_pool2d + flatten for audio (basic_model.py:61, 64), regroup T +
        adaptive_avg_pool3d + flatten for visual (:56-65)."""
        B = x.shape[0]
        f = enc.forward(x)
        if out is None:
            out = self._feat_buffers(B)[tag]
        n, h, w, c = f.shape
        enc._pa = (n // B) * h * w                                           # pooled pixels per sample (for the backward)
        ops.avgpool_fwd(f, out, B, enc._pa, c)
        return out

    def _calls(self, spec: torch.Tensor, image: torch.Tensor):
        """a, v = model(spec.unsqueeze(1).float(), image.float())  (main.py:431; basic_model.py:52-77); the trainers and
        evaluators hand the spectrogram over as the loader yields it, (B, H, W)."""
        if spec.dim() == 3:
            spec = spec.unsqueeze(1)
        audio, visual = spec.float(), image.float()
        if visual.shape[0] != audio.shape[0]:
            raise MLAHipError("audio/visual batch mismatch")
        return audio.shape[0], [lambda out=None: self._pooled("a", self.audio_net, audio, out),
                                lambda out=None: self._pooled("v", self.visual_net, visual, out)]

    def forward(self, audio: torch.Tensor, visual: torch.Tensor):
        """gs_flag false: a, v, out = model(...) (main.py:273; basic_model.py:72-74)."""
        a, v = super().forward(audio, visual)
        return (a, v) if self.gs_flag or self.qmf_heads is not None else self.fusion_module(a, v)
