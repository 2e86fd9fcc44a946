"""--fusion_method sum | film | gated (main.py:24) for the joint step: the reference's SumFusion, FiLM and GatedFusion
(models/fusion_modules.py:5-13, 38-67, 70-98) as attachable heads on the HIP kernels of csrc/fusion_head.hip.

`args.fusion_method != "concat"` keeps raising in the classifiers' constructors; the three methods come in the way QMF does: build the
model with fusion_method "concat", gs_flag false and modulation "Normal", then

    fusion = attach_fusion(model, "film")                 # replaces model.fusion_module
    trainer = JointTrainer(model)                          # or the protocol path: a, v, out = model(...); loss.backward(); opt.step()

What is reproduced: the modules' arithmetic, parameter names and layouts, and for `sum` the per-modality logits out_a / out_v of the
joint loop with the reference's bias quirk (the full bias in training, main.py:292-295; half of it in valid(), main.py:610-614).
What is refused: OGM / OGM-GE on film / gated (the reference defines no per-modality logits for them), three modalities (the modules
take two inputs), gs_flag models, models with QMF heads, data parallel.

Every parameter of the attached module is an nn.Parameter view of ONE flat buffer (module.py), so FusedSGD updates the head in one launch.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from ._lib import MLAHipError
from .autograd import FiLMHead, GatedFusionHead, SumFusionHead, make_anchor
from .module import FlatModule, _bare_init

METHODS = ("sum", "film", "gated")


class LinearHolder(nn.Linear):
    """`isinstance(m, nn.Linear)` leaf of an attached fusion module: weight (out, in) and bias are views of the module's flat buffer."""

    def __init__(self, weight: nn.Parameter, bias: nn.Parameter):
        _bare_init(self)
        self.out_features, self.in_features = weight.shape
        self.weight, self.bias = weight, bias

    def forward(self, *a, **k):
        raise MLAHipError("the Linear layers of an attached fusion run inside the fusion kernels; call the fusion module")


class AttachedFusion(FlatModule):
    """What SumFusion / FiLM / GatedFusion share: the flat owner of every Linear of the module (reference names and order), the
    xavier_normal_ / zero-bias initialisation of `weight_init` (utils/utils.py:106-109), the reused buffers of the fused driver."""
    joint = True                     # a joint-step fusion module (JointTrainer / JointEvaluator)
    attached_fusion = True           # module.is_attached_fusion
    method = ""
    per_modality = False             # True: the joint loop defines out_a / out_v for it (sum)

    def __init__(self, linears: List[Tuple[str, int, int]], D: int, C: int, device, seed: Optional[int]):
        super().__init__()
        if D <= 0 or D % 64 != 0:
            raise MLAHipError(f"{type(self).__name__}: the feature dimension must be a positive multiple of 64, got {D}")
        self.in_features, self.out_features = D, C
        self.device = torch.device(device)
        self._alloc_flat([(f"{name}.{part}", shp) for name, out_f, in_f in linears
                          for part, shp in (("weight", (out_f, in_f)), ("bias", (out_f,)))])
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed) if seed is not None else gen.seed()
        for name, out_f, in_f in linears:
            wn, bn = f"{name}.weight", f"{name}.bias"
            weight = self._param_view(self.p[wn], self.g[wn], lambda t: t, wn)
            bias = self._param_view(self.p[bn], self.g[bn], lambda t: t, bn)
            with torch.no_grad():
                weight.copy_(torch.randn((out_f, in_f), generator=gen) * math.sqrt(2.0 / (in_f + out_f)))
            self.add_module(name, LinearHolder(weight, bias))
        self._ws: dict = {}
        self._anchor = make_anchor(self.device)

    def _f32(self, *shape) -> torch.Tensor:
        return torch.empty(shape, device=self.device, dtype=torch.float32)

    def _check(self, x, y):
        D = self.in_features
        if x.dim() != 2 or tuple(x.shape) != tuple(y.shape) or x.shape[1] != D:
            raise MLAHipError(f"{type(self).__name__}: expects 2 x (B, {D}), got {[tuple(x.shape), tuple(y.shape)]}")

    def _bufs(self, B: int, slot: str) -> dict:
        if (B, slot) not in self._ws:
            D, C = self.in_features, self.out_features
            self._ws[(B, slot)] = {"out": self._f32(B, C), "out_m": self._f32(2, B, C), "loss": self._f32(3), "h": self._f32(B, 2 * D),
                                   "z": self._f32(B, D), "dX": [self._f32(B, D), self._f32(B, D)],
                                   "ws": self._f32(ops.fusion_ws_elems(B, D, C))}
        return self._ws[(B, slot)]

    def forward(self, x, y):
        """Differentiable whenever grad mode is on, as SharedHead.forward is: the private anchor starts the recording, so the
        parameters receive their gradients also behind features without history (CLIPClassifier's stored features)."""
        self._check(x, y)
        if torch.is_grad_enabled():
            return self._outputs(x, y, self._head.apply(self._anchor, self, x, y))
        return self._outputs(x, y, self._forward_plain(x.detach().contiguous(), y.detach().contiguous()))


class SumFusion(AttachedFusion):
    """models/fusion_modules.py:5-13: fc_x, fc_y = Linear(D, C); forward(x, y) -> (x, y, fc_x(x) + fc_y(y))."""
    method, per_modality, _head = "sum", True, SumFusionHead

    def __init__(self, input_dim: int = 512, output_dim: int = 100, device="cuda", seed: Optional[int] = None):
        super().__init__([("fc_x", output_dim, input_dim), ("fc_y", output_dim, input_dim)], input_dim, output_dim, device, seed)

    def _outputs(self, x, y, out):
        return x, y, out

    def _forward_plain(self, x, y):
        return self.logits([x, y], 1.0, slot=None)[0]

    def forward_backward(self, xs, labels, inv_batch: float, last: dict, slot: str = ""):
        """Fused joint-step head (main.py:273-310) in two launches: (out, out_m (2, B, C) = [fc_x(a), fc_y(v)] with the full bias,
        losses [loss, loss_a, loss_v], [dX, dY]); the gradients land in self.grad."""
        x, y = xs
        p, g, buf = self.p, self.g, self._bufs(x.shape[0], slot)
        om = buf["out_m"]
        ops.fusion_sum_ce_fwd_bwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], labels, buf["out"], om[0], om[1],
                                  buf["loss"], g["fc_x.weight"], g["fc_x.bias"], g["fc_y.weight"], g["fc_y.bias"], buf["dX"][0], buf["dX"][1],
                                  buf["ws"], inv_batch, 1.0)
        return buf["out"], om, buf["loss"], buf["dX"]

    def logits(self, xs, bias_scale: float = 0.5, slot: Optional[str] = "eval"):
        """(out, out_m) without gradients; out_m carries `bias_scale` times the bias: 0.5 in valid() (main.py:610-614)."""
        x, y = xs
        B, C, p = x.shape[0], self.out_features, self.p
        out, om = (self._f32(B, C), self._f32(2, B, C)) if slot is None else (lambda b: (b["out"], b["out_m"]))(self._bufs(B, slot))
        ops.fusion_sum_fwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], out, om[0], om[1], bias_scale)
        return out, om


class FiLM(AttachedFusion):
    """models/fusion_modules.py:38-67: fc = Linear(D, 2 D), fc_out = Linear(D, C); gamma, beta = split(fc(film)); forward(x, y) ->
    (x, y, fc_out(gamma * to_be_film + beta)), film = x when x_film else y."""
    method, _head = "film", FiLMHead

    def __init__(self, input_dim: int = 512, dim: int = 512, output_dim: int = 100, x_film: bool = True, device="cuda",
                 seed: Optional[int] = None):
        if dim != input_dim:
            raise MLAHipError(f"FiLM: dim ({dim}) must equal input_dim ({input_dim}): gamma multiplies the other feature element-wise")
        super().__init__([("fc", 2 * dim, input_dim), ("fc_out", output_dim, dim)], input_dim, output_dim, device, seed)
        self.dim, self.x_film = input_dim, bool(x_film)

    def _outputs(self, x, y, out):
        return x, y, out

    def _forward_plain(self, x, y):
        return self.logits([x, y], slot=None)[0]

    def forward_backward(self, xs, labels, inv_batch: float, last: dict, slot: str = ""):
        """Fused joint-step head in three launches: (out, None, losses [loss], [dX, dY]); `last` receives h (gamma | beta) and z."""
        k = 0 if self.x_film else 1
        film, t = xs[k], xs[1 - k]
        p, g, buf = self.p, self.g, self._bufs(film.shape[0], slot)
        ops.fusion_film_ce_fwd_bwd(film, t, p["fc.weight"], p["fc.bias"], p["fc_out.weight"], p["fc_out.bias"], labels, buf["out"], buf["h"],
                                   buf["z"], buf["loss"][:1], g["fc.weight"], g["fc.bias"], g["fc_out.weight"], g["fc_out.bias"],
                                   buf["dX"][k], buf["dX"][1 - k], buf["ws"], inv_batch)
        last.update(h=buf["h"], z=buf["z"])
        return buf["out"], None, buf["loss"][:1], buf["dX"]

    def logits(self, xs, bias_scale: float = 0.5, slot: Optional[str] = "eval"):
        k = 0 if self.x_film else 1
        film, t = xs[k], xs[1 - k]
        B, D, C, p = film.shape[0], self.in_features, self.out_features, self.p
        out, h, z = ((self._f32(B, C), self._f32(B, 2 * D), self._f32(B, D)) if slot is None
                     else (lambda b: (b["out"], b["h"], b["z"]))(self._bufs(B, slot)))
        ops.fusion_film_fwd(film, t, p["fc.weight"], p["fc.bias"], p["fc_out.weight"], p["fc_out.bias"], out, h, z)
        return out, None


class GatedFusion(AttachedFusion):
    """models/fusion_modules.py:70-98: fc_x, fc_y = Linear(D, D), fc_out = Linear(D, C); forward(x, y) -> (fc_x(x), fc_y(y),
    fc_out(sigmoid(fc_x(x)) * fc_y(y))) under x_gate, else fc_out(fc_x(x) * sigmoid(fc_y(y))).

    Restriction against the reference: of the three results only `out` carries autograd history.  `out_x` and `out_y` are returned
    detached (GatedFusionHead marks them non-differentiable: the kernels form no gradient from them), so a loss built on `out_x` or
    `out_y` fails with torch's "does not require grad" error.  The reference's loop never differentiates them."""
    method, _head = "gated", GatedFusionHead

    def __init__(self, input_dim: int = 512, dim: int = 512, output_dim: int = 100, x_gate: bool = True, device="cuda",
                 seed: Optional[int] = None):
        if dim != input_dim:
            raise MLAHipError(f"GatedFusion: the kernels take dim == input_dim (got {dim}, {input_dim})")
        super().__init__([("fc_x", dim, input_dim), ("fc_y", dim, input_dim), ("fc_out", output_dim, dim)], input_dim, output_dim, device,
                         seed)
        self.x_gate = bool(x_gate)

    def _outputs(self, x, y, res):
        return res                                   # (out_x, out_y, out), fusion_modules.py:98

    def _forward_plain(self, x, y):
        B, D, C, p = x.shape[0], self.in_features, self.out_features, self.p
        out, hx, hy, z = self._f32(B, C), self._f32(B, D), self._f32(B, D), self._f32(B, D)
        ops.fusion_gated_fwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], p["fc_out.weight"], p["fc_out.bias"],
                             out, hx, hy, z, self.x_gate)
        return hx, hy, out

    def forward_backward(self, xs, labels, inv_batch: float, last: dict, slot: str = ""):
        """Fused joint-step head in three launches: (out, None, losses [loss], [dX, dY]); `last` receives out_x, out_y and z."""
        x, y = xs
        B, D = x.shape
        p, g, buf = self.p, self.g, self._bufs(B, slot)
        hx, hy = buf["h"].view(2, B, D)
        ops.fusion_gated_ce_fwd_bwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], p["fc_out.weight"],
                                    p["fc_out.bias"], labels, buf["out"], hx, hy, buf["z"], buf["loss"][:1], g["fc_x.weight"], g["fc_x.bias"],
                                    g["fc_y.weight"], g["fc_y.bias"], g["fc_out.weight"], g["fc_out.bias"], buf["dX"][0], buf["dX"][1],
                                    buf["ws"], self.x_gate, inv_batch)
        last.update(out_x=hx, out_y=hy, z=buf["z"])
        return buf["out"], None, buf["loss"][:1], buf["dX"]

    def logits(self, xs, bias_scale: float = 0.5, slot: Optional[str] = "eval"):
        x, y = xs
        B, D = x.shape
        p, buf = self.p, self._bufs(B, slot)
        hx, hy = buf["h"].view(2, B, D)
        ops.fusion_gated_fwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], p["fc_out.weight"], p["fc_out.bias"],
                             buf["out"], hx, hy, buf["z"], self.x_gate)
        return buf["out"], None


def attach_fusion(model, method: str, seed: Optional[int] = None, x_film: bool = True, x_gate: bool = True) -> AttachedFusion:
    """Replace `model.fusion_module` (ConcatFusion of a two-encoder classifier built with gs_flag false: AVClassifier, M3AEClassifier,
    CAVClassifier, CLIPClassifier) with the reference's SumFusion / FiLM / GatedFusion on D = model.feat_dim and the model's classes.
    `x` is the first encoder in mla_encoders() order.  `seed` keys the initialisation (None: a fresh one, like SharedHead).  From then on
    `model(...)` / `model.fusion_module(a, v)`, `state_dict()` and `parameters()` speak the new module; JointTrainer and JointEvaluator
    accept the model.  Returns the new module."""
    if method not in METHODS:
        raise MLAHipError(f"attach_fusion: method must be one of {' | '.join(METHODS)}, got {method!r}")
    old = model.fusion_module
    if isinstance(old, AttachedFusion):
        raise MLAHipError(f"attach_fusion: this model already has an attached {old.method} fusion; build a new model to attach another")
    if getattr(model, "gs_flag", False):
        raise MLAHipError("attach_fusion needs a classifier built with gs_flag false: the gs_flag (MLA) loop applies fc_out per modality")
    if len(model.mla_encoders()) != 2:
        raise MLAHipError("attach_fusion: sum / film / gated fusion take two inputs (fusion_modules.py:11, 53, 87); this model has "
                          f"{len(model.mla_encoders())} modalities")
    if model.qmf_heads is not None:
        raise MLAHipError("attach_fusion: this model has QMF heads attached (attach_qmf_heads / QMFTrainer); QMF does not use the fusion module")
    D, C, dev = model.feat_dim, old.fc_out.out_features, model.device
    if method == "sum":
        new = SumFusion(D, C, dev, seed)
    elif method == "film":
        new = FiLM(D, D, C, x_film, dev, seed)
    else:
        new = GatedFusion(D, D, C, x_gate, dev, seed)
    model.fusion_module = new
    return new
