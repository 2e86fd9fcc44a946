"""nn.Module face of the flat-buffer objects: the object protocol main.py programs against.

The reference has no FFI; what `main.py` touches is the PyTorch protocol -- `model(...)` returning tensors with
autograd history, `named_parameters()` / `parameters()` / `state_dict()` / `load_state_dict()` under the
reference's dotted names and layouts, `p.grad` mutated in place by `GSPlugin.before_update`
(utils/utils.py:30-41), `model.apply(weight_init)` (main.py:719), `optim.SGD(model.parameters(), ...)`
(main.py:749).  The HIP kernels work on ONE flat fp32 buffer per encoder (HWIO / [in][out] layouts), so the
protocol objects here are *views*:

  * every reference parameter is an `nn.Parameter` whose storage IS the flat buffer -- a strided view in the
    reference's logical layout (OIHW conv weights = HWIO permuted, nn.Linear (out,in) = [in][out] transposed);
    in-place writes through it (load_state_dict, nn.init.*) land in the flat buffer, nothing is copied;
  * after a HIP backward the parameters' `.grad` are set to the same kind of views of the flat GRADIENT buffer,
    with autograd's accumulation rule (None -> set, otherwise add);
  * leaf holders subclass nn.Conv2d / nn.BatchNorm2d / nn.Linear (without allocating their own storage) so
    `isinstance` dispatch in the reference's `weight_init` (utils/utils.py:106-114) works unchanged.

The modules are pinned to the device and dtype they were built with: `.to()/.cuda()/.float()` that would
re-allocate storage raise (the views would silently detach from the kernels' buffers otherwise); no-op moves
(main.py:730, 734) pass.
"""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from ._lib import MLAHipError


class Holder(nn.Module):
    """Interior node of a reference module path (`layer1`, `layer1.0`, `encoder.blocks.3`, ...): carries names only."""

    def forward(self, *a, **k):
        raise MLAHipError("this submodule only carries parameter names; call the owning encoder / classifier")


def _alias(view: torch.Tensor) -> torch.Tensor:
    """A tensor on the same memory as `view` that autograd sees as a LEAF, not as a view of the flat gradient buffer.
    The reference modulates gradients in place (`parms.grad *= coeff_a`, main.py:402), and coeff_a carries autograd history
    because it is computed from out_a, which reads fc_out.weight.  On a view of the flat buffer, that in-place op puts the
    whole buffer into the graph, and the next parameter's view then fails as an in-place op on a leaf that requires grad.
    On an independent leaf it behaves as on the reference's own gradient tensors."""
    t = torch.empty(0, device=view.device, dtype=view.dtype)
    with torch.no_grad():
        t.set_(view.untyped_storage(), view.storage_offset(), view.shape, view.stride())
    return t


def is_attached_fusion(fusion) -> bool:
    """True for a sum / film / gated fusion module put in place by mla_hip.fusion.attach_fusion (it owns its Linears in one flat
    buffer and has no shared `fc_out` head), False for ConcatFusion / ConcatFusion3."""
    return bool(getattr(fusion, "attached_fusion", False))


def _joint_fusion(model):
    fusion = model.fusion_module
    if not getattr(fusion, "joint", False):
        raise MLAHipError("the joint step needs a classifier built with gs_flag false (ConcatFusion on cat(a, v[, t]))")
    return fusion


def _attached(fusion, comm, modulation: str = "Normal"):
    """The attached sum / film / gated fusion module (mla_hip.fusion) of a joint model, or None for concat fusion."""
    if not is_attached_fusion(fusion):
        return None
    if comm is not None and comm.world > 1:
        raise NotImplementedError("data-parallel training / evaluation (comm.world > 1) with an attached sum / film / gated fusion is "
                                  "not implemented")
    if modulation != "Normal" and not fusion.per_modality:
        raise NotImplementedError(f"--modulation {modulation} with --fusion_method {fusion.method}: the reference defines no per-modality "
                                  "logits out_a / out_v for film / gated fusion (main.py:291-302), so OGM / OGM-GE have no coefficients")
    return fusion


def _bare_init(self) -> None:
    nn.Module.__init__(self)


class Conv2dHolder(nn.Conv2d):
    """`isinstance(m, nn.Conv2d)` leaf whose `weight` (OIHW) is a view of the encoder's flat HWIO buffer."""

    def __init__(self, weight: nn.Parameter, stride: int, padding: int):
        _bare_init(self)
        co, ci, kh, kw = weight.shape
        self.in_channels, self.out_channels, self.kernel_size = ci, co, (kh, kw)
        self.stride, self.padding, self.dilation, self.groups = (stride, stride), (padding, padding), (1, 1), 1
        self.transposed, self.output_padding, self.padding_mode = False, (0, 0), "zeros"
        self._reversed_padding_repeated_twice = (padding,) * 4
        self.weight = weight
        self.register_parameter("bias", None)                                     # backbone.py:4-12: bias=False

    def forward(self, *a, **k):
        raise MLAHipError("convolutions run inside the encoder's launch plan; call the encoder / classifier")


class BatchNorm2dHolder(nn.BatchNorm2d):
    """`isinstance(m, nn.BatchNorm2d)` leaf: weight / bias views of the flat parameter buffer, running statistics
    views of the encoder's flat running buffer (momentum 0.1, eps 1e-5: backbone.py:22)."""

    def __init__(self, weight: nn.Parameter, bias: nn.Parameter, running_mean: torch.Tensor, running_var: torch.Tensor):
        _bare_init(self)
        self.num_features, self.eps, self.momentum = weight.shape[0], 1e-5, 0.1
        self.affine, self.track_running_stats = True, True
        self.weight, self.bias = weight, bias
        self.register_buffer("running_mean", running_mean)
        self.register_buffer("running_var", running_var)
        self.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.long, device=weight.device))

    def forward(self, *a, **k):
        raise MLAHipError("batch norm runs inside the encoder's launch plan; call the encoder / classifier")


class FlatModule(nn.Module):
    """Base of every object that owns flat `flat` / `grad` buffers and exposes them under reference names."""

    # Stream that carries this object's training chain (set on encoders by the trainers): anything that touches it from another
    # stream first waits for that one (stream-ordered semantics for forward / state_dict / eval without a device sync).
    tail_stream: Optional[torch.cuda.Stream] = None

    def __init__(self):
        nn.Module.__init__(self)        # explicit: subclasses also inherit nn.Linear (SharedHead), whose ctor allocates
        self._entries: List[Tuple[str, nn.Parameter, torch.Tensor]] = []      # (reference name, parameter, grad view)
        self._published: Optional[List[torch.Tensor]] = None                  # grad views currently installed as p.grad
        self.comm = None                                                      # set by mla_hip.DataParallel

    def _await_tail(self) -> None:
        ts = self.tail_stream
        if ts is not None:
            cur = torch.cuda.current_stream()
            if cur != ts:
                cur.wait_stream(ts)

    # ---- registration -------------------------------------------------------------------------------------
    def _alloc_flat(self, entries: List[Tuple[str, Tuple[int, ...]]]) -> None:
        """`layout` name -> (offset, shape) in the order given, the `flat` / `grad` buffers and their per-name views `p` / `g`."""
        self.layout: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        off = 0
        for name, shp in entries:
            self.layout[name] = (off, shp)
            off += math.prod(shp)
        self.numel = off
        self.flat = torch.zeros(off, device=self.device, dtype=torch.float32)
        self.grad = torch.zeros(off, device=self.device, dtype=torch.float32)
        self.p = {k: self.flat[o:o + math.prod(s)].view(s) for k, (o, s) in self.layout.items()}
        self.g = {k: self.grad[o:o + math.prod(s)].view(s) for k, (o, s) in self.layout.items()}

    def _param_view(self, internal: torch.Tensor, grad_internal: torch.Tensor, to_ref: Callable[[torch.Tensor], torch.Tensor],
                    name: str) -> nn.Parameter:
        """Parameter = `to_ref(internal)` (a VIEW of the flat buffer, reference layout) + the matching gradient view."""
        v = to_ref(internal)
        if v.untyped_storage().data_ptr() != internal.untyped_storage().data_ptr():
            raise MLAHipError(f"{name}: reference view does not alias the flat buffer")
        p = nn.Parameter(v, requires_grad=True)
        p._mla_owner = self
        p._mla_index = len(self._entries)
        self._entries.append((name, p, _alias(to_ref(grad_internal))))
        return p

    @staticmethod
    def _descend(root: nn.Module, dotted: str) -> Tuple[nn.Module, str]:
        parts = dotted.split(".")
        m = root
        for part in parts[:-1]:
            if part not in m._modules:
                m.add_module(part, Holder())
            m = m._modules[part]
        return m, parts[-1]

    # ---- gradients: autograd's AccumulateGrad rule on top of kernels that overwrite the flat gradient ----------
    def grads_pending(self):
        """Call BEFORE a HIP backward: returns what must be added back afterwards (None in the common case where
        every .grad is None, i.e. after optimizer.zero_grad() / `del p.grad`, main.py:440, 468-470)."""
        keep = None
        alias_snapshot = None
        for i, (_n, p, gv) in enumerate(self._entries):
            g = p.grad
            if g is None:
                continue
            if keep is None:
                keep = []
            if self._published is not None and g is self._published[i]:
                if alias_snapshot is None:
                    alias_snapshot = self.grad.clone()                    # the kernels are about to overwrite it
                keep.append((i, None))
            else:
                keep.append((i, g))
        return None if keep is None else (keep, alias_snapshot)

    def publish_grads(self, pending=None) -> None:
        """Call AFTER a HIP backward filled `self.grad`: p.grad <- view (or accumulated)."""
        if pending is not None:
            keep, snap = pending
            aliased = [i for i, g in keep if g is None]
            if len(aliased) == len(self._entries):
                self.grad.add_(snap)                                      # the usual accumulation case: one flat add
            else:
                for i in aliased:
                    self._entries[i][2].add_(self._snap_view(snap, i))
            for i, g in keep:
                if g is not None:                                         # a gradient tensor somebody else assigned
                    self._entries[i][2].add_(g)
        pub = []
        for i, (n, p, gv) in enumerate(self._entries):
            if gv.requires_grad:          # the reference's `p.grad *= coeff` (main.py:402) with a coefficient that carries history
                gv = _alias(gv.detach())  # made the published view part of that graph: publish a fresh alias instead
                self._entries[i] = (n, p, gv)
            p.grad = gv
            pub.append(gv)
        self._published = pub

    def _snap_view(self, snap: torch.Tensor, i: int) -> torch.Tensor:
        gv = self._entries[i][2]
        return torch.as_strided(snap, gv.shape, gv.stride(), gv.storage_offset() - self.grad.storage_offset())

    def segments(self) -> List[Tuple[int, int]]:
        """(offset, numel) of every registered parameter inside the flat buffers (each is one contiguous range)."""
        base = self.grad.storage_offset()
        return [(gv.storage_offset() - base, gv.numel()) for _n, _p, gv in self._entries]

    def grads_alias_flat(self) -> Optional[bool]:
        """True: every p.grad is the published view (one fused optimizer launch is legal); None: every p.grad is None;
        False: anything else (foreign / partial gradients)."""
        some, none, alias = False, False, True
        for i, (_n, p, _gv) in enumerate(self._entries):
            g = p.grad
            if g is None:
                none = True
            else:
                some = True
                if self._published is None or g is not self._published[i]:
                    alias = False
        if not some:
            return None
        return alias and not none

    # ---- device / dtype pinning -----------------------------------------------------------------------------
    def _apply(self, fn, recurse=True):
        probe = torch.empty(0, device=self.device, dtype=torch.float32)
        out = fn(probe)
        if out.device != probe.device or out.dtype != probe.dtype:
            raise MLAHipError(f"mla_hip modules are pinned to {probe.device} / float32 (their parameters are views of the "
                              f"kernels' flat buffers); requested {out.device} / {out.dtype}")
        return self


# Shipped default arithmetic of the conv / Linear contractions: "split" = every fp32 operand split exactly into three
# bf16 terms, six bf16 MFMAs per fp32 product, fp32 accumulate -- fp32 in / out, error against fp64 no larger than the fp32
# MFMA's (tests/test_ops_gpu.py::test_conv_split_is_not_reduced_precision), 1.2-1.3x the throughput.  "f32" = v_mfma_f32_32x32x2_f32.
# "bf16" = each operand rounded once to bf16, ONE product per fp32 product, fp32 accumulate: reduced precision, opt-in only.
DEFAULT_CONV_MATH = "split"


def _await_tail_hook(module, prefix, keep_vars) -> None:
    module._await_tail()                                     # state_dict(): stream-order after the encoder's training chain


class FlatEncoder(FlatModule):
    """What every modality encoder shares: the arithmetic switch `conv_math` ("split" / "f32" / "bf16", default $MLA_CONV_MATH), the
    bf16 images of its GEMM weights (three planes under "split", one under "bf16"; rebuilt at the top of a forward), and the
    hand-over to the stream that carries its training chain (`tail_stream`).  Subclasses add their layout, reference name tree
    and launch plans.  The arithmetic belongs to the instance: encoders of different conv_math share a process."""
    # True: the weight-gradient GEMMs may run on a side stream, `wgrad_stream` (None = on the calling stream)
    side_wgrad = False

    def __init__(self, device, conv_math: Optional[str]):
        super().__init__()
        self.conv_math = conv_math or os.environ.get("MLA_CONV_MATH", DEFAULT_CONV_MATH)
        if self.conv_math not in ("f32", "split", "bf16"):
            raise MLAHipError(f"conv_math must be 'f32' or 'split' or 'bf16', got {self.conv_math!r}")
        self.bf16 = self.conv_math == "bf16"
        self.device = torch.device(device)
        # name -> (forward image, input-gradient image) of the weights _build_wsplit lists; empty under conv_math == "f32"
        self.wsp: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._wsplit_dirty = True
        self.register_state_dict_pre_hook(_await_tail_hook)

    def _build_wsplit(self, weights: List[Tuple[str, str, int, int, int]]) -> None:
        """weights: (wsp key, layout name, taps, K, N) of every [taps][K][N] weight the split arithmetic contracts (a Linear
        [K][N] is a 1-tap conv weight).  Per weight a transposed image for the forward GEMM and a straight one for the
        input-gradient GEMM, 3 bf16 planes each (one under conv_math "bf16"), in one int16 buffer, and the descriptor rows of
        mla_conv2d_wsplit_batch / mla_conv2d_wimage_batch_bf16."""
        if self.conv_math == "f32":
            return
        planes = 1 if self.bf16 else 3
        tot16 = sum(2 * planes * taps * K * N for _k, _n, taps, K, N in weights)
        self._wsplit_flat = torch.empty(tot16, device=self.device, dtype=torch.int16)
        o16, rows, blocks = 0, [], 0
        for key, name, taps, K, N in weights:
            n16 = planes * taps * K * N
            self.wsp[key] = (self._wsplit_flat[o16:o16 + n16], self._wsplit_flat[o16 + n16:o16 + 2 * n16])
            nb = taps * ((K + 31) // 32) * ((N + 31) // 32)
            for transposed, off in ((1, o16), (0, o16 + n16)):
                rows.append([self.layout[name][0], off, taps, K, N, transposed, blocks, 0])
                blocks += nb
            o16 += 2 * n16
        self._wsplit_desc = torch.tensor(rows, dtype=torch.int32, device=self.device)
        self._wsplit_blocks = blocks

    def _refresh_wsplit(self, st) -> None:
        """Re-split the weights (they change with every optimizer step; in eval mode only when marked dirty)."""
        batch = ops.conv2d_wimage_batch_bf16 if self.bf16 else ops.conv2d_wsplit_batch
        batch(self.flat, self._wsplit_flat, self._wsplit_desc, self._wsplit_blocks, stream=st)
        self._wsplit_dirty = False

    def train(self, mode: bool = True):
        super().train(mode)
        self._wsplit_dirty = True
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        self._await_tail()                                   # the copies below must not race the training chain
        self._wsplit_dirty = True
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
