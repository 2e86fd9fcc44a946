"""Thin tensor-level wrappers over the C ABI (include/mla_hip.h).

Every function takes CUDA(HIP) fp32 contiguous tensors, enqueues on `stream` (a raw
hipStream_t handle; default = torch's current stream) and returns immediately.
Activations are NHWC, conv weights HWIO.  No fallbacks: errors raise MLAHipError.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import MLAHipError, check

BN_EPS = 1e-5        # nn.BatchNorm2d default (models/backbone.py:22)
BN_MOMENTUM = 0.1


class KernelTimer:
    """Optional HIP-event bracket around kernel launches (bench.py roofline).  Events are recorded on
    the stream the kernels are launched on (torch's current stream), so elapsed_time is the launch's
    device duration.  Off (None) in normal operation: zero overhead."""

    def __init__(self):
        self.records = []          # (kind, algorithmic work, start event, end event)

    def begin(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, kind: str, work: float, start, moved: float = 0.0) -> None:
        """work = algorithmic FLOPs / bytes of the call; moved = bytes the kernels really move (HBM family)."""
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.records.append((kind, work, start, e, moved))

    def summary(self) -> dict:
        """kind -> {'launches', 'ms', 'ms_raw', 'work', 'moved', 'stalls'} (call after torch.cuda.synchronize()).
        The same call (kind, work) repeats every step; an elapsed time above 4x the median of its repeats and more than 1 ms
        over it is a host / profiler stall between the two event records, not kernel time (seen under rocprofv3: one 100 ms
        buffer flush inside a 0.2 ms bracket): it is replaced by that median and counted in 'stalls'."""
        groups: dict = {}
        for kind, work, s, e, moved in self.records:
            groups.setdefault((kind, work), []).append(s.elapsed_time(e))
        med = {k: sorted(v)[len(v) // 2] for k, v in groups.items()}
        out: dict = {}
        for kind, work, s, e, moved in self.records:
            d = out.setdefault(kind, {"launches": 0, "ms": 0.0, "ms_raw": 0.0, "work": 0.0, "moved": 0.0, "stalls": 0})
            t, m = s.elapsed_time(e), med[(kind, work)]
            d["ms_raw"] += t                       # as measured, stalled brackets included (reported beside the corrected sum)
            if len(groups[(kind, work)]) >= 3 and t > 4.0 * m and t > m + 1.0:
                t = m
                d["stalls"] += 1
            d["launches"] += 1
            d["ms"] += t
            d["work"] += work
            d["moved"] += moved
        return out


TIMER: Optional[KernelTimer] = None


def cur_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor], dtype=torch.float32) -> Optional[int]:
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise MLAHipError(f"expected a contiguous {dtype} device tensor, got {t.dtype} {t.device} "
                          f"contiguous={t.is_contiguous()}")
    return t.data_ptr()


def _call(name: str, *args) -> None:
    """Run the status-returning C entry point `name`; a non-zero status raises MLAHipError with mla_last_error()."""
    check(getattr(_lib.load(), name)(*args), name)


def _begin():
    """Timer bracket around a launch: t0 = _begin(); _call(...); _end(t0, kind, work[, moved]).  TIMER off: one comparison each."""
    return None if TIMER is None else TIMER.begin()


def _end(t0, kind: str, work: float, moved: float = 0.0) -> None:
    if t0 is not None:
        TIMER.end(kind, work, t0, moved)


def conv_out(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


def _want(who: str, **named) -> None:
    """name=(tensor or None, shape): refuse a tensor that is not of its shape before any pointer of it reaches a kernel -- the
    C entry points take sizes from the input alone and would write a smaller buffer out of bounds."""
    for name, (t, shape) in named.items():
        if t is not None and tuple(t.shape) != tuple(shape):
            raise MLAHipError(f"{who}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")


def _dims(who: str, name: str, t: torch.Tensor, n: int) -> Tuple[int, ...]:
    if t.dim() != n:
        raise MLAHipError(f"{who}: {name} has shape {tuple(t.shape)}, expected {n} dimensions")
    return tuple(t.shape)


# ---- layout -------------------------------------------------------------------------------------
def video_to_nhwc(src: torch.Tensor, dst: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    B, C, T, H, W = _dims("video_to_nhwc", "src", src, 5)
    if dst is None:
        dst = torch.empty((B * T, H, W, C), device=src.device, dtype=torch.float32)
    _want("video_to_nhwc", dst=(dst, (B * T, H, W, C)))
    _call("mla_video_to_nhwc", _p(src), _p(dst), B, C, T, H, W, stream or cur_stream())
    return dst


def nchw_to_nhwc(src: torch.Tensor, stream: Optional[int] = None) -> torch.Tensor:
    N, C, H, W = _dims("nchw_to_nhwc", "src", src, 4)
    dst = torch.empty((N, H, W, C), device=src.device, dtype=torch.float32)
    _call("mla_nchw_to_nhwc", _p(src), _p(dst), N, C, H, W, stream or cur_stream())
    return dst


def nhwc_to_nchw(src: torch.Tensor, stream: Optional[int] = None) -> torch.Tensor:
    N, H, W, C = _dims("nhwc_to_nchw", "src", src, 4)
    dst = torch.empty((N, C, H, W), device=src.device, dtype=torch.float32)
    _call("mla_nhwc_to_nchw", _p(src), _p(dst), N, C, H, W, stream or cur_stream())
    return dst


# ---- convolution --------------------------------------------------------------------------------
def conv2d_f32_cfg(cfg: int = -1) -> int:
    """Measurement hook: force the fp32 conv kernels' tile (0..3) or restore the automatic choice (-1)."""
    return int(_lib.load().mla_conv2d_f32_cfg(int(cfg)))


def conv2d_fwd_partial_elems(N, H, W, Cin, Cout, KH, KW, stride, pad) -> int:
    return int(_lib.load().mla_conv2d_fwd_partial_elems(N, H, W, Cin, Cout, KH, KW, stride, pad))


def _conv_fwd(who: str, entry: str, kind: str, x, w, w_dtype, w_shape, stride: int, pad: int, y, bn_partial, stream, bn_in=(),
              min_partial: int = 0) -> Tuple[torch.Tensor, int]:
    """The body of every forward wrapper: `entry`(x, w, y, dims, [bn_in,] bn_partial, &tiles, stream) under a `kind` timer record."""
    N, H, W, Cin = x.shape
    KH, KW, Cin2, Cout = w_shape
    if Cin2 != Cin:
        raise MLAHipError(f"{who}: x has {Cin} channels, weight expects {Cin2}")
    if y is None:
        y = torch.empty((N, conv_out(H, KH, stride, pad), conv_out(W, KW, stride, pad), Cout), device=x.device, dtype=torch.float32)
    if bn_partial is not None and bn_partial.numel() < min_partial:
        raise MLAHipError(f"{who}: bn_partial too small")
    tiles = ctypes.c_int(0)
    t0 = _begin()
    _call(entry, _p(x), _p(w, w_dtype), _p(y), N, H, W, Cin, Cout, KH, KW, stride, pad, *[_p(t) for t in bn_in[:4]], _p(bn_partial),
          ctypes.addressof(tiles), stream or cur_stream())
    _end(t0, kind, 2.0 * y.numel() * KH * KW * Cin)
    return y, tiles.value


def conv2d_fwd(x: torch.Tensor, w_hwio: torch.Tensor, stride: int, pad: int, y: Optional[torch.Tensor] = None,
               bn_partial: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """Returns (y, tiles).  If `bn_partial` is given it receives [tiles][2][Cout] column sums / sums of squares."""
    return _conv_fwd("conv2d_fwd", "mla_conv2d_fwd", "conv_fwd", x, w_hwio, torch.float32, w_hwio.shape, stride, pad, y, bn_partial, stream)


class _BnReduceReq(ctypes.Structure):     # include/mla_hip.h: mla_bn_reduce_req
    _fields_ = [("x", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("invstd", ctypes.c_void_p), ("partial", ctypes.c_void_p)]


def conv2d_dgrad_bn_partial_elems(N: int, H: int, W: int, Cin: int) -> int:
    return int(_lib.load().mla_conv2d_dgrad_bn_partial_elems(N, H, W, Cin))


def _bn_reqs(bn_reqs, x_shape):
    """bn_reqs: sequence of (x, mean, invstd, partial) -- BatchNorm layers whose backward consumes dx (<= 2)."""
    if not bn_reqs:
        return None, 0
    if len(bn_reqs) > 2:
        raise MLAHipError("conv2d_dgrad: at most two BatchNorm reduction requests")
    N, H, W, Cin = x_shape
    need = conv2d_dgrad_bn_partial_elems(N, H, W, Cin)
    arr = (_BnReduceReq * len(bn_reqs))()
    for q, (x, mean, invstd, partial) in enumerate(bn_reqs):
        if tuple(x.shape) != tuple(x_shape) or mean.numel() != Cin or invstd.numel() != Cin or partial.numel() < need:
            raise MLAHipError(f"conv2d_dgrad: BatchNorm request {q} does not match dx {tuple(x_shape)} (partial >= {need} floats)")
        arr[q].x, arr[q].mean, arr[q].invstd, arr[q].partial = _p(x), _p(mean), _p(invstd), _p(partial)
    return arr, len(bn_reqs)


def _conv_dgrad(entry: str, dy, w, w_dtype, w_shape, x_shape, stride: int, pad: int, dx, bn_reqs, stream, before=(), after=()):
    """The body of every input-gradient wrapper: `entry`(dy, w, dx, dims, *before (tensors), requests, nreq, &tiles, *after (tensors or
    ints), stream).  Returns (dx, tiles) with requests, dx without."""
    N, H, W, Cin = x_shape
    KH, KW, _, Cout = w_shape
    if dx is None:
        dx = torch.empty((N, H, W, Cin), device=dy.device, dtype=torch.float32)
    arr, nreq = _bn_reqs(bn_reqs, x_shape)
    tiles = ctypes.c_int(0)
    t0 = _begin()
    _call(entry, _p(dy), _p(w, w_dtype), _p(dx), N, H, W, Cin, Cout, KH, KW, stride, pad, *[_p(t) for t in before],
          ctypes.addressof(arr) if nreq else None, nreq, ctypes.addressof(tiles), *[a if isinstance(a, int) else _p(a) for a in after],
          stream or cur_stream())
    _end(t0, "conv_dgrad", 2.0 * dy.numel() * KH * KW * Cin)
    return (dx, tiles.value) if nreq else dx


def conv2d_dgrad(dy: torch.Tensor, w_hwio: torch.Tensor, x_shape, stride: int, pad: int, wt_ws: torch.Tensor,
                 dx: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                 relu_src: Optional[torch.Tensor] = None, stream: Optional[int] = None, bn_reqs=None,
                 class_mask: int = 0xF, residual_mask: int = 0xF):
    """Input gradient.  With bn_reqs (see _bn_reqs) the epilogue also forms the reduction pass of those BatchNorm
    backwards and the call returns (dx, tiles) for bn_bwd_from_partial.  class_mask / residual_mask: output parity classes
    (bit py * stride + px) to compute / to add `residual` in (include/mla_hip.h: mla_conv2d_dgrad_classes)."""
    if wt_ws.numel() < w_hwio.numel():
        raise MLAHipError("conv2d_dgrad: wt_ws too small")
    return _conv_dgrad("mla_conv2d_dgrad_classes", dy, w_hwio, torch.float32, w_hwio.shape, x_shape, stride, pad, dx, bn_reqs, stream,
                       before=(residual, relu_src, wt_ws), after=(class_mask, residual_mask))


def conv2d_wsplit(w_hwio: torch.Tensor, transposed: bool, out: Optional[torch.Tensor] = None,
                  stream: Optional[int] = None) -> torch.Tensor:
    """Three bf16 planes of the conv weights (int16 storage, [3][taps][n][k]) for the split-bf16 kernels:
    transposed=True for conv2d_fwd_split (n=Cout, k=Cin), False for conv2d_dgrad_split (n=Cin, k=Cout)."""
    KH, KW, Cin, Cout = w_hwio.shape
    n = int(_lib.load().mla_conv2d_wsplit_bytes(Cin, Cout, KH, KW)) // 2
    if out is None:
        out = torch.empty(n, device=w_hwio.device, dtype=torch.int16)
    if out.numel() < n or out.dtype != torch.int16:
        raise MLAHipError("conv2d_wsplit: out must hold 3*KH*KW*Cin*Cout int16")
    _call("mla_conv2d_wsplit", _p(w_hwio), _p(out, torch.int16), Cin, Cout, KH, KW, int(transposed), stream or cur_stream())
    return out


def conv2d_wsplit_batch(params: torch.Tensor, wsplit: torch.Tensor, desc: torch.Tensor, total_blocks: int,
                        stream: Optional[int] = None) -> None:
    """One launch that re-splits every conv listed in `desc` (int32 device tensor, n x 8; see include/mla_hip.h)."""
    _call("mla_conv2d_wsplit_batch", _p(params), _p(wsplit, torch.int16), _p(desc, torch.int32), desc.shape[0], int(total_blocks),
          stream or cur_stream())


def conv2d_fwd_split(x: torch.Tensor, wsplit_t: torch.Tensor, w_shape, stride: int, pad: int,
                     y: Optional[torch.Tensor] = None, bn_partial: Optional[torch.Tensor] = None,
                     stream: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """conv2d_fwd on the split-bf16 MFMA path; `wsplit_t` = conv2d_wsplit(w, True), w_shape = (KH, KW, Cin, Cout)."""
    return _conv_fwd("conv2d_fwd_split", "mla_conv2d_fwd_split", "conv_fwd", x, wsplit_t, torch.int16, w_shape, stride, pad, y, bn_partial,
                     stream)


def conv2d_dgrad_split(dy: torch.Tensor, wsplit: torch.Tensor, w_shape, x_shape, stride: int, pad: int,
                       dx: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                       relu_src: Optional[torch.Tensor] = None, stream: Optional[int] = None, bn_reqs=None,
                       class_mask: int = 0xF, residual_mask: int = 0xF):
    """conv2d_dgrad on the split-bf16 MFMA path; `wsplit` = conv2d_wsplit(w, False).  bn_reqs as in conv2d_dgrad."""
    return _conv_dgrad("mla_conv2d_dgrad_split_classes", dy, wsplit, torch.int16, w_shape, x_shape, stride, pad, dx, bn_reqs, stream,
                       before=(residual, relu_src), after=(class_mask, residual_mask))


# ---- conv_math "bf16": one bf16 rounding per operand, one product (include/mla_hip.h: mla_conv2d_*_bf16) -----------------------------
def conv2d_wimage_bf16(w_hwio: torch.Tensor, transposed: bool, out: Optional[torch.Tensor] = None,
                       stream: Optional[int] = None) -> torch.Tensor:
    """One bf16 plane of the conv weights (int16 storage, [taps][n][k]) for the bf16 kernels: transposed=True for conv2d_fwd_bf16
    (n=Cout, k=Cin), False for conv2d_dgrad_bf16 (n=Cin, k=Cout)."""
    KH, KW, Cin, Cout = w_hwio.shape
    n = int(_lib.load().mla_conv2d_wimage_bytes_bf16(Cin, Cout, KH, KW)) // 2
    if out is None:
        out = torch.empty(n, device=w_hwio.device, dtype=torch.int16)
    if out.numel() < n or out.dtype != torch.int16:
        raise MLAHipError("conv2d_wimage_bf16: out must hold KH*KW*Cin*Cout int16")
    _call("mla_conv2d_wimage_bf16", _p(w_hwio), _p(out, torch.int16), Cin, Cout, KH, KW, int(transposed), stream or cur_stream())
    return out


def conv2d_wimage_batch_bf16(params: torch.Tensor, wimage: torch.Tensor, desc: torch.Tensor, total_blocks: int,
                             stream: Optional[int] = None) -> None:
    """conv2d_wsplit_batch for the one-plane images (same descriptor rows, out_off in 16-bit elements of `wimage`)."""
    _call("mla_conv2d_wimage_batch_bf16", _p(params), _p(wimage, torch.int16), _p(desc, torch.int32), desc.shape[0], int(total_blocks),
          stream or cur_stream())


def conv2d_tile_bf16(M: int, Cout: int, k_total: int) -> int:
    """Diagnostic / test query: the tile (index into 256x128, 128x128, 128x64, 64x64, 256x64, 192x128) a bf16 gather-GEMM of these
    dims runs on, on the current device (the choice depends on its CU count)."""
    return int(_lib.load().mla_conv2d_tile_bf16(int(M), int(Cout), int(k_total)))


def conv2d_fwd_bf16(x: torch.Tensor, wimage_t: torch.Tensor, w_shape, stride: int, pad: int, y: Optional[torch.Tensor] = None,
                    bn_partial: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """conv2d_fwd on the single-product bf16 arithmetic; `wimage_t` = conv2d_wimage_bf16(w, True), w_shape = (KH, KW, Cin, Cout)."""
    return _conv_fwd("conv2d_fwd_bf16", "mla_conv2d_fwd_bf16", "conv_fwd", x, wimage_t, torch.int16, w_shape, stride, pad, y, bn_partial,
                     stream)


def conv2d_dgrad_bf16(dy: torch.Tensor, wimage: torch.Tensor, w_shape, x_shape, stride: int, pad: int,
                      dx: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                      relu_src: Optional[torch.Tensor] = None, stream: Optional[int] = None, class_mask: int = 0xF,
                      residual_mask: int = 0xF) -> torch.Tensor:
    """conv2d_dgrad on the single-product bf16 arithmetic; `wimage` = conv2d_wimage_bf16(w, False).  One launch per parity class."""
    N, H, W, Cin = x_shape
    KH, KW, _, Cout = w_shape
    if dx is None:
        dx = torch.empty((N, H, W, Cin), device=dy.device, dtype=torch.float32)
    t0 = _begin()
    _call("mla_conv2d_dgrad_bf16", _p(dy), _p(wimage, torch.int16), _p(dx), N, H, W, Cin, Cout, KH, KW, stride, pad, _p(residual), _p(relu_src),
          class_mask, residual_mask, stream or cur_stream())
    _end(t0, "conv_dgrad", 2.0 * dy.numel() * KH * KW * Cin)
    return dx


def conv2d_wgrad_ws_bytes_bf16(N, H, W, Cin, Cout, KH, KW, stride, pad) -> int:
    return int(_lib.load().mla_conv2d_wgrad_ws_bytes_bf16(N, H, W, Cin, Cout, KH, KW, stride, pad))


def conv2d_wgrad_bf16(x: torch.Tensor, dy: torch.Tensor, dw_hwio: torch.Tensor, stride: int, pad: int, ws: torch.Tensor,
                      stream: Optional[int] = None) -> torch.Tensor:
    """conv2d_wgrad on the single-product bf16 arithmetic (per-tap kernel; Cin a multiple of 64); ws >= conv2d_wgrad_ws_bytes_bf16."""
    return _conv_wgrad("mla_conv2d_wgrad_bf16", "conv_wgrad", x, dy, dw_hwio, stride, pad, ws, stream)


def conv2d_bnfold_supported(N: int, H: int, W: int, Cin: int, Cout: int, KH: int, KW: int, stride: int, pad: int) -> bool:
    """True where relu(bn(.)) can be folded into the operands of a convolution (64 -> 64 channels, 3x3 / 1 / 1, split arithmetic)."""
    return bool(_lib.load().mla_conv2d_bnfold_supported(N, H, W, Cin, Cout, KH, KW, stride, pad))


def conv2d_fwd_split_bnin(x: torch.Tensor, wsplit_t: torch.Tensor, w_shape, stride: int, pad: int, bn_in, y: Optional[torch.Tensor] = None,
                          bn_partial: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """conv2d_fwd_split over relu(bn(x)); bn_in = (mean, invstd, gamma, beta) per input channel.  x is the BatchNorm's input."""
    return _conv_fwd("conv2d_fwd_split_bnin", "mla_conv2d_fwd_split_bnin", "conv_fwd", x, wsplit_t, torch.int16, w_shape, stride, pad, y,
                     bn_partial, stream, bn_in=bn_in)


def conv2d_wgrad_split_bnin(x: torch.Tensor, dy: torch.Tensor, dw_hwio: torch.Tensor, stride: int, pad: int, ws: torch.Tensor, bn_in,
                            stream: Optional[int] = None) -> torch.Tensor:
    """conv2d_wgrad_split with relu(bn(x)) as the input operand; bn_in = (mean, invstd, gamma, beta)."""
    return _conv_wgrad("mla_conv2d_wgrad_split_bnin", "conv_wgrad", x, dy, dw_hwio, stride, pad, ws, stream, bn_in=bn_in)


def conv2d_dgrad_split_bnmask(dy: torch.Tensor, wsplit: torch.Tensor, w_shape, x_shape, stride: int, pad: int, dx: torch.Tensor, bn_req,
                              mask_gamma: torch.Tensor, mask_beta: torch.Tensor, stream: Optional[int] = None):
    """conv2d_dgrad_split whose ReLU mask is relu(bn(bn_req.x)) > 0 -- the BatchNorm whose backward reduction the epilogue forms anyway
    (bn_req = (x, mean, invstd, partial)).  Returns (dx, tiles)."""
    return _conv_dgrad("mla_conv2d_dgrad_split_bnmask", dy, wsplit, torch.int16, w_shape, x_shape, stride, pad, dx, [bn_req], stream,
                       after=(mask_gamma, mask_beta))


def conv2d_stem_supported(Cin: int, Cout: int, KH: int, KW: int, stride: int, pad: int) -> bool:
    """True where the persistent split-arithmetic stem kernels apply (7x7 / 2 / 3, 1 or 3 -> 64 channels)."""
    return bool(_lib.load().mla_conv2d_stem_supported(Cin, Cout, KH, KW, stride, pad))


def conv2d_stem_waves(waves: int = -1) -> int:
    """Measurement hook: force 4 or 8 waves per stem-forward workgroup; 0 = automatic; -1: query."""
    return int(_lib.load().mla_conv2d_stem_waves(int(waves)))


def conv2d_stem_fwd_partial_elems() -> int:
    return int(_lib.load().mla_conv2d_stem_fwd_partial_elems())


def conv2d_stem_fwd_split(x: torch.Tensor, w_hwio: torch.Tensor, y: Optional[torch.Tensor] = None,
                          bn_partial: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """The stem convolution (backbone.py:79-83, 149) on the split arithmetic, persistent patch-loader kernel; plain fp32 HWIO
    weights.  Returns (y, partial rows) like conv2d_fwd."""
    return _conv_fwd("conv2d_stem_fwd_split", "mla_conv2d_stem_fwd_split", "stem_fwd", x, w_hwio, torch.float32, w_hwio.shape, 2, 3, y,
                     bn_partial, stream, min_partial=conv2d_stem_fwd_partial_elems() if bn_partial is not None else 0)


def conv2d_stem_wgrad_split_ws_bytes(Cin: int) -> int:
    return int(_lib.load().mla_conv2d_stem_wgrad_split_ws_bytes(Cin))


def _conv_wgrad(entry: str, kind: str, x, dy, dw_hwio, stride: int, pad: int, ws, stream, bn_in=()) -> torch.Tensor:
    """The body of every weight-gradient wrapper: `entry`(x, dy, dw, dims, [bn_in,] ws, its bytes, stream) under a `kind` timer record."""
    N, H, W, Cin = x.shape
    KH, KW, _, Cout = dw_hwio.shape
    t0 = _begin()
    _call(entry, _p(x), _p(dy), _p(dw_hwio), N, H, W, Cin, Cout, KH, KW, stride, pad, *[_p(t) for t in bn_in[:4]], _p(ws),
          ws.numel() * ws.element_size(), stream or cur_stream())
    _end(t0, kind, 2.0 * dy.numel() * KH * KW * Cin)
    return dw_hwio


def conv2d_stem_wgrad_split(x: torch.Tensor, dy: torch.Tensor, dw_hwio: torch.Tensor, stride: int, pad: int, ws: torch.Tensor,
                            stream: Optional[int] = None) -> torch.Tensor:
    """Stem weight gradient on the split arithmetic (same call shape as conv2d_wgrad)."""
    return _conv_wgrad("mla_conv2d_stem_wgrad_split", "stem_wgrad", x, dy, dw_hwio, stride, pad, ws, stream)


def conv2d_stem_wgrad_split_bnpool(x: torch.Tensor, dpool: torch.Tensor, idx: torch.Tensor, y: torch.Tensor, mean, invstd, gamma, beta,
                                   dgamma, dbeta, dw_hwio: torch.Tensor, ws: torch.Tensor, stream: Optional[int] = None) -> torch.Tensor:
    """Stem weight gradient that forms conv1's gradient itself: the apply pass of bn_bwd_pooled runs where conv2d_stem_wgrad_split
    loads dy (same bits); dgamma / dbeta from bn_bwd_pooled(dy=None).  ws as conv2d_stem_wgrad_split."""
    N, H, W, Cin = x.shape
    KH, KW, _, Cout = dw_hwio.shape
    t0 = _begin()
    _call("mla_conv2d_stem_wgrad_split_bnpool", _p(x), _p(dpool), _p(idx, torch.uint8), _p(y), _p(mean), _p(invstd), _p(gamma), _p(beta),
          _p(dgamma), _p(dbeta), _p(dw_hwio), N, H, W, Cin, Cout, KH, KW, 2, 3, _p(ws), ws.numel() * ws.element_size(), stream or cur_stream())
    _end(t0, "stem_wgrad", 2.0 * y.numel() * KH * KW * Cin)
    return dw_hwio


def conv2d_wgrad_tr(on: int = -1) -> int:
    """Measurement hook: 0 / 1 = per-tap / persistent all-taps split weight gradient for the 64 -> 64 3x3 convs; -1: query."""
    return int(_lib.load().mla_conv2d_wgrad_tr(int(on)))


def conv2d_patch(on: int = -1) -> int:
    """Measurement hook: 0 / 1 = per-tap gather-GEMM / LDS-patch kernel for the 3x3 stride-1 split forward and input gradient; -1: query."""
    return int(_lib.load().mla_conv2d_patch(int(on)))


def conv2d_dgrad_merge(on: int = -1) -> int:
    """Measurement hook: 0 / 1 = one launch per parity class / all classes in one launch for the stride-2 split input gradient; -1: query."""
    return int(_lib.load().mla_conv2d_dgrad_merge(int(on)))


def conv2d_two_phase(on: int = -1) -> int:
    """Measurement hook: 0 / 1 = single launch / whole rounds of a big tile + one launch for the remaining rows (split gather-GEMM); -1: query."""
    return int(_lib.load().mla_conv2d_two_phase(int(on)))


def conv2d_split_terms(terms: int = 0) -> int:
    """Select (3, 6, 8) or query (anything else) the bf16 product set of the split kernels; 6 = fp32-equivalent."""
    return int(_lib.load().mla_conv2d_split_terms(int(terms)))


def conv2d_split_cfg(cfg: int = -1) -> int:
    """Measurement hook: force the split kernels' tile (0..3) or restore the automatic choice (-1)."""
    return int(_lib.load().mla_conv2d_split_cfg(int(cfg)))


def conv2d_wgrad_ws_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad) -> int:
    return int(_lib.load().mla_conv2d_wgrad_ws_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad))


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, dw_hwio: torch.Tensor, stride: int, pad: int, ws: torch.Tensor,
                 stream: Optional[int] = None) -> torch.Tensor:
    return _conv_wgrad("mla_conv2d_wgrad", "conv_wgrad", x, dy, dw_hwio, stride, pad, ws, stream)


def conv2d_wgrad_split_ws_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad) -> int:
    return int(_lib.load().mla_conv2d_wgrad_split_ws_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad))


def conv2d_wgrad_split(x: torch.Tensor, dy: torch.Tensor, dw_hwio: torch.Tensor, stride: int, pad: int, ws: torch.Tensor,
                       stream: Optional[int] = None) -> torch.Tensor:
    """conv2d_wgrad on the split-bf16 MFMA path (Cin a multiple of 64); ws >= conv2d_wgrad_split_ws_bytes."""
    return _conv_wgrad("mla_conv2d_wgrad_split", "conv_wgrad", x, dy, dw_hwio, stride, pad, ws, stream)


# ---- batch norm ---------------------------------------------------------------------------------
def bn_partial_scratch_elems(C: int) -> int:
    """Floats of the two-stage reduction's scratch tail that follows the [tiles][2][C] rows of every partial buffer."""
    return int(_lib.load().mla_bn_partial_scratch_elems(C))


def bn_stats_partial_elems(M: int, C: int) -> int:
    return int(_lib.load().mla_bn_stats_partial_elems(M, C))


def bn_stats_partial(x2d: torch.Tensor, M: int, C: int, partial: torch.Tensor, stream: Optional[int] = None) -> int:
    tiles = ctypes.c_int(0)
    _call("mla_bn_stats_partial", _p(x2d), M, C, _p(partial), ctypes.addressof(tiles), stream or cur_stream())
    return tiles.value


def bn_finalize(partial: torch.Tensor, tiles: int, M: int, C: int, mean: torch.Tensor, invstd: torch.Tensor,
                running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor],
                eps: float = BN_EPS, momentum: float = BN_MOMENTUM, stream: Optional[int] = None) -> None:
    t0 = _begin()
    _call("mla_bn_finalize", _p(partial), tiles, M, C, eps, momentum, _p(mean), _p(invstd), _p(running_mean), _p(running_var), stream or cur_stream())
    _end(t0, "bn_fwd", 0.0)      # statistics finalize: its time belongs to the BN forward, its bytes are negligible


def bn_apply(x: torch.Tensor, mean, invstd, gamma, beta, out: torch.Tensor, M: int, C: int, relu: bool,
             residual: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    t0 = _begin()
    _call("mla_bn_apply", _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(residual), _p(out), M, C, int(relu), stream or cur_stream())
    # BN-fwd-train = 12 B/elem algorithmic; this path moves 8 (+4 with a residual)
    _end(t0, "bn_fwd", 12.0 * M * C, (12.0 if residual is not None else 8.0) * M * C)
    return out


def bn_bwd_ws_elems(M: int, C: int) -> int:
    return int(_lib.load().mla_bn_bwd_ws_elems(M, C))


def bn_bwd(dout, x, mean, invstd, gamma, dx, dgamma, dbeta, ws, M: int, C: int, relu_out=None, g_out=None,
           stream: Optional[int] = None) -> None:
    t0 = _begin()
    _call("mla_bn_bwd", _p(dout), _p(relu_out), _p(x), _p(mean), _p(invstd), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), _p(g_out), _p(ws), M, C,
          stream or cur_stream())
    _end(t0, "bn_bwd", 20.0 * M * C, 20.0 * M * C)   # BN-bwd = 20 B/elem (dy, x for the reductions; dy, x again; write dx)


def bn_relu_maxpool_fwd(y, mean, invstd, gamma, beta, out, idx, stream: Optional[int] = None) -> None:
    """maxpool3x3s2(relu(bn(y))) without materialising the ReLU output (stem, backbone.py:150-152)."""
    N, H, W, C = _dims("bn_relu_maxpool_fwd", "y", y, 4)
    pooled = (N, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), C)
    _want("bn_relu_maxpool_fwd", mean=(mean, (C,)), invstd=(invstd, (C,)), gamma=(gamma, (C,)), beta=(beta, (C,)), out=(out, pooled),
          idx=(idx, pooled))
    t0 = _begin()
    _call("mla_bn_relu_maxpool_fwd", _p(y), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(out), _p(idx, torch.uint8), N, H, W, C,
          stream or cur_stream())
    by = 4.0 * N * H * W * C + 5.0 * out.numel()   # read y once, write the pooled quarter + its index bytes
    _end(t0, "bn_fwd", by, by)


def bn_bwd_pooled(dpool, idx, y, mean, invstd, gamma, beta, dy, dgamma, dbeta, ws, stream: Optional[int] = None) -> None:
    """BatchNorm backward fed by the pooled gradient (max-pool scatter + ReLU mask recomputed on the fly).  dy = None: the
    reduction half alone (dgamma, dbeta), for conv2d_stem_wgrad_split_bnpool."""
    N, H, W, C = _dims("bn_bwd_pooled", "y", y, 4)
    pooled = (N, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), C)
    _want("bn_bwd_pooled", dpool=(dpool, pooled), idx=(idx, pooled), mean=(mean, (C,)), invstd=(invstd, (C,)), gamma=(gamma, (C,)),
          beta=(beta, (C,)), dy=(dy, (N, H, W, C)), dgamma=(dgamma, (C,)), dbeta=(dbeta, (C,)))
    need = bn_bwd_ws_elems(N * H * W, C) if 0 < N * H * W < 2 ** 31 else 0      # (sizes out of range: the entry point refuses them)
    if ws is not None and ws.numel() < need:
        raise MLAHipError(f"bn_bwd_pooled: ws has {ws.numel()} elements, bn_bwd_ws_elems({N * H * W}, {C}) = {need}")
    t0 = _begin()
    _call("mla_bn_bwd_pooled", _p(dpool), _p(idx, torch.uint8), _p(y), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(dy), _p(dgamma), _p(dbeta),
          _p(ws), N, H, W, C, stream or cur_stream())
    if dy is None:
        by = 9.0 * dpool.numel()                        # the pooled gradient + index once, one selected y value per pooled output
    else:
        by = 12.0 * N * H * W * C + 10.0 * dpool.numel()   # y twice, dy once, the pooled gradient + index twice
    _end(t0, "bn_bwd", by, by)


def bn_bwd_from_partial(dout, x, mean, invstd, gamma, dx, dgamma, dbeta, partial, tiles: int, M: int, C: int,
                        stream: Optional[int] = None) -> None:
    """BatchNorm backward whose reduction pass was formed by the input-gradient kernel that wrote `dout` (bn_reqs)."""
    t0 = _begin()
    _call("mla_bn_bwd_from_partial", _p(dout), _p(x), _p(mean), _p(invstd), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), _p(partial), tiles, M, C,
          stream or cur_stream())
    _end(t0, "bn_bwd", 12.0 * M * C, 12.0 * M * C)   # dy, x read once; dx written


# ---- pooling ------------------------------------------------------------------------------------
def maxpool_fwd(x: torch.Tensor, y: torch.Tensor, idx: torch.Tensor, stream: Optional[int] = None) -> None:
    N, H, W, C = _dims("maxpool_fwd", "x", x, 4)
    pooled = (N, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), C)
    _want("maxpool_fwd", y=(y, pooled), idx=(idx, pooled))
    _call("mla_maxpool3x3s2_fwd", _p(x), _p(y), _p(idx, torch.uint8), N, H, W, C, stream or cur_stream())


def maxpool_bwd(dy, idx, dx, x_shape, relu_src=None, stream: Optional[int] = None) -> None:
    if len(x_shape) != 4:
        raise MLAHipError(f"maxpool_bwd: x_shape {tuple(x_shape)} must be (N, H, W, C)")
    N, H, W, C = x_shape
    pooled = (N, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), C)
    _want("maxpool_bwd", dy=(dy, pooled), idx=(idx, pooled), dx=(dx, x_shape), relu_src=(relu_src, x_shape))
    _call("mla_maxpool3x3s2_bwd", _p(dy), _p(idx, torch.uint8), _p(relu_src), _p(dx), N, H, W, C, stream or cur_stream())


def _want_numel(who: str, **named) -> None:
    """name=(tensor or None, element count): the average pool takes [NB][P][C] activations in whatever shape holds them."""
    for name, (t, n) in named.items():
        if t is not None and t.numel() != n:
            raise MLAHipError(f"{who}: {name} has {t.numel()} elements (shape {tuple(t.shape)}), expected {n}")


def avgpool_fwd(x, y, NB: int, P: int, C: int, stream: Optional[int] = None) -> None:
    _want_numel("avgpool_fwd", x=(x, NB * P * C), y=(y, NB * C))
    _call("mla_avgpool_fwd", _p(x), _p(y), NB, P, C, stream or cur_stream())


def avgpool_bwd(dy, dx, NB: int, P: int, C: int, relu_src=None, stream: Optional[int] = None) -> None:
    _want_numel("avgpool_bwd", dy=(dy, NB * C), dx=(dx, NB * P * C), relu_src=(relu_src, NB * P * C))
    _call("mla_avgpool_bwd", _p(dy), _p(relu_src), _p(dx), NB, P, C, stream or cur_stream())


# ---- head / projection / optimiser ----------------------------------------------------------------
def head_ws_elems(B: int, C: int) -> int:
    return int(_lib.load().mla_head_ws_elems(B, C))


def head_ce_fwd_bwd(X, W, b, labels, logits, loss, dW, db, dX, ws, inv_batch: float, stream: Optional[int] = None) -> None:
    B, D = X.shape
    C = W.shape[0]
    _call("mla_head_ce_fwd_bwd", _p(X), _p(W), _p(b), _p(labels, torch.int64), _p(logits), _p(loss), _p(dW), _p(db), _p(dX), _p(ws), B, D, C,
          inv_batch, stream or cur_stream())


def ce_fwd_bwd(logits, labels, loss, dlogits, ws, inv_batch: float, stream: Optional[int] = None) -> None:
    """nn.CrossEntropyLoss() forward + d logits (main.py:130, 434); ws: B floats."""
    B, C = logits.shape
    _call("mla_ce_fwd_bwd", _p(logits), _p(labels, torch.int64), _p(loss), _p(dlogits), _p(ws), B, C, inv_batch, stream or cur_stream())


def head_bwd(X, W, dlogits, dW, db, dX, scale: float = 1.0, stream: Optional[int] = None) -> None:
    """autograd of fc_out for a given d logits: dW, db, dX (all times `scale`)."""
    B, D = X.shape
    C = W.shape[0]
    if tuple(dlogits.shape) != (B, C):
        raise MLAHipError(f"head_bwd: dlogits {tuple(dlogits.shape)} does not match ({B}, {C})")
    _call("mla_head_bwd", _p(X), _p(W), _p(dlogits), _p(dW), _p(db), _p(dX), B, D, C, scale, stream or cur_stream())


def _concat_ptrs(xs, who: str):
    M = len(xs)
    if M not in (2, 3):
        raise MLAHipError(f"{who}: needs 2 or 3 feature tensors, got {M}")
    B, D = xs[0].shape
    for x in xs[1:]:
        if tuple(x.shape) != (B, D):
            raise MLAHipError(f"{who}: every modality must have the same (B, D); got {[tuple(t.shape) for t in xs]}")
    return [_p(x) for x in xs] + [None] * (3 - M), M, B, D


def concat_head_ws_elems(B: int, C: int, M: int) -> int:
    return int(_lib.load().mla_concat_head_ws_elems(B, C, M))


def concat_head_ce_fwd_bwd(xs, W, b, labels, out, out_m, loss, loss_m, dW, db, dxs, ws, inv_batch: float,
                           stream: Optional[int] = None) -> None:
    """Joint head (main.py:273-311): out = fc_out(cat(xs)), out_m (M, B, C), CE loss / per-modality losses and all gradients."""
    x, M, B, D = _concat_ptrs(xs, "concat_head_ce_fwd_bwd")
    C = W.shape[0]
    if tuple(W.shape) != (C, M * D) or len(dxs) != M:
        raise MLAHipError(f"concat_head_ce_fwd_bwd: W {tuple(W.shape)} does not match {M} x (B, {D})")
    dx = [_p(t) for t in dxs] + [None] * (3 - M)
    _call("mla_concat_head_ce_fwd_bwd", x[0], x[1], x[2], _p(W), _p(b), _p(labels, torch.int64), _p(out), _p(out_m), _p(loss), _p(loss_m), _p(dW),
          _p(db), dx[0], dx[1], dx[2], _p(ws), M, B, D, C, inv_batch, stream or cur_stream())


def concat_head_fwd(xs, W, b, out, out_m, stream: Optional[int] = None) -> None:
    """out = fc_out(cat(xs)) and out_m = xs[m] W_m^T + b / M, no gradients (valid(); the autograd forward)."""
    x, M, B, D = _concat_ptrs(xs, "concat_head_fwd")
    C = W.shape[0]
    if tuple(W.shape) != (C, M * D):
        raise MLAHipError(f"concat_head_fwd: W {tuple(W.shape)} does not match {M} x (B, {D})")
    _call("mla_concat_head_fwd", x[0], x[1], x[2], _p(W), _p(b), _p(out), _p(out_m), M, B, D, C, stream or cur_stream())


def concat_head_bwd(xs, W, dlogits, dW, db, dxs, scale: float = 1.0, stream: Optional[int] = None) -> None:
    """autograd of the concatenated fc_out for a given d out: dW, db, dX_m (all times `scale`)."""
    x, M, B, D = _concat_ptrs(xs, "concat_head_bwd")
    C = W.shape[0]
    if tuple(W.shape) != (C, M * D) or tuple(dlogits.shape) != (B, C) or len(dxs) != M:
        raise MLAHipError(f"concat_head_bwd: W {tuple(W.shape)} / dlogits {tuple(dlogits.shape)} do not match {M} x ({B}, {D})")
    dx = [_p(t) for t in dxs] + [None] * (3 - M)
    _call("mla_concat_head_bwd", x[0], x[1], x[2], _p(W), _p(dlogits), _p(dW), _p(db), dx[0], dx[1], dx[2], M, B, D, C, scale, stream or cur_stream())


# ---- sum / FiLM / gated fusion heads (csrc/fusion_head.hip) ---------------------------------------------------------------------------
def fusion_ws_elems(B: int, D: int, C: int) -> int:
    return int(_lib.load().mla_fusion_ws_elems(B, D, C))


def _fusion_dims(who: str, x, y, Wout, hidden=(), ws=None, labels=None):
    """(B, D, C) of a fusion head call; `hidden`: (tensor, shape) pairs that must match (biases, bias gradients and loss vectors
    included: the kernels write them unchecked); `ws` at least fusion_ws_elems(B, D, C) floats; `labels` (B,)."""
    B, D = x.shape
    C = Wout.shape[0]
    if tuple(y.shape) != (B, D) or tuple(Wout.shape) != (C, D):
        raise MLAHipError(f"{who}: features {tuple(x.shape)} / {tuple(y.shape)} and the output weight {tuple(Wout.shape)} do not match")
    for t, shp in hidden:
        if tuple(t.shape) != tuple(shp(B, D, C)):
            raise MLAHipError(f"{who}: a tensor of shape {tuple(t.shape)} where {tuple(shp(B, D, C))} is expected")
    if labels is not None and tuple(labels.shape) != (B,):
        raise MLAHipError(f"{who}: labels of shape {tuple(labels.shape)} where ({B},) is expected")
    if ws is not None and ws.numel() < fusion_ws_elems(B, D, C):
        raise MLAHipError(f"{who}: workspace of {ws.numel()} floats, fusion_ws_elems({B}, {D}, {C}) = {fusion_ws_elems(B, D, C)} needed")
    return B, D, C


_BC, _BD, _B2D, _DD, _2DD, _CD = ((lambda B, D, C: (B, C)), (lambda B, D, C: (B, D)), (lambda B, D, C: (B, 2 * D)),
                                  (lambda B, D, C: (D, D)), (lambda B, D, C: (2 * D, D)), (lambda B, D, C: (C, D)))
_vC, _vD, _v2D, _v1, _v3 = ((lambda B, D, C: (C,)), (lambda B, D, C: (D,)), (lambda B, D, C: (2 * D,)), (lambda B, D, C: (1,)),
                            (lambda B, D, C: (3,)))


def fusion_sum_ce_fwd_bwd(x, y, Wx, bx, Wy, by, labels, out, out_a, out_v, losses, dWx, dbx, dWy, dby, dX, dY, ws, inv_batch: float,
                          bias_scale: float = 1.0, stream: Optional[int] = None) -> None:
    """SumFusion training head (fusion_modules.py:11-13; main.py:292-295, 305-310): out, out_a / out_v (bias times `bias_scale`),
    losses [loss, loss_a, loss_v] and every gradient."""
    B, D, C = _fusion_dims("fusion_sum_ce_fwd_bwd", x, y, Wx, [(Wy, _CD), (out, _BC), (out_a, _BC), (out_v, _BC), (dWx, _CD), (dWy, _CD),
                                                               (dX, _BD), (dY, _BD), (bx, _vC), (by, _vC), (dbx, _vC), (dby, _vC),
                                                               (losses, _v3)], ws, labels)
    _call("mla_fusion_sum_ce_fwd_bwd", _p(x), _p(y), _p(Wx), _p(bx), _p(Wy), _p(by), _p(labels, torch.int64), _p(out), _p(out_a), _p(out_v),
          _p(losses), _p(dWx), _p(dbx), _p(dWy), _p(dby), _p(dX), _p(dY), _p(ws), B, D, C, inv_batch, bias_scale, stream or cur_stream())


def fusion_sum_fwd(x, y, Wx, bx, Wy, by, out, out_a, out_v, bias_scale: float = 1.0, stream: Optional[int] = None) -> None:
    """out = fc_x(x) + fc_y(y) and out_a / out_v with the bias times `bias_scale` (0.5 in valid(), main.py:610-614); no gradients."""
    B, D, C = _fusion_dims("fusion_sum_fwd", x, y, Wx, [(Wy, _CD), (out, _BC), (out_a, _BC), (out_v, _BC), (bx, _vC), (by, _vC)])
    _call("mla_fusion_sum_fwd", _p(x), _p(y), _p(Wx), _p(bx), _p(Wy), _p(by), _p(out), _p(out_a), _p(out_v), B, D, C, bias_scale,
          stream or cur_stream())


def fusion_sum_bwd(x, y, Wx, Wy, dlogits, dWx, dbx, dWy, dby, dX, dY, ws, scale: float = 1.0, stream: Optional[int] = None) -> None:
    """autograd of SumFusion for a given d out (all times `scale`)."""
    B, D, C = _fusion_dims("fusion_sum_bwd", x, y, Wx, [(Wy, _CD), (dlogits, _BC), (dWx, _CD), (dWy, _CD), (dX, _BD), (dY, _BD), (dbx, _vC),
                                                        (dby, _vC)], ws)
    _call("mla_fusion_sum_bwd", _p(x), _p(y), _p(Wx), _p(Wy), _p(dlogits), _p(dWx), _p(dbx), _p(dWy), _p(dby), _p(dX), _p(dY), _p(ws),
          B, D, C, scale, stream or cur_stream())


def fusion_film_ce_fwd_bwd(film, t, W, b, Wout, bout, labels, out, h, z, loss, dW, db, dWout, dbout, dfilm, dt, ws, inv_batch: float,
                           stream: Optional[int] = None) -> None:
    """FiLM training head (fusion_modules.py:53-67; main.py:305-310): out, h = fc(film) (gamma | beta), z, the loss and every gradient."""
    B, D, C = _fusion_dims("fusion_film_ce_fwd_bwd", film, t, Wout, [(W, _2DD), (out, _BC), (h, _B2D), (z, _BD), (dW, _2DD), (dWout, _CD),
                                                                     (dfilm, _BD), (dt, _BD), (b, _v2D), (bout, _vC), (db, _v2D),
                                                                     (dbout, _vC), (loss, _v1)], ws, labels)
    _call("mla_fusion_film_ce_fwd_bwd", _p(film), _p(t), _p(W), _p(b), _p(Wout), _p(bout), _p(labels, torch.int64), _p(out), _p(h), _p(z),
          _p(loss), _p(dW), _p(db), _p(dWout), _p(dbout), _p(dfilm), _p(dt), _p(ws), B, D, C, inv_batch, stream or cur_stream())


def fusion_film_fwd(film, t, W, b, Wout, bout, out, h, z, stream: Optional[int] = None) -> None:
    B, D, C = _fusion_dims("fusion_film_fwd", film, t, Wout, [(W, _2DD), (out, _BC), (h, _B2D), (z, _BD), (b, _v2D), (bout, _vC)])
    _call("mla_fusion_film_fwd", _p(film), _p(t), _p(W), _p(b), _p(Wout), _p(bout), _p(out), _p(h), _p(z), B, D, C, stream or cur_stream())


def fusion_film_bwd(film, t, W, Wout, h, z, dlogits, dW, db, dWout, dbout, dfilm, dt, ws, scale: float = 1.0,
                    stream: Optional[int] = None) -> None:
    """autograd of FiLM for a given d out (all times `scale`), from the forward's h and z."""
    B, D, C = _fusion_dims("fusion_film_bwd", film, t, Wout, [(W, _2DD), (h, _B2D), (z, _BD), (dlogits, _BC), (dW, _2DD), (dWout, _CD),
                                                              (dfilm, _BD), (dt, _BD), (db, _v2D), (dbout, _vC)], ws)
    _call("mla_fusion_film_bwd", _p(film), _p(t), _p(W), _p(Wout), _p(h), _p(z), _p(dlogits), _p(dW), _p(db), _p(dWout), _p(dbout),
          _p(dfilm), _p(dt), _p(ws), B, D, C, scale, stream or cur_stream())


def fusion_gated_ce_fwd_bwd(x, y, Wx, bx, Wy, by, Wout, bout, labels, out, hx, hy, z, loss, dWx, dbx, dWy, dby, dWout, dbout, dX, dY, ws,
                            x_gate: bool, inv_batch: float, stream: Optional[int] = None) -> None:
    """GatedFusion training head (fusion_modules.py:87-98; main.py:305-310): out, hx = fc_x(x), hy = fc_y(y), z, the loss and every
    gradient."""
    B, D, C = _fusion_dims("fusion_gated_ce_fwd_bwd", x, y, Wout, [(Wx, _DD), (Wy, _DD), (out, _BC), (hx, _BD), (hy, _BD), (z, _BD),
                                                                   (dWx, _DD), (dWy, _DD), (dWout, _CD), (dX, _BD), (dY, _BD),
                                                                   (bx, _vD), (by, _vD), (bout, _vC), (dbx, _vD), (dby, _vD), (dbout, _vC),
                                                                   (loss, _v1)], ws, labels)
    _call("mla_fusion_gated_ce_fwd_bwd", _p(x), _p(y), _p(Wx), _p(bx), _p(Wy), _p(by), _p(Wout), _p(bout), _p(labels, torch.int64), _p(out),
          _p(hx), _p(hy), _p(z), _p(loss), _p(dWx), _p(dbx), _p(dWy), _p(dby), _p(dWout), _p(dbout), _p(dX), _p(dY), _p(ws), B, D, C,
          int(bool(x_gate)), inv_batch, stream or cur_stream())


def fusion_gated_fwd(x, y, Wx, bx, Wy, by, Wout, bout, out, hx, hy, z, x_gate: bool, stream: Optional[int] = None) -> None:
    B, D, C = _fusion_dims("fusion_gated_fwd", x, y, Wout, [(Wx, _DD), (Wy, _DD), (out, _BC), (hx, _BD), (hy, _BD), (z, _BD), (bx, _vD), (by, _vD),
                                                            (bout, _vC)])
    _call("mla_fusion_gated_fwd", _p(x), _p(y), _p(Wx), _p(bx), _p(Wy), _p(by), _p(Wout), _p(bout), _p(out), _p(hx), _p(hy), _p(z), B, D, C,
          int(bool(x_gate)), stream or cur_stream())


def fusion_gated_bwd(x, y, Wx, Wy, Wout, hx, hy, z, dlogits, dWx, dbx, dWy, dby, dWout, dbout, dX, dY, ws, x_gate: bool,
                     scale: float = 1.0, stream: Optional[int] = None) -> None:
    """autograd of GatedFusion for a given d out (all times `scale`), from the forward's hx, hy and z."""
    B, D, C = _fusion_dims("fusion_gated_bwd", x, y, Wout, [(Wx, _DD), (Wy, _DD), (hx, _BD), (hy, _BD), (z, _BD), (dlogits, _BC),
                                                            (dWx, _DD), (dWy, _DD), (dWout, _CD), (dX, _BD), (dY, _BD), (dbx, _vD),
                                                            (dby, _vD), (dbout, _vC)], ws)
    _call("mla_fusion_gated_bwd", _p(x), _p(y), _p(Wx), _p(Wy), _p(Wout), _p(hx), _p(hy), _p(z), _p(dlogits), _p(dWx), _p(dbx), _p(dWy),
          _p(dby), _p(dWout), _p(dbout), _p(dX), _p(dY), _p(ws), B, D, C, int(bool(x_gate)), scale, stream or cur_stream())


def qmf_head_ws_elems(B: int, C: int, M: int) -> int:
    return int(_lib.load().mla_qmf_head_ws_elems(B, C, M))


def _qmf_ptrs(xs, Ws, bs, who: str):
    x, M, B, D = _concat_ptrs(xs, who)
    C = Ws[0].shape[0]
    if len(Ws) != M or len(bs) != M or any(tuple(W.shape) != (C, D) for W in Ws) or any(tuple(b.shape) != (C,) for b in bs):
        raise MLAHipError(f"{who}: needs {M} heads of shape ({C}, {D}) / ({C},); got {[tuple(W.shape) for W in Ws]}")
    pad = [None] * (3 - M)
    return x, [_p(W) for W in Ws] + pad, [_p(b) for b in bs] + pad, M, B, D, C


def qmf_head_fwd_bwd(xs, Ws, bs, labels, idx, correctness, confidence, z, out, conf, ell, target, margin, losses, dWs, dbs, dxs, ws,
                     w_cml: float, w_crl: float, inv_batch: float, stream: Optional[int] = None) -> None:
    """QMF training head (main.py:239-268 / 170-229): per-modality logits z (M, B, C), fused `out`, confidences, the History update
    (correctness / confidence: fp64 (M, n_data), updated in place), ranking targets / margins, losses [L, CE_m.., rank_m.., CE(out)]
    and every gradient."""
    x, W, b, M, B, D, C = _qmf_ptrs(xs, Ws, bs, "qmf_head_fwd_bwd")
    n_data = correctness.shape[1]
    if tuple(correctness.shape) != (M, n_data) or tuple(confidence.shape) != (M, n_data) or idx.numel() != B or labels.numel() != B:
        raise MLAHipError(f"qmf_head_fwd_bwd: history {tuple(correctness.shape)} / {tuple(confidence.shape)} must be ({M}, n_data), "
                          f"labels / idx must hold {B} entries")
    if len(dWs) != M or len(dbs) != M or len(dxs) != M or ws.numel() < qmf_head_ws_elems(B, C, M):
        raise MLAHipError("qmf_head_fwd_bwd: one dW / db / dX per modality and a workspace of qmf_head_ws_elems floats are needed")
    pad = [None] * (3 - M)
    dW, db, dx = [_p(t) for t in dWs] + pad, [_p(t) for t in dbs] + pad, [_p(t) for t in dxs] + pad
    _call("mla_qmf_head_fwd_bwd", *x, *W, *b, _p(labels, torch.int64), _p(idx, torch.int64), _p(correctness, torch.float64),
          _p(confidence, torch.float64), n_data, _p(z), _p(out), _p(conf), _p(ell), _p(target), _p(margin), _p(losses), *dW, *db, *dx,
          _p(ws), M, B, D, C, w_cml, w_crl, inv_batch, stream or cur_stream())


def qmf_head_fwd(xs, Ws, bs, z, out, conf, stream: Optional[int] = None) -> None:
    """z_m = fc_m(x_m), out = sum_m conf_m z_m, conf_m = logsumexp(z_m) / 10, no gradients (valid(), main.py:576-586)."""
    x, W, b, M, B, D, C = _qmf_ptrs(xs, Ws, bs, "qmf_head_fwd")
    _call("mla_qmf_head_fwd", *x, *W, *b, _p(z), _p(out), _p(conf), M, B, D, C, stream or cur_stream())


def scale_by_device_scalar(x, scalar, stream: Optional[int] = None) -> None:
    _call("mla_scale_by_device_scalar", _p(x), _p(scalar), x.numel(), stream or cur_stream())


def colsum(X, r, scale: float, stream: Optional[int] = None) -> None:
    B, D = X.shape
    _call("mla_colsum", _p(X), _p(r), B, D, scale, stream or cur_stream())


def gs_ws_elems(D: int, C: int) -> int:
    return int(_lib.load().mla_gs_ws_elems(D, C))


def gs_project(Pl, r, G, alpha: float, ws, stream: Optional[int] = None) -> None:
    D = Pl.shape[0]
    C = G.shape[0]
    _call("mla_gs_project", _p(Pl), _p(r), _p(G), D, C, alpha, _p(ws), stream or cur_stream())


def gs_owm_ws_elems(D: int, C: int) -> int:
    return int(_lib.load().mla_gs_owm_ws_elems(D, C))


def gs_project_owm(Pl, r, G, alpha: float, ws, stream: Optional[int] = None) -> None:
    """gs_mode="owm": k = Pl r, s = alpha + r . k, Pl <- Pl - k k^T / s, G <- G Pl^T, in place (include/mla_hip.h, mla_gs_project_owm)."""
    D = Pl.shape[0]
    C = G.shape[0]
    if tuple(Pl.shape) != (D, D) or r.numel() != D or G.dim() != 2 or G.shape[1] != D or ws.numel() < gs_owm_ws_elems(D, C):
        raise MLAHipError(f"gs_project_owm: Pl {tuple(Pl.shape)} / r {tuple(r.shape)} / G {tuple(G.shape)} / workspace {ws.numel()} "
                          f"do not match D={D}, C={C}")
    _call("mla_gs_project_owm", _p(Pl), _p(r), _p(G), D, C, alpha, _p(ws), stream or cur_stream())


def sgd_step(p, g, buf, lr: float, momentum: float, wd: float, first: bool, stream: Optional[int] = None) -> None:
    _call("mla_sgd_step", _p(p), _p(g), _p(buf), p.numel(), lr, momentum, wd, int(first), stream or cur_stream())


def feature_ws_elems(B: int, D: int, C: int) -> int:
    return int(_lib.load().mla_feature_ws_elems(B, D, C))


def feature_phase(X, labels, W, b, buf, Pl, logits, loss, ws, inv_batch: float, project: bool, alpha: float, lr: float,
                  momentum: float, wd: float, first: bool, stream: Optional[int] = None, owm: bool = False) -> None:
    """One head-only modality phase (main.py:432-442) on stored features, in place: logits / loss out; W (C, D), b (C), the
    momentum buffer `buf` over [W | b] and, when `project`, Pl (D, D) updated (see include/mla_hip.h, mla_feature_phase).
    owm: the projection is the scalar-denominator rule of gs_project_owm (mla_feature_phase_owm)."""
    if X.dim() != 2 or W.dim() != 2 or W.shape[1] != X.shape[1]:
        raise MLAHipError(f"feature_phase: X {tuple(X.shape)} {X.dtype} does not match the head weight {tuple(W.shape)}")
    B, D = X.shape
    C = W.shape[0]
    if labels.numel() != B or b.numel() != C or buf.numel() != C * D + C or tuple(logits.shape) != (B, C) or loss.numel() != 1 \
            or (project and (Pl is None or tuple(Pl.shape) != (D, D))) or (C <= 128 and ws.numel() < feature_ws_elems(B, D, C)):
        raise MLAHipError(f"feature_phase: labels {tuple(labels.shape)} / bias {tuple(b.shape)} / momentum {tuple(buf.shape)} / logits "
                          f"{tuple(logits.shape)} / Pl {None if Pl is None else tuple(Pl.shape)} / workspace {ws.numel()} do not match "
                          f"B={B}, D={D}, C={C}")
    _call("mla_feature_phase_owm" if owm else "mla_feature_phase", _p(X), _p(labels, torch.int64), _p(W), _p(b), _p(buf), _p(Pl), _p(logits), _p(loss), _p(ws), B, D, C,
          inv_batch, int(bool(project)), alpha, lr, momentum, wd, int(bool(first)), stream or cur_stream())


def gather_index_check(idx_host: torch.Tensor, N: int) -> None:
    """Refuse an index vector (host int64) with an entry outside [0, N) before it is uploaded (no GPU)."""
    if idx_host.is_cuda or idx_host.dtype != torch.int64 or not idx_host.is_contiguous():
        raise MLAHipError(f"gather index: expected a contiguous host int64 tensor, got {idx_host.dtype} on {idx_host.device}")
    _call("mla_gather_index_check", idx_host.data_ptr(), idx_host.numel(), N)


def gather_rows2(T0, T1, labels, idx, out0, out1, out_label, out_idx, stream: Optional[int] = None) -> None:
    """Rows idx (B) int64 of the device tables T0, T1 (N, D) fp32 and of labels (N) int64 -> out0, out1 (B, D), out_label (B),
    out_idx (B, 1), one launch (see include/mla_hip.h, mla_gather_rows2)."""
    if T0.dim() != 2 or tuple(T1.shape) != tuple(T0.shape) or labels.numel() != T0.shape[0]:
        raise MLAHipError(f"gather_rows2: tables {tuple(T0.shape)} / {tuple(T1.shape)} / labels {tuple(labels.shape)} do not match (N, D)")
    N, D = T0.shape
    B = idx.numel()
    if tuple(out0.shape) != (B, D) or tuple(out1.shape) != (B, D) or out_label.numel() != B or out_idx.numel() != B:
        raise MLAHipError(f"gather_rows2: outputs {tuple(out0.shape)} / {tuple(out1.shape)} / {tuple(out_label.shape)} / "
                          f"{tuple(out_idx.shape)} do not match B={B}, D={D}")
    _call("mla_gather_rows2", _p(T0), _p(T1), _p(labels, torch.int64), _p(idx, torch.int64), _p(out0), _p(out1), _p(out_label, torch.int64),
          _p(out_idx, torch.int64), N, D, B, stream or cur_stream())


def adam_step(p, g, m, v, lr: float, beta1: float, beta2: float, eps: float, wd: float, step: int,
              stream: Optional[int] = None) -> None:
    """torch.optim.Adam's single-tensor rule on one flat range (any 4-byte-aligned start); g None = zero gradient."""
    if not (p.numel() == m.numel() == v.numel() and (g is None or g.numel() == p.numel())):
        raise MLAHipError("adam_step: p, g, m and v must have the same number of elements")
    _call("mla_adam_step", _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, wd, int(step), stream or cur_stream())


# ---- transformer encoders (M3AE / CAV-MAE) -----------------------------------------------------------
LN_EPS = 1e-5     # nn.LayerNorm default (models/m3ae.py:138)


def linear_fwd(x, w_kn, bias, y, groups: int, rows: int, K: int, N: int, x_group_rows: Optional[int] = None, x_off: int = 0,
               y_group_rows: Optional[int] = None, y_off: int = 0, residual=None, y_gelu=None, stream: Optional[int] = None,
               wsplit=None, bf16: bool = False):
    """y[g][y_off+r] = x[g][x_off+r] @ w_kn (+bias) (+residual); y_gelu (optional) also receives gelu(y).
    wsplit: conv2d_wsplit(w_kn.view(1, 1, K, N), True) selects the split-bf16 arithmetic; with bf16=True it is
    conv2d_wimage_bf16(w_kn.view(1, 1, K, N), True) and selects the single-product bf16 arithmetic."""
    if bf16 and wsplit is None:
        raise MLAHipError("linear_fwd: bf16 needs the weight image (conv2d_wimage_bf16)")
    if wsplit is not None:
        _call("mla_linear_fwd_bf16" if bf16 else "mla_linear_fwd_split", _p(x), _p(wsplit, torch.int16), _p(bias), _p(residual), _p(y), _p(y_gelu), groups, rows, x_group_rows or rows,
              x_off, y_group_rows or rows, y_off, K, N, stream or cur_stream())
        return
    _call("mla_linear_fwd", _p(x), _p(w_kn), _p(bias), _p(residual), _p(y), _p(y_gelu), groups, rows, x_group_rows or rows, x_off,
          y_group_rows or rows, y_off, K, N, stream or cur_stream())


def linear_dgrad(dy, w_kn, dx, wt_ws, groups: int, rows: int, K: int, N: int, residual=None, gelu_src=None,
                 stream: Optional[int] = None, wsplit=None, bf16: bool = False):
    """dx = dy @ w_kn^T (+residual) (* gelu'(gelu_src)); dense rows.  wsplit: conv2d_wsplit(w_kn.view(1, 1, K, N), False), or with
    bf16=True conv2d_wimage_bf16(w_kn.view(1, 1, K, N), False)."""
    if bf16 and wsplit is None:
        raise MLAHipError("linear_dgrad: bf16 needs the weight image (conv2d_wimage_bf16)")
    if wsplit is not None:
        _call("mla_linear_dgrad_bf16" if bf16 else "mla_linear_dgrad_split", _p(dy), _p(wsplit, torch.int16), _p(dx), _p(residual), _p(gelu_src), groups, rows, rows, 0, rows, 0, K, N,
              stream or cur_stream())
        return
    _call("mla_linear_dgrad", _p(dy), _p(w_kn), _p(dx), _p(residual), _p(gelu_src), _p(wt_ws), groups, rows, rows, 0, rows, 0, K, N,
          stream or cur_stream())


def linear_wgrad_ws_bytes(M: int, K: int, N: int, split: bool = False, bf16: bool = False) -> int:
    if bf16:
        return int(_lib.load().mla_linear_wgrad_ws_bytes_bf16(M, K, N))
    if split:
        return int(_lib.load().mla_linear_wgrad_split_ws_bytes(M, K, N))
    return int(_lib.load().mla_linear_wgrad_ws_bytes(M, K, N))


def linear_wgrad(x, dy, dw_kn, ws, groups: int, rows: int, K: int, N: int, x_group_rows: Optional[int] = None, x_off: int = 0,
                 stream: Optional[int] = None, split: bool = False, dbias: Optional[torch.Tensor] = None, bf16: bool = False):
    """dw_kn = x^T dy (K, N).  split (or bf16) + dbias: the bias gradient (column sums of dy, fp32) comes out of the same pass."""
    if split or bf16:
        _call("mla_linear_wgrad_bias_bf16" if bf16 else "mla_linear_wgrad_split_bias", _p(x), _p(dy), _p(dw_kn), _p(dbias), groups, rows, x_group_rows or rows, x_off, K, N, _p(ws),
              ws.numel() * ws.element_size(), stream or cur_stream())
        return
    if dbias is not None:
        raise MLAHipError("linear_wgrad: the fused bias gradient exists on the split arithmetic only (use colsum_rows)")
    _call("mla_linear_wgrad", _p(x), _p(dy), _p(dw_kn), groups, rows, x_group_rows or rows, x_off, K, N, _p(ws), ws.numel() * ws.element_size(),
          stream or cur_stream())


def colreduce_ws_elems(M: int, C: int) -> int:
    return int(_lib.load().mla_colreduce_ws_elems(M, C))


def colsum_rows(x, out, ws, M: int, C: int, stream: Optional[int] = None):
    _call("mla_colsum_rows", _p(x), _p(out), _p(ws), M, C, stream or cur_stream())


def layernorm_fwd(x, w, b, y, mean, rstd, M: int, D: int, eps: float = LN_EPS, stream: Optional[int] = None):
    _call("mla_layernorm_fwd", _p(x), _p(w), _p(b), _p(y), _p(mean), _p(rstd), M, D, eps, stream or cur_stream())


def layernorm_bwd(dy, x, w, mean, rstd, dx, dw, db, ws, M: int, D: int, add=None, stream: Optional[int] = None):
    _call("mla_layernorm_bwd", _p(dy), _p(x), _p(w), _p(mean), _p(rstd), _p(add), _p(dx), _p(dw), _p(db), _p(ws), M, D, stream or cur_stream())


def bgemm(A, B, C, batches: int, heads: int, M: int, N: int, K: int, a_strides, b_strides, c_strides, alpha: float = 1.0,
          a_off: int = 0, b_off: int = 0, c_off: int = 0, stream: Optional[int] = None):
    """C[z] = alpha * A[z] @ B[z]; strides in elements (batch, head, row, col-or-k); *_off: element offsets into the buffers."""
    L4 = ctypes.c_long * 4
    sa, sb, sc = L4(*a_strides), L4(*b_strides), L4(*c_strides)      # keep alive across the call (no temporaries!)
    pa, pb, pc = _p(A) + 4 * a_off, _p(B) + 4 * b_off, _p(C) + 4 * c_off
    if min(a_off, b_off, c_off) < 0 or a_off >= A.numel() or b_off >= B.numel() or c_off >= C.numel():
        raise MLAHipError("bgemm: element offset outside its buffer")
    _call("mla_bgemm", pa, pb, pc, batches, heads, M, N, K, ctypes.addressof(sa), ctypes.addressof(sb), ctypes.addressof(sc), A.numel() - a_off,
          B.numel() - b_off, C.numel() - c_off, alpha, stream or cur_stream())


def softmax_fwd(S, pad_mask, B: int, H: int, n: int, stream: Optional[int] = None):
    _call("mla_softmax_fwd", _p(S), _p(pad_mask), B, H, n, stream or cur_stream())


def softmax_bwd(P, dP, B: int, H: int, n: int, stream: Optional[int] = None):
    _call("mla_softmax_bwd", _p(P), _p(dP), B, H, n, stream or cur_stream())


ATTENTION_MATHS = ("f32", "split")


def _attention_symbol(base: str, math: str) -> str:
    """math "f32": the fp32-MFMA kernels (attention.hip); "split": the same kernels on the exact three-way bf16 split
    (attention_split.hip), fp32-equivalent."""
    if math not in ATTENTION_MATHS:
        raise MLAHipError(f"attention math must be 'f32' or 'split', got {math!r}")
    return base if math == "f32" else base + "_split"


def attention_fwd(qkv, pad_mask, o, lse, B: int, H: int, n: int, hd: int, stream: Optional[int] = None, math: str = "f32"):
    """o = softmax(mask(q k^T * hd^-0.5)) v, fused (models/m3ae.py:102-125); lse (B, H, n) is kept for the backward."""
    _call(_attention_symbol("mla_attention_fwd", math), _p(qkv), _p(pad_mask), _p(o), _p(lse), B, H, n, hd, stream or cur_stream())


def attention_bwd(do, qkv, o, lse, pad_mask, dqkv, dvec, B: int, H: int, n: int, hd: int, stream: Optional[int] = None,
                  math: str = "f32"):
    _call(_attention_symbol("mla_attention_bwd", math), _p(do), _p(qkv), _p(o), _p(lse), _p(pad_mask), _p(dqkv), _p(dvec), B, H, n, hd,
          stream or cur_stream())


def tokens_assemble(x0, table, ids, pos, type_emb, cls, B: int, L: int, D: int, stream: Optional[int] = None):
    V = table.shape[0] if table is not None else 0
    _call("mla_tokens_assemble", _p(x0), _p(table), _p(ids, torch.int64), _p(pos), _p(type_emb), _p(cls), B, L, D, V, stream or cur_stream())


def tokens_assemble_bwd_ws_bytes(B: int, L: int, D: int) -> int:
    return int(_lib.load().mla_tokens_assemble_bwd_ws_bytes(B, L, D))


def tokens_assemble_bwd(dx0, colsum_all, ids, dcls, dtype, dtable, B: int, L: int, D: int, stream: Optional[int] = None,
                        ws: Optional[torch.Tensor] = None):
    """ws (uint8, >= tokens_assemble_bwd_ws_bytes): scratch of the deterministic embedding scatter (text path only)."""
    V = dtable.shape[0] if dtable is not None else 0
    if dtable is not None and ws is None:
        ws = torch.empty(tokens_assemble_bwd_ws_bytes(B, L, D), device=dx0.device, dtype=torch.uint8)
    _call("mla_tokens_assemble_bwd", _p(dx0), _p(colsum_all), _p(ids, torch.int64), _p(dcls), _p(dtype), _p(dtable), B, L, D, V,
          _p(ws, torch.uint8) if ws is not None else None, ws.numel() if ws is not None else 0, stream or cur_stream())


def patchify(img, out, P: int = 16, transposed_hw: Optional[tuple] = None, stream: Optional[int] = None):
    """img (B,C,H,W) -> out (B*(H/P)*(W/P), C*P*P).  transposed_hw=(H, W): img is stored (B, W, H) with C == 1."""
    if transposed_hw is None:
        B, C, H, W = img.shape
        tr = 0
    else:
        B, C = img.shape[0], 1
        H, W = transposed_hw
        tr = 1
    _call("mla_patchify", _p(img), _p(out), B, C, H, W, P, tr, stream or cur_stream())


# ---- evaluation path ------------------------------------------------------------------------------------
def head_logits(X, W, b, logits, stream: Optional[int] = None):
    B, D = X.shape
    _call("mla_head_logits", _p(X), _p(W), _p(b), _p(logits), B, D, W.shape[0], stream or cur_stream())


def _padded(tensors, n: int, alphas=()):
    """What a C entry point with n pointer slots and three alpha slots takes: the tensors' pointers, then None up to n (a list longer
    than n is cut: the entry point refuses its count); the alphas as floats, then 0.0 up to three."""
    return ([_p(t) for t in tensors] + [None] * n)[:n], ([float(v) for v in alphas] + [0.0] * 3)[:3]


def eval_fuse(outs, labels, counts, weights_out, dynamic: bool, alphas, stream: Optional[int] = None):
    M = len(outs)
    B, C = outs[0].shape
    o, al = _padded(outs, 3, alphas)
    _call("mla_eval_fuse", *o, _p(labels, torch.int64), _p(counts, torch.int32), _p(weights_out), M, B, C, int(dynamic), *al,
          stream or cur_stream())


def eval_head(feats, W, b, labels, counts, logits_out, *, mode: int, alphas, present=None, fused_out=None, weights_out=None,
              pred_out=None, stream: Optional[int] = None):
    """One batch from features to counters in one launch with per-SAMPLE fusion weights (see include/mla_hip.h, mla_eval_head).
    feats: M = 2 or 3 (B, D) feature matrices; W (C, D), b (C): the shared head; counts int32 (C * (2 + M)), accumulated;
    logits_out (M, B, C).  mode 0: the fixed `alphas`; mode 1: entropy gating of each row.  present: device uint8 (B, M) or None.
    fused_out (B, C), weights_out (B, M), pred_out int32 (B, 1 + M): optional per-row outputs."""
    M = len(feats)
    if M < 1 or feats[0].dim() != 2 or W.dim() != 2:
        raise MLAHipError(f"eval_head: expected M (B, D) feature matrices and a (C, D) head weight, got {M} and {tuple(W.shape)}")
    B, D = feats[0].shape
    C = W.shape[0]
    if any(tuple(f.shape) != (B, D) for f in feats) or W.shape[1] != D or tuple(b.shape) != (C,):
        raise MLAHipError(f"eval_head: features {[tuple(f.shape) for f in feats]} / bias {tuple(b.shape)} do not match the head weight "
                          f"{tuple(W.shape)}")
    _want("eval_head", labels=(labels, (B,)), counts=(counts, (C * (2 + M),)), logits_out=(logits_out, (M, B, C)),
          present=(present, (B, M)), fused_out=(fused_out, (B, C)), weights_out=(weights_out, (B, M)), pred_out=(pred_out, (B, 1 + M)))
    x, al = _padded(feats, 3, alphas)
    _call("mla_eval_head", *x, _p(W), _p(b), _p(labels, torch.int64), _p(present, torch.uint8), _p(counts, torch.int32),
          _p(logits_out), _p(fused_out), _p(weights_out), _p(pred_out, torch.int32), M, B, D, C, int(mode), *al, stream or cur_stream())


def _store_shape(who: str, scores, pred, labels):
    """(H, C, cap) of a score store (see include/mla_hip.h, mla_scores_append); pred may be None."""
    if scores.dim() != 3 or (pred is not None and tuple(pred.shape) != (scores.shape[0], scores.shape[2])) \
            or tuple(labels.shape) != (scores.shape[2],):
        raise MLAHipError(f"{who}: expected scores (H, C, cap), pred (H, cap) and labels (cap), got {tuple(scores.shape)}, "
                          f"{None if pred is None else tuple(pred.shape)} and {tuple(labels.shape)}")
    return tuple(scores.shape)


def scores_append(logits, labels, scores, pred, store_labels, pos: int, weights=None, stream: Optional[int] = None):
    """Rows pos .. pos + B - 1 of a score store from one batch, in one launch: class-major softmax scores (H, C, cap), the arg-max
    of the logits (H, cap) and the labels (cap).  logits: the H (B, C) matrices, fused first; with `weights` (a device vector of
    H - 1 floats, what eval_fuse wrote) logits[0] is None and head 0 is formed as eval_fuse forms it."""
    H, C, cap = _store_shape("scores_append", scores, pred, store_labels)
    if len(logits) != H or H > 4 or any(t is not None and (t.dim() != 2 or t.shape[1] != C) for t in logits):
        raise MLAHipError(f"scores_append: expected {H} (B, {C}) logit matrices for a store of {H} heads (at most 4), got "
                          f"{[None if t is None else tuple(t.shape) for t in logits]}")
    B = labels.shape[0]
    if any(t is not None and t.shape[0] != B for t in logits) or (weights is not None and weights.numel() < H - 1):
        raise MLAHipError(f"scores_append: {B} labels for logits {[None if t is None else tuple(t.shape) for t in logits]}, weights "
                          f"{None if weights is None else tuple(weights.shape)}")
    _call("mla_scores_append", *_padded(logits, 4)[0], _p(weights), _p(labels, torch.int64), _p(scores), _p(pred, torch.int32),
          _p(store_labels, torch.int32), H, B, C, int(pos), cap, stream or cur_stream())


def metrics_ws_bytes(cap: int, H: int) -> int:
    return int(_lib.load().mla_metrics_ws_bytes(cap, H))


def average_precision(scores, labels, N: int, ap, npos, ws, stream: Optional[int] = None):
    """ap float64 (H, C) and npos int32 (C) over the first N rows of scores (H, C, cap) / labels int32 (cap); ws: float64 (H, cap),
    holds the per-row terms afterwards.  See include/mla_hip.h, mla_average_precision."""
    H, C, cap = _store_shape("average_precision", scores, None, labels)
    if tuple(ap.shape) != (H, C) or tuple(npos.shape) != (C,) or ws.numel() * 8 < metrics_ws_bytes(cap, H):
        raise MLAHipError(f"average_precision: ap {tuple(ap.shape)} / npos {tuple(npos.shape)} / ws {tuple(ws.shape)} do not fit "
                          f"scores {tuple(scores.shape)}")
    _call("mla_average_precision", _p(scores), _p(labels, torch.int32), int(N), cap, H, C, _p(ap, torch.float64), _p(npos, torch.int32),
          _p(ws, torch.float64), stream or cur_stream())


def confusion_count(pred, labels, N: int, conf, stream: Optional[int] = None):
    """conf int32 (H, C, C) [true][predicted], accumulated, over the first N rows of pred int32 (H, cap) / labels int32 (cap)."""
    if pred.dim() != 2 or tuple(labels.shape) != (pred.shape[1],) or conf.dim() != 3 or conf.shape[0] != pred.shape[0] \
            or conf.shape[1] != conf.shape[2]:
        raise MLAHipError(f"confusion_count: expected pred (H, cap), labels (cap) and conf (H, C, C), got {tuple(pred.shape)}, "
                          f"{tuple(labels.shape)} and {tuple(conf.shape)}")
    H, cap = pred.shape
    _call("mla_confusion_count", _p(pred, torch.int32), _p(labels, torch.int32), int(N), cap, H, conf.shape[1], _p(conf, torch.int32),
          stream or cur_stream())


def fusion_sweep(outs, labels, grid, tp, pp, num=None, present=None, stream: Optional[int] = None):
    """The fixed-weight fusion of one batch at every point of a grid of fusion weights, in one launch (see include/mla_hip.h,
    mla_fusion_sweep).  outs: M = 2 or 3 (B, C) logit matrices; grid: device fp32 (G, M); tp, pp int32 (G, C) and num int32 (C) or
    None, accumulated; present: device uint8 (B, M) or None."""
    M = len(outs)
    if M < 1 or outs[0].dim() != 2 or grid.dim() != 2:
        raise MLAHipError(f"fusion_sweep: expected M (B, C) logit matrices and a (G, M) grid, got {M} and {tuple(grid.shape)}")
    B, C = outs[0].shape
    G = grid.shape[0]
    if any(tuple(t.shape) != (B, C) for t in outs) or grid.shape[1] != M:
        raise MLAHipError(f"fusion_sweep: logits {[tuple(t.shape) for t in outs]} do not match each other or the grid {tuple(grid.shape)}")
    _want("fusion_sweep", labels=(labels, (B,)), tp=(tp, (G, C)), pp=(pp, (G, C)), num=(num, (C,)), present=(present, (B, M)))
    _call("mla_fusion_sweep", *_padded(outs, 3)[0], _p(labels, torch.int64), _p(present, torch.uint8), _p(grid), _p(tp, torch.int32),
          _p(pp, torch.int32), _p(num, torch.int32), M, B, C, G, stream or cur_stream())


def gate_sweep(outs, labels, grid, tp, pp, num=None, present=None, ent_out=None, stream: Optional[int] = None):
    """The gated fusion w_m ~ a_m exp(-beta H_m) of one batch at every gate of a grid, in one launch (see include/mla_hip.h,
    mla_gate_sweep).  outs: M = 2 or 3 (B, C) logit matrices; grid: device fp32 (G, M + 1), row = (a_0 .. a_{M-1}, beta), inside the
    contract on a gate (mla_hip.gate.check_gate_grid); tp, pp int32 (G, C) and num int32 (C) or None, accumulated; present: device
    uint8 (B, M) or None; ent_out: fp32 (B, M) or None, receives the entropies."""
    M = len(outs)
    if M < 1 or outs[0].dim() != 2 or grid.dim() != 2:
        raise MLAHipError(f"gate_sweep: expected M (B, C) logit matrices and a (G, M + 1) grid, got {M} and {tuple(grid.shape)}")
    B, C = outs[0].shape
    G = grid.shape[0]
    if any(tuple(t.shape) != (B, C) for t in outs) or grid.shape[1] != M + 1:
        raise MLAHipError(f"gate_sweep: logits {[tuple(t.shape) for t in outs]} do not match each other or the grid {tuple(grid.shape)}")
    _want("gate_sweep", labels=(labels, (B,)), tp=(tp, (G, C)), pp=(pp, (G, C)), num=(num, (C,)), present=(present, (B, M)),
          ent_out=(ent_out, (B, M)))
    _call("mla_gate_sweep", *_padded(outs, 3)[0], _p(labels, torch.int64), _p(present, torch.uint8), _p(grid), _p(tp, torch.int32),
          _p(pp, torch.int32), _p(num, torch.int32), _p(ent_out), M, B, C, G, stream or cur_stream())


def gate_sweep_tile(rows: int = -1) -> int:
    """The batch rows a gate_sweep workgroup stages at a time: 1, 2 or 4 sets it, anything else queries (scripts/bench_gate_sweep.py)."""
    return int(_lib.load().mla_gate_sweep_tile(int(rows)))


def eval_head_gated(feats, W, b, labels, counts, logits_out, *, prior, beta: float, present=None, fused_out=None, weights_out=None,
                    pred_out=None, stream: Optional[int] = None):
    """ops.eval_head under the gate (prior (M floats), beta): w_m ~ prior_m exp(-beta H_m) per row (see include/mla_hip.h,
    mla_eval_head_gated).  Every other argument is eval_head's."""
    M = len(feats)
    if M < 1 or feats[0].dim() != 2 or W.dim() != 2 or len(prior) != M:
        raise MLAHipError(f"eval_head_gated: expected M (B, D) feature matrices, a (C, D) head weight and M priors, got {M}, "
                          f"{tuple(W.shape)} and {len(prior)}")
    B, D = feats[0].shape
    C = W.shape[0]
    if any(tuple(f.shape) != (B, D) for f in feats) or W.shape[1] != D or tuple(b.shape) != (C,):
        raise MLAHipError(f"eval_head_gated: features {[tuple(f.shape) for f in feats]} / bias {tuple(b.shape)} do not match the head "
                          f"weight {tuple(W.shape)}")
    _want("eval_head_gated", labels=(labels, (B,)), counts=(counts, (C * (2 + M),)), logits_out=(logits_out, (M, B, C)),
          present=(present, (B, M)), fused_out=(fused_out, (B, C)), weights_out=(weights_out, (B, M)), pred_out=(pred_out, (B, 1 + M)))
    x, pr = _padded(feats, 3, prior)
    _call("mla_eval_head_gated", *x, _p(W), _p(b), _p(labels, torch.int64), _p(present, torch.uint8), _p(counts, torch.int32),
          _p(logits_out), _p(fused_out), _p(weights_out), _p(pred_out, torch.int32), M, B, D, C, *pr, float(beta), stream or cur_stream())


def bn_invstd(var, invstd, eps: float = BN_EPS, stream: Optional[int] = None):
    _call("mla_bn_invstd", _p(var), _p(invstd), var.numel(), eps, stream or cur_stream())


# ---- OGM / OGM-GE gradient modulation (main.py:312-410) ---------------------------------------------------------------------
def ogm_coeff(outs, labels, alpha: float, coeff, info=None, stream: Optional[int] = None):
    M = len(outs)
    B, C = outs[0].shape
    ptrs = [_p(t) for t in outs] + [None] * (3 - M)
    _call("mla_ogm_coeff", ptrs[0], ptrs[1], ptrs[2], _p(labels, torch.int64), M, B, C, alpha, _p(coeff), _p(info), stream or cur_stream())


def ogm_chunk_elems() -> int:
    return int(_lib.load().mla_ogm_chunk_elems())


def ogm_ws_bytes(total_chunks: int, n_seg: int) -> int:
    return int(_lib.load().mla_ogm_ws_bytes(total_chunks, n_seg))


def ogm_modulate(grad, seg_desc, first_chunk, n_seg: int, total_chunks: int, coeff, ge: bool, seed: int, step: int, ws,
                 stream: Optional[int] = None):
    _call("mla_ogm_modulate", _p(grad), _p(seg_desc, torch.int64), _p(first_chunk, torch.int32), n_seg, total_chunks, _p(coeff), int(ge), seed, step,
          _p(ws, torch.uint8) if ws is not None else None, ws.numel() if ws is not None else 0, stream or cur_stream())


# ---- CREMA-D frame augmentation (dataset/dataset.py:128-153) --------------------------------------------------------------
def _desc_host(desc_host: torch.Tensor) -> torch.Tensor:
    if desc_host.is_cuda or desc_host.dtype != torch.int64 or desc_host.dim() != 2 or desc_host.shape[1] != 8 \
            or not desc_host.is_contiguous():
        raise MLAHipError(f"frame descriptors: expected a contiguous host int64 (N, 8) tensor, got {desc_host.dtype} "
                          f"{tuple(desc_host.shape)} on {desc_host.device}")
    return desc_host


def frames_check(desc_host: torch.Tensor, B: int, T: int, frames_bytes: int, out_h: int = 224, out_w: int = 224) -> None:
    """The host checks of frames_resample alone (no GPU): raises MLAHipError on a descriptor the kernel must not run."""
    d = _desc_host(desc_host)
    _call("mla_frames_check", d.data_ptr(), d.shape[0], B, T, frames_bytes, out_h, out_w)


def frames_resample(frames: torch.Tensor, desc: torch.Tensor, desc_host: torch.Tensor, lut: torch.Tensor, out: torch.Tensor,
                    T: int, stream: Optional[int] = None) -> torch.Tensor:
    """frames uint8 (device, packed HWC frames), desc int64 (N, 8) on the device and the same table on the host, lut fp32 (3, 256)
    -> out fp32 (B, 3, T, out_h, out_w) (see include/mla_hip.h, mla_frames_resample)."""
    d = _desc_host(desc_host)
    if tuple(desc.shape) != tuple(d.shape):
        raise MLAHipError(f"frame descriptors: device table {tuple(desc.shape)} and host table {tuple(d.shape)} differ")
    if tuple(lut.shape) != (3, 256) or out.dim() != 5 or out.shape[1] != 3 or out.shape[2] != T:
        raise MLAHipError(f"frames_resample: lut {tuple(lut.shape)} / out {tuple(out.shape)} do not match (3, 256) / (B, 3, {T}, H, W)")
    B, _, _, OH, OW = out.shape
    _call("mla_frames_resample", _p(frames, torch.uint8), frames.numel(), _p(desc, torch.int64), d.data_ptr(), _p(lut), _p(out), d.shape[0], B, T, OH,
          OW, stream or cur_stream())
    return out


# ---- CAV-MAE batch feed (dataset/dataset.py:251-256, 281-294, 303-321) -----------------------------------------------------
def _table_host(t: torch.Tensor, cols: int, what: str) -> torch.Tensor:
    if t.is_cuda or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous():
        raise MLAHipError(f"{what}: expected a contiguous host int64 (N, {cols}) tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def image_check(desc_host: torch.Tensor, B: int, T: int, frames_bytes: int, out_h: int = 224, out_w: int = 224, filter: int = 1) -> None:
    """The host checks of image_resample alone (no GPU): raises MLAHipError on a descriptor the kernel must not run."""
    d = _table_host(desc_host, 12, "image descriptors")
    _call("mla_image_check", d.data_ptr(), d.shape[0], B, T, frames_bytes, out_h, out_w, filter)


def image_resample(frames: torch.Tensor, desc: torch.Tensor, desc_host: torch.Tensor, lut: torch.Tensor, out: torch.Tensor,
                   T: int, filter: int = 1, stream: Optional[int] = None) -> torch.Tensor:
    """frames uint8 (device, packed HWC frames), desc int64 (N, 12) on the device and the same table on the host, lut fp32 (3, 256)
    -> out fp32 (B, 3, T, out_h, out_w); filter 0 = bilinear, 1 = bicubic (see include/mla_hip.h, mla_image_resample)."""
    d = _table_host(desc_host, 12, "image descriptors")
    if tuple(desc.shape) != tuple(d.shape):
        raise MLAHipError(f"image descriptors: device table {tuple(desc.shape)} and host table {tuple(d.shape)} differ")
    if tuple(lut.shape) != (3, 256) or out.dim() != 5 or out.shape[1] != 3 or out.shape[2] != T:
        raise MLAHipError(f"image_resample: lut {tuple(lut.shape)} / out {tuple(out.shape)} do not match (3, 256) / (B, 3, {T}, H, W)")
    B, _, _, OH, OW = out.shape
    _call("mla_image_resample", _p(frames, torch.uint8), frames.numel(), _p(desc, torch.int64), d.data_ptr(), _p(lut), _p(out), d.shape[0], B, T,
          OH, OW, filter, stream or cur_stream())
    return out


# ---- M3AE / Food-101 train image transform (dataset/dataset.py:401-412) ------------------------------------------------------
def image_augment_check(desc_host: torch.Tensor, jitter_host: torch.Tensor, frames_bytes: int, out_h: int = 256, out_w: int = 256,
                        staging_bytes: Optional[int] = None, partials_count: Optional[int] = None) -> None:
    """The host checks of image_augment alone (no GPU): raises MLAHipError on tables or buffer sizes the kernels must not run with.
    staging_bytes / partials_count default to the sizes that always suffice (N * out_h * out_w * 3, N * out_h)."""
    d, j = _table_host(desc_host, 12, "image descriptors"), _table_host(jitter_host, 7, "jitter descriptors")
    if j.shape[0] != d.shape[0]:
        raise MLAHipError(f"image_augment: {d.shape[0]} image descriptors but {j.shape[0]} jitter descriptors")
    N = d.shape[0]
    _call("mla_image_augment_check", d.data_ptr(), j.data_ptr(), N, frames_bytes, out_h, out_w,
          N * out_h * out_w * 3 if staging_bytes is None else staging_bytes, N * out_h if partials_count is None else partials_count)


def image_augment(frames: torch.Tensor, desc: torch.Tensor, desc_host: torch.Tensor, jitter: torch.Tensor, jitter_host: torch.Tensor,
                  lut: torch.Tensor, out: torch.Tensor, staging: torch.Tensor, partials: torch.Tensor,
                  stream: Optional[int] = None) -> torch.Tensor:
    """frames uint8 (device, packed HWC frames), desc int64 (N, 12) and jitter int64 (N, 7), each on the device and the same table
    on the host, lut fp32 (3, 256) -> out fp32 (N, 3, 1, out_h, out_w): crop, bicubic resize, flip, ColorJitter, LUT.  staging uint8
    and partials int64 are device work buffers (see include/mla_hip.h, mla_image_augment)."""
    d, j = _table_host(desc_host, 12, "image descriptors"), _table_host(jitter_host, 7, "jitter descriptors")
    if tuple(desc.shape) != tuple(d.shape) or tuple(jitter.shape) != tuple(j.shape) or j.shape[0] != d.shape[0]:
        raise MLAHipError(f"image_augment: device tables {tuple(desc.shape)}, {tuple(jitter.shape)} and host tables {tuple(d.shape)}, "
                          f"{tuple(j.shape)} differ")
    if tuple(lut.shape) != (3, 256) or out.dim() != 5 or tuple(out.shape[:3]) != (d.shape[0], 3, 1):
        raise MLAHipError(f"image_augment: lut {tuple(lut.shape)} / out {tuple(out.shape)} do not match (3, 256) / ({d.shape[0]}, 3, 1, H, W)")
    N, _, _, OH, OW = out.shape
    _call("mla_image_augment", _p(frames, torch.uint8), frames.numel(), _p(desc, torch.int64), d.data_ptr(), _p(jitter, torch.int64),
          j.data_ptr(), _p(lut), _p(out), _p(staging, torch.uint8), staging.numel(), _p(partials, torch.int64), partials.numel(), N, OH, OW,
          stream or cur_stream())
    return out


def fbank_check(desc_host: torch.Tensor, T: int = 1024, F: int = 128, std: float = 4.4849) -> None:
    """The host checks of fbank_augment alone (no GPU): raises MLAHipError on a descriptor the kernel must not run, or std == 0."""
    d = _table_host(desc_host, 8, "fbank descriptors")
    if not float(std) != 0.0:                # 0 and NaN
        raise MLAHipError(f"fbank: std {std} (std == 0 or NaN)")
    _call("mla_fbank_check", d.data_ptr(), d.shape[0], T, F)


def fbank_augment(x: torch.Tensor, out: torch.Tensor, desc: torch.Tensor, desc_host: torch.Tensor, mean: float, std: float, seed: int,
                  stream: Optional[int] = None) -> torch.Tensor:
    """x fp32 (B, T, F) -> out (another buffer): SpecAug masks, (x - mean) / std, Philox noise and roll per the descriptor rows
    int64 (B, 8), on the device and the same table on the host (see include/mla_hip.h, mla_fbank_augment)."""
    d = _table_host(desc_host, 8, "fbank descriptors")
    if x.dim() != 3 or tuple(out.shape) != tuple(x.shape) or tuple(desc.shape) != (x.shape[0], 8) or d.shape[0] != x.shape[0]:
        raise MLAHipError(f"fbank_augment: x {tuple(x.shape)} / out {tuple(out.shape)} / descriptors {tuple(desc.shape)}, {tuple(d.shape)} do not "
                          "match (B, T, F) / (B, T, F) / (B, 8)")
    B, T, F = x.shape
    _call("mla_fbank_augment", _p(x), _p(out), _p(desc, torch.int64), d.data_ptr(), B, T, F, mean, std, int(seed) & 0xFFFFFFFFFFFFFFFF,
          stream or cur_stream())
    return out


# ---- Modal3Dataset missing-modality masks (dataset/dataset.py:794-801) --------------------------------------------------------
def modal3_assemble_check(mask_desc_host: torch.Tensor, P: int, S: int = 256, TF: int = 1024 * 128, L: int = 256) -> None:
    """The size and table checks of modal3_assemble alone (no GPU): raises MLAHipError on a mask table the kernel must not run."""
    d = _table_host(mask_desc_host, 4, "mask descriptors")
    _call("mla_modal3_assemble_check", d.data_ptr(), d.shape[0], P, S, TF, L)


def modal3_assemble(image_compact: Optional[torch.Tensor], spec: torch.Tensor, token: torch.Tensor, pm: torch.Tensor,
                    mask_desc: torch.Tensor, mask_desc_host: torch.Tensor, image_out: torch.Tensor,
                    stream: Optional[int] = None) -> torch.Tensor:
    """image_compact fp32 (P, 3, S, S) (None when no sample has an image) -> image_out fp32 (B, 3, S, S): row b is the compact
    image of its slot, or zeros; spec fp32 (B, ...), token int64 (B, ...) and pm fp32 (B, ...) get the rows of absent modalities
    zeroed in place.  mask_desc int64 (B, 4) (audio, image, text present, image slot) on the device and the same table on the host
    (see include/mla_hip.h, mla_modal3_assemble)."""
    d = _table_host(mask_desc_host, 4, "mask descriptors")
    B = d.shape[0]
    P = 0 if image_compact is None else image_compact.shape[0]
    if tuple(mask_desc.shape) != tuple(d.shape):
        raise MLAHipError(f"mask descriptors: device table {tuple(mask_desc.shape)} and host table {tuple(d.shape)} differ")
    if B == 0 or image_out.dim() != 4 or tuple(image_out.shape[:2]) != (B, 3) or image_out.shape[2] != image_out.shape[3] \
            or (P and image_compact.numel() != P * image_out[0].numel()) or spec.shape[0] != B or token.shape[0] != B \
            or tuple(pm.shape) != tuple(token.shape):
        raise MLAHipError(f"modal3_assemble: image_compact {None if image_compact is None else tuple(image_compact.shape)} / spec "
                          f"{tuple(spec.shape)} / token {tuple(token.shape)} / pm {tuple(pm.shape)} / image_out {tuple(image_out.shape)} do "
                          f"not match (P, 3, S, S) / (B, ...) / (B, ...) / token's shape / (B, 3, S, S) with B = {B}")
    _call("mla_modal3_assemble", _p(image_compact) if P else None, _p(spec), _p(token, torch.int64), _p(pm), _p(mask_desc, torch.int64),
          d.data_ptr(), _p(image_out), B, P, image_out.shape[2], spec[0].numel(), token[0].numel(), stream or cur_stream())
    return image_out


# ---- rows of a batch: gather, expand, compact-and-sum (csrc/rows.hip; Modal3Classifier(..., present=)) --------------------------
def _index_host(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.is_cuda or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
        raise MLAHipError(f"{what}: expected a contiguous host int64 vector, got "
                          f"{(t.dtype, tuple(t.shape), str(t.device)) if isinstance(t, torch.Tensor) else type(t).__name__}")
    return t


def _index_pair(dev: torch.Tensor, host: torch.Tensor, what: str) -> Tuple[Optional[int], Optional[int], int]:
    """(device pointer, host pointer, entries) of an index table handed over on both sides; (None, None, 0) when it is empty."""
    h = _index_host(host, what)
    if dev.dim() != 1 or dev.numel() != h.numel():
        raise MLAHipError(f"{what}: device table {tuple(dev.shape)} and host table {tuple(h.shape)} differ")
    n = h.numel()
    return (_p(dev, torch.int64), h.data_ptr(), n) if n else (None, None, 0)


def _rows2d(t: torch.Tensor, what: str) -> Tuple[int, int]:
    if t.dim() < 1 or t.shape[0] == 0 or t.numel() == 0 or not t.is_contiguous():
        raise MLAHipError(f"{what}: expected a contiguous tensor of at least one non-empty row, got {tuple(t.shape)}")
    return t.shape[0], t.numel() // t.shape[0]


def rows_gather(src: torch.Tensor, idx: torch.Tensor, idx_host: torch.Tensor, dst: torch.Tensor, zero_tail_rows: int = 0,
                stream: Optional[int] = None) -> torch.Tensor:
    """src (B, ...) fp32 or int64, idx int64 (P) on the device and the same entries on the host -> dst (P + zero_tail_rows, ...):
    dst[j] = src[idx[j]], then `zero_tail_rows` rows of zeros (see include/mla_hip.h, mla_rows_gather)."""
    ip, hp, P = _index_pair(idx, idx_host, "rows_gather: idx")
    B, row = _rows2d(src, "rows_gather: src")
    if src.dtype not in (torch.float32, torch.int64) or dst.dtype != src.dtype:
        raise MLAHipError(f"rows_gather: src {src.dtype} / dst {dst.dtype} must both be float32 or both int64")
    if zero_tail_rows < 0 or dst.dim() < 1 or dst.shape[0] != P + zero_tail_rows or dst.numel() != dst.shape[0] * row:
        raise MLAHipError(f"rows_gather: dst {tuple(dst.shape)} does not hold P + zero_tail_rows = {P} + {zero_tail_rows} rows of {row} elements")
    _call("mla_rows_gather", _p(src, src.dtype), ip, hp, _p(dst, dst.dtype), B, P, row, src.element_size(), int(zero_tail_rows),
          stream or cur_stream())
    return dst


def rows_expand_map(idx_host: torch.Tensor, fill_row: int, B: int, src_rows: int) -> torch.Tensor:
    """The per-destination-row source map of rows_expand, host int64 (B): map[idx[j]] = j, every other row `fill_row`.  Refuses an
    index outside [0, B), one named twice, more indices than source rows and a fill row outside the source (no GPU)."""
    h = _index_host(idx_host, "rows_expand: idx")
    P = h.numel()
    if B <= 0 or P > B or P > src_rows or not 0 <= fill_row < src_rows:
        raise MLAHipError(f"rows_expand: need 0 <= P <= B, P <= src_rows and 0 <= fill_row < src_rows (got P={P}, B={B}, src_rows={src_rows}, "
                          f"fill_row={fill_row})")
    if P and (int(h.min()) < 0 or int(h.max()) >= B or torch.unique(h).numel() != P):
        raise MLAHipError(f"rows_expand: idx {h.tolist()} must name {P} different rows of [0, {B})")
    m = torch.full((B,), int(fill_row), dtype=torch.int64)
    m[h] = torch.arange(P, dtype=torch.int64)
    return m


def rows_expand(src: torch.Tensor, map: torch.Tensor, map_host: torch.Tensor, dst: torch.Tensor, stream: Optional[int] = None) -> torch.Tensor:
    """src fp32 or int64 (S, ...), map int64 (B) on the device and the same entries on the host (rows_expand_map) -> dst (B, ...):
    dst[b] = src[map[b]], every row written once (see include/mla_hip.h, mla_rows_expand)."""
    mp, hp, B = _index_pair(map, map_host, "rows_expand: map")
    S, row = _rows2d(src, "rows_expand: src")
    if src.dtype not in (torch.float32, torch.int64) or dst.dtype != src.dtype:
        raise MLAHipError(f"rows_expand: src {src.dtype} / dst {dst.dtype} must both be float32 or both int64")
    if dst.dim() < 1 or dst.shape[0] != B or dst.numel() != B * row:
        raise MLAHipError(f"rows_expand: dst {tuple(dst.shape)} does not hold {B} rows of {row} elements")
    _call("mla_rows_expand", _p(src, src.dtype), mp, hp, _p(dst, dst.dtype), B, S, row, src.element_size(), stream or cur_stream())
    return dst


def rows_compact_sum(src: torch.Tensor, idx: torch.Tensor, idx_host: torch.Tensor, absent: torch.Tensor, absent_host: torch.Tensor,
                     dst: torch.Tensor, stream: Optional[int] = None) -> torch.Tensor:
    """src fp32 (B, ...), idx int64 (P) and absent int64 (A), each on the device and on the host -> dst (P + 1, ...):
    dst[j] = src[idx[j]]; dst[P] = the fp32 sum of the rows src[absent[a]] in that order (see include/mla_hip.h, mla_rows_compact_sum)."""
    ip, ihp, P = _index_pair(idx, idx_host, "rows_compact_sum: idx")
    ap, ahp, A = _index_pair(absent, absent_host, "rows_compact_sum: absent")
    B, row = _rows2d(src, "rows_compact_sum: src")
    if dst.dim() < 1 or dst.shape[0] != P + 1 or dst.numel() != (P + 1) * row:
        raise MLAHipError(f"rows_compact_sum: dst {tuple(dst.shape)} does not hold P + 1 = {P + 1} rows of {row} elements")
    _call("mla_rows_compact_sum", _p(src), ip, ihp, ap, ahp, _p(dst), B, P, A, row, stream or cur_stream())
    return dst


# ---- Kaldi log-mel filterbank from PCM16 clips (data/extract_fbank.py:8-54) ------------------------------------------------------
def _mel_runs_host(tables) -> Tuple[torch.Tensor, torch.Tensor]:
    s, l = tables.mel_start_host, tables.mel_len_host
    for t in (s, l):
        if t.is_cuda or t.dtype != torch.int32 or tuple(t.shape) != (128,) or not t.is_contiguous():
            raise MLAHipError(f"mel runs: expected contiguous host int32 (128,) tensors, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return s, l


def wav_fbank_check(desc_host: torch.Tensor, wav_samples: int, tables, target_length: int = 1024) -> None:
    """The size and table checks of wav_fbank alone (no GPU): raises MLAHipError on a clip table or mel runs the kernel must not run."""
    d = _table_host(desc_host, 4, "clip descriptors")
    s, l = _mel_runs_host(tables)
    _call("mla_wav_fbank_check", d.data_ptr(), d.shape[0], wav_samples, target_length, s.data_ptr(), l.data_ptr(), tables.mel_weight.numel())


def wav_fbank(wav: torch.Tensor, desc: torch.Tensor, desc_host: torch.Tensor, tables, out: torch.Tensor,
              stream: Optional[int] = None) -> torch.Tensor:
    """wav int16 (device, packed mono 16 kHz clips), desc int64 (B, 4) rows (offset_samples, n_samples, sample_sum, 0) on the device
    and the same table on the host, tables = wav_feed.fbank_tables() moved to the device (window, twiddle, mel_start, mel_len,
    mel_weight there; mel_start_host, mel_len_host here) -> out fp32 (B, target_length, 128): each clip's Kaldi log-mel filterbank,
    zero rows beyond its frames (see include/mla_hip.h, mla_wav_fbank)."""
    d = _table_host(desc_host, 4, "clip descriptors")
    s, l = _mel_runs_host(tables)
    if tuple(desc.shape) != tuple(d.shape):
        raise MLAHipError(f"clip descriptors: device table {tuple(desc.shape)} and host table {tuple(d.shape)} differ")
    if wav.dim() != 1 or out.dim() != 3 or out.shape[0] != d.shape[0] or out.shape[2] != 128 or tuple(tables.window.shape) != (400,) \
            or tuple(tables.twiddle.shape) != (512, 2) or tuple(tables.mel_start.shape) != (128,) or tuple(tables.mel_len.shape) != (128,) \
            or tables.mel_weight.dim() != 1:
        raise MLAHipError(f"wav_fbank: wav {tuple(wav.shape)} / out {tuple(out.shape)} / window {tuple(tables.window.shape)} / twiddle "
                          f"{tuple(tables.twiddle.shape)} do not match (n,) / ({d.shape[0]}, target_length, 128) / (400,) / (512, 2)")
    _call("mla_wav_fbank", _p(wav, torch.int16) if wav.numel() else None, wav.numel(), _p(desc, torch.int64), d.data_ptr(),
          _p(tables.window), _p(tables.twiddle), _p(tables.mel_start, torch.int32), _p(tables.mel_len, torch.int32), s.data_ptr(),
          l.data_ptr(), _p(tables.mel_weight), tables.mel_weight.numel(), _p(out), d.shape[0], out.shape[1], stream or cur_stream())
    return out


# ---- HBM-resident CREMA-D feed (csrc/resident.hip) ------------------------------------------------------------------------------
class ResidentPlan(NamedTuple):
    """mla_resident_plan's result: plan5 = host int32 (band, rows_cap, kh, kv, lds) for one output size; a plan made with `train`
    holds for eval batches too, one made without holds for those only."""
    plan5: torch.Tensor
    out_h: int
    out_w: int
    train: bool


def resident_plan(table_host: torch.Tensor, T: int, frames_bytes: int, out_h: int = 224, out_w: int = 224, train: bool = True) -> ResidentPlan:
    """Validate the host frame table int64 (N * T, 3) rows (byte offset, H, W) against a buffer of `frames_bytes` and plan the
    resample launch for every crop the device draw can make of it (no GPU; see include/mla_hip.h, mla_resident_plan)."""
    t = _table_host(table_host, 3, "frame table")
    plan5 = torch.zeros(5, dtype=torch.int32)
    _call("mla_resident_plan", t.data_ptr(), t.shape[0], T, frames_bytes, out_h, out_w, int(bool(train)), plan5.data_ptr())
    return ResidentPlan(plan5, int(out_h), int(out_w), bool(train))


def resident_batch(frames: torch.Tensor, table: torch.Tensor, spec_table: Optional[torch.Tensor], labels: torch.Tensor, order: torch.Tensor,
                   T: int, pos: int, b: int, seed: int, epoch: int, train: bool, plan: ResidentPlan, lut: torch.Tensor, desc_out: torch.Tensor,
                   image_out: torch.Tensor, spec_out: Optional[torch.Tensor], label_out: torch.Tensor, idx_out: torch.Tensor,
                   stream: Optional[int] = None) -> None:
    """Batch slots 0..b-1 from the samples order[pos : pos + b] of a device-resident dataset: frames uint8, table int64 (N * T, 3),
    spec_table fp32 (N, 1024, 128) or None, labels / order int64 (N) -> desc_out int64 (b * T, 8), image_out fp32 (b, 3, T, out_h,
    out_w), spec_out fp32 (b, 1024, 128), label_out int64 (b), idx_out int64 (b, 1); three launches on the stream, nothing else (see
    include/mla_hip.h, mla_resident_batch).  The order vector is checked where it is made (gather_index_check)."""
    N = labels.numel()
    if frames.dim() != 1 or table.dim() != 2 or tuple(table.shape) != (N * T, 3) or order.numel() != N:
        raise MLAHipError(f"resident_batch: frames {tuple(frames.shape)} / table {tuple(table.shape)} / labels {tuple(labels.shape)} / order "
                          f"{tuple(order.shape)} do not match (bytes,) / (N * {T}, 3) / (N,) / (N,)")
    if seed < 0 or epoch < 0:
        raise MLAHipError(f"resident_batch: seed {seed} and epoch {epoch} must lie in [0, 2^32)")
    if train and not plan.train:
        raise MLAHipError("resident_batch: a plan made for whole frames (train=False) does not hold for drawn crops")
    if tuple(lut.shape) != (3, 256) or tuple(desc_out.shape) != (b * T, 8) or tuple(image_out.shape) != (b, 3, T, plan.out_h, plan.out_w) \
            or label_out.numel() != b or idx_out.numel() != b:
        raise MLAHipError(f"resident_batch: lut {tuple(lut.shape)} / desc_out {tuple(desc_out.shape)} / image_out {tuple(image_out.shape)} / "
                          f"label_out {tuple(label_out.shape)} / idx_out {tuple(idx_out.shape)} do not match (3, 256) / ({b * T}, 8) / "
                          f"({b}, 3, {T}, {plan.out_h}, {plan.out_w}) / ({b},) / ({b}, 1)")
    if spec_table is not None and (tuple(spec_table.shape) != (N, 1024, 128) or spec_out is None or tuple(spec_out.shape) != (b, 1024, 128)):
        raise MLAHipError(f"resident_batch: spec_table {tuple(spec_table.shape)} / spec_out "
                          f"{None if spec_out is None else tuple(spec_out.shape)} do not match ({N}, 1024, 128) / ({b}, 1024, 128)")
    _call("mla_resident_batch", _p(frames, torch.uint8), frames.numel(), _p(table, torch.int64), _p(spec_table), _p(labels, torch.int64),
          _p(order, torch.int64), N, T, pos, b, seed, epoch, int(bool(train)), plan.plan5.data_ptr(), _p(lut), _p(desc_out, torch.int64),
          _p(image_out), _p(spec_out) if spec_table is not None else None, _p(label_out, torch.int64), _p(idx_out, torch.int64), plan.out_h,
          plan.out_w, stream or cur_stream())
