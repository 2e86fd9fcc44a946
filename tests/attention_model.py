"""CPU side of the fused-attention tests (csrc/attention_kernels.h, attention.hip): the kernel-selection logic restated, the case table, the
padding-mask layouts and a plain autograd reference in fp32 / fp64.

  att_main_rows, att_waves   the two host functions of csrc/attention_common.h, restated line for line
  att_path                   which kernel a length n is routed to: ("tail", rows) or (W, TAIL, workgroups per (b, h))
  CASES                      every (W, TAIL) instantiation and the tail-only kernels at the smallest n that reaches them
  mask_layout                the padding-mask layouts "a" .. "f"
  attention_ref              autograd of Attention.forward (models/m3ae.py:102-125): o, lse, dqkv, dvec
  reference                  inputs + attention_ref in both precisions, computed once per (n, B, H, layout, std)
"""
import functools

import torch
import torch.nn.functional as F

from oracle import mla_oracle as O

HD = 64
ATT_TAIL_MAX = 3          # attention_common.h
ATT_TAIL_N = 4096         # attention_common.h


def att_main_rows(n):
    """attention_common.h, att_main_rows: rows the MFMA kernels own."""
    r = n % 32
    return n - r if (0 < r <= ATT_TAIL_MAX and n <= ATT_TAIL_N) else n


def att_waves(n):
    """attention_common.h, att_waves: waves per workgroup, the width that leaves the fewest idle waves (ties: the widest)."""
    blocks = (n + 31) // 32
    best, best_idle = 4, 1 << 30
    for w in (4, 3, 2):
        idle = -(-blocks // w) * w - blocks
        if idle < best_idle:
            best, best_idle = w, idle
    return best


def att_path(n):
    """The launch mla_attention_fwd / mla_attention_bwd make for n tokens (att_launch in attention_common.h; the nm == 0 branches of attention.hip)."""
    nm = att_main_rows(n)
    if nm == 0:
        return ("tail", n)
    W = att_waves(nm)
    tail = 0 if nm == n else (1 if nm + 1 == n else ATT_TAIL_MAX)
    return (W, tail, -(-nm // (32 * W)))


# n values of test_m3ae_gpu.py::test_fused_attention_vs_autograd (they stay there)
EXISTING_N = (257, 50, 130, 512, 1, 33, 128)

# (n, B, H, expected path, layouts next to "a").  The layouts rotate so that each one meets a W = 2, a W = 3, a W = 4 and -- where it
# exists at n <= 3 -- a tail-only case; W = 2 and W = 4 have two shapes each for five layouts, so one of each carries three.
CASES = (
    (2, 2, 3, ("tail", 2), "de"),          # blockIdx.y > 0 in the three tail kernels
    (3, 2, 3, ("tail", 3), "de"),
    (35, 2, 3, (2, 3, 1), "cde"),
    (64, 2, 3, (2, 0, 1), "bf"),           # full tiles only
    (80, 2, 3, (3, 0, 1), "bc"),           # ragged last tile (16 live rows), the launch-bounds-3 forward
    (96, 2, 3, (3, 0, 1), "de"),           # full tiles
    (97, 2, 3, (3, 1, 1), "fc"),
    (99, 2, 3, (3, 3, 1), "be"),
    (129, 2, 3, (4, 1, 1), "bcd"),         # single workgroup
    (159, 2, 3, (3, 0, 2), "fd"),          # last tile has 31 live rows
    (163, 2, 3, (3, 3, 2), "bc"),          # workgroup 1 has an idle wave; workgroup 0 owns the remainder
    (193, 2, 3, (3, 1, 2), "df"),
    (196, 2, 3, (4, 0, 2), "ef"),          # r = 4, just above ATT_TAIL_MAX: padded tile with 4 live rows; the cav_visual length
    (288, 2, 3, (3, 0, 3), "ce"),
    (4097, 1, 1, (3, 0, 43), "bc"),        # n > ATT_TAIL_N with r = 1: the padded-tile path, not the remainder path
)

LAYOUT_MIN_N = {"a": 1, "b": 64, "c": 33, "d": 2, "e": 2, "f": 64}
SCATTERED = (5, 17, 70, 101, 150, 250, 1000, 4000)     # single padded keys of layouts b / f (those below n)


def case_params():
    return [(n, B, H, lay) for n, B, H, _path, lays in CASES for lay in "a" + lays]


def mask_layout(layout, B, n):
    """(B, n) padding mask (> 0: padded) or None.  Every row attends at least key 0 or one key beyond 32.
      a  no mask (null pointer)
      b  keys [32, 64) padded + scattered single keys; the keys of the last partial tile padded in batch row 0, attended in the others
      c  keys [0, 32) padded, the rest attended
      d  every odd key padded
      e  only key 0 attended
      f  layout b, padded entries from {0.5, 2.0, 1e-3}, attended ones from {0.0, -0.0, -1.0}"""
    assert n >= LAYOUT_MIN_N[layout], (layout, n)
    if layout == "a":
        return None
    pm = torch.zeros(B, n)
    if layout in "bf":
        pm[:, 32:64] = 1.0
        for k in SCATTERED:
            if k < n:
                pm[:, k] = 1.0
        r0 = n - n % 32
        pm[0, r0:] = 1.0
        pm[1:, r0:] = 0.0
        if layout == "f":
            idx = torch.arange(B * n).view(B, n)
            pm = torch.where(pm > 0, torch.tensor([0.5, 2.0, 1e-3])[idx % 3], torch.tensor([0.0, -0.0, -1.0])[idx % 3])
    elif layout == "c":
        pm[:, :32] = 1.0
    elif layout == "d":
        pm[:, 1::2] = 1.0
    elif layout == "e":
        pm[:, 1:] = 1.0
    return pm


def attention_inputs(n, B, H, std):
    qkv = O.portable_normal(n + B, (B, n, 3 * H * HD), stream=1, std=std)
    dO = O.portable_normal(n, (B, n, H * HD), stream=2)
    return qkv, dO


def attention_ref(qkv, pm, dO, H, dtype):
    """Autograd of Attention.forward (m3ae.py:102-125) in `dtype`: o (B, n, H*hd), lse (B, H, n), dqkv, dvec (B, H, n)."""
    B, n, D3 = qkv.shape
    hd = D3 // (3 * H)
    x = qkv.detach().to(dtype, copy=True).requires_grad_(True)
    q4 = x.view(B, n, 3, H, hd).permute(2, 0, 3, 1, 4)
    att = torch.matmul(q4[0], q4[1].transpose(-2, -1)) * hd ** -0.5
    if pm is not None:
        att = torch.where(pm[:, None, None, :].expand(att.shape) > 0, torch.tensor(-1e7, dtype=dtype), att)
    o = torch.matmul(F.softmax(att, dim=-1), q4[2]).permute(0, 2, 1, 3).reshape(B, n, H * hd)
    o.backward(dO.to(dtype))
    lse = torch.logsumexp(att.detach(), dim=-1)
    o = o.detach()
    dvec = (dO.to(dtype) * o).view(B, n, H, hd).sum(-1).permute(0, 2, 1).contiguous()
    return {"o": o, "lse": lse, "dqkv": x.grad, "dvec": dvec}


@functools.lru_cache(maxsize=None)
def reference(n, B, H, layout, std=0.7):
    """Inputs and both references of one case; computed once, shared by the tests, never written to."""
    qkv, dO = attention_inputs(n, B, H, std)
    pm = mask_layout(layout, B, n)
    return {"qkv": qkv, "dO": dO, "pm": pm, "f32": attention_ref(qkv, pm, dO, H, torch.float32),
            "f64": attention_ref(qkv, pm, dO, H, torch.float64)}


def split_dqkv(dqkv, H):
    """(B, n, 3*H*hd) -> dq, dk, dv as (B, n, H, hd) views."""
    B, n, _ = dqkv.shape
    v = dqkv.view(B, n, 3, H, -1)
    return v[:, :, 0], v[:, :, 1], v[:, :, 2]


def rel_max_err(got, want):
    """max|got - want| / max|want| in fp64."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return ((got - want).abs().max() / want.abs().max()).item()
