"""conv_math="bf16" without a GPU: the switch, the C ABI, and that the inputs of the bit-exact GPU tests (test_bf16_gpu.py) suit them."""
import os
import re

import pytest
import torch

import exact as X
import bf16_model as M
from test_exact_gpu import dgrad_case, fwd_case, wgrad_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mla_conv2d_fwd_bf16", "mla_conv2d_dgrad_bf16", "mla_conv2d_wgrad_bf16", "mla_conv2d_wgrad_ws_bytes_bf16",
           "mla_conv2d_wimage_bf16", "mla_conv2d_wimage_bytes_bf16", "mla_conv2d_wimage_batch_bf16", "mla_conv2d_tile_bf16",
           "mla_linear_fwd_bf16", "mla_linear_dgrad_bf16", "mla_linear_wgrad_bf16", "mla_linear_wgrad_bias_bf16",
           "mla_linear_wgrad_ws_bytes_bf16"]


class Args:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", True, "Normal"


def test_conv_math_bf16_constructs_on_cpu(monkeypatch):
    from mla_hip import AVClassifier, MLAHipError
    from mla_hip.encoder import ResNet18Encoder
    from mla_hip.m3ae import M3AEEncoder
    m = AVClassifier(Args(), device="cpu", seed=0, conv_math="bf16")
    for enc in (m.audio_net, m.visual_net):
        assert enc.conv_math == "bf16" and enc.bf16 and enc.stem_split and not enc.fuse_bn_reduce
        # one plane per image: forward + input-gradient image of every 64..512-channel conv weight, 2 bytes per element
        n = sum(k * k * ci * co for _n, ci, co, k, _s, _p in enc.specs if ci % 64 == 0)
        assert enc._wsplit_flat.numel() == 2 * n and "conv1" not in enc.wsp
    monkeypatch.setenv("MLA_CONV_MATH", "bf16")
    assert ResNet18Encoder("audio", device="cpu", seed=0).conv_math == "bf16"
    t = M3AEEncoder("image", device="cpu", depth=1, seed=0)
    assert t.conv_math == "bf16" and t.bf16 and t.split
    monkeypatch.setenv("MLA_CONV_MATH", "split")
    e = ResNet18Encoder("audio", device="cpu", seed=0)
    assert e.conv_math == "split" and not e.bf16
    assert ResNet18Encoder("audio", device="cpu", seed=0, conv_math="bf16").bf16          # the argument wins over the environment
    for bad in ("fp16", "bf16x3", "BF16"):
        with pytest.raises(MLAHipError, match="conv_math must be 'f32' or 'split'"):
            ResNet18Encoder("audio", device="cpu", seed=0, conv_math=bad)


def test_abi_has_the_bf16_entry_points():
    from mla_hip import _lib
    txt = open(os.path.join(ROOT, "include", "mla_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/mla_hip.h"
        assert hasattr(lib, name), f"libmla_hip.so does not export {name}"
        assert name in _lib.PROTOTYPES
    assert lib.mla_abi_version() == 3
    assert lib.mla_conv2d_wimage_bytes_bf16(64, 128, 3, 3) * 3 == lib.mla_conv2d_wsplit_bytes(64, 128, 3, 3)
    assert lib.mla_conv2d_tile_bf16(100, 63, 576) == -1


def _differs(A, B, contract, cls, name):
    """On SA, SB and SMM the one-product model differs from the six-product model in more than half of the outputs."""
    one, six = M.one_term(A, B, contract), X.six_term(A, B, contract=contract)
    frac = (one != six).double().mean().item()
    if cls == "D":
        assert frac == 0.0, f"{name}: class D has hi * hi only"
    else:
        assert frac > 0.5, f"{name} {cls}: only {frac:.1%} of the outputs tell one product from six"
    # and the fp32 contraction of the hi planes is that model (what the GPU tests compare with)
    assert torch.equal(contract(M.hi(A), M.hi(B)).double(), one), f"{name} {cls}: fp32 contraction of the hi planes is not exact"


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("geom", M.GG_BF16, ids=lambda g: "x".join(map(str, g)))
def test_gather_gemm_inputs_suit_bf16(geom, cls):
    N, H, W, Cin, Cout, k, s, p = geom
    x, w, u, _y, _sq = fwd_case(cls, geom)
    con = lambda a, b: X.conv_fwd(a, b, s, p)
    M.assert_hi_budget(x, w, u, contract=con, name=f"fwd {cls} {geom}")
    _differs(x, w, con, cls, f"fwd {geom}")
    dy, w2, u, _dx, res, _m = dgrad_case(cls, geom)
    con = lambda a, b: X.conv_dgrad(a, b, (N, H, W, Cin), s, p)
    M.assert_hi_budget(dy, w2, u, contract=con, extra=res, name=f"dgrad + residual {cls} {geom}")
    M.assert_hi_budget(dy, w2, u, contract=con, scale=2.0, name=f"dgrad accumulate {cls} {geom}")
    if k * k * Cout // (s * s) >= 64:       # (the 1x1 / 2 downsample reaches a quarter of the pixels: the others are exact zeros in both models)
        _differs(dy, w2, con, cls, f"dgrad {geom}")


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("geom", M.WGRAD_BF16, ids=lambda g: "x".join(map(str, g)))
def test_wgrad_inputs_suit_bf16(geom, cls):
    N, H, W, Cin, Cout, k, s, p = geom
    x, dy, u, _dw = wgrad_case(cls, geom)
    con = lambda a, b: X.conv_wgrad(a, b, k, s, p)
    M.assert_hi_budget(x, dy, u, contract=con, name=f"wgrad {cls} {geom}")
    _differs(x, dy, con, cls, f"wgrad {geom}")


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("case", M.LINEAR_BF16, ids=lambda g: "x".join(map(str, g)))
def test_linear_inputs_suit_bf16(case, cls):
    """The inputs of test_linear_bf16, all three contractions: exactly summable under hi * hi, and a Linear launch that ran the split
    kernels would fail on SA, SB and SMM."""
    groups, rows, xg, xo, yg, yo, K, N = case
    (x, w, u), (dy, w2, u2), (x3, dy3, u3) = M.linear_case(cls, case)
    mm = lambda a, b: a @ b
    xs = x[:, xo:xo + rows]
    M.assert_hi_budget(xs, w, u, name=f"linear fwd {cls} {case}")
    _differs(xs, w, mm, cls, f"linear fwd {case}")
    M.assert_hi_budget(dy, w2.t(), u2, name=f"linear dgrad {cls} {case}")
    _differs(dy, w2.t(), mm, cls, f"linear dgrad {case}")
    xs3 = x3[:, xo:xo + rows].reshape(groups * rows, K)
    M.assert_hi_budget(xs3.t(), dy3, u3, name=f"linear wgrad {cls} {case}")
    _differs(xs3.t(), dy3, mm, cls, f"linear wgrad {case}")


def test_class_r_suits_bf16():
    x, w, u = M.dense_r((2, 9, 7, 64), (3, 3, 64, 64), 3)
    con = lambda a, b: X.conv_fwd(a, b, 1, 1)
    M.assert_hi_budget(x, w, u, contract=con, name="class R")
    _differs(x, w, con, "R", "class R")
    assert 576 * 2 * 3 / u + 2 ** 19 < 2 ** 24             # the bound of the large shapes (K = 576) plus a residual, whatever the draw
