"""Fused attention on the split-bf16 arithmetic (csrc/attention_split.hip, math="split" / attention_math="split").

The mode claims fp32 accuracy, so it is held to the bounds of the fp32-MFMA kernels (tests/test_attention_gpu.py): the same case
table at the same tolerances, the same score-range criterion with the same SCORE_K, plus exact cases with no tolerance (inputs
pinned by tests/test_attention_split_cpu.py) that a lost bf16 plane, a mis-paired product or a k order that differs between the
accumulator operand and the transposed read cannot pass.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_model as A  # noqa: E402
import attention_split_model as S  # noqa: E402
import exact as X  # noqa: E402
from test_attention_gpu import SCORE_K, _six, assert_case, guarded, guards_intact  # noqa: E402
from test_attention_gpu import run_hip as run_default  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    return _ops


def run_hip(ops, qkv, pm, dO, H, **kw):
    """test_attention_gpu.py::run_hip with the arithmetic passed on (kw: math=...)."""
    B, n, _ = qkv.shape
    D = H * A.HD
    _, qd = guarded(qkv.shape, qkv)
    _, dOd = guarded(dO.shape, dO)
    pmd = None if pm is None else guarded(pm.shape, pm)[1]
    bufs, out = {}, {}
    for name, shape in (("o", (B, n, D)), ("lse", (B, H, n)), ("dqkv", (B, n, 3 * D)), ("dvec", (B, H, n))):
        bufs[name], out[name] = guarded(shape)
    ops.attention_fwd(qd, pmd, out["o"], out["lse"], B, H, n, A.HD, **kw)
    ops.attention_bwd(dOd, qd, out["o"], out["lse"], pmd, out["dqkv"], out["dvec"], B, H, n, A.HD, **kw)
    torch.cuda.synchronize()
    for name in out:
        assert guards_intact(bufs[name]), f"{name}: a store left the buffer"
        assert not torch.isnan(out[name]).any(), f"{name}: an element was not written (or a read left an input buffer)"
    return out


@pytest.mark.parametrize("n,B,H,layout", A.case_params())
def test_split_instantiations_and_masks(ops, n, B, H, layout):
    """test_attention_instantiations_and_masks on math="split": every (W, TAIL) instantiation, ragged tiles, all six mask layouts."""
    ref = A.reference(n, B, H, layout, 0.7)
    qkv, dO, pm = ref["qkv"], ref["dO"], ref["pm"]
    out = run_hip(ops, qkv, pm, dO, H, math="split")
    assert_case(out, ref, H, "f32")
    assert_case(out, ref, H, "f64")
    if pm is not None:
        _dq, dk, dv = A.split_dqkv(out["dqkv"].cpu(), H)
        padded = pm > 0
        assert (dk[padded] == 0).all() and (dv[padded] == 0).all(), "dK / dV of a padded key must be exactly 0"
    if layout == "e":          # p = 1 and the split is exact: hi + mid + lo of v, summed in that order, is v
        v0 = qkv.view(B, n, 3, H, A.HD)[:, :1, 2]
        assert torch.equal(out["o"].cpu().view(B, n, H, A.HD), v0.expand(B, n, H, A.HD)), "one attended key: o must be its v, bit for bit"
    again = run_hip(ops, qkv, A.mask_layout("b", B, n) if layout == "f" else pm, dO, H, math="split")
    for k in out:
        assert torch.equal(out[k], again[k]), f"{k}: " + ("mask values other than 0 / 1 changed the result" if layout == "f" else "not bit-reproducible")


_REPORT = {}


@pytest.mark.parametrize("std", [0.7, 2.0, 3.0])
@pytest.mark.parametrize("layout", ["a", "b"])
@pytest.mark.parametrize("n", [99, 163, 257])
def test_split_score_range(ops, n, layout, std):
    """e_hip <= SCORE_K * e_ref for o, lse, dq, dk, dv, dvec: the bound of the fp32-MFMA kernels, unchanged.  (Dropping P's lo plane
    costs 2^-17 relative: within assert_case, outside this.)  Every figure is written to the report before the assertion."""
    B, H = 2, 3
    ref = A.reference(n, B, H, layout, std)
    out = run_hip(ops, ref["qkv"], ref["pm"], ref["dO"], H, math="split")
    hip, r32, r64 = _six(out, H), _six(ref["f32"], H), _six(ref["f64"], H)
    x = ref["qkv"].double().view(B, n, 3, H, A.HD)
    rec = {"max_abs_score": (torch.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1]) / 8.0).abs().max().item()}
    for k in SCORE_K:
        e_hip, e_ref = A.rel_max_err(hip[k], r64[k]), A.rel_max_err(r32[k], r64[k])
        rec[k] = {"e_hip": e_hip, "e_ref": e_ref, "ratio": e_hip / e_ref}
    _REPORT[f"n{n}_{layout}_std{std}"] = rec
    from test_m3ae_gpu import _dump_report
    _dump_report("attention_split_score_range.json", _REPORT)
    print(f"n={n} layout={layout} std={std}: " + " ".join(f"{k}={v['ratio']:.2f}" if isinstance(v, dict) else f"|s|={v:.1f}" for k, v in rec.items()))
    for k, K in SCORE_K.items():
        assert rec[k]["e_hip"] <= K * rec[k]["e_ref"], f"{k}: e_hip {rec[k]['e_hip']:.3e} > {K} x e_ref {rec[k]['e_ref']:.3e}"


@pytest.mark.parametrize("n", S.EXACT_N)
@pytest.mark.parametrize("cls", X.CLASSES)
def test_split_exact_products_and_lane_maps(ops, cls, n):
    """No tolerance: batch row b attends key b only (attention_split_model.py), so lse is the exact score / 8, o the attended v,
    dV[b, b] the sum of dO over the queries and every other dV row 0 -- for a key at every position of every tile and the remainder
    key.  dq, dk, dvec leave the exact range and are held to assert_case."""
    c = S.exact_case(cls, n)
    B, H = n, 1
    out = run_hip(ops, c["qkv"], c["pm"], c["dO"], H, math="split")
    want_lse = (S.attended_scores(c) * 0.125).view(B, 1, n)
    assert torch.equal(out["lse"].cpu(), want_lse), f"lse: {(out['lse'].cpu() != want_lse).sum().item()} of {want_lse.numel()} scores are not exact"
    want_o = c["v"][torch.arange(B), torch.arange(B)].view(B, 1, A.HD).expand(B, n, A.HD)
    assert torch.equal(out["o"].cpu(), want_o), "o must be the attended key's v, bit for bit"
    _dq, _dk, dv = A.split_dqkv(out["dqkv"].cpu(), H)
    want_dv = torch.zeros(B, n, 1, A.HD)
    want_dv[torch.arange(B), torch.arange(B), 0] = c["dO"].sum(1)
    assert torch.equal(dv, want_dv), "dV[b, b] must be sum_q dO[b, q] and every other row exactly 0"
    ref = {w: A.attention_ref(c["qkv"], c["pm"], c["dO"], H, dt) for w, dt in (("f32", torch.float32), ("f64", torch.float64))}
    assert_case(out, ref, H, "f32")
    assert_case(out, ref, H, "f64")


def test_split_dispatch(ops):
    """math="f32" is the default call bit for bit; an unknown arithmetic raises; the split entry points reject hd != 64 and n <= 0
    before any launch."""
    from mla_hip._lib import MLAHipError
    B, H, n = 2, 3, 99
    ref = A.reference(n, B, H, "b", 0.7)
    base = run_default(ops, ref["qkv"], ref["pm"], ref["dO"], H)          # the call without the math argument
    f32 = run_hip(ops, ref["qkv"], ref["pm"], ref["dO"], H, math="f32")
    for k in base:
        assert torch.equal(base[k], f32[k]), f"{k}: math='f32' differs from the default call"
    f = lambda *s: torch.zeros(s, device="cuda")
    for math in ("bf16", "", None):
        with pytest.raises(MLAHipError):
            ops.attention_fwd(f(B, n, 3 * H * 64), None, f(B, n, H * 64), f(B, H, n), B, H, n, 64, math=math)
    for bad_n, hd in ((5, 32), (0, 64)):
        rows, D = max(bad_n, 1), H * A.HD
        qkv, o, lse, dqkv, dvec, dO = f(B, rows, 3 * D), f(B, rows, D), f(B, H, rows), f(B, rows, 3 * D), f(B, H, rows), f(B, rows, D)
        with pytest.raises(MLAHipError):
            ops.attention_fwd(qkv, None, o, lse, B, H, bad_n, hd, math="split")
        with pytest.raises(MLAHipError):
            ops.attention_bwd(dO, qkv, o, lse, None, dqkv, dvec, B, H, bad_n, hd, math="split")
        torch.cuda.synchronize()
        assert not o.any() and not dqkv.any() and not dvec.any(), "nothing may have been launched"


def test_split_torch_ops(ops):
    """torch.ops.mla_hip.attention_fwd_split / attention_bwd_split return what ops.attention_* (math="split") writes."""
    import mla_hip.torch_ops  # noqa: F401
    B, H, n = 2, 3, 99
    ref = A.reference(n, B, H, "b", 0.7)
    want = run_hip(ops, ref["qkv"], ref["pm"], ref["dO"], H, math="split")
    qkv, pm, dO = ref["qkv"].cuda(), ref["pm"].cuda(), ref["dO"].cuda()
    o, lse = torch.ops.mla_hip.attention_fwd_split(qkv, pm, H)
    dqkv = torch.ops.mla_hip.attention_bwd_split(dO, qkv, o, lse, pm, H)
    assert torch.equal(o, want["o"]) and torch.equal(lse, want["lse"]) and torch.equal(dqkv, want["dqkv"])


@pytest.mark.parametrize("conv_math", ["split", "f32"])
def test_split_encoder_vs_reference_golden(golden_dir, monkeypatch, conv_math):
    """tests/test_m3ae_gpu.py's m3ae_small.npz comparison (features, losses, head and encoder gradients, SGD; padding mask, n = 257)
    with both encoders on attention_math="split", at that test's tolerances, under either conv_math."""
    import mla_hip
    import test_m3ae_gpu as T
    real, made = mla_hip.M3AEClassifier, []

    def make(*a, **k):
        made.append(real(*a, attention_math="split", **k))
        return made[-1]

    monkeypatch.setattr(mla_hip, "M3AEClassifier", make)
    monkeypatch.setattr(T, "_dump_report", lambda name, obj: None)      # the f32-attention run owns that report
    T.test_m3ae_step_vs_reference_golden(golden_dir, conv_math)
    assert len(made) == 1
    for enc in (made[0].mae_a, made[0].mae_v):
        assert enc.attention_math == "split" and enc.conv_math == conv_math


def test_attention_math_switch(monkeypatch):
    """Default "f32"; $MLA_ATTENTION_MATH is read when the argument is None; unknown values and split + materialized raise."""
    from mla_hip._lib import MLAHipError
    from mla_hip.m3ae import M3AEEncoder
    kw = dict(depth=1, text_vocab_size=64, seed=0)
    monkeypatch.delenv("MLA_ATTENTION_MATH", raising=False)
    monkeypatch.delenv("MLA_ATTENTION", raising=False)
    assert M3AEEncoder("text", **kw).attention_math == "f32"
    assert M3AEEncoder("text", conv_math="bf16", **kw).attention_math == "f32"          # conv_math does not turn it on
    assert M3AEEncoder("text", attention_math="split", **kw).attention_math == "split"
    monkeypatch.setenv("MLA_ATTENTION_MATH", "split")
    assert M3AEEncoder("text", **kw).attention_math == "split"
    assert M3AEEncoder("text", attention_math="f32", **kw).attention_math == "f32"
    with pytest.raises(MLAHipError):
        M3AEEncoder("text", attention_math="bf16", **kw)
    monkeypatch.setenv("MLA_ATTENTION", "materialized")
    with pytest.raises(MLAHipError):
        M3AEEncoder("text", **kw)
