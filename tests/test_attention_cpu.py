"""CPU: the case table of tests/test_attention_gpu.py reaches every fused-attention instantiation (csrc/attention.hip), and the
reference helper / mask layouts it uses are what they claim to be.  att_main_rows / att_waves are restated in
tests/attention_model.py from csrc/attention_common.h: when someone retunes them, the first test says which shapes to re-pick."""
import pytest
import torch

import attention_model as A


def test_case_table_reaches_every_instantiation():
    for n, _B, _H, path, _lays in A.CASES:
        assert A.att_path(n) == path, f"n = {n}: the host functions give {A.att_path(n)}, the table expects {path}"
    reached = {A.att_path(n)[:2] for n in tuple(c[0] for c in A.CASES) + A.EXISTING_N}
    want = {(W, T) for W in (2, 3, 4) for T in (0, 1, A.ATT_TAIL_MAX)} | {("tail", r) for r in (1, 2, 3)}
    assert reached == want, f"not reached: {sorted(map(str, want - reached))}"
    # what the table was picked for beyond the pair itself
    assert A.att_main_rows(196) == 196 and A.att_main_rows(195) == 192            # r = 4 pads a tile, r = 3 does not
    assert A.att_main_rows(4097) == 4097 and A.att_main_rows(4065) == 4064        # beyond ATT_TAIL_N r = 1 pads a tile as well
    assert A.att_path(163)[2] == 2 and 2 * 3 * 32 - A.att_main_rows(163) == 32    # workgroup 1 of n = 163 has one idle wave
    for n, W, T in ((257, 4, 1), (512, 4, 0), (130, 4, 3), (33, 2, 1), (50, 2, 0), (128, 4, 0)):   # the lengths of test_m3ae_gpu.py
        assert A.att_path(n)[:2] == (W, T)


def test_layouts_rotate_over_every_kernel_width():
    met = {lay: set() for lay in "abcdef"}
    for n, B, H, path, lays in A.CASES:
        assert B * H >= 6 or n > 4096, "B >= 2 and H = 3 wherever cost allows"
        assert len(lays) >= 2 and "a" not in lays and len(set(lays)) == len(lays)
        for lay in "a" + lays:
            assert n >= A.LAYOUT_MIN_N[lay], f"layout {lay} does not exist at n = {n}"
            met[lay].add(path[0])
    for lay, widths in met.items():
        want = {2, 3, 4} | ({"tail"} if A.LAYOUT_MIN_N[lay] <= A.ATT_TAIL_MAX else set())
        assert widths >= want, f"layout {lay} meets {widths}, wants {want}"
    assert len(A.case_params()) == len(set(A.case_params()))


@pytest.mark.parametrize("n,B", [(3, 2), (35, 2), (64, 2), (99, 2), (163, 2), (257, 2)])
def test_mask_layouts(n, B):
    for lay in "bcdef":
        if n < A.LAYOUT_MIN_N[lay]:
            continue
        pm = A.mask_layout(lay, B, n)
        assert pm.shape == (B, n) and pm.dtype == torch.float32
        assert ((pm > 0).sum(1) < n).all(), "every row attends at least one key"
    assert A.mask_layout("a", B, n) is None
    if n >= 64:
        b, f = A.mask_layout("b", B, n), A.mask_layout("f", B, n)
        assert set(b.unique().tolist()) <= {0.0, 1.0}
        assert torch.equal(b > 0, f > 0), "layout f pads the keys of layout b"
        assert (b[:, 32:64] > 0).all() and (b[:, 5] > 0).all() and not (b[:, 0] > 0).any()
        assert torch.equal(f[f > 0].unique(), torch.tensor([1e-3, 0.5, 2.0]))
        att = f[~(f > 0)]
        assert (att == -1.0).any() and (att == 0).any() and torch.signbit(att[att == 0]).any() and not torch.signbit(att[att == 0]).all()
        if n % 32:
            r0 = n - n % 32
            assert (b[0, r0:] > 0).all() and not (b[1, r0:] > 0).any(), "remainder keys: padded in row 0, attended in row 1"
    if n > 32:
        c = A.mask_layout("c", B, n)
        assert (c[:, :32] > 0).all() and not (c[:, 32:] > 0).any()
    e = A.mask_layout("e", B, n)
    assert not (e[:, 0] > 0).any() and (e[:, 1:] > 0).all()
    d = A.mask_layout("d", B, n)
    assert (d[:, 1::2] > 0).all() and not (d[:, 0::2] > 0).any()


@pytest.mark.parametrize("n,lay", [(3, "d"), (35, "c"), (99, "b"), (64, "e")])
def test_reference_helper(n, lay):
    """attention_ref against a direct evaluation: o and lse from explicit probabilities, dvec from its definition, padded keys
    get exactly zero dK / dV, fp32 within rounding of fp64, and layout e is exactly one-hot."""
    B, H = 2, 3
    ref = A.reference(n, B, H, lay)
    qkv, dO, pm = ref["qkv"], ref["dO"], ref["pm"]
    r64, r32 = ref["f64"], ref["f32"]
    assert r64["o"].dtype == torch.float64 and r32["o"].dtype == torch.float32
    assert r64["o"].shape == (B, n, H * A.HD) and r64["lse"].shape == (B, H, n) == r64["dvec"].shape and r64["dqkv"].shape == qkv.shape
    x = qkv.double().view(B, n, 3, H, A.HD)
    s = torch.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1]) / 8.0
    s = s.masked_fill((pm > 0)[:, None, None, :], -1e7)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    z = p.sum(-1, keepdim=True)
    o = torch.einsum("bhqk,bkhd->bqhd", p / z, x[:, :, 2]).reshape(B, n, -1)
    assert (o - r64["o"]).abs().max() < 1e-13
    assert ((s.amax(-1) + z.squeeze(-1).log()) - r64["lse"]).abs().max() < 1e-12
    assert ((dO.double() * o).view(B, n, H, A.HD).sum(-1).permute(0, 2, 1) - r64["dvec"]).abs().max() < 1e-12
    _dq, dk, dv = A.split_dqkv(r64["dqkv"], H)
    assert (dk[pm > 0] == 0).all() and (dv[pm > 0] == 0).all()
    for k in ("o", "lse", "dqkv", "dvec"):
        assert A.rel_max_err(r32[k], r64[k]) < 2e-6, k
    if lay == "e":
        assert torch.equal(r32["o"].view(B, n, H, A.HD), qkv.view(B, n, 3, H, A.HD)[:, :1, 2].expand(B, n, H, A.HD))
    assert A.reference(n, B, H, lay) is ref, "computed once"
