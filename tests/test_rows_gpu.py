"""The three row kernels (csrc/rows.hip) through mla_hip.ops and torch.ops.mla_hip: gather and expand against index_select /
indexed assignment bit for bit, compact_sum against an int64 sum on integer-valued data, bit for bit.

Outputs live in guarded buffers as in test_attention_gpu.py::guarded: a sentinel on either side that must come back unchanged, a
NaN interior of which nothing may be left.  Rows of 1, 3 and 257 elements take the 4-byte path (257: rows that start at different
offsets mod 16), 64 and 196 608 (one 3 x 256 x 256 image) the 16-byte path; 196 608 needs more than one workgroup per row.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 1024                 # elements on either side of every output buffer
SENTINEL = {torch.float32: -12345.5, torch.int64: -0x123456789ABCDEF}
POISON = {torch.float32: float("nan"), torch.int64: 0x7FC000007FC00000}       # int64: two fp32 NaNs side by side
B = 5
ROW_ELEMS = (1, 3, 64, 257, 196608)
IDX = ([0, 1, 2, 3, 4], [], [4, 0], [2])


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    return _ops


def guarded(shape, dtype):
    numel = math.prod(shape)
    buf = torch.full((numel + 2 * GUARD,), SENTINEL[dtype], device="cuda", dtype=dtype)
    view = buf[GUARD:GUARD + numel].view(shape)
    view.fill_(POISON[dtype])
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return buf, view


def check_guarded(buf, view, dtype):
    assert bool((buf[:GUARD] == SENTINEL[dtype]).all()) and bool((buf[-GUARD:] == SENTINEL[dtype]).all()), "guard overwritten"
    left = torch.isnan(view).any() if dtype == torch.float32 else (view == POISON[dtype]).any()
    assert not bool(left), "a destination element was not written"


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def make_src(rows, row_elems, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int64:
        return torch.randint(-2 ** 40, 2 ** 40, (rows, row_elems), generator=g).cuda()
    x = torch.randn((rows, row_elems), generator=g)
    x.view(-1)[::7] = -0.0                              # a sign bit that a multiply by the mask would lose
    return x.cuda()


def dev(idx):
    h = torch.tensor(idx, dtype=torch.int64)
    return h.cuda(), h


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64], ids=["f32", "i64"])
@pytest.mark.parametrize("row_elems", ROW_ELEMS)
def test_gather_equals_index_select(ops, dtype, row_elems):
    src = make_src(B, row_elems, dtype, row_elems)
    for idx in IDX:
        for tail in ((1, 0) if idx else (1,)):
            d, h = dev(idx)
            buf, out = guarded((len(idx) + tail, row_elems), dtype)
            ops.rows_gather(src, d, h, out, zero_tail_rows=tail)
            torch.cuda.synchronize()
            check_guarded(buf, out, dtype)
            want = torch.cat([src.index_select(0, d), torch.zeros((tail, row_elems), dtype=dtype, device="cuda")])
            assert torch.equal(bits(out), bits(want)), (idx, tail)       # the zero tail is +0.0: every bit clear
            got = torch.ops.mla_hip.rows_gather(src, h, tail)
            assert got.dtype == dtype and torch.equal(bits(got), bits(want)), (idx, tail)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64], ids=["f32", "i64"])
@pytest.mark.parametrize("row_elems", ROW_ELEMS)
def test_expand_equals_indexed_assignment(ops, dtype, row_elems):
    for idx in IDX:
        P = len(idx)
        src = make_src(P + 1, row_elems, dtype, row_elems + P)          # P compact rows, then the fill row
        d, h = dev(idx)
        want = src[P].expand(B, row_elems).clone()
        want[d] = src[:P]
        m = ops.rows_expand_map(h, P, B, P + 1)
        assert m.tolist() == [idx.index(b) if b in idx else P for b in range(B)]
        buf, out = guarded((B, row_elems), dtype)
        ops.rows_expand(src, m.cuda(), m, out)
        torch.cuda.synchronize()
        check_guarded(buf, out, dtype)
        assert torch.equal(bits(out), bits(want)), idx
        got = torch.ops.mla_hip.rows_expand(src, h, P, B)
        assert torch.equal(bits(got), bits(want)), idx


@pytest.mark.parametrize("A", [0, 1, 4, 33])
@pytest.mark.parametrize("row_elems", [1, 3, 64, 257, 768])
def test_compact_sum_is_exact_on_integers(ops, A, row_elems):
    """Integer-valued fp32 rows, |x| <= 2^7: a sum of 33 of them is exact in fp32 in any order, so the kernel's sum row must equal
    the int64 sum bit for bit (an empty sum is +0.0), and a present row is moved, not recomputed."""
    rows = 40
    g = torch.Generator().manual_seed(1000 * A + row_elems)
    src = torch.randint(-128, 129, (rows, row_elems), generator=g).float().cuda()
    perm = torch.randperm(rows, generator=g)
    absent, idx = perm[:A].contiguous(), perm[A:A + 5].contiguous()      # in no particular order, disjoint
    buf, out = guarded((idx.numel() + 1, row_elems), torch.float32)
    ops.rows_compact_sum(src, idx.cuda(), idx, absent.cuda(), absent, out)
    torch.cuda.synchronize()
    check_guarded(buf, out, torch.float32)
    want = torch.cat([src[idx.cuda()], src.long()[absent.cuda()].sum(dim=0, keepdim=True).float()])
    assert torch.equal(bits(out), bits(want))
    got = torch.ops.mla_hip.rows_compact_sum(src, idx, absent)
    assert torch.equal(bits(got), bits(want))


def test_argument_errors_launch_nothing(ops):
    from mla_hip import MLAHipError
    src = make_src(B, 64, torch.float32, 1)
    out = torch.zeros((3, 64), device="cuda")
    big = torch.zeros((B + 2, 64), device="cuda")

    def refused(fn, *args, **kw):
        with pytest.raises(MLAHipError):
            fn(*args, **kw)
    refused(ops.rows_gather, src, *dev([0, 5]), out, zero_tail_rows=1)                   # an index outside [0, B)
    refused(ops.rows_gather, src, *dev([0, -1]), out, zero_tail_rows=1)
    refused(ops.rows_gather, src, *dev([0, 1, 2, 3, 4, 0]), big, zero_tail_rows=1)       # P > B
    refused(ops.rows_gather, src, *dev([0, 1]), out, zero_tail_rows=0)                   # dst holds another number of rows
    refused(ops.rows_gather, src, *dev([]), out[:0], zero_tail_rows=0)                   # nothing to write
    refused(ops.rows_gather, src, *dev([0, 1]), out.long(), zero_tail_rows=1)            # dtypes differ
    refused(ops.rows_gather, src, dev([0, 1])[0], torch.tensor([0, 1, 2]), out, 1)       # device and host tables differ
    refused(ops.rows_gather, src[:, :0], *dev([0, 1]), out[:, :0], zero_tail_rows=1)     # empty rows
    refused(ops.rows_gather, src, *dev([0, 1]), src[2:5], zero_tail_rows=1)              # dst overlaps src
    refused(ops.rows_expand_map, torch.tensor([1, 1]), 2, B, 3)                          # a row named twice
    refused(ops.rows_expand_map, torch.tensor([1, 5]), 2, B, 3)
    refused(ops.rows_expand_map, torch.tensor([1, 2]), 3, B, 3)                          # fill row outside the source
    refused(ops.rows_expand_map, torch.tensor([0, 1, 2, 3, 4, 0]), 0, B, 7)              # P > B
    bad = torch.tensor([0, 1, 3])                                                         # a map entry outside the 3 source rows
    refused(ops.rows_expand, src[:3], bad.cuda(), bad, out)
    refused(ops.rows_compact_sum, src, *dev([0, 1]), *dev([7]), out)                     # an absent index outside [0, B)
    refused(ops.rows_compact_sum, src, *dev([0, 9]), *dev([2]), out)
    refused(ops.rows_compact_sum, src, *dev([0]), *dev([2]), out)                        # dst is not P + 1 rows
    with pytest.raises(Exception):
        torch.ops.mla_hip.rows_gather(src, torch.tensor([0, 5]), 1)
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(big.any()), "a refused call wrote to its output"
