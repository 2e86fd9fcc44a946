"""The exactly-summable input classes of tests/exact.py, checked on the CPU: a condition on the INPUTS of test_exact_gpu.py.

For every class and every reduction length the GPU tests use: the fp32 budget holds; the six-product model of the split
arithmetic equals the exact result; a CPU fp32 matmul / conv2d equals it in natural and in permuted summation order (so it is a
valid reference).  And the inputs have power: dropping any one of the six products from the model changes at least a quarter of
the outputs of the class that is meant to prove that product -- otherwise a later edit of the generators could make the GPU
tests blind without anything failing."""
import pytest
import torch

import exact as X

# reduction lengths of test_exact_gpu.py: 1x1 and 3x3 convolutions of 64..512 channels, the stems (49, 147), the Linears (768, 3072),
# pixel counts of the weight gradients (ragged 126 / 1122, 4113 rows)
K_LENGTHS = [49, 147, 64, 128, 256, 512, 576, 1152, 2304, 4608, 768, 3072, 126, 1122, 4113]
R, C = 96, 64


def _matmul_pair(cls, K, seed=0):
    """A (R x K), B (K x C) of one class, the sparse operand with its structured positions."""
    pos = X.k_positions(K)
    fa = X.forced_mask((R, K), (1,), pos, 4)
    fb = X.forced_mask((K, C), (0,), pos, 4)
    return X.pair(cls, (R, K), (K, C), seed + K, axis_a=(1,), axis_b=(0,), forced_a=fa, forced_b=fb)


@pytest.mark.parametrize("K", K_LENGTHS)
@pytest.mark.parametrize("cls", X.CLASSES)
def test_classes_are_exact_on_the_cpu(cls, K):
    A, B, u = _matmul_pair(cls, K)
    bits = X.assert_exact_budget(A, B, u, name=f"{cls} K={K}")
    assert bits < 24
    exact = X.matmul64(A, B)
    assert torch.equal(X.six_term(A, B), exact), "the six-product model must reproduce the exact result"
    assert torch.equal(X.six_term(A, B, terms=X.SIX + ((1, 2), (2, 1))), exact), "the 2^-24 products are zero"
    assert torch.equal((A @ B).double(), exact), "CPU fp32 matmul, natural order"
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    assert torch.equal((A[:, perm] @ B[perm]).double(), exact), "CPU fp32 matmul, permuted K order"
    acc = torch.zeros((R, C))
    for k0 in range(0, K, 37):                                    # a third order: ragged K slabs accumulated in fp32
        acc = acc + A[:, k0:k0 + 37] @ B[k0:k0 + 37]
    assert torch.equal(acc.double(), exact), "CPU fp32, slab order"
    # the three products the kernels drop are exactly zero on these inputs
    pa, pb = X.split3(A), X.split3(B)
    for (i, j) in ((1, 2), (2, 1), (2, 2)):
        assert not X.matmul64(pa[i], pb[j]).any()
    for t in (A, B):
        assert torch.equal(sum(p.double() for p in X.split3(t)), t.double()), "hi + mid + lo == x"


def test_budget_check_is_not_decoration():
    """|a| < 16 with 16 non-zeros: the budget is exceeded, and the check says so."""
    gen = torch.Generator().manual_seed(1)
    A = (torch.randint(-(2 ** 20 - 1), 2 ** 20, (R, 1152), generator=gen).double() * 2.0 ** -16).float()
    B = X.operand("sparse9", (1152, C), 3, sparse_axis=(0,)).sign() * 1.5
    with pytest.raises(AssertionError, match="not exact"):
        X.assert_exact_budget(A, B, 2.0 ** -17)


@pytest.mark.parametrize("K", [147, 576, 1152, 4608, 3072, 1122])
@pytest.mark.parametrize("term", X.SIX, ids=lambda t: "p%d%d" % t)
def test_inputs_have_power(term, K):
    """Dropping one product changes >= 25 % of the outputs of the class that proves it (and nothing where it is zero)."""
    cls = X.PROVES[term]
    A, B, u = _matmul_pair(cls, K)
    full = X.six_term(A, B)
    frac = (X.six_term(A, B, drop=term) != full).double().mean().item()
    assert frac >= 0.25, f"class {cls}, K={K}: dropping product {term} changes only {frac:.1%} of the outputs"
    # the bf16x3 set (what conv2d_split_terms(3) selects) must be visibly wrong on SA, SB and SMM, and exact on D
    three = (X.six_term(A, B, terms=X.SIX[:3]) != full).double().mean().item()
    assert (three == 0.0) if cls == "D" else (three >= 0.25), (cls, three)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("geom", [(2, 9, 7, 64, 64, 3, 1, 1), (2, 9, 7, 64, 128, 3, 2, 1), (2, 9, 7, 64, 128, 1, 2, 0), (2, 20, 12, 3, 64, 7, 2, 3)],
                         ids=lambda g: "x".join(map(str, g)))
def test_convolution_operands(cls, geom):
    """The window-sparse operands (x of the forward, dy of the input gradient): budget by an abs() convolution, model == exact ==
    CPU fp32 conv2d, and power through the convolution."""
    N, H, W, Cin, Cout, k, s, p = geom
    OH, OW = X.conv_out(H, k, s, p), X.conv_out(W, k, s, p)
    fwd = lambda a, b: X.conv_fwd(a, b, s, p)
    x, w, u = X.pair(cls, (N, H, W, Cin), (k, k, Cin, Cout), 11, count_a=X.window_count(k, s, p), axis_b=(0, 1, 2),
                     forced_a=X.window_forced((N, H, W, Cin)), forced_b=X.forced_mask((k, k, Cin, Cout), (0, 1, 2), X.k_positions(k * k * Cin), 4))
    X.assert_exact_budget(x, w, u, contract=fwd)
    exact = fwd(x.double(), w.double())
    assert torch.equal(X.six_term(x, w, contract=fwd), exact) and torch.equal(fwd(x, w).double(), exact)
    for term in [t for t in X.SIX if X.PROVES[t] == cls]:
        frac = (X.six_term(x, w, drop=term, contract=fwd) != exact).double().mean().item()
        assert frac >= 0.25, (cls, term, frac)
    if X.is_sparse(X.SPEC[cls][0]):
        assert X.window_count(k, s, p)((x != 0).double()).max().item() <= X.NNZ[X.SPEC[cls][0]]
    if Cin % 64:
        return
    dg = lambda a, b: X.conv_dgrad(a, b, (N, H, W, Cin), s, p)
    dy, w2, u = X.pair(cls, (N, OH, OW, Cout), (k, k, Cin, Cout), 12, count_a=X.window_count_t(k, s, p, H, W), axis_b=(0, 1, 3),
                       forced_a=X.window_forced((N, OH, OW, Cout)))
    X.assert_exact_budget(dy, w2, u, contract=dg)
    exact = dg(dy.double(), w2.double())
    assert torch.equal(X.six_term(dy, w2, contract=dg), exact) and torch.equal(dg(dy, w2).double(), exact)
    # weight gradient: sparse over pixels
    wg = lambda a, b: X.conv_wgrad(a, b, k, s, p)
    x3, dy3, u = X.pair(cls, (N, H, W, Cin), (N, OH, OW, Cout), 13, axis_a=(0, 1, 2), axis_b=(0, 1, 2))
    X.assert_exact_budget(x3, dy3, u, contract=wg)
    exact = wg(x3.double(), dy3.double())
    assert torch.equal(X.six_term(x3, dy3, contract=wg), exact) and torch.equal(wg(x3, dy3).double(), exact)
    want = torch.nn.grad.conv2d_weight(x3.double().permute(0, 3, 1, 2), (Cout, Cin, k, k), dy3.double().permute(0, 3, 1, 2), stride=s, padding=p)
    assert torch.equal(exact, want.permute(2, 3, 1, 0)), "conv_wgrad is the weight gradient of conv_fwd"


def test_structured_positions_are_present():
    """First / last index, both sides of every K-stage boundary, every tap; for pixel-sparse operands first / last pixel of every
    image, image row, 64- and 256-pixel tile."""
    for kind in ("half3", "sparse9"):
        for (k, Cin, Cout) in ((3, 64, 128), (3, 128, 128), (1, 64, 128), (7, 3, 64), (7, 1, 64)):
            shape, K = (k, k, Cin, Cout), k * k * Cin
            w = X.operand(kind, shape, 5, sparse_axis=(0, 1, 2), forced=X.forced_mask(shape, (0, 1, 2), X.k_positions(K), 4))
            nz = (w != 0)
            assert nz.sum(dim=(0, 1, 2)).max().item() <= X.NNZ[kind]
            used = nz.reshape(K, Cout).any(1)
            want = X.k_positions(K)
            assert {0, K - 1} <= set(want) and all(b in want and b - 1 in want for b in range(16, K, 16))
            assert used[want].all(), "a structured reduction index is missing"
            assert nz.any(dim=3).any(dim=2).all(), "every tap of the window"
        for (N, H, W, C) in ((2, 33, 17, 128), (5, 9, 11, 64), (3, 3, 1, 128), (4, 32, 4, 512)):
            pos = X.pixel_positions(N, H, W)
            M = N * H * W
            assert {0, M - 1, H * W - 1, H * W, W - 1, min(W, M - 1), min(63, M - 1), min(255, M - 1)} <= set(pos)
            t = X.operand(kind, (N, H, W, C), 6, sparse_axis=(0, 1, 2), forced=X.forced_mask((N, H, W, C), (0, 1, 2), pos, 4))
            nz = (t != 0).reshape(M, C)
            assert nz.sum(0).max().item() <= X.NNZ[kind]
            assert nz.any(1)[pos].all(), "a structured pixel is missing"
        # Linear: reduction along K (768, 3072) and along the rows
        for K in (768, 3072):
            w = X.operand(kind, (K, 768), 7, sparse_axis=(0,), forced=X.forced_mask((K, 768), (0,), X.k_positions(K), 4))
            assert (w != 0).any(1)[X.k_positions(K)].all() and (w != 0).sum(0).max().item() <= X.NNZ[kind]


def test_assert_bitwise_reports_where():
    a = torch.zeros((4, 6))
    b = a.clone()
    X.assert_bitwise(a, b, "same")
    b[2, 3] = 2.0 ** -10
    b[3, 1] = -(2.0 ** -12)
    with pytest.raises(AssertionError) as e:
        X.assert_bitwise(b, a, "probe", unit=2.0 ** -17)
    msg = str(e.value)
    assert "2 of 24" in msg and "[2, 3]" in msg and "128.0 units" in msg
