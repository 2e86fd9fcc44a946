"""The token-path kernels of csrc/transformer.hip at every regime, on the inputs of tests/exact_tokens.py.

Bitwise (no tolerance): the embedding gradient with its [cls] / type sums, every bgemm instantiation, the softmax backward, token assembly,
patchify, and the exact rows of the LayerNorm forward.  Against fp64 with bounds derived from the formats: the softmax forward (tolerance of
test_attention_pieces) and the LayerNorm forward (exact_tokens.lnf_bounds).  Every output is filled with NaN (or a stated canary where the
kernel accumulates) before the launch, and buffers carry a guard tail that must come back unchanged.  test_tokens_exact_cpu.py proves
without a GPU that the inputs meet their budgets and that the case tables reach every regime."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_tokens as T  # noqa: E402
from exact_tokens import assert_bitwise  # noqa: E402
from oracle import mla_oracle as O  # noqa: E402

NAN = float("nan")
CANARY = -12345.0


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _guarded(t, guard, fill=CANARY):
    """A flat device buffer holding t followed by `guard` canary elements; returns (buffer, view of t's part)."""
    buf = torch.full((t.numel() + guard,), fill, device="cuda")
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf, buf[:t.numel()].view(t.shape)


def _guard_intact(buf, n, name, fill=CANARY):
    assert bool((buf[n:] == fill).all()), f"{name}: the guard tail behind the buffer was written"


# ---- 1. embedding gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.EMB_CASES)
def test_embedding_gradient(ops, name):
    """dtable accumulates (integer prefill), rows of no valid id keep the prefill bit for bit, two calls agree bit for bit -- the second
    on a workspace full of plausible stale keys and partial sums; dcls and dtype are exact too.  tot comes from colsum_rows where it supports D (D % 64 == 0), else from the exact integer total."""
    c = T.emb_case(name)
    B, L, D, V = c.B, c.L, c.D, c.V
    dx0, ids = c.dx0.cuda(), c.ids.cuda()
    if D % 64 == 0:
        tot = _nan(D)
        ops.colsum_rows(dx0.view(-1, D), tot, torch.empty(ops.colreduce_ws_elems(B * (L + 1), D), device="cuda"), B * (L + 1), D)
        assert_bitwise(tot, c.tot, f"{name}: column totals", 1.0)
    else:
        tot = c.tot.cuda()
    # second call: a workspace whose previous content looks like more of the last run (keys) and like large partial sums (floats)
    stale = torch.empty(ops.tokens_assemble_bwd_ws_bytes(B, L, D), device="cuda", dtype=torch.uint8)
    key = T.emb_stale_key(c.ids, L, V)
    stale[:4 * T.EMB_CHUNK].view(torch.int32).fill_(key - 2 ** 32 if key >= 2 ** 31 else key)
    stale[4 * T.EMB_CHUNK:].view(torch.float32).fill_(1000.0)
    runs = []
    for ws in (None, stale):
        buf, dtable = _guarded(c.prefill, 4 * D)
        dcls, dtype = _nan(D), _nan(D)
        ops.tokens_assemble_bwd(dx0, tot, ids, dcls, dtype, dtable, B, L, D, ws=ws)
        _guard_intact(buf, V * D, name)
        runs.append((dtable, dcls, dtype))
    dtable, dcls, dtype = runs[0]
    assert_bitwise(dtable, c.dtable, f"{name}: dtable", 1.0)
    assert_bitwise(dtable.cpu()[~c.touched], c.prefill[~c.touched], f"{name}: rows of no valid id")
    assert_bitwise(dcls, c.dcls, f"{name}: dcls", 1.0)
    assert_bitwise(dtype, c.dtype, f"{name}: dtype", 1.0)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), f"{name}: two calls on the same inputs differ"
    assert torch.equal(dx0.cpu(), c.dx0) and torch.equal(ids.cpu(), c.ids), "inputs must not be written"


@pytest.mark.parametrize("B,L,D", [(3, 5, 64), (2, 7, 768), (5, 33, 1024)])
def test_assemble_backward_without_cls(ops, B, L, D):
    """CAV-MAE: no [cls] row, rows laid out (B, L, D), no embedding: dtype == tot bitwise."""
    dx = T.rand_ints((B, L, D), -7, 7, T.case_seed(B, L, D)).float()
    tot = _nan(D)
    ops.colsum_rows(dx.cuda().view(-1, D), tot, torch.empty(ops.colreduce_ws_elems(B * L, D), device="cuda"), B * L, D)
    dtype = _nan(D)
    ops.tokens_assemble_bwd(dx.cuda(), tot, None, None, dtype, None, B, L, D)
    assert_bitwise(dtype, dx.long().sum((0, 1)).float(), "dtype without [cls]", 1.0)
    assert torch.equal(dtype, tot)


# ---- 2. bgemm -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.BGEMM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_bgemm(ops, case):
    c = T.bgemm_case(case)
    B, H, M, N, K = c.dims
    C = _nan(c.nc)
    A, Bm = c.A.cuda(), c.B.cuda()
    ops.bgemm(A, Bm, C, B, H, M, N, K, c.sa, c.sb, c.sc, c.alpha, a_off=T.BGEMM_OFFS[0], b_off=T.BGEMM_OFFS[1], c_off=T.BGEMM_OFFS[2])
    got = C.cpu()
    assert torch.isnan(got[~c.window]).all(), "a cell outside the C window was written"
    assert_bitwise(got[c.window], c.want[c.window], f"bgemm {case}", c.alpha)
    assert torch.equal(A.cpu(), c.A) and torch.equal(Bm.cpu(), c.B)


# ---- 3. softmax ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.SOFTMAX_N)
def test_softmax_backward(ops, n):
    c = T.softmax_bwd_case(n)
    buf, dP = _guarded(c.g, T.SOFTMAX_GUARD)
    pbuf, P = _guarded(c.P, T.SOFTMAX_GUARD)
    ops.softmax_bwd(P, dP, c.B, c.H, n)                                  # in place in dP
    assert_bitwise(dP, c.want, f"softmax backward n={n}", 2.0 ** -12)
    _guard_intact(buf, c.g.numel(), f"softmax backward n={n}")
    assert torch.equal(pbuf.cpu()[:c.P.numel()].view(c.P.shape), c.P) and bool((pbuf[c.P.numel():] == CANARY).all())


def _softmax(ops, s, pm):
    B, H, n = s.shape[:3]
    buf, S = _guarded(s, T.SOFTMAX_GUARD)
    ops.softmax_fwd(S, pm.cuda() if pm is not None else None, B, H, n)
    _guard_intact(buf, s.numel(), f"softmax forward n={n}")
    return S.cpu()


@pytest.mark.parametrize("n,family,masked", T.SOFTMAX_FWD_CASES)
def test_softmax_forward(ops, n, family, masked):
    s = T.softmax_scores(n, family, T.case_seed(n, len(family), masked))
    pm = T.softmax_mask(n) if masked else None
    ref = T.softmax_ref(s, pm)
    got = _softmax(ops, s, pm)
    err, tol = (got.double() - ref).abs().max().item(), T.softmax_tol(ref)
    print(f"softmax forward n={n} {family} masked={masked}: max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol and bool(torch.isfinite(got).all())
    if masked and n > 1:
        cols = (pm > 0)[:, None, None, :].expand(got.shape)
        assert cols.any() and bool((got[cols] == 0.0).all()), "a masked column must be exactly 0"
        # non-finite values under the mask are never seen: same bits as with zeros there
        junk = torch.tensor([NAN, float("inf"), float("-inf")])[torch.arange(n) % 3].expand(got.shape)
        got_junk = _softmax(ops, torch.where(cols, junk, s), pm)
        got_zero = _softmax(ops, torch.where(cols, torch.zeros(()), s), pm)
        assert bool(torch.isfinite(got_junk).all())
        assert_bitwise(got_junk, got_zero, "non-finite values under the mask")
        assert_bitwise(got_zero, got, "values under the mask do not matter")


@pytest.mark.parametrize("n", [1, 2, 65, 1024])
def test_softmax_forward_fully_masked_batch_element(ops, n):
    """Every column of batch element 1 is masked: all scores become -1e7, each row is uniform -- bit-identical entries near 1 / n."""
    s = T.softmax_scores(n, "normal", n)
    pm = T.softmax_mask(n)
    pm[1] = torch.tensor([1.0, 0.5])[torch.arange(n) % 2]
    ref = T.softmax_ref(s, pm)
    got = _softmax(ops, s, pm)
    assert (got.double() - ref).abs().max().item() <= T.softmax_tol(ref)
    row = got[1]
    assert bool((row == row[..., :1]).all()), "a fully masked row must be uniform bit for bit"
    assert (row.double() - 1.0 / n).abs().max().item() <= 2e-6 + 1e-5 / n


# ---- 4. LayerNorm forward -------------------------------------------------------------------------------------------------------------------
def _ln(ops, c, eps=None):
    M, D = c.M, c.D
    ybuf, y = _guarded(torch.full((M, D), NAN), 2 * D)
    mean, rstd = _nan(M + 8), _nan(M + 8)
    kw = {} if eps is None else {"eps": eps}
    ops.layernorm_fwd(c.x.cuda(), c.w.cuda(), c.b.cuda(), y, mean, rstd, M, D, **kw)
    _guard_intact(ybuf, M * D, "LayerNorm y")
    assert bool(torch.isnan(mean[M:]).all() and torch.isnan(rstd[M:]).all()), "mean / rstd written behind row M"
    return y.cpu(), mean[:M].cpu(), rstd[:M].cpu()


@pytest.mark.parametrize("D,M,fam", T.LNF_CASES)
def test_layernorm_forward(ops, D, M, fam):
    c = T.lnf_case(D, M, fam)
    y64, mean64, rstd64 = T.lnf_ref(c.x, c.w, c.b)
    mb, rb, yb = T.lnf_bounds(c.x, c.w, c.b, y64, rstd64)
    y, mean, rstd = _ln(ops, c)
    r_m = ((mean.double() - mean64).abs() / mb).max().item()
    r_r = ((rstd.double() / rstd64 - 1).abs() / rb).max().item()
    r_y = ((y.double() - y64).abs() / yb).max().item()
    print(f"LayerNorm forward D={D} M={M} family={T.LNF_FAMILIES[fam]}: error / bound: mean {r_m:.3f}, rstd {r_r:.3f}, y {r_y:.3f}")
    assert r_m <= 1.0 and r_r <= 1.0 and r_y <= 1.0            # NaN fails all three


@pytest.mark.parametrize("D", T.LNF_D)
def test_layernorm_forward_exact_rows(ops, D):
    c = T.lnf_const_case(D)
    y, mean, rstd = _ln(ops, c)
    assert_bitwise(mean, c.c, "constant rows: mean")
    assert_bitwise(y, c.b.expand(c.M, D), "constant rows: y == b")
    want = 1.0 / T.LN_EPS32 ** 0.5
    assert ((rstd.double() / want - 1).abs() <= 2.4e-7).all(), "constant rows: rstd within 2 ulp of 1 / sqrt(eps)"
    p = T.lnf_pm_case(D)
    y, mean, rstd = _ln(ops, p, eps=0.0)
    assert_bitwise(mean, p.m, "+-2^k rows: mean")
    assert ((rstd.double() * 2.0 ** p.k - 1).abs() <= 2.4e-7).all(), "+-2^k rows: rstd within 2 ulp of 2^-k"
    y64 = T.lnf_ref(p.x, p.w, p.b, eps=0.0)[0]
    # x - mean = +-2^k exactly: xhat carries rstd's 2 ulp (4 u), the multiply by w rounds once, the add of b once
    assert ((y.double() - y64).abs() <= 6 * T.U24 * p.w.double().abs() + T.U24 * y64.abs()).all(), "+-2^k rows: y"


# ---- 5. assembly and patchify -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,D", T.ASM_CASES)
def test_tokens_assemble(ops, B, L, D):
    c = T.asm_case(B, L, D)
    pos, typ, cls = c.pos.cuda(), c.type.cuda(), c.cls.cuda()
    add = (c.pos.double() + c.type.double())[None]
    bad = (c.ids < 0) | (c.ids >= c.V)
    # text: [cls] + table[ids] + pos + type; an id out of range poisons its own row and nothing else
    buf, x0 = _guarded(torch.full((B, L + 1, D), NAN), T.ASM_GUARD)
    ops.tokens_assemble(x0, c.table.cuda(), c.ids.cuda(), pos, typ, cls, B, L, D)
    _guard_intact(buf, x0.numel(), "assemble (text)")
    got = x0.cpu()
    want = torch.cat([c.cls.expand(B, 1, D), (c.table.double()[c.ids.clamp(0, c.V - 1)] + add).float()], 1)
    assert bool(torch.isnan(got[:, 1:][bad]).all()) and int(bad.sum()) == 2
    keep = torch.cat([torch.ones(B, 1, dtype=torch.bool), ~bad], 1)
    assert_bitwise(got[keep], want[keep], "assemble (text)", 2.0 ** -8)
    # image: in place over the patch Linear's output
    buf, x1 = _guarded(torch.cat([torch.full((B, 1, D), NAN), c.lin], 1), T.ASM_GUARD)
    ops.tokens_assemble(x1, None, None, pos, typ, cls, B, L, D)
    _guard_intact(buf, x1.numel(), "assemble (image)")
    assert_bitwise(x1, torch.cat([c.cls.expand(B, 1, D), (c.lin.double() + add).float()], 1), "assemble (image)", 2.0 ** -8)
    # no [cls]: rows laid out (B, L, D)
    buf, x2 = _guarded(c.lin, T.ASM_GUARD)
    ops.tokens_assemble(x2, None, None, pos, typ, None, B, L, D)
    _guard_intact(buf, x2.numel(), "assemble (no [cls])")
    assert_bitwise(x2, (c.lin.double() + add).float(), "assemble (no [cls])", 2.0 ** -8)


@pytest.mark.parametrize("case", T.PATCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_patchify(ops, case):
    B, C, H, W, P, tr = case
    img = T.patch_image(case)
    rows, F_ = B * (H // P) * (W // P), C * P * P
    buf, out = _guarded(torch.full((rows, F_), NAN), 256)
    ops.patchify(img.cuda(), out, P, transposed_hw=(H, W) if tr else None)
    _guard_intact(buf, rows * F_, f"patchify {case}")
    want = O.patchify(img.unsqueeze(1).transpose(2, 3) if tr else img, P)
    assert torch.equal(out.cpu().view(want.shape), want), f"patchify {case}"
