"""The kernels between backward and the next forward, and at evaluation, against the models of tests/tail_model.py: called through
mla_hip.ops on hand-built buffers and tables, not through models.

  exact (bit for bit)   OGM scaling and every float outside a segment; SGD on the 2^-4 grid at every size and misalignment;
                        scale_by_device_scalar; colsum on integers; the fixed-weight fusion counters on integer logits with ties
  derived bound         OGM-GE noise (1e-5 in z), OGM-GE std (1 fp32 ulp), OGM coefficients ((B + 8) 2^-23 on the scores), bn_invstd
                        (2 ulp), GS projection (2e-5 of max |want|), dynamic fusion weights (1e-5; the serial-sum bound on the entropy
                        difference at the stride-crossing shapes)

tests/test_tail_cpu.py proves the input conditions these bounds rest on.  Every test prints the figure it measures before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tail_model as T  # noqa: E402
from oracle import mla_oracle as O  # noqa: E402

F32, F64 = np.float32, np.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t.to(device="cuda", dtype=dtype).contiguous()


def bits(x):
    """fp32 array -> its bit patterns (NaN-safe, -0 != +0)."""
    return np.ascontiguousarray(x, dtype=F32).view(np.int32)


def assert_bits(got, want, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == F32 and got.shape == want.shape, f"{name}: {got.dtype} {got.shape} vs {want.shape}"
    bad = np.flatnonzero(bits(got) != bits(want.astype(F32)))
    assert bad.size == 0, f"{name}: {bad.size} of {got.size} elements differ, first at {bad[0]}: got {got.ravel()[bad[0]]!r}, want {want.ravel()[bad[0]]!r}"


# ---- 1. OGM modulation ---------------------------------------------------------------------------------------------------------------
def run_ogm(ops, t, coeff, ge, seed=0, step=0):
    """-> (buffer after the call, stdv read back from the workspace tail: 2 * total_chunks doubles, then n_seg floats)."""
    buf, seg, fc = dev(t.buf), dev(t.seg), dev(t.first_chunk)
    cf = torch.tensor([coeff], device="cuda", dtype=torch.float32)
    ws = torch.zeros(ops.ogm_ws_bytes(t.total_chunks, t.n_seg), device="cuda", dtype=torch.uint8) if ge else None
    ops.ogm_modulate(buf, seg, fc, t.n_seg, t.total_chunks, cf, ge, seed, step, ws)
    torch.cuda.synchronize()
    stdv = None
    if ge:
        o = 16 * t.total_chunks
        stdv = ws[o:o + 4 * t.n_seg].cpu().numpy().view(F32)
    return buf.cpu().numpy(), stdv


def check_outside(t, out, name):
    assert (bits(out)[~t.inside] == bits(t.buf)[~t.inside]).all(), f"{name}: a float outside the segments changed"


def check_noise(t, out, stdv, coeff, seed, step, name, segments=None):
    """|out - (g coeff + sd z)| <= sd 1e-5 + 2^-23 |out| per element, sd = stdv_s + 1e-8 in fp32 as the kernel forms it: 1e-5 in z
    (about 3x the sum of the OpenCL-class ulp bounds of logf, sqrtf and sincosf on |z| <= 5.9) plus the final add's rounding.
    Returns the largest deviation in z over the elements where the rounding term is below the noise term."""
    worst = 0.0
    for s in (range(t.n_seg) if segments is None else segments):
        o, n = (int(v) for v in t.seg[s])
        if n == 0 or not np.isfinite(stdv[s]):
            continue
        sd = F64(F32(stdv[s]) + T.OGM_EPS)
        z = T.ogm_noise(n, s, step, seed)
        got = out[o:o + n].astype(F64)
        err = np.abs(got - (t.vals[s].astype(F64) * coeff + sd * z))
        tol = sd * 1e-5 + 2.0 ** -23 * np.abs(got)
        i = int(np.argmax(err - tol))
        assert (err <= tol).all(), (f"{name} segment {s} element {i}: got {got[i]!r}, g {t.vals[s][i]!r}, sd {sd!r}, model z {z[i]!r}, "
                                    f"kernel z {(got[i] - t.vals[s][i] * coeff) / sd!r}")
        tight = 2.0 ** -23 * np.abs(got) < sd * 1e-6
        if tight.any():
            worst = max(worst, float((err[tight] / sd).max()))
    return worst


@pytest.mark.parametrize("coeff", [0.5, 0.25, 1.0])
def test_ogm_scaling_is_exact_and_stays_inside_the_segments(ops, coeff):
    """OGM mode on the main table (offsets of every residue mod 4; n = 2, 5, 16383, 16384, 16385, 2 * 16384 + 3; a zero-length segment
    in the middle): every segment equals g * coeff bit for bit, every float outside a segment keeps its bits."""
    t = T.ogm_main()
    out, _ = run_ogm(ops, t, coeff, ge=False)
    assert_bits(out, T.ogm_scaled(t, coeff), f"OGM coeff={coeff}")
    one = T.ogm_one()
    out, _ = run_ogm(ops, one, coeff, ge=False)
    assert_bits(out, T.ogm_scaled(one, coeff), f"OGM coeff={coeff}, n = 1 table")


def test_ogm_ge_noise_and_statistics(ops):
    """OGM-GE on the main table, seed 2^40 + 3, step 5.

    Statistics: stdv of every segment within 1 fp32 ulp of float32(sqrt(var)) of the exact variance -- integers, the large-mean family
    1000 + k 2^-6 (an fp32 or naive accumulation misses by more than the variance itself), a constant segment (var exactly 0: stdv
    == 0, sd = 1e-8).  Noise: every element within 1e-5 of the model's z (check_noise); floats outside the segments unchanged.

    Measured on an MI355X: largest deviation in z 5.1e-7 here (2.9e-7 ... 3.8e-7 on the geometry tables below), a twentieth of the
    bound; stdv bit-equal to the model on every segment (0.00 ulp)."""
    t = T.ogm_main()
    seed, step, coeff = T.OGM_SEEDS[1], 5, 0.5
    out, stdv = run_ogm(ops, t, coeff, ge=True, seed=seed, step=step)
    check_outside(t, out, "OGM-GE")
    for s, (n, kind) in enumerate(t.spec):
        if n == 0:
            continue
        want = F64(t.stdv[s])
        print(f"segment {s} ({kind}, n={n}): stdv {stdv[s]!r}, model {t.stdv[s]!r}, off by {abs(F64(stdv[s]) - want) / T.ulp32(want):.2f} ulp")
        assert abs(F64(stdv[s]) - want) <= T.ulp32(want), (s, kind, stdv[s], t.stdv[s])
        if kind == "const":
            assert stdv[s] == 0.0
    worst = check_noise(t, out, stdv, coeff, seed, step, "OGM-GE")
    print(f"OGM-GE noise: largest |z_kernel - z_model| = {worst:.3g}")


def test_ogm_ge_single_element_segment_is_nan(ops):
    """n = 1: torch's std of one element is NaN, so the element becomes NaN; its neighbours take their noise, the gaps stay."""
    t = T.ogm_one()
    out, stdv = run_ogm(ops, t, 0.5, ge=True, seed=3, step=1)
    check_outside(t, out, "OGM-GE n = 1")
    assert np.isnan(stdv[1]) and np.isnan(out[t.seg[1, 0]])
    assert np.isfinite(out[t.inside]).sum() == t.inside.sum() - 1
    for s in (0, 2):
        assert abs(F64(stdv[s]) - F64(t.stdv[s])) <= T.ulp32(t.stdv[s])
    check_noise(t, out, stdv, 0.5, 3, 1, "OGM-GE n = 1", segments=(0, 2))


def test_ogm_ge_noise_is_independent_of_geometry_and_separate_per_stream(ops):
    """The same values at table index s = 1 behind a 5-element segment 0 (table A) and behind a 3-chunk segment 0 (table B, another
    chunk index, block and alignment): identical bits.  Table A holds them again at s = 2: other noise, and each matches the model
    -- at steps 0 and 5 and seeds 0 and 2^40 + 3 (the high key word), all four pairwise different."""
    a, b = T.ogm_geom("A"), T.ogm_geom("B")
    n = T.OGM_X[0]
    cut = lambda t, out, s: out[int(t.seg[s, 0]):int(t.seg[s, 0]) + n]
    seen = []
    for seed in T.OGM_SEEDS:
        for step in T.OGM_STEPS:
            out, stdv = run_ogm(ops, a, 0.25, ge=True, seed=seed, step=step)
            check_outside(a, out, "table A")
            worst = check_noise(a, out, stdv, 0.25, seed, step, f"table A seed={seed} step={step}")
            print(f"seed={seed} step={step}: largest |z_kernel - z_model| = {worst:.3g}")
            x1, x2 = cut(a, out, 1), cut(a, out, 2)
            assert stdv[1] == stdv[2] and (bits(x1) != bits(x2)).mean() > 0.9, "s = 1 and s = 2 must draw different noise"
            assert all((bits(x1) != bits(y)).mean() > 0.9 for y in seen), "another seed or step must draw different noise"
            seen.append(x1)
            if step == 5:
                outb, stdvb = run_ogm(ops, b, 0.25, ge=True, seed=seed, step=step)
                check_outside(b, outb, "table B")
                assert stdvb[1] == stdv[1]
                assert_bits(cut(b, outb, 1), x1, f"segment at s = 1 behind 3 chunks vs behind 5 elements, seed={seed}")
                check_noise(b, outb, stdvb, 0.25, seed, step, "table B")


# ---- 2. OGM coefficients ------------------------------------------------------------------------------------------------------------
def run_coeff(ops, outs, label, alpha=T.COEFF_ALPHA):
    coeff = torch.full((3,), NAN, device="cuda")
    info = torch.full((6,), NAN, device="cuda")
    ops.ogm_coeff([dev(o) for o in outs], dev(label), alpha, coeff, info)
    torch.cuda.synchronize()
    M = len(outs)
    return coeff.cpu().numpy()[:M].astype(F64), info.cpu().numpy()[:M].astype(F64), info.cpu().numpy()[3:3 + M].astype(F64)


def check_coeff(ops, outs, label, name):
    B = outs[0].shape[0]
    cf, sc, ra = run_coeff(ops, outs, label)
    wcf, wsc, wra = T.coeff_ref(outs, label)
    rt = T.coeff_score_rtol(B)
    print(f"{name}: scores off by {np.abs(sc / wsc - 1).max() / rt:.3g}, ratios by {np.abs(ra / wra - 1).max() / (2 * rt):.3g} of the "
          f"bound, coefficients by {np.abs(cf - wcf).max():.3g}")
    assert (np.abs(sc - wsc) <= rt * np.abs(wsc)).all(), (name, sc, wsc)
    assert (np.abs(ra - wra) <= 2 * rt * np.abs(wra)).all(), (name, ra, wra)
    assert (np.abs(cf - wcf) <= 1e-6).all(), (name, cf, wcf)
    assert ((cf == 1.0) == (wcf == 1.0)).all(), (name, cf, wcf)                          # the same branch
    return cf, sc, ra


@pytest.mark.parametrize("M,B,C", T.COEFF_SHAPES)
def test_ogm_coeff_vs_fp64(ops, M, B, C):
    """O.ogm_coefficients on doubles; scores to (B + 8) 2^-23 (the ordered fp32 sum of B terms plus a few ulp of expf and the
    division), ratios to twice that, coefficients to 1e-6 (tanhf).  Families: unit normal; rows at +-1e4 with a spread of 200; two
    modalities with identical logits (ratio_v == 1 exactly: the else branch modulates modality 0).  C up to 300: no class cap.
    Measured on an MI355X over all cases: scores at most 0.51 of their bound, ratios 0.21, coefficients off by at most 1.2e-7."""
    for fam in T.COEFF_FAMILIES:
        outs, label = T.coeff_case(M, B, C, fam)
        cf, sc, ra = check_coeff(ops, outs, label, f"M={M} B={B} C={C} {fam}")
        if fam == "same":
            assert sc[0] == sc[1]
            if M == 2:
                assert ra[1] == 1.0 and ra[0] == 1.0 and cf[1] == 1.0 and cf[0] < 1.0


@pytest.mark.parametrize("B,C", T.COEFF_BRANCH_SHAPES)
def test_ogm_coeff_three_modality_branches(ops, B, C):
    for branch, which in zip(T.COEFF_BRANCHES, (1, 2, 0)):
        outs, label = T.coeff_branch_case(B, C, branch)
        cf, _sc, _ra = check_coeff(ops, outs, label, f"B={B} C={C} {branch}")
        assert cf[which] < 0.99 and all(cf[m] == 1.0 for m in range(3) if m != which)


@pytest.mark.parametrize("bad", [-1, "C"])
def test_ogm_coeff_bad_label_is_nan(ops, bad):
    """A label outside [0, C): NaN scores and ratios, and the coefficient the rule then modulates is NaN as in the reference
    (relu and tanh pass a NaN on), never a silent 1.  The logits are a whole allocation each: nothing lies behind them to read."""
    for M, B, C in ((2, 5, 6), (3, 70, 101)):
        outs, label = T.coeff_case(M, B, C, "normal")
        label = label.clone()
        label[B // 2] = C if bad == "C" else -1
        cf, sc, ra = run_coeff(ops, outs, label)
        assert np.isnan(sc).all() and np.isnan(ra).all(), (sc, ra)
        assert np.isnan(cf[0]) and (cf[1:] == 1.0).all(), cf


# ---- 3. SGD ------------------------------------------------------------------------------------------------------------------------------
GUARD, SENTINEL = 16, 123.0


def banded(x, off):
    """`x` inside a larger device allocation: GUARD + off floats in front (the range starts `off` floats past a 16-byte boundary)."""
    n = len(x)
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 * off
    return buf, view


def guards_intact(buf, off, n):
    return bool((buf[:GUARD + off] == SENTINEL).all() and (buf[GUARD + off + n:] == SENTINEL).all())


def run_sgd(ops, c, off_p=0, off_g=None, off_b=None):
    """The steps of a case through mla_sgd_step -> [(p, buf) after each], with the guard bands checked after every step."""
    off_g = off_p if off_g is None else off_g
    off_b = off_p if off_b is None else off_b
    n = len(c.p)
    pbuf, p = banded(c.p, off_p)
    bbuf, b = banded(c.buf, off_b)
    out = []
    for k, g in enumerate(c.gs):
        gbuf = gd = None
        if g is not None:
            gbuf, gd = banded(g, off_g)
        ops.sgd_step(p, gd, b, T.SGD_LR, T.SGD_MOM, T.SGD_WD, k == 0)
        torch.cuda.synchronize()
        assert guards_intact(pbuf, off_p, n) and guards_intact(bbuf, off_b, n), f"n={n} step {k}: a guard band was written"
        if gbuf is not None:
            assert guards_intact(gbuf, off_g, n) and (gd.cpu().numpy() == g).all(), "the gradient is read-only"
        out.append((p.cpu().numpy(), b.cpu().numpy()))
    return out


def check_sgd_exact(ops, n, off_p=0, off_g=None, off_b=None):
    """Both exact families: three steps with |p| <= 4/16, two steps with |p| <= 7/16 (tail_model.sgd_case)."""
    for wide in (False, True):
        c = T.sgd_case(n, wide=wide)
        for k, ((p, b), (p64, b64)) in enumerate(zip(run_sgd(ops, c, off_p, off_g, off_b), T.sgd_run(c))):
            name = f"sgd n={n} wide={wide} offsets p={off_p} g={off_g} buf={off_b} step {k}"
            assert_bits(p, p64.astype(F32), name + ": p")
            assert_bits(b, b64.astype(F32), name + ": buf")


@pytest.mark.parametrize("n", T.SGD_SIZES)
def test_sgd_is_exact(ops, n):
    """Three steps (first, steady, g = None) on the 2^-4 grid, bit for bit against fp64; n = 4096 * 256 * 4 + 7 takes a second trip of
    the capped grid-stride loop and the scalar tail."""
    check_sgd_exact(ops, n)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_sgd_misaligned_range(ops, off):
    """p, g and buf start `off` floats past a 16-byte boundary, as the slices flat[o:o+n] of FusedSGD._launch_segments do: scalar head up
    to p's first boundary, float4 body, scalar tail; the floats before and after the range are untouched."""
    for n in T.SGD_SMALL:
        check_sgd_exact(ops, n, off)


@pytest.mark.parametrize("n,off,off_g", [(1027, 1, 3), (1023, 0, 2), (5, 2, 0), (4, 3, 1)])
def test_sgd_gradient_misaligned_on_its_own(ops, n, off, off_g):
    check_sgd_exact(ops, n, off, off_g=off_g)


@pytest.mark.parametrize("n,off,off_b", [(1027, 0, 1), (1023, 3, 2), (3, 1, 0), (5, 2, 3)])
def test_sgd_state_misaligned_against_p(ops, n, off, off_b):
    """buf at another misalignment than p: no common 16-byte grid, the whole range runs scalar."""
    check_sgd_exact(ops, n, off, off_b=off_b)


def test_sgd_result_does_not_depend_on_the_offset(ops):
    """Non-exact random input, two steps: an element lands in the scalar head, the float4 body or the tail depending on the start
    offset, and on the all-scalar launch when buf is off p; its result is the same bits everywhere."""
    c = T.sgd_random_case(1027)
    base = run_sgd(ops, c, 0)
    for off_p, off_b in ((1, None), (2, None), (3, None), (0, 1)):
        for k, ((p, b), (p0, b0)) in enumerate(zip(run_sgd(ops, c, off_p, off_b=off_b), base)):
            assert_bits(p, p0, f"offset {off_p} (buf {off_b}) vs 0, step {k}: p")
            assert_bits(b, b0, f"offset {off_p} (buf {off_b}) vs 0, step {k}: buf")
    p64, b64 = T.sgd_model(c.p, c.gs[0], c.buf, True)
    assert np.abs(base[0][0] - p64).max() <= 2.0 ** -23 * np.abs(p64).max() and np.abs(base[0][1] - b64).max() <= 2.0 ** -23 * np.abs(b64).max()


def test_fused_sgd_steps_a_head_whose_bias_is_misaligned(ops):
    """FusedSGD over SharedHead(70, 3): C * D = 210, so the bias slice starts 8 bytes off a 16-byte boundary.  Step 1 with the bias
    gradient None, step 2 with both gradients, step 3 with the weight gradient None: the per-parameter launches of
    FusedSGD._launch_segments.  Bit-equal to O.sgd_step per parameter (the inputs are exact)."""
    from mla_hip import FusedSGD, SharedHead
    head = SharedHead(T.HEAD_D, T.HEAD_C, seed=0)
    W, b, steps = T.head_case()
    with torch.no_grad():
        head.weight.copy_(W)
        head.bias.copy_(b)
    assert head.bias.data_ptr() % 16 != 0
    opt = FusedSGD(head.parameters(), lr=T.SGD_LR, momentum=T.SGD_MOM, weight_decay=T.SGD_WD)
    for k, ((gW, gb), (wW, wb)) in enumerate(zip(steps, T.head_run())):
        head.weight.grad = None if gW is None else gW.cuda()
        head.bias.grad = None if gb is None else gb.cuda()
        opt.step()
        torch.cuda.synchronize()
        assert_bits(head.weight.detach().cpu().numpy(), wW.float().numpy(), f"step {k}: weight")
        assert_bits(head.bias.detach().cpu().numpy(), wb.float().numpy(), f"step {k}: bias")


# ---- 4. scale_by_device_scalar, colsum, bn_invstd -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.SCALE_SIZES)
def test_scale_by_device_scalar(ops, n):
    """x *= *scalar: one fp32 product is correctly rounded, so torch.equal against x * float32(s); 2048 * 256 + 3 elements cross the
    block cap; n = 0 is a no-op (on a live pointer: an empty tensor has none)."""
    from mla_hip import _lib
    for s in T.SCALE_SCALARS:
        x = T.scale_case(max(n, 1))
        buf, view = banded(x, 0)
        sc = torch.tensor([s], device="cuda", dtype=torch.float32)
        if n == 0:
            assert _lib.load().mla_scale_by_device_scalar(view.data_ptr(), sc.data_ptr(), 0, ops.cur_stream()) == 0
            torch.cuda.synchronize()
            assert_bits(view.cpu().numpy(), x, "n = 0")
        else:
            ops.scale_by_device_scalar(view, sc)
            torch.cuda.synchronize()
            assert torch.equal(view.cpu(), torch.from_numpy(x) * torch.tensor(s, dtype=torch.float32)), f"n={n} s={s}"
        assert guards_intact(buf, 0, max(n, 1))


@pytest.mark.parametrize("B,D", T.COLSUM_SHAPES)
def test_colsum_is_exact(ops, B, D):
    x = T.colsum_case(B, D)
    r = torch.full((D + 8,), NAN, device="cuda")
    ops.colsum(dev(x), r[:D], T.COLSUM_SCALE)
    torch.cuda.synchronize()
    assert_bits(r[:D].cpu().numpy(), (x.astype(F64).sum(0) * T.COLSUM_SCALE).astype(F32), f"colsum {B}x{D}")
    assert torch.isnan(r[D:]).all()


@pytest.mark.parametrize("n", T.INVSTD_SIZES)
def test_bn_invstd_vs_fp64(ops, n):
    """1 / sqrt(var + eps) within 2 fp32 ulp of fp64: one rounded add (a quarter ulp after the root), a correctly rounded sqrtf and
    divide.  Measured on an MI355X: 1.62 ulp at worst."""
    var, want = T.invstd_case(n)
    out = torch.full((n + 8,), NAN, device="cuda")
    ops.bn_invstd(dev(var), out[:n], T.INVSTD_EPS)
    torch.cuda.synchronize()
    err = np.abs(out[:n].cpu().numpy().astype(F64) - want) / T.ulp32(want)
    print(f"bn_invstd n={n}: worst {err.max():.2f} ulp")
    assert (err <= 2).all() and torch.isnan(out[n:]).all()


# ---- 5. GS projection --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,C", T.GS_CASES)
def test_gs_project_vs_fp64(ops, D, C):
    """Two consecutive calls (the second from a non-identity Pl) against utils/utils.py:34-41 on doubles, Pl and G within 2e-5 of
    max |want|; the workspace starts as NaN, so a class or row that is not written shows; ||Pl||_F = 1 within 1e-6.
    Measured on an MI355X: at most 1.6 % of the tolerance."""
    c = T.gs_case(D, C)
    Pl, G = torch.eye(D, device="cuda"), dev(c.G)
    ws = torch.full((ops.gs_ws_elems(D, C),), NAN, device="cuda")
    for call in range(2):
        ops.gs_project(Pl, dev(c.rs[call]), G, T.GS_ALPHA, ws)
        torch.cuda.synchronize()
        wPl, wG = c.want[call]
        for name, got, want in (("Pl", Pl, wPl), ("G", G, wG)):
            got = got.cpu().double()
            assert torch.isfinite(got).all(), f"D={D} C={C} call {call}: {name} not fully written"
            err, tol = (got - want).abs().max().item(), T.GS_RTOL * want.abs().max().item()
            print(f"gs D={D} C={C} call {call} {name}: error / tolerance = {err / tol:.3g}")
            assert err <= tol, (name, call, err, tol)
        assert abs(Pl.cpu().double().norm().item() - 1.0) <= 1e-6
        ws.fill_(NAN)


# ---- 6. evaluation fusion ------------------------------------------------------------------------------------------------------------------
def run_eval(ops, outs, label, dynamic, alphas, calls=1):
    M, C = len(outs), outs[0].shape[1]
    counts = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)
    w = torch.full((3,), -7.0, device="cuda")
    d = [dev(o) for o in outs]
    lab = dev(label, torch.int64)
    for _ in range(calls):
        ops.eval_fuse(d, lab, counts, w, dynamic, list(alphas))
    torch.cuda.synchronize()
    return w.cpu().numpy(), counts.view(2 + M, C).cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("M,B,C", T.EVAL_FIXED_SHAPES)
def test_eval_fuse_fixed_weights_counts_are_exact(ops, M, B, C):
    """Integer logits with exact ties, alphas (0.5, 0.5) / (0.5, 0.25, 0.25): the fused values are exact, the arg-max is the first
    maximum; B on both sides of the 256-thread row stride; a second call accumulates into the same counters."""
    outs, label = T.eval_fixed_case(M, B, C)
    al = T.EVAL_ALPHAS[M]
    want = T.eval_counts(outs, label, al)
    w, counts = run_eval(ops, outs, label, False, al)
    assert (w[:M] == np.array(al, dtype=F32)).all() and (w[M:] == -7.0).all()
    assert (counts == want).all(), (counts, want)
    _w, counts2 = run_eval(ops, outs, label, False, al, calls=2)
    assert (counts2 == 2 * want).all()


@pytest.mark.parametrize("M,B,C", T.EVAL_DYN_SMALL)
def test_eval_fuse_dynamic_small(ops, M, B, C):
    """Entropy-gated weights within 1e-5 of O.valid_batch on doubles; counts exact (every row's fused top-2 margin is above 1e-4)."""
    outs, label = T.eval_small_case(M, B, C)
    w_ref, c_ref = O.valid_batch([torch.from_numpy(o).double() for o in outs], torch.from_numpy(label), C, True, [])
    w, counts = run_eval(ops, outs, label, True, T.EVAL_ALPHAS[M])
    print(f"eval dynamic M={M} B={B} C={C}: weights off by {np.abs(w[:M] - np.array(w_ref)).max():.3g}")
    assert (np.abs(w[:M].astype(F64) - np.array(w_ref)) <= 1e-5).all(), (w, w_ref)
    assert (counts == c_ref.numpy()).all()


@pytest.mark.parametrize("B,C", T.EVAL_DYN_STRIDE)
def test_eval_fuse_dynamic_crosses_the_stride(ops, B, C):
    """The entropy difference of the two modalities sits entirely behind the 256-thread stride (columns c >= 256, or the row r = 256):
    a kernel that drops the last column or row is off by all of it (0.9 ... 1.5).  Recovered from the weights, -ln(w_m / w_max), it
    must match fp64 within 2 (B + 264) 2^-24 max_m ent_m, the worst case of the kernel's serial fp32 sums.

    Measured on an MI355X, |dent_kernel - dent_ref| and its share of the bound: (257, 6) 1.8e-6, 0.1 %; (8, 257) 6.8e-6, 0.05 %;
    (257, 300) 3.1e-3, 3 %."""
    outs, label = T.eval_stride_case(B, C)
    w_ref, ent = T.gating(outs)
    w, counts = run_eval(ops, outs, label, True, (0.5, 0.5))
    dev_ = np.abs(T.dent_of(w[:2]) - T.dent_of(w_ref)).max()
    tol = T.dent_tol(B, ent)
    print(f"eval stride B={B} C={C}: weights {w[:2]}, fp64 {w_ref}; entropy difference off by {dev_:.3g} = {dev_ / tol:.3g} of the bound {tol:.3g}")
    assert dev_ <= tol
    assert abs(float(w[0]) + float(w[1]) - 1) <= 1e-6
    assert (counts[0] == np.bincount(label, minlength=C)).all()


@pytest.mark.parametrize("bad", [-1, "C"])
def test_eval_fuse_bad_label_poisons_the_weights_only(ops, bad):
    """A bad label at row 200 of 257 (a thread of the fourth wave; thread 0 writes weights_out[0]): weights_out[0] is NaN, the row is
    counted nowhere, every other row's counts are intact."""
    M, B, C = 2, 257, 6
    outs, label = T.eval_fixed_case(M, B, C)
    label = label.copy()
    label[T.EVAL_BAD_ROW] = C if bad == "C" else -1
    want = T.eval_counts(outs, label, T.EVAL_ALPHAS[M])
    assert want[0].sum() == B - 1
    w, counts = run_eval(ops, outs, label, False, T.EVAL_ALPHAS[M])
    assert np.isnan(w[0]) and w[1] == F32(0.5)
    assert (counts == want).all()
