"""mla_adam_step against an fp64 evaluation of torch.optim.Adam's single-tensor rule (amsgrad=False, maximize=False):

    g' = g + wd*p;  m = beta1*m + (1-beta1)*g';  v = beta2*v + (1-beta2)*g'*g'
    p -= (lr / (1-beta1^step)) * m / (sqrt(v)/sqrt(1-beta2^step) + eps)           (g None = zero gradient)

Inputs.  The C ABI carries lr, beta1, beta2, eps and wd as fp32, so each hyper-parameter set is rounded to fp32 first and the SAME
values go to the kernel, to the fp64 evaluation and to CPU torch.optim.Adam (beta2 = 0.999 is then 0.99900001287..., for all three).

Tolerance.  Nothing is fixed here: on the same inputs the test measures d, the largest absolute error of CPU fp32
torch.optim.Adam(foreach=False) against fp64, and the kernel's absolute error against fp64 may be at most 4 d plus one fp32 ulp of
the element, for each of p, m and v, after every one of five consecutive steps.  |g| spans nine decades, and so do m and v: one d
per tensor would test the largest decade only.  So the elements are grouped by the decade of |m| (fp64, after the step; decades with
fewer than 32 elements join the next larger one, which only loosens their bound towards the whole-tensor one), d is taken per group
and the kernel is held to 4 d + ulp inside each group -- never looser than one d per tensor.  Elements with p = 0 and g = 0 must stay
exactly 0.  Every case prints its d as the largest ratio d / (one ulp of the group's largest element); over all cases the run on the
MI355X host printed at most d_p = 2.05, d_v = 2.74 and d_m = 13774 (a decade that holds an element where g - m cancels; 0.4 ... 3
in the others).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402

GUARD, SENTINEL = 16, 123.0
SIZES = [1, 3, 4, 5, 255, 4099, 262147]
f32 = lambda x: float(np.float32(x))
# (lr, beta1, beta2, eps, wd): the reference's --cav_opti set (main.py:744-747, lr 1e-3 / 10 ... 1e-3), one without weight decay,
# one with a large weight decay and an eps that matters
HYPERS = [tuple(map(f32, h)) for h in ((1e-3, 0.95, 0.999, 1e-8, 5e-7), (1e-4, 0.9, 0.999, 1e-8, 0.0), (1e-2, 0.95, 0.999, 1e-3, 1e-2))]
STEPS = 5


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    return _ops


def make_case(n: int, seed: int, steps: int = STEPS):
    """p ~ N(0, 1); per step a gradient of random sign with |g| log-uniform in 1e-6 ... 1e3; every fifth element (from index 2)
    has p = 0 and g = 0 at every step, so its denominator is eps and it must stay exactly 0.  Step 3 (index 2) has g = None."""
    p = O.portable_normal(seed, (n,), stream=1)
    zero = (torch.arange(n) % 5) == 2
    p[zero] = 0.0
    gs = []
    for k in range(steps):
        u = torch.from_numpy(O.portable_uniform(seed + k, 2 * n, stream=2)).float()
        g = torch.where(u[:n] < 0.5, -1.0, 1.0) * torch.pow(10.0, u[n:] * 9.0 - 6.0)
        g[zero] = 0.0
        gs.append(None if k == 2 else g.float())
    return p.float(), gs, zero


def adam64(p, g, m, v, hp, step):
    lr, b1, b2, eps, wd = hp
    g = torch.zeros_like(p) if g is None else g.double()
    g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** step)) * m / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
    return p, m, v


def ulp32(x64: torch.Tensor) -> torch.Tensor:
    """fp32 unit in the last place at the magnitude of each fp64 element (2^-149 at zero)."""
    _m, e = torch.frexp(x64.abs().float())
    return torch.clamp(torch.ldexp(torch.ones_like(x64), (e - 24).to(torch.int32)), min=2.0 ** -149)


def groups_by_decade(m64: torch.Tensor, min_count: int = 32):
    """Index sets of the elements by floor(log10 |m|), largest decade first; a set with fewer than min_count elements is joined
    with the next smaller decade's until it has enough, and what is left at the end joins the last set made.  Exact zeros (the
    p = 0, g = 0 elements) are left out: they are checked for equality."""
    nz = torch.nonzero(m64 != 0).flatten()
    dec = torch.floor(torch.log10(m64[nz].abs())).long()
    out, cur = [], []
    for dv in sorted(set(dec.tolist()), reverse=True):
        cur.append(nz[dec == dv])
        if sum(len(c) for c in cur) >= min_count:
            out.append(torch.cat(cur))
            cur = []
    if cur:
        out = out[:-1] + [torch.cat(out[-1:] + cur)]
    return out


def banded(t: torch.Tensor, off: int, n: int):
    """`t` inside a larger device allocation: GUARD + off floats in front (start misaligned by `off` floats), GUARD behind."""
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(t)
    return buf, view


def guards_intact(buf: torch.Tensor, off: int, n: int) -> bool:
    return bool((buf[:GUARD + off] == SENTINEL).all() and (buf[GUARD + off + n:] == SENTINEL).all())


def run_case(ops, n, off, hp, off_g=None, off_m=None, seed=0, steps=STEPS):
    off_g = off if off_g is None else off_g
    off_m = off if off_m is None else off_m
    p0, gs, zero = make_case(n, 1000 + n + seed, steps)
    lr, b1, b2, eps, wd = hp
    # the three evaluations
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pt = p0.clone().requires_grad_(True)
    topt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    pbuf, pd = banded(p0, off, n)
    mbuf, md = banded(torch.zeros(n), off_m, n)
    vbuf, vd = banded(torch.zeros(n), off, n)
    dmax = {"p": 0.0, "m": 0.0, "v": 0.0}
    for k, g in enumerate(gs):
        step = k + 1
        p64, m64, v64 = adam64(p64, g, m64, v64, hp, step)
        pt.grad = torch.zeros(n) if g is None else g.clone()          # zeroed, not None: torch would skip a None gradient
        topt.step()
        st = topt.state[pt]
        assert int(st["step"]) == step
        gbuf = gd = None
        if g is not None:
            gbuf, gd = banded(g, off_g, n)
        ops.adam_step(pd, gd, md, vd, lr, b1, b2, eps, wd, step)
        torch.cuda.synchronize()
        groups = groups_by_decade(m64)
        for name, x64, xt, xk, buf, o in (("p", p64, pt.detach(), pd, pbuf, off), ("m", m64, st["exp_avg"], md, mbuf, off_m),
                                          ("v", v64, st["exp_avg_sq"], vd, vbuf, off)):
            et, ek, unit = (xt.double() - x64).abs(), (xk.cpu().double() - x64).abs(), ulp32(x64)
            for idx in groups:
                d = et[idx].max().item()
                dmax[name] = max(dmax[name], d / unit[idx].max().item())
                over = ek[idx] - (4 * d + unit[idx])
                w = idx[int(over.argmax())]
                assert over.max().item() <= 0, (f"n={n} off={off} step={step} {name}[{int(w)}]: kernel error {ek[w].item():.3e} > 4 * "
                                                f"{d:.3e} + {unit[w].item():.3e} (fp64 {x64[w].item():.9e}, kernel {xk[w].item():.9e})")
            assert guards_intact(buf, o, n), f"n={n} off={off} step={step}: guard band of {name} written"
            assert bool((xk.cpu()[zero] == 0).all()), f"{name}: p = 0, g = 0 elements must stay exactly 0"
        if gbuf is not None:
            assert guards_intact(gbuf, off_g, n) and torch.equal(gd.cpu(), g), "the gradient is read-only"
    print(f"adam n={n} off={off} hp={hp}: d_p={dmax['p']:.2f} d_m={dmax['m']:.2f} d_v={dmax['v']:.2f} ulp")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_vs_fp64(ops, n, off):
    """Every size (shorter than a float4, exactly one, ragged, one workgroup, 257 workgroups) at every start misalignment, p / g / m /
    v misaligned alike, under the three hyper-parameter sets."""
    for hp in HYPERS:
        run_case(ops, n, off, hp)


@pytest.mark.parametrize("n,off,off_g", [(4099, 1, 3), (255, 0, 2), (5, 2, 0)])
def test_adam_step_gradient_misaligned_on_its_own(ops, n, off, off_g):
    """g at another misalignment than p / m / v: the body keeps its 16-byte p / m / v accesses and loads g dword by dword."""
    run_case(ops, n, off, HYPERS[0], off_g=off_g)


@pytest.mark.parametrize("n,off,off_m", [(4099, 0, 1), (255, 3, 2), (3, 1, 0)])
def test_adam_step_state_misaligned_against_p(ops, n, off, off_m):
    """m at another misalignment than p: no common 16-byte grid, the whole range takes the scalar launch."""
    run_case(ops, n, off, HYPERS[2], off_m=off_m)


def test_adam_step_grid_stride(ops):
    """More float4s than the capped grid has threads (8 workgroups of 256 per CU): 4 * 256 * 8 * CUs + 7 elements, misaligned by one
    float, two steps against fp64 under the same bound."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    run_case(ops, 4 * 256 * 8 * cus + 7, 1, HYPERS[0], steps=2)


def test_adam_torch_op_and_argument_errors(ops):
    from mla_hip import MLAHipError
    p, m, v = torch.ones(8, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    g = torch.full((8,), 0.5, device="cuda")
    torch.ops.mla_hip.adam_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    torch.cuda.synchronize()
    assert torch.allclose(p.cpu(), torch.full((8,), 1 - 1e-3), atol=1e-7)          # step 1: m / sqrt(v) = sign(g)
    assert torch.allclose(m.cpu(), torch.full((8,), 0.05), atol=1e-8) and torch.allclose(v.cpu(), torch.full((8,), 2.5e-4), atol=1e-9)
    with pytest.raises(Exception):                                                  # no CPU implementation registered
        torch.ops.mla_hip.adam_step(p.cpu(), g.cpu(), m.cpu(), v.cpu(), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    with pytest.raises(MLAHipError, match="step must be >= 1"):
        ops.adam_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0)
    e = torch.empty(0, device="cuda")
    with pytest.raises(MLAHipError):
        ops.adam_step(e, e, e, e, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)                   # n == 0
    with pytest.raises(MLAHipError, match="same number of elements"):
        ops.adam_step(p, g[:4], m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
