"""fp64 torch restatement of the reference's SumFusion, FiLM and GatedFusion (models/fusion_modules.py:5-13, 38-67, 70-98) with mean-
reduced cross entropy, every gradient by autograd, and the inputs the fusion-head kernels (csrc/fusion_head.hip) are tested on.
tests/golden/make_fusion_golden.py holds it to the reference's own modules (1e-12) before it writes fusion_small.npz; test_fusion_cpu.py
holds it to that fixture; test_fusion_gpu.py holds the kernels to it.  Not product code.

Parameter names are the reference's (`fc_x.weight` ...).  `run(method, x, y, params, labels, flag, inv)` returns a dict: `out`, `loss`,
`loss_a` / `loss_v` and `out_a` / `out_v` (sum, at `bias_scale`), `h` / `hx`, `hy`, `z`, `dlogits`, `d<param name>`, `dx`, `dy` -- all fp64.
A label outside [0, C): NaN loss, zero dlogits row (the head family's policy).
"""
import functools
from types import SimpleNamespace

import torch

from exact import assert_sum_budget, case_seed, rand_ints
from oracle import mla_oracle as O

F64, F32 = torch.float64, torch.float32
PARAMS = {"sum": ("fc_x", "fc_y"), "film": ("fc", "fc_out"), "gated": ("fc_x", "fc_y", "fc_out")}
INV = 2.0 ** -7                    # inv_batch of the exact classes (head_exact.INV)


def param_shapes(method, D, C):
    """name -> shape, in the reference's registration order."""
    lin = {"sum": [("fc_x", C, D), ("fc_y", C, D)], "film": [("fc", 2 * D, D), ("fc_out", C, D)],
           "gated": [("fc_x", D, D), ("fc_y", D, D), ("fc_out", C, D)]}[method]
    return {f"{n}.{part}": shp for n, o, i in lin for part, shp in (("weight", (o, i)), ("bias", (o,)))}


class ExactGate(torch.autograd.Function):
    """sigmoid evaluated in fp32 as the kernel does, 1 / (1 + exp(-h)), and carried in fp64: on the exact inputs (h <= -128, 0, >= 32)
    the gate is exactly 0, 0.5 or 1 and g (1 - g) exactly 0 or 0.25, where fp64's own sigmoid(-128) would be 2.6e-56."""

    @staticmethod
    def forward(ctx, h):
        g = (1.0 / (1.0 + torch.exp(-h.float()))).double()
        ctx.save_for_backward(g)
        return g

    @staticmethod
    def backward(ctx, dg):
        (g,) = ctx.saved_tensors
        return dg * (g * (1.0 - g))


def ce(out, labels, inv):
    """(loss, ok rows): -sum log softmax(out)[label] * inv over the rows with a label in [0, C); NaN when any row has none."""
    B, C = out.shape
    labels = torch.as_tensor(labels).long()
    ok = (labels >= 0) & (labels < C)
    lab = labels.clamp(0, C - 1)
    rows = -torch.log_softmax(out, 1)[torch.arange(B), lab] * inv
    loss = torch.where(ok, rows, torch.zeros((), dtype=out.dtype)).sum()
    return loss, ok


def run(method, x, y, params, labels, flag=True, inv=None, bias_scale=1.0, gate=torch.sigmoid):
    """`flag`: x_film / x_gate.  `gate`: torch.sigmoid, or ExactGate.apply on the exact inputs."""
    x, y = x.to(F64).clone().requires_grad_(True), y.to(F64).clone().requires_grad_(True)
    P = {k: v.to(F64).clone().requires_grad_(True) for k, v in params.items()}
    B = x.shape[0]
    inv = 1.0 / B if inv is None else inv
    r = {}
    lin = lambda n, t: t @ P[n + ".weight"].T + P[n + ".bias"]                   # noqa: E731
    if method == "sum":
        out = lin("fc_x", x) + lin("fc_y", y)
        with torch.no_grad():
            r["out_a"] = x @ P["fc_x.weight"].T + P["fc_x.bias"] * bias_scale
            r["out_v"] = y @ P["fc_y.weight"].T + P["fc_y.bias"] * bias_scale
            r["loss_a"], r["loss_v"] = ce(r["out_a"], labels, inv)[0], ce(r["out_v"], labels, inv)[0]
    elif method == "film":
        film, t = (x, y) if flag else (y, x)
        h = lin("fc", film)
        D = x.shape[1]
        z = h[:, :D] * t + h[:, D:]
        out = lin("fc_out", z)
        r["h"], r["z"] = h.detach(), z.detach()
    else:
        hx, hy = lin("fc_x", x), lin("fc_y", y)
        z = gate(hx) * hy if flag else hx * gate(hy)
        out = lin("fc_out", z)
        r["hx"], r["hy"], r["z"] = hx.detach(), hy.detach(), z.detach()
    out.retain_grad()
    loss, ok = ce(out, labels, inv)
    loss.backward()
    r["out"] = out.detach()
    r["loss"] = loss.detach() if bool(ok.all()) else torch.tensor(float("nan"), dtype=F64)
    if not bool(ok.all()):
        for k in ("loss_a", "loss_v"):
            if k in r:
                r[k] = torch.tensor(float("nan"), dtype=F64)
    r["dlogits"] = out.grad
    r["dx"], r["dy"] = x.grad, y.grad
    for k, v in P.items():
        r["d" + k] = v.grad
    return r


# ---- dense inputs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(method, B, D, C):
    """Head-like random features and xavier-normal parameters times 4 (biases random too), so neither the softmax nor the gate is flat
    or saturated."""
    seed = case_seed(B, D, C, len(method)) + 9000
    x = O.portable_normal(seed, (B, D), stream=31, mean=0.3, std=0.7)
    y = O.portable_normal(seed + 1, (B, D), stream=32, mean=0.3, std=0.7)
    params = {}
    for i, (k, shp) in enumerate(param_shapes(method, D, C).items()):
        if k.endswith("weight"):
            params[k] = O.portable_normal(seed + 10 + i, shp, stream=33) * (1.5 * (2.0 / (shp[0] + shp[1])) ** 0.5)
        else:
            params[k] = O.portable_normal(seed + 10 + i, shp, stream=34) * 0.25
    return SimpleNamespace(B=B, D=D, C=C, x=x, y=y, params=params, labels=O.portable_labels(seed, B, C))


# ---- exactly-summable inputs ------------------------------------------------------------------------------------------------------------
# Every value is a small integer (features, hidden weights) or a multiple of 1/4 (output weights), so every product and every partial
# sum of every stage is exact in fp32 in any order (assert_sum_budget on the sums of |terms|).  The last feature column is 1 in x and y
# and carries, in the hidden layers, what the test wants the pre-activations to be; all other hidden weights are zero except a +-1 on
# the diagonal in FiLM (gamma and beta then vary with the features).  The output layer carries head_exact's SAT code in its first seven
# columns (`sat`: one-hot softmax, dlogits 0 or +-INV) or is zero with a constant bias (`uni`: equal logits, p = fl(1 / C)).
GATE_H = (-128.0, 0.0, 32.0)               # gated pre-activations: sigmoid is exactly 0, 0.5, 1 in fp32
AMP, NBITS = 16.0, 7                       # the winner's logit leads by 2 * AMP^2 = 512 minus the noise: asserted >= 128


def _code(classes):
    bits = (torch.as_tensor(classes).long().reshape(-1, 1) >> torch.arange(NBITS)) & 1
    return (bits.double() * 2 - 1).float() * AMP


@functools.lru_cache(maxsize=None)
def exact_case(method, B, D, C, pattern, flag=True):
    """pattern 'sat' | 'uni'.  The winner class of a row is coded in z's first seven columns: the hidden layers are built so that z there
    equals the +-32 code of the row's winner (sum: x carries it directly)."""
    seed = case_seed(B, D, C, len(method), int(flag), len(pattern)) * 16
    win = rand_ints((B,), 0, C - 1, seed + 1)
    win[0] = C - 1
    labels = win.clone()
    for r in range(B):                                                    # every third row: the label is the runner-up, not the winner
        w = int(win[r])
        setbits = [k for k in range(NBITS) if w >> k & 1]
        if C > 1 and r % 3 != 0:
            labels[r] = w ^ (1 << setbits[r % len(setbits)]) if setbits else 1
    x = rand_ints((B, D), -2, 2, seed + 2).float()
    y = rand_ints((B, D), -2, 2, seed + 3).float()
    x[:, D - 1] = 1.0
    y[:, D - 1] = 1.0
    code = _code(win)
    shapes = param_shapes(method, D, C)
    P = {k: torch.zeros(s) for k, s in shapes.items()}
    # noise columns of the output layers: at most 16, on both sides of the 64- and 256-column boundaries, so that the noise of a logit
    # (<= 16 * 8 * 3/4 per layer) cannot close the 2 * AMP^2 gap between the winner and the runner-up
    noise = torch.zeros(D)
    noise[[d for d in (7, 8, 62, 63, 64, 65, 127, 128, 255, 256, 257, 319, 320, D // 2, D - 3, D - 2) if NBITS <= d < D - 1]] = 1.0
    Wout = (rand_ints((C, D), -3, 3, seed + 4, nonzero=True).double() / 4).float() * noise
    Wout[:, :NBITS] = _code(torch.arange(C))
    bout = (rand_ints((C,), -3, 3, seed + 5).double() / 4).float()
    if pattern == "uni":
        Wout, bout = torch.zeros((C, D)), torch.full((C,), 0.75)
    if method == "sum":
        x[:, :NBITS] = code
        y[:, :NBITS] = 0.0
        P["fc_x.weight"], P["fc_x.bias"] = Wout, bout
        Wy = (rand_ints((C, D), -3, 3, seed + 6, nonzero=True).double() / 4).float() * noise
        P["fc_y.weight"] = torch.zeros((C, D)) if pattern == "uni" else Wy
        P["fc_y.bias"] = torch.zeros(C) if pattern == "uni" else (rand_ints((C,), -3, 3, seed + 7).double() / 4).float()
    elif method == "film":
        # gamma = +-film (diagonal), beta = film's neighbour column + an integer bias; on the code columns gamma = 0 and beta = the code:
        # the film feature carries the code in its first seven columns and beta copies it
        film = x if flag else y
        film[:, :NBITS] = code
        W, b = P["fc.weight"], P["fc.bias"]
        sign = rand_ints((D,), -1, 1, seed + 8, nonzero=True).float()
        for d in range(NBITS, D):
            W[d, d] = sign[d]                                             # gamma_d = +-film_d
            W[D + d, (d + 1) % D if (d + 1) % D >= NBITS else D - 1] = 1.0    # beta_d = a film column
        for d in range(NBITS):
            W[D + d, d] = 1.0                                             # beta_d = code, gamma_d = 0
        b[D + NBITS:] = rand_ints((D - NBITS,), -2, 2, seed + 9).float()
        P["fc_out.weight"], P["fc_out.bias"] = Wout, bout
    else:
        # hidden pre-activations from the constant-1 column: the gate side draws from GATE_H per column (+ nothing else), the other side
        # is a signed copy of its feature; on the code columns the gate is 1 (h = 32) and the other side is the code
        gx, other = (x, y) if flag else (y, x)
        gname, oname = ("fc_x", "fc_y") if flag else ("fc_y", "fc_x")
        other[:, :NBITS] = code
        hsel = rand_ints((D,), 0, 2, seed + 10)
        hsel[:NBITS] = 2
        hsel[NBITS:NBITS + 3] = torch.tensor([0, 1, 2])                   # every gate value occurs
        P[gname + ".bias"] = torch.tensor(GATE_H)[hsel] * 2               # bias 2 h, weight -h on the constant-1 column: h in total,
        P[gname + ".weight"][:, D - 1] = -torch.tensor(GATE_H)[hsel]      # so a dropped bias or column shows
        sign = rand_ints((D,), -1, 1, seed + 11, nonzero=True).float()
        sign[:NBITS] = 1.0
        P[oname + ".weight"][torch.arange(D), torch.arange(D)] = sign
        P[oname + ".weight"][D - 1, D - 1] = 0.0
        P[oname + ".bias"][D - 1] = 1.0
        P["fc_out.weight"], P["fc_out.bias"] = Wout, bout
    c = SimpleNamespace(method=method, B=B, D=D, C=C, pattern=pattern, flag=flag, x=x, y=y, params=P, labels=labels, win=win)
    check_exact_case(c)
    return c


def check_exact_case(c):
    """The conditions the exact comparison rests on, proven on the CPU: integer grids and sum budgets of every stage, the gate values,
    and the softmax pattern (saturated with margin >= 128, or all logits equal)."""
    quarter = lambda t: torch.equal(t * 4, (t * 4).round())                        # noqa: E731
    for t in (c.x, c.y, *c.params.values()):
        assert quarter(t), "operand off the quarter grid"
    gate = ExactGate.apply if c.method == "gated" else torch.sigmoid
    r = run(c.method, c.x, c.y, c.params, c.labels, c.flag, INV, gate=gate)
    D = c.D
    if c.method == "gated":
        hg = r["hx"] if c.flag else r["hy"]
        assert set(hg.unique().tolist()) <= set(GATE_H) and len(hg.unique()) == 3, "gated pre-activations off {-128, 0, 32}"
        g32 = 1.0 / (1.0 + torch.exp(-hg.float()))
        assert set(g32.unique().tolist()) == {0.0, 0.5, 1.0}, "the fp32 gate is not exactly 0 / 0.5 / 1"
        assert set((g32 * (1 - g32)).unique().tolist()) == {0.0, 0.25}
    # budgets, in units of 1/16 (quarters times quarters), of the forward sums with |terms|
    ax, ay = c.x.abs().double(), c.y.abs().double()
    for n in PARAMS[c.method]:
        Wa = c.params[n + ".weight"].abs().double()
        src = r["z"].abs() if n == "fc_out" else (ay if (n == "fc_y" or (n == "fc" and not c.flag)) else ax)
        assert_sum_budget(((src @ Wa.T + c.params[n + ".bias"].abs().double()) * 16).max(), f"{c.method} {n} forward")
    out = r["out"]
    if c.pattern == "uni":
        assert bool((out == out[:, :1]).all()), "UNI: the logits of a row differ"
    elif c.C > 1:
        top = out.topk(2, dim=1).values
        assert (top[:, 0] - top[:, 1]).min().item() >= 128.0, "SAT: margin below 128"
        assert torch.equal(out.argmax(1), c.win)
    if c.pattern == "uni":
        return r        # dlogits = (fl(1 / C) - onehot) INV is an fp32 rounding: only what it cannot reach is compared exactly
    # backward, SAT: dlogits is 0 or +-INV; every term of every gradient sum is a multiple of u = INV / 64, and the sums of |terms|,
    # formed here from the actual operands, stay below 2^24 u
    u = INV / 64

    def budget(a, b, name):
        assert_sum_budget((a.abs().double() @ b.abs().double()).max() / u, f"{c.method} {name}")
    dl = torch.where(r["dlogits"].abs() < INV / 2, torch.zeros((), dtype=F64), r["dlogits"])
    assert set(dl.abs().unique().tolist()) <= {0.0, INV}
    P = c.params
    if c.method == "sum":
        for n, src in (("fc_x", c.x), ("fc_y", c.y)):
            budget(dl.T, src, n + " dW")
            budget(dl, P[n + ".weight"], n + " dX")
        return r
    budget(dl.T, r["z"], "fc_out dW")
    budget(dl, P["fc_out.weight"], "dz")
    dz = dl @ P["fc_out.weight"].double()
    if c.method == "film":
        film, t = (c.x, c.y) if c.flag else (c.y, c.x)
        jobs = [("fc", torch.cat([dz * t.double(), dz], 1), film)]
    else:
        hg, ho = (r["hx"], r["hy"]) if c.flag else (r["hy"], r["hx"])
        g = ExactGate.apply(hg)
        dgate, dlin = dz * ho * (g * (1 - g)), dz * g
        jobs = [("fc_x", dgate if c.flag else dlin, c.x), ("fc_y", dlin if c.flag else dgate, c.y)]
    for n, dh, src in jobs:
        budget(dh.T, src, n + " dW")
        budget(dh, P[n + ".weight"], n + " dX")
    return r


def fp32_restatement_uni(C, labels, inv=INV):
    """dlogits of an all-equal row in fp32: (fl(1 / C) - onehot) * inv, one rounding each (head_exact's UNI class)."""
    B = len(labels)
    p = (torch.ones((), dtype=F32) / torch.tensor(float(C), dtype=F32))
    oh = torch.zeros((B, C), dtype=F32)
    oh[torch.arange(B), torch.as_tensor(labels).long()] = 1
    return (p - oh) * torch.tensor(inv, dtype=F32)
