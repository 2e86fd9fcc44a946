"""GPU: the sum / FiLM / gated fusion-head kernels (csrc/fusion_head.hip) against the fp64 restatement (fusion_model.py) -- dense inputs
within a derived bound, exactly-summable inputs bit for bit, the reference fixture, guards -- and JointTrainer / JointEvaluator with an
attached fusion against the protocol path.

The dense bound (`bounds`) is the serial-sum bound of every dot product, (K + 1) u sum |a_i b_i| with u = 2^-24 for K terms and the
bias, propagated to first order through the stage: an input error e_a of a enters a product a b as e_a |b|; softmax turns a logit error
e into at most 2 p max(e) plus its own roundings (expf's argument l - max rounds by u |l - max|, expf and the division by a few u, the
sum by C u); sigmoid turns e_h into g (1 - g) e_h + 4 u g.  The first-order terms are doubled to cover the second-order ones."""
import os

import numpy as np
import pytest
import torch

import fusion_model as F
from exact import assert_bitwise

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CASES = [("sum", True), ("film", True), ("film", False), ("gated", True), ("gated", False)]
# B in {1, 5, 64}; D in {64, 320, 512, 768}: below one 256-thread pass, a pass and a remainder, the two model sizes; C in {1, 6, 64, 65,
# 101, 128}: both softmax slots and their edge
SHAPES = [(1, 64, 1), (5, 320, 6), (64, 512, 64), (64, 768, 65), (5, 512, 101), (64, 320, 128)]


def dev(t):
    return t.cuda().contiguous()


def call_fused(method, x, y, P, labels, flag, inv, bias_scale=1.0):
    """The fused training call through torch.ops; results under the restatement's names."""
    import mla_hip  # noqa: F401
    T = torch.ops.mla_hip
    x, y, lab = dev(x), dev(y), dev(labels)
    p = {k: dev(v) for k, v in P.items()}
    if method == "sum":
        out, oa, ov, L, dWx, dbx, dWy, dby, dX, dY = T.fusion_sum_ce_fwd_bwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"],
                                                                             p["fc_y.bias"], lab, inv, bias_scale)
        r = {"out": out, "out_a": oa, "out_v": ov, "loss": L[0], "loss_a": L[1], "loss_v": L[2], "dfc_x.weight": dWx, "dfc_x.bias": dbx,
             "dfc_y.weight": dWy, "dfc_y.bias": dby, "dx": dX, "dy": dY}
    elif method == "film":
        film, t = (x, y) if flag else (y, x)
        out, h, z, L, dW, db, dWo, dbo, dfilm, dt = T.fusion_film_ce_fwd_bwd(film, t, p["fc.weight"], p["fc.bias"], p["fc_out.weight"],
                                                                             p["fc_out.bias"], lab, inv)
        r = {"out": out, "h": h, "z": z, "loss": L[0], "dfc.weight": dW, "dfc.bias": db, "dfc_out.weight": dWo, "dfc_out.bias": dbo,
             "dx": dfilm if flag else dt, "dy": dt if flag else dfilm}
    else:
        out, hx, hy, z, L, dWx, dbx, dWy, dby, dWo, dbo, dX, dY = T.fusion_gated_ce_fwd_bwd(
            x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], p["fc_out.weight"], p["fc_out.bias"], lab, flag, inv)
        r = {"out": out, "hx": hx, "hy": hy, "z": z, "loss": L[0], "dfc_x.weight": dWx, "dfc_x.bias": dbx, "dfc_y.weight": dWy,
             "dfc_y.bias": dby, "dfc_out.weight": dWo, "dfc_out.bias": dbo, "dx": dX, "dy": dY}
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in r.items()}


def call_split(method, x, y, P, dlogits, flag, scale):
    """The evaluation forward, then the autograd backward from a given dlogits."""
    import mla_hip  # noqa: F401
    T = torch.ops.mla_hip
    x, y, dl = dev(x), dev(y), dev(dlogits)
    p = {k: dev(v) for k, v in P.items()}
    if method == "sum":
        out, _oa, _ov = T.fusion_sum_fwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], 0.5)
        g = T.fusion_sum_bwd(x, y, p["fc_x.weight"], p["fc_y.weight"], dl, scale)
        names = ["dfc_x.weight", "dfc_x.bias", "dfc_y.weight", "dfc_y.bias", "dx", "dy"]
    elif method == "film":
        film, t = (x, y) if flag else (y, x)
        out, h, z = T.fusion_film_fwd(film, t, p["fc.weight"], p["fc.bias"], p["fc_out.weight"], p["fc_out.bias"])
        g = T.fusion_film_bwd(film, t, p["fc.weight"], p["fc_out.weight"], h, z, dl, scale)
        names = ["dfc.weight", "dfc.bias", "dfc_out.weight", "dfc_out.bias"] + (["dx", "dy"] if flag else ["dy", "dx"])
    else:
        out, hx, hy, z = T.fusion_gated_fwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], p["fc_out.weight"],
                                            p["fc_out.bias"], flag)
        g = T.fusion_gated_bwd(x, y, p["fc_x.weight"], p["fc_y.weight"], p["fc_out.weight"], hx, hy, z, dl, flag, scale)
        names = ["dfc_x.weight", "dfc_x.bias", "dfc_y.weight", "dfc_y.bias", "dfc_out.weight", "dfc_out.bias", "dx", "dy"]
    torch.cuda.synchronize()
    r = {n: v.cpu() for n, v in zip(names, g)}
    r["out"] = out.cpu()
    return r


def module_fused(method, c, flag, inv):
    """The fused training call through the module (mla_hip.fusion), whose workspace the caller can read: (dlogits (B, C), loss, out)."""
    from mla_hip import fusion as MF
    B, D = c.x.shape
    C = c.params[("fc_x" if method == "sum" else "fc_out") + ".weight"].shape[0]
    mod = (MF.SumFusion(D, C, "cuda", 0) if method == "sum" else
           MF.FiLM(D, D, C, flag, "cuda", 0) if method == "film" else MF.GatedFusion(D, D, C, flag, "cuda", 0))
    mod.load_state_dict(c.params)
    out, _om, L, _dX = mod.forward_backward([dev(c.x), dev(c.y)], dev(c.labels), inv, {})
    torch.cuda.synchronize()
    return mod._bufs(B, "")["ws"][:B * C].view(B, C).cpu(), L[0].cpu(), out.cpu()


# ---- the derived bound ---------------------------------------------------------------------------------------------------------------------
def _lin(a, W, b, e_a):
    """Error bound of a W^T + b (K terms and the bias), given the bound e_a of a."""
    K = a.shape[1]
    return (K + 1) * U * (a.abs() @ W.abs().T + b.abs()) + e_a @ W.abs().T


def _back(g, e_g, src, e_src, W):
    """Bounds of dW = g^T src (B terms), db = colsum g and din = g W (N terms)."""
    B, N = g.shape
    dW = (B + 1) * U * (g.abs().T @ src.abs()) + e_g.T @ src.abs() + g.abs().T @ e_src
    db = (B + 1) * U * g.abs().sum(0) + e_g.sum(0)
    din = None if W is None else (N + 1) * U * (g.abs() @ W.abs()) + e_g @ W.abs()
    return dW, db, din


def bounds_bwd(method, c, r, flag, inv):
    """The same for the autograd entry points mla_fusion_*_bwd fed the restatement's dlogits rounded to fp32 (e_dl = u |dl|, the only
    error of the given gradient) and the h / z of the forward kernels (their forward bounds): the gradient names only."""
    return {k: v for k, v in bounds(method, c, r, flag, inv, given_dl=True).items() if k.startswith("d")}


def bounds(method, c, r, flag, inv, given_dl=False):
    """name -> elementwise bound of |kernel - fp64| for the restatement result r (fp64) of case c."""
    P = {k: v.double() for k, v in c.params.items()}
    x, y = c.x.double(), c.y.double()
    zero = torch.zeros_like(x)
    b = {}
    if method == "sum":
        e_out = _lin(x, P["fc_x.weight"], P["fc_x.bias"], zero) + _lin(y, P["fc_y.weight"], P["fc_y.bias"], zero) + U * r["out"].abs()
        b["out_a"] = _lin(x, P["fc_x.weight"], P["fc_x.bias"], zero)
        b["out_v"] = _lin(y, P["fc_y.weight"], P["fc_y.bias"], zero)
        z, e_z, Wo = None, None, None
    elif method == "film":
        film, t = (x, y) if flag else (y, x)
        D = x.shape[1]
        e_h = _lin(film, P["fc.weight"], P["fc.bias"], zero)
        gamma = r["h"][:, :D]
        z, e_z = r["z"], e_h[:, :D] * t.abs() + e_h[:, D:] + 2 * U * ((gamma * t).abs() + r["h"][:, D:].abs())
        b["h"], Wo = e_h, P["fc_out.weight"]
    else:
        e_hx, e_hy = _lin(x, P["fc_x.weight"], P["fc_x.bias"], zero), _lin(y, P["fc_y.weight"], P["fc_y.bias"], zero)
        hg, ho, e_hg, e_ho = (r["hx"], r["hy"], e_hx, e_hy) if flag else (r["hy"], r["hx"], e_hy, e_hx)
        g = torch.sigmoid(hg)
        e_g = g * (1 - g) * e_hg + 4 * U * g
        z, e_z = r["z"], e_g * ho.abs() + g * e_ho + U * r["z"].abs()
        b["hx"], b["hy"], Wo = e_hx, e_hy, P["fc_out.weight"]
    if method != "sum":
        b["z"] = e_z
        e_out = _lin(z, Wo, P["fc_out.bias"], e_z)
    b["out"] = e_out
    # softmax / CE
    out = r["out"]
    C = out.shape[1]
    p = torch.softmax(out, 1)
    spread = (out.max(1, keepdim=True).values - out).max(1, keepdim=True).values
    rel = 2 * e_out.max(1, keepdim=True).values + (spread + C + 8) * U
    dl = r["dlogits"]
    e_dl = U * dl.abs() if given_dl else inv * p * rel + U * dl.abs()
    rowloss = -torch.log_softmax(out, 1)[torch.arange(len(out)), c.labels] * inv
    b["loss"] = (inv * rel).sum() + (len(out) + 2) * U * rowloss.abs().sum()
    if method == "sum":
        for n, src in (("fc_x", x), ("fc_y", y)):
            b[f"d{n}.weight"], b[f"d{n}.bias"], b["dx" if n == "fc_x" else "dy"] = _back(dl, e_dl, src, zero, P[n + ".weight"])
        return {k: 2 * v for k, v in b.items()}
    b["dfc_out.weight"], b["dfc_out.bias"], e_dz = _back(dl, e_dl, z, e_z, Wo)
    dz = dl @ Wo
    if method == "film":
        dh = torch.cat([dz * t, dz], 1)
        e_dh = torch.cat([e_dz * t.abs() + U * (dz * t).abs(), e_dz], 1)
        b["dfc.weight"], b["dfc.bias"], e_dfilm = _back(dh, e_dh, film, zero, P["fc.weight"])
        e_dt = e_dz * gamma.abs() + dz.abs() * e_h[:, :D] + U * (dz * gamma).abs()
        b["dx"], b["dy"] = (e_dfilm, e_dt) if flag else (e_dt, e_dfilm)
    else:
        s = g * (1 - g)
        e_s = e_g + 2 * U * s
        dgate, dlin = dz * ho * s, dz * g
        e_dgate = e_dz * ho.abs() * s + dz.abs() * e_ho * s + (dz * ho).abs() * e_s + 3 * U * dgate.abs()
        e_dlin = e_dz * g + dz.abs() * e_g + U * dlin.abs()
        (dhx, e_dhx), (dhy, e_dhy) = ((dgate, e_dgate), (dlin, e_dlin)) if flag else ((dlin, e_dlin), (dgate, e_dgate))
        b["dfc_x.weight"], b["dfc_x.bias"], b["dx"] = _back(dhx, e_dhx, x, zero, P["fc_x.weight"])
        b["dfc_y.weight"], b["dfc_y.bias"], b["dy"] = _back(dhy, e_dhy, y, zero, P["fc_y.weight"])
    return {k: 2 * v for k, v in b.items()}


def assert_within(got, ref, bound, name):
    worst = 0.0
    for k, bnd in bound.items():
        err = (got[k].double() - ref[k]).abs()
        ratio = (err / torch.as_tensor(bnd).clamp_min(1e-300)).max().item()
        worst = max(worst, ratio)
        print(f"{name} {k}: max err {err.max().item():.3e}, max err / bound {ratio:.3f}")
        assert bool((err <= bnd).all()), f"{name} {k}: max err / bound {ratio:.3f}"
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("method,flag", CASES)
def test_dense_kernels_vs_fp64_within_derived_bound(method, flag, shape):
    B, D, C = shape
    c = F.dense_case(method, B, D, C)
    inv = 1.0 / B
    ref = F.run(method, c.x, c.y, c.params, c.labels, flag, inv)
    got = call_fused(method, c.x, c.y, c.params, c.labels, flag, inv)
    assert_within(got, ref, bounds(method, c, ref, flag, inv), f"{method} {flag} {shape}")
    # two runs are bitwise equal; the evaluation forward gives the same `out`, the autograd backward from the fp32 dlogits of the
    # restatement at scale 0.5 exactly half of what it gives at scale 1 (a power of two)
    again = call_fused(method, c.x, c.y, c.params, c.labels, flag, inv)
    for k in got:
        assert_bitwise(again[k], got[k], f"{method} rerun {k}")
    dl = ref["dlogits"].float()
    one, half = call_split(method, c.x, c.y, c.params, dl, flag, 1.0), call_split(method, c.x, c.y, c.params, dl, flag, 0.5)
    assert_bitwise(one["out"], got["out"], f"{method} fwd out")
    for k in one:
        if k != "out":
            assert_bitwise(half[k], one[k] * 0.5, f"{method} bwd scale {k}")
    assert_within(one, ref, bounds_bwd(method, c, ref, flag, inv), f"{method} {flag} {shape} bwd")


@pytest.mark.parametrize("shape", [(1, 64, 1), (5, 320, 65), (64, 768, 128), (5, 512, 6)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("method,flag", CASES)
def test_exact_inputs_bit_for_bit(method, flag, shape):
    B, D, C = shape
    for pattern in ("sat", "uni"):
        c = F.exact_case(method, B, D, C, pattern, flag)                  # proves its conditions on the CPU (check_exact_case)
        ref = F.run(method, c.x, c.y, c.params, c.labels, flag, F.INV, gate=F.ExactGate.apply)
        got = call_fused(method, c.x, c.y, c.params, c.labels, flag, F.INV)
        if pattern == "sat":
            for k in got:
                if k == "loss_v":
                    # only x carries the winner's code: out_v (exact itself) is an ordinary softmax row, its reported loss a dense
                    # quantity: the CE part of `bounds` with an exact logit
                    ov = ref["out_v"]
                    spread = (ov.max(1).values - ov.min(1).values)
                    rows = -torch.log_softmax(ov, 1)[torch.arange(B), c.labels] * F.INV
                    bound = 2 * ((F.INV * (spread + C + 8) * U).sum() + (B + 2) * U * rows.abs().sum()).item()
                    assert abs(got[k].item() - ref[k].item()) <= bound, (got[k].item(), ref[k].item(), bound)
                    continue
                assert_bitwise(got[k], ref[k].float(), f"{method} {flag} {shape} SAT {k}")
        else:
            # equal logits: dlogits = (fl(1 / C) - onehot) INV is an fp32 rounding the fp64 model does not make.  Exact: everything before
            # the softmax, and every gradient behind a zero output weight (FiLM / gated: dz = 0)
            for k in ("out", "out_a", "out_v", "h", "hx", "hy", "z"):
                if k in got:
                    assert_bitwise(got[k], ref[k].float(), f"{method} {flag} {shape} UNI {k}")
            # dlogits itself, read from the caller-owned workspace of the module's fused call: bit-equal to the fp32 restatement
            dl32 = F.fp32_restatement_uni(C, c.labels)
            dl_got, loss_mod, out_mod = module_fused(method, c, flag, F.INV)
            assert_bitwise(dl_got, dl32, f"{method} {flag} {shape} UNI dlogits")
            assert_bitwise(out_mod, got["out"], f"{method} UNI module out = op out")
            assert_bitwise(loss_mod, got["loss"], f"{method} UNI module loss = op loss")
            # loss = sum of B copies of logf(C) INV: the device's logf within 2 u, the sum within (B + 2) u
            want_loss = B * F.INV * float(np.log(C))
            assert abs(got["loss"].item() - want_loss) <= (B + 4) * U * want_loss, (got["loss"].item(), want_loss)
            # the output weights are zero: every gradient behind them is exactly zero
            zero = ("dx", "dy") if method == "sum" else [k for k in got if k.startswith("d") and "fc_out" not in k]
            for k in zero:
                assert not got[k].any(), f"{method} UNI {k} is not zero"
            # the gradients formed FROM dlogits (B-term sums of fp32 products): against fp64 on the fp32 dlogits, serial-sum bound
            dl64 = dl32.double()
            srcs = {"dfc_x": c.x, "dfc_y": c.y} if method == "sum" else {"dfc_out": ref["z"]}
            for n, src in srcs.items():
                for k, want, mag in ((n + ".weight", dl64.T @ src.double(), dl64.abs().T @ src.double().abs()),
                                     (n + ".bias", dl64.sum(0), dl64.abs().sum(0))):
                    err = (got[k].double() - want).abs()
                    assert bool((err <= (B + 1) * U * mag).all()), f"{method} UNI {k}: {err.max().item():.3e}"
            if B == 1:
                assert_bitwise(got["dfc_out.bias" if method != "sum" else "dfc_x.bias"], dl32[0], f"{method} UNI db = dlogits")


@pytest.mark.parametrize("method,flag", CASES)
def test_reference_fixture_within_derived_bound(method, flag, golden_dir):
    from test_fusion_cpu import load_case
    x, y, labels, params, want = load_case(golden_dir, method, flag)
    from types import SimpleNamespace
    c = SimpleNamespace(x=x, y=y, params=params, labels=labels)
    ref = F.run(method, x, y, params, labels, flag)
    got = call_fused(method, x, y, params, labels, flag, 1.0 / len(labels))
    bnd = bounds(method, c, ref, flag, 1.0 / len(labels))
    for k, v in want.items():
        if k in bnd and k in got:
            slack = 0.0 if v.dtype == torch.float64 else 2.0 ** -24 * v.abs().max().item()       # fp32-stored gradients
            err = (got[k].double() - v.double()).abs()
            assert bool((err <= bnd[k] + slack).all()), f"{method} {flag} fixture {k}: {err.max().item():.3e}"


@pytest.mark.parametrize("method", ["sum", "film", "gated"])
def test_guards_bad_label(method):
    """Output buffers with canaries on both sides stay intact; a bad label gives a NaN loss and a zero dlogits row (its gradients are
    those of the other rows)."""
    import mla_hip
    from mla_hip import ops
    B, D, C = 5, 320, 65
    c = F.dense_case(method, B, D, C)
    model_p = {k: dev(v) for k, v in c.params.items()}
    pool, views = [], {}

    def guarded(name, *shape):
        n = int(np.prod(shape))
        full = torch.full((n + 128,), 12345.0, device="cuda")
        pool.append(full)
        views[name] = full[64:64 + n].view(shape)
        return views[name]
    x, y = dev(c.x), dev(c.y)
    labels = c.labels.clone()
    labels[1] = C
    lab = dev(labels)
    ws = guarded("ws", ops.fusion_ws_elems(B, D, C))
    p = model_p
    if method == "sum":
        ops.fusion_sum_ce_fwd_bwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], lab, guarded("out", B, C),
                                  guarded("oa", B, C), guarded("ov", B, C), guarded("L", 3), guarded("dWx", C, D), guarded("dbx", C),
                                  guarded("dWy", C, D), guarded("dby", C), guarded("dX", B, D), guarded("dY", B, D), ws, 1.0 / B)
    elif method == "film":
        ops.fusion_film_ce_fwd_bwd(x, y, p["fc.weight"], p["fc.bias"], p["fc_out.weight"], p["fc_out.bias"], lab, guarded("out", B, C),
                                   guarded("h", B, 2 * D), guarded("z", B, D), guarded("L", 1), guarded("dW", 2 * D, D), guarded("db", 2 * D),
                                   guarded("dWo", C, D), guarded("dbo", C), guarded("dX", B, D), guarded("dY", B, D), ws, 1.0 / B)
    else:
        ops.fusion_gated_ce_fwd_bwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], p["fc_out.weight"],
                                    p["fc_out.bias"], lab, guarded("out", B, C), guarded("hx", B, D), guarded("hy", B, D), guarded("z", B, D),
                                    guarded("L", 1), guarded("dWx", D, D), guarded("dbx", D), guarded("dWy", D, D), guarded("dby", D),
                                    guarded("dWo", C, D), guarded("dbo", C), guarded("dX", B, D), guarded("dY", B, D), ws, True, 1.0 / B)
    torch.cuda.synchronize()
    for full in pool:
        assert bool((full[:64] == 12345.0).all()) and bool((full[-64:] == 12345.0).all()), "a canary was overwritten"
    for name, v in views.items():
        if name not in ("ws", "L"):
            assert not bool((v == 12345.0).all()), f"{name} was not written"
    assert torch.isnan(views["L"]).all()
    assert not views["ws"][:B * C].view(B, C)[1].any()                    # the zero dlogits row
    assert not views["dX"][1].any() and not views["dY"][1].any()
    assert torch.isfinite(views["dX"]).all() and torch.isfinite(views["out"]).all()
    assert mla_hip.LIB_PATH
    # the launchers refuse a workspace or a loss vector that is too short before anything is written
    from mla_hip import MLAHipError
    if method == "sum":
        with pytest.raises(MLAHipError, match="workspace"):
            ops.fusion_sum_bwd(x, y, p["fc_x.weight"], p["fc_y.weight"], views["out"], views["dWx"], views["dbx"], views["dWy"],
                               views["dby"], views["dX"], views["dY"], views["ws"][:-1])
        with pytest.raises(MLAHipError, match="is expected"):
            ops.fusion_sum_ce_fwd_bwd(x, y, p["fc_x.weight"], p["fc_x.bias"], p["fc_y.weight"], p["fc_y.bias"], lab, views["out"],
                                      views["oa"], views["ov"], views["L"][:2], views["dWx"], views["dbx"], views["dWy"], views["dby"],
                                      views["dX"], views["dY"], views["ws"], 1.0 / B)


# ---- the step: JointTrainer / JointEvaluator with an attached fusion against the protocol path -------------------------------------------
# The small-input shapes of tests/test_joint_gpu.py's loop test: AVClassifier at batch 4, spectrogram 128 x 64, 2 frames of 96 x 96;
# M3AEClassifier at batch 4, 256 tokens, a 256 x 256 image.
from oracle import mla_oracle as O  # noqa: E402

TOL = 2e-4                 # INTEGRATION.md, numerical contract
VOCAB = 200


class AVArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"
    lorb, clip, modal3 = "base", False, False


class M3Args(AVArgs):
    dataset, lorb = "MVSA", "m3ae"


def _model(which, method=None, seed=31):
    """A model of the seeded state every call gives again: AVClassifier / M3AEClassifier(depth=1) with concat fusion, then the attached
    `method` (seed 77) unless it is None."""
    import mla_hip
    if which == "av":
        m = mla_hip.AVClassifier(AVArgs(), seed=0, conv_math="f32")
        sd = {f"audio_net.{k}": v for k, v in O.make_resnet18_params("audio", seed).items()}
        sd.update({f"visual_net.{k}": v for k, v in O.make_resnet18_params("visual", seed + 1).items()})
        sd.update({f"fusion_module.fc_out.{k}": v for k, v in O.make_head_params(1024, 6, seed + 2).items()})
    else:
        m = mla_hip.M3AEClassifier(M3Args(), depth=1, text_vocab_size=VOCAB, seed=0, conv_math="f32")
        sd = {f"mae_a.{k}": v for k, v in O.make_m3ae_params(seed, depth=1, vocab=VOCAB).items()}
        sd.update({f"mae_v.{k}": v for k, v in O.make_m3ae_params(seed + 1, depth=1, vocab=VOCAB).items()})
        sd.update({f"fusion_module.fc_out.{k}": v for k, v in O.make_head_params(1536, 3, seed + 2).items()})
    m.load_state_dict(sd)
    if method is not None:
        mla_hip.attach_fusion(m, method, seed=77)
    return m


def _inputs(which, s, seed=31, B=4):
    """(inputs as train_step takes them, label) of step s, on the device."""
    if which == "av":
        spec = O.portable_normal(seed + 100 + s, (B, 128, 64), stream=1, mean=-5.081, std=4.4849)
        image = O.portable_normal(seed + 100 + s, (B, 3, 2, 96, 96), stream=2)
        return [spec.cuda(), image.cuda()], O.portable_labels(seed + 100 + s, B, 6).cuda()
    token = torch.from_numpy(np.minimum((O.portable_uniform(seed + s, B * 256, 7) * VOCAB).astype(np.int64), VOCAB - 1)).view(B, 1, 256)
    pm = torch.zeros(B, 1, 256)
    for b in range(B):
        pm[b, 0, 30 + 41 * b:] = 1.0
    image = O.portable_normal(seed + s, (B, 3, 256, 256), stream=3)
    return [token.cuda(), pm.cuda(), image.cuda()], O.portable_labels(seed + s, B, 3).cuda()


def _protocol_forward(which, model, inputs):
    """a, v, out as the reference's loop gets them: main.py:273 (AVClassifier returns out) | main.py:235-237 (M3AE: the loop calls
    model.module.fusion_module(a, v) itself)."""
    if which == "av":
        spec, image = inputs
        return model(spec.unsqueeze(1).float(), image.float())
    a, v = model(*inputs)
    _, _, out = model.module.fusion_module(a, v)
    return a, v, out


@pytest.mark.parametrize("which,method", [("av", "sum"), ("av", "film"), ("av", "gated"), ("m3ae", "sum")])
def test_joint_trainer_equals_protocol_path(which, method):
    """Two JointTrainer steps against the same two steps written as the reference writes them (model(...), torch's CrossEntropyLoss,
    backward, FusedSGD) from the same state; step-level quantities to the project's standing 2e-4, the head alone against the fp64
    restatement on the trainer's own features to its derived bound; JointEvaluator against torch on the raw features."""
    import mla_hip
    from types import SimpleNamespace
    proto, fused = _model(which, method), _model(which, method)
    opt = mla_hip.FusedSGD(proto.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    tr = mla_hip.JointTrainer(fused, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    crit = torch.nn.CrossEntropyLoss()
    inv = 0.25
    for s in range(2):
        inputs, label = _inputs(which, s)
        before = {k: v.detach().cpu().clone() for k, v in fused.fusion_module.state_dict().items()}
        proto.train()
        opt.zero_grad()
        a, v, out = _protocol_forward(which, proto, inputs)
        loss = crit(out, label)
        loss.backward()
        opt.step()
        losses = tr.train_step(*inputs, label, s)
        torch.cuda.synchronize()
        assert tuple(tr.last["a"].shape) == (4, fused.feat_dim)
        assert (tr.last["out"] - out.detach()).abs().max().item() <= TOL
        assert abs(losses["loss"].item() - loss.item()) <= TOL
        assert set(losses) == ({"loss", "loss_a", "loss_v"} if method == "sum" else {"loss"})
        fa, fv = tr.last["a"].cpu(), tr.last["v"].cpu()
        c = SimpleNamespace(x=fa, y=fv, params=before, labels=label.cpu())
        ref = F.run(method, fa, fv, before, label.cpu(), True, inv)
        bnd = bounds(method, c, ref, True, inv)
        got = {"out": tr.last["out"].cpu(), "loss": losses["loss"].cpu().reshape(())}
        if method == "sum":
            got.update(out_a=tr.last["out_m"][0].cpu(), out_v=tr.last["out_m"][1].cpu())
            assert abs(losses["loss_a"].item() - ref["loss_a"].item()) <= TOL and abs(losses["loss_v"].item() - ref["loss_v"].item()) <= TOL
        else:
            assert "z" in tr.last and tr.last["out_m"] is None
        assert_within(got, ref, {k: bnd[k] for k in got}, f"{which} {method} step {s} head")
        sp, sf = proto.state_dict(), fused.state_dict()
        for k in sp:
            if k.startswith("fusion_module."):
                assert (sp[k] - sf[k]).abs().max().item() <= TOL, (method, s, k)
                assert (sf[k].cpu() - before[k[len("fusion_module."):]]).abs().max().item() > 0, f"{k} did not move"
    # evaluation: `out` and (sum) the half-bias out_a / out_v (main.py:610-614) against torch on the raw features; arg-max counts
    ev = mla_hip.JointEvaluator(fused)
    inputs, label = _inputs(which, 5)
    out, out_m = ev.update(*inputs, label)
    res = ev.result()
    a, v = (t.clone() for t in fused.forward_raw(*inputs))
    P = {k: t.detach().cpu() for k, t in fused.fusion_module.state_dict().items()}
    want = F.run(method, a.cpu(), v.cpu(), P, label.cpu(), True, inv, bias_scale=0.5)
    assert (out.cpu().double() - want["out"]).abs().max().item() <= TOL
    acc = (want["out"].argmax(1) == label.cpu()).double().mean().item()
    if method == "sum":
        assert (out_m[0].cpu().double() - want["out_a"]).abs().max().item() <= TOL
        assert (out_m[1].cpu().double() - want["out_v"]).abs().max().item() <= TOL
        accs = tuple((want[k].argmax(1) == label.cpu()).double().mean().item() for k in ("out_a", "out_v"))
        assert res == pytest.approx((acc,) + accs, abs=1e-6)
    else:
        assert out_m is None and res == pytest.approx((acc,), abs=1e-6)


@pytest.mark.parametrize("method", ["sum", "film", "gated"])
def test_protocol_path_on_stored_features(method):
    """CLIPClassifier: the features carry no autograd history, and `a, v, out = model(...)`; loss.backward() must still fill every
    parameter gradient of the attached module (the anchor starts the recording), equal to the fp64 restatement's."""
    import mla_hip
    from types import SimpleNamespace

    class A(AVArgs):
        clip = True
    model = mla_hip.CLIPClassifier(A(), seed=0)
    mla_hip.attach_fusion(model, method, seed=5)
    model.train()
    B, D = 5, model.feat_dim
    tok = O.portable_normal(41, (B, 1, D), stream=31, mean=0.3, std=0.7).cuda()
    vis = O.portable_normal(42, (B, 1, D), stream=32, mean=0.3, std=0.7).cuda()
    label = O.portable_labels(43, B, 6).cuda()
    P = {k: t.detach().cpu().clone() for k, t in model.fusion_module.state_dict().items()}
    _a, _v, out = model(tok, vis)
    assert out.requires_grad
    torch.nn.CrossEntropyLoss()(out, label).backward()
    torch.cuda.synchronize()
    x, y = tok.cpu().reshape(B, D), vis.cpu().reshape(B, D)
    ref = F.run(method, x, y, P, label.cpu(), True)
    bnd = bounds_bwd(method, SimpleNamespace(x=x, y=y, params=P, labels=label.cpu()), ref, True, 1.0 / B)
    for k, p in model.fusion_module.named_parameters():
        assert p.grad is not None, k
        # dlogits comes from torch's CrossEntropyLoss on the kernel's `out` here: its error is that of the fused call's softmax
        full = bounds(method, SimpleNamespace(x=x, y=y, params=P, labels=label.cpu()), ref, True, 1.0 / B)["d" + k]
        err = (p.grad.cpu().double() - ref["d" + k]).abs()
        assert bool((err <= full + bnd["d" + k]).all()), f"{method} {k}: {err.max().item():.3e}"


def test_sum_ogm_ge_coefficients_from_full_bias_logits():
    """sum + OGM_GE: the coefficients come from out_a = fc_x(a), out_v = fc_y(v) with the full bias, as the oracle's coefficient function
    gives them for those logits."""
    import mla_hip
    fused = _model("av", "sum")
    tr = mla_hip.JointTrainer(fused, modulation="OGM_GE", alpha=0.3, modulation_starts=0, modulation_ends=50)
    inputs, label = _inputs("av", 0)
    fm = fused.fusion_module
    Wx, bx, Wy, by = (t.detach().clone() for t in (fm.fc_x.weight, fm.fc_x.bias, fm.fc_y.weight, fm.fc_y.bias))
    tr.train_step(*inputs, label, 0)
    torch.cuda.synchronize()
    a, v = tr.last["a"], tr.last["v"]
    oa, ov = a @ Wx.T + bx, v @ Wy.T + by
    assert (tr.last["out_m"][0] - oa).abs().max().item() <= TOL and (tr.last["out_m"][1] - ov).abs().max().item() <= TOL
    coeffs, _scores, _ratios = O.ogm_coefficients([tr.last["out_m"][0].cpu(), tr.last["out_m"][1].cpu()], label.cpu(), 0.3)
    want = torch.tensor([float(c) for c in coeffs], dtype=torch.float64)
    assert (tr.last["coeff"].cpu().double()[:2] - want).abs().max().item() <= 1e-5


def test_concat_path_unchanged_by_the_attach_path():
    """A model never passed to attach_fusion takes two JointTrainer steps; the same steps from a second identical model after
    mla_hip.fusion has been used on another model in this process are bitwise equal."""
    import mla_hip

    def two_steps():
        m = _model("av")
        t = mla_hip.JointTrainer(m, lr=1e-3, momentum=0.9, weight_decay=1e-4)
        seen = []
        for s in range(2):
            inputs, label = _inputs("av", s)
            t.train_step(*inputs, label, s)
            seen.append((t.last["out"].clone(), t.losses["loss"].clone()))
        torch.cuda.synchronize()
        return m, seen
    m1, first = two_steps()
    other = _model("av", "gated")
    inputs, label = _inputs("av", 0)
    mla_hip.JointTrainer(other).train_step(*inputs, label, 0)
    m2, second = two_steps()
    for s in range(2):
        assert_bitwise(second[s][0], first[s][0], f"concat out step {s}")
        assert_bitwise(second[s][1], first[s][1], f"concat loss step {s}")
    for (k, a), (_k, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k

