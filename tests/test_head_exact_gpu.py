"""GPU: the Linear head + cross entropy kernels (shared head, concat head, QMF heads, fused feature phase; csrc/head_common.h) against
the models of tests/head_exact.py, at every regime of their loops (head_exact.TABLE / WIDE; test_head_exact_cpu.py proves the inputs).

  LIN / SAT / UNI-dlogits comparisons are `torch.equal` with the exact value: no tolerance.  Every tolerance elsewhere is one the suite
  already has, cited where it is applied:
    HEAD   test_ops_gpu.py::test_head_ce                        logits, loss 2e-6 + 2e-6 max|ref|; dW, db 1e-7 + 1e-5; dX 1e-8 + 1e-5
    CONCAT test_joint_gpu.py::test_concat_head_kernels_vs_fp64  2e-5 + 1e-5 max|ref|; dX 2e-6 + 1e-5
    PHASE  test_clip_gpu.py::PHASE_CASES, first phase           head and momentum 1e-7 + 1e-6 max|ref|
    QMF    test_qmf_gpu.py::test_head_kernels_vs_reference_fixture   2e-5 max|ref|
    exact_tokens.softmax_tol for dlogits / inv_batch of the standalone cross entropy, and test_head_ce's loss tolerance applied to the
    condition of the sum, 2e-6 sum_r |row loss| + 2e-6.

  Guards: every output and workspace is a view into a larger buffer prefilled with a NaN bit pattern, 256 floats on either side; after
  the call the guards are unchanged bit for bit and no output element still holds the fill; workspaces are exactly *_ws_elems long.

  Bad labels: -1 and C at rows 0 and B - 1 give a NaN loss, the good run's logits, and the gradients of the batch with those rows'
  dlogits zeroed, in the fused shared head and the feature phase as in ce_fwd_bwd, the concat head and the QMF heads."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_exact as H  # noqa: E402
from exact import assert_bitwise  # noqa: E402
from exact_tokens import softmax_tol  # noqa: E402
from util import assert_close  # noqa: E402

FILL = 0x7FC0BEEF          # a quiet NaN no kernel produces
GUARD = 256
IDS = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)       # noqa: E731
HEAD_TOL = {"logits": (2e-6, 2e-6), "loss": (2e-6, 2e-6), "dW": (1e-7, 1e-5), "db": (1e-7, 1e-5), "dX": (1e-8, 1e-5)}
CONCAT_TOL, CONCAT_DX_TOL = (2e-5, 1e-5), (2e-6, 1e-5)
PHASE_TOL = (1e-7, 1e-6)
QMF_REL = 2e-5


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as o
    return o


class Arena:
    """Guarded device buffers of one call."""

    def __init__(self):
        self.bufs = []

    def _new(self, shape, name, must_fill):
        n = math.prod(shape)
        flat = torch.full((n + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
        self.bufs.append((flat, n, must_fill, name))
        return flat.view(torch.float32)[GUARD:GUARD + n].view(shape)

    def out(self, *shape, name="out"):
        return self._new(shape, name, True)

    def ws(self, n, name="ws"):
        """A workspace: exactly n floats; parts of it may stay unwritten."""
        return self._new((int(n),), name, False)

    def load(self, t, name="inout"):
        """A buffer the call updates in place."""
        v = self._new(tuple(t.shape), name, False)
        v.copy_(t)
        return v

    def check(self):
        torch.cuda.synchronize()
        for flat, n, must_fill, name in self.bufs:
            assert bool((flat[:GUARD] == FILL).all()) and bool((flat[GUARD + n:] == FILL).all()), f"{name}: a guard was overwritten"
            if must_fill:
                left = int((flat[GUARD:GUARD + n] == FILL).sum())
                assert left == 0, f"{name}: {left} of {n} elements were never written"


def dev(t):
    return t.cuda() if isinstance(t, torch.Tensor) else [x.cuda() for x in t]


def exact(got, want64, name):
    assert_bitwise(got, H.exact32(want64), name)


def close(got, want, tol, name):
    err = assert_close(got, want, atol=tol[0], rtol=tol[1], name=name)
    print(f"{name}: max|d| {err:.3e}")


def ce_loss_close(loss, rowloss64, name):
    """test_head_ce's loss tolerance on the condition of the sum."""
    want, bound = rowloss64.sum().item(), 2e-6 * rowloss64.abs().sum().item() + 2e-6
    print(f"{name}: |d| {abs(loss.item() - want):.3e} bound {bound:.3e}")
    assert abs(loss.item() - want) <= bound, f"{name}: {loss.item()!r} vs {want!r}, bound {bound:.3e}"


# ---- the split entry points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", H.TABLE + H.WIDE, ids=IDS)
def test_head_logits_lin(ops, shape):
    c = H.lin_case(*shape)
    a = Arena()
    logits = a.out(c.B, c.C, name="logits")
    ops.head_logits(dev(c.X), dev(c.W), dev(c.b), logits)
    a.check()
    exact(logits, H.logits_model(c.X, c.W, c.b), "head_logits LIN")


def _ce(ops, logits, labels, inv):
    a = Arena()
    B, C = logits.shape
    loss, dl, ws = a.out(1, name="loss"), a.out(B, C, name="dlogits"), a.ws(B, "ce ws")
    ops.ce_fwd_bwd(dev(logits), dev(labels), loss, dl, ws, inv)
    a.check()
    return loss, dl, ws


@pytest.mark.parametrize("shape", H.TABLE, ids=IDS)
def test_ce_fwd_bwd_sat(ops, shape):
    c = H.sat_case(*shape)
    logits64 = H.logits_model(c.X, c.W, c.b)
    rowloss, dl64, loss64 = H.ce_model(logits64, c.labels, H.INV)
    loss, dl, ws = _ce(ops, H.exact32(logits64), c.labels, H.INV)
    exact(ws, rowloss, "ce_fwd_bwd SAT row losses")
    exact(loss, loss64.reshape(1), "ce_fwd_bwd SAT loss")
    exact(dl, dl64, "ce_fwd_bwd SAT dlogits")


@pytest.mark.parametrize("shape", H.TABLE + H.WIDE, ids=IDS)
def test_ce_fwd_bwd_uni(ops, shape):
    c = H.uni_case(*shape)
    loss, dl, _ = _ce(ops, c.logits, c.labels, H.INV)
    assert_bitwise(dl, H.ce_model(c.logits, c.labels, H.INV, dt=torch.float32)[1], "ce_fwd_bwd UNI dlogits vs the float32 restatement")
    close(loss, H.ce_model(c.logits, c.labels, H.INV)[2].reshape(1), HEAD_TOL["loss"], "ce_fwd_bwd UNI loss")


@pytest.mark.parametrize("B,C", sorted({(B, C) for B, _, C in H.TABLE + H.WIDE}), ids=IDS)
def test_ce_fwd_bwd_dense(ops, B, C):
    for family in H.CE_FAMILIES:
        c = H.dense_ce_case(B, C, family)
        inv = 1.0 / B
        rowloss, dl64, _ = H.ce_model(c.logits, c.labels, inv)
        loss, dl, _ = _ce(ops, c.logits, c.labels, inv)
        ref = dl64 / inv
        err = (dl.double().cpu() / inv - ref).abs().max().item()
        print(f"{family}: dlogits / inv max|d| {err:.3e} bound {softmax_tol(ref):.3e}")
        assert err <= softmax_tol(ref), f"{family}: dlogits / inv_batch max|d| {err:.3e} > {softmax_tol(ref):.3e}"
        ce_loss_close(loss, rowloss, f"ce_fwd_bwd {family} loss")


@pytest.mark.parametrize("shape", H.TABLE + H.WIDE, ids=IDS)
def test_head_bwd_lin(ops, shape):
    c = H.lin_case(*shape)
    X, W, dl = dev(c.X), dev(c.W), dev(c.dl)
    for scale in H.SCALES:
        a = Arena()
        dW, db, dX = a.out(c.C, c.D, name="dW"), a.out(c.C, name="db"), a.out(c.B, c.D, name="dX")
        ops.head_bwd(X, W, dl, dW, db, dX, scale)
        a.check()
        dW64, db64, (dX64,) = H.bwd_model(c.xs, c.W, c.dl, scale)
        exact(dW, dW64, f"head_bwd LIN dW, scale {scale}")
        exact(db, db64, f"head_bwd LIN db, scale {scale}")
        exact(dX, dX64, f"head_bwd LIN dX, scale {scale}")


# ---- the fused shared head ---------------------------------------------------------------------------------------------------------
def _head(ops, c, labels, inv):
    a = Arena()
    B, D, C = c.B, c.D, c.C
    assert ops.head_ws_elems(B, C) == B * C + B
    o = dict(logits=a.out(B, C, name="logits"), loss=a.out(1, name="loss"), dW=a.out(C, D, name="dW"), db=a.out(C, name="db"),
             dX=a.out(B, D, name="dX"))
    ws = a.ws(ops.head_ws_elems(B, C), "head ws")
    ops.head_ce_fwd_bwd(dev(c.X), dev(c.W), dev(c.b), dev(labels), o["logits"], o["loss"], o["dW"], o["db"], o["dX"], ws, inv)
    a.check()
    o["dl"], o["rowloss"] = ws[:B * C].view(B, C), ws[B * C:]
    return o


@pytest.mark.parametrize("shape", H.TABLE, ids=IDS)
def test_head_ce_fwd_bwd_exact(ops, shape):
    B, D, C = shape
    lin, sat, uni = H.lin_case(*shape), H.sat_case(*shape), H.uni_case(*shape)
    exact(_head(ops, lin, uni.labels, H.INV)["logits"], H.logits_model(lin.X, lin.W, lin.b), "head_ce_fwd_bwd LIN logits")
    # SAT: the whole call
    o, m = _head(ops, sat, sat.labels, H.INV), H.head_model(sat.X, sat.W, sat.b, sat.labels, H.INV)
    for k in ("logits", "dl", "rowloss", "dW", "db", "dX"):
        exact(o[k], getattr(m, k), f"head_ce_fwd_bwd SAT {k}")
    exact(o["loss"], m.loss.reshape(1), "head_ce_fwd_bwd SAT loss")
    # UNI: s = C through both softmax slots
    o = _head(ops, uni, uni.labels, H.INV)
    m32 = H.head_model(uni.X, uni.W, uni.b, uni.labels, H.INV, dt=torch.float32)
    assert_bitwise(o["logits"], m32.logits, "head_ce_fwd_bwd UNI logits")
    assert_bitwise(o["dl"], m32.dl, "head_ce_fwd_bwd UNI dlogits vs the float32 restatement")
    db64 = m32.dl.double().sum(0)                                   # of the float32 dlogits
    if C & (C - 1) == 0:                                            # 1 / C a power of two: the sum of the rows is exact, too
        exact(o["db"], db64, "head_ce_fwd_bwd UNI db")
    else:
        close(o["db"], db64, HEAD_TOL["db"], "head_ce_fwd_bwd UNI db")
    close(o["loss"], H.head_model(uni.X, uni.W, uni.b, uni.labels, H.INV).loss.reshape(1), HEAD_TOL["loss"], "head_ce_fwd_bwd UNI loss")


@pytest.mark.parametrize("shape", H.TABLE, ids=IDS)
def test_head_ce_fwd_bwd_dense(ops, shape):
    c = H.dense_case(*shape)
    o, m = _head(ops, c, c.labels, 1.0 / c.B), H.head_model(c.X, c.W, c.b, c.labels, 1.0 / c.B)
    for k, tol in HEAD_TOL.items():
        close(o[k], getattr(m, k).reshape(o[k].shape), tol, f"head_ce_fwd_bwd DENSE {k}")


# ---- the concat head -----------------------------------------------------------------------------------------------------------------
def _concat(ops, c, labels, inv):
    a = Arena()
    M, B, D, C = c.M, c.B, c.D, c.C
    assert ops.concat_head_ws_elems(B, C, M) == B * C + B * (M + 1)
    o = dict(out=a.out(B, C, name="out"), out_m=a.out(M, B, C, name="out_m"), loss=a.out(1, name="loss"), loss_m=a.out(M, name="loss_m"),
             dW=a.out(C, M * D, name="dW"), db=a.out(C, name="db"), dxs=[a.out(B, D, name=f"dx{m}") for m in range(M)])
    ws = a.ws(ops.concat_head_ws_elems(B, C, M), "concat ws")
    ops.concat_head_ce_fwd_bwd(dev(c.xs), dev(c.W), dev(c.b), dev(labels), o["out"], o["out_m"], o["loss"], o["loss_m"], o["dW"], o["db"],
                               o["dxs"], ws, inv)
    a.check()
    o["dl"] = ws[:B * C].view(B, C)
    return o


@pytest.mark.parametrize("M,shape", list(zip(H.MODS, H.TABLE)), ids=IDS)
def test_concat_head_exact(ops, M, shape):
    B, D, C = shape
    lin, sat = H.lin_case(B, D, C, M), H.sat_case(B, D, C, M)
    xs, W, b, dl = dev(lin.xs), dev(lin.W), dev(lin.b), dev(lin.dl)
    out64, out_m64 = H.concat_fwd_model(lin.xs, lin.W, lin.b)
    a = Arena()
    out, out_m = a.out(B, C, name="out"), a.out(M, B, C, name="out_m")
    ops.concat_head_fwd(xs, W, b, out, out_m)
    a.check()
    exact(out, out64, "concat_head_fwd LIN out")
    exact(out_m, out_m64, "concat_head_fwd LIN out_m")
    for scale in H.SCALES:
        a = Arena()
        dW, db, dxs = a.out(C, M * D, name="dW"), a.out(C, name="db"), [a.out(B, D, name=f"dx{m}") for m in range(M)]
        ops.concat_head_bwd(xs, W, dl, dW, db, dxs, scale)
        a.check()
        dW64, db64, dxs64 = H.bwd_model(lin.xs, lin.W, lin.dl, scale)
        exact(dW, dW64, f"concat_head_bwd LIN dW, scale {scale}")
        exact(db, db64, f"concat_head_bwd LIN db, scale {scale}")
        for m in range(M):
            exact(dxs[m], dxs64[m], f"concat_head_bwd LIN dx[{m}], scale {scale}")
    o = _concat(ops, lin, sat.labels, H.INV)
    exact(o["out"], out64, "concat_head_ce_fwd_bwd LIN out")
    exact(o["out_m"], out_m64, "concat_head_ce_fwd_bwd LIN out_m")
    # SAT: the code lives in modality 0's columns, `out` is saturated; loss_m is not
    o, m = _concat(ops, sat, sat.labels, H.INV), H.concat_model(sat.xs, sat.W, sat.b, sat.labels, H.INV)
    for k in ("out", "out_m", "dl", "dW", "db"):
        exact(o[k], getattr(m, k), f"concat_head_ce_fwd_bwd SAT {k}")
    exact(o["loss"], m.loss.reshape(1), "concat_head_ce_fwd_bwd SAT loss")
    for i in range(M):
        exact(o["dxs"][i], m.dxs[i], f"concat_head_ce_fwd_bwd SAT dx[{i}]")
    close(o["loss_m"], m.loss_m, CONCAT_TOL, "concat_head_ce_fwd_bwd SAT loss_m")


@pytest.mark.parametrize("M,shape", list(zip(H.MODS, H.TABLE)), ids=IDS)
def test_concat_head_dense(ops, M, shape):
    c = H.dense_case(*shape, M)
    o, m = _concat(ops, c, c.labels, 1.0 / c.B), H.concat_model(c.xs, c.W, c.b, c.labels, 1.0 / c.B)
    for k in ("out", "out_m", "loss", "loss_m", "dW", "db"):
        close(o[k], getattr(m, k).reshape(o[k].shape), CONCAT_TOL, f"concat_head_ce_fwd_bwd DENSE {k}")
    for i in range(M):
        close(o["dxs"][i], m.dxs[i], CONCAT_DX_TOL, f"concat_head_ce_fwd_bwd DENSE dx[{i}]")


# ---- the fused feature phase (project = 0) ---------------------------------------------------------------------------------------------
def _phase(ops, c, labels, inv):
    """first = 1, wd = 0, lr = 2^-3: buf is the raw gradient of [W | b]."""
    a = Arena()
    B, D, C = c.B, c.D, c.C
    want_ws = ((B * C + B + 3) & ~3) + 6 * D + C * D
    assert ops.feature_ws_elems(B, D, C) == want_ws
    o = dict(W=a.load(c.W, "W"), b=a.load(c.b, "b"), buf=a.out(C * D + C, name="buf"), logits=a.out(B, C, name="logits"), loss=a.out(1, name="loss"))
    ws = a.ws(want_ws, "feature ws")
    ops.feature_phase(dev(c.X), dev(labels), o["W"], o["b"], o["buf"], None, o["logits"], o["loss"], ws, inv, False, 0.1, H.LR, 0.9, 0.0, True)
    a.check()
    o["dl"] = ws[:B * C].view(B, C)
    return o


@pytest.mark.parametrize("shape", H.TABLE, ids=IDS)
def test_feature_phase_exact(ops, shape):
    lin, sat = H.lin_case(*shape), H.sat_case(*shape)
    exact(_phase(ops, lin, sat.labels, H.INV)["logits"], H.logits_model(lin.X, lin.W, lin.b), "feature_phase LIN logits")
    o, m = _phase(ops, sat, sat.labels, H.INV), H.feature_model(sat.X, sat.W, sat.b, sat.labels, H.INV, H.LR)
    for k in ("logits", "dl", "buf", "W", "b"):
        exact(o[k], getattr(m, k), f"feature_phase SAT {k}")
    exact(o["loss"], m.loss.reshape(1), "feature_phase SAT loss")


@pytest.mark.parametrize("shape", H.TABLE, ids=IDS)
def test_feature_phase_dense(ops, shape):
    c = H.dense_case(*shape)
    o, m = _phase(ops, c, c.labels, 1.0 / c.B), H.feature_model(c.X, c.W, c.b, c.labels, 1.0 / c.B, H.LR)
    close(o["logits"], m.logits, HEAD_TOL["logits"], "feature_phase DENSE logits")
    close(o["loss"], m.loss.reshape(1), HEAD_TOL["loss"], "feature_phase DENSE loss")
    for k in ("W", "b", "buf"):
        close(o[k], getattr(m, k), PHASE_TOL, f"feature_phase DENSE {k}")


# ---- bad labels: one policy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 70, 65), (65, 257, 128)], ids=IDS)
def test_bad_labels_zero_their_rows(ops, shape):
    """SAT inputs: everything is exact, so the fused calls are held to the model AND to the split chain on the zeroed dlogits."""
    B, D, C = shape
    c = H.sat_case(B, D, C)
    bad = H.with_bad_labels(c.labels, C)
    assert int(bad[0]) == -1 and int(bad[-1]) == C
    keep = torch.ones(B, dtype=torch.bool)
    keep[0] = keep[-1] = False
    good, o, m = _head(ops, c, c.labels, H.INV), _head(ops, c, bad, H.INV), H.head_model(c.X, c.W, c.b, bad, H.INV)
    assert torch.isnan(o["loss"]).all() and torch.isnan(m.loss)
    assert torch.isfinite(o["logits"]).all()
    assert_bitwise(o["logits"], good["logits"], "bad labels: logits vs the good-label run")
    zeroed = good["dl"] * dev(keep)[:, None].float()
    assert_bitwise(o["dl"], zeroed, "bad labels: dlogits vs the good run's with the bad rows zeroed")
    assert bool((o["dl"][~dev(keep)] == 0).all())
    a = Arena()
    dW, db, dX = a.out(C, D, name="dW"), a.out(C, name="db"), a.out(B, D, name="dX")
    ops.head_bwd(dev(c.X), dev(c.W), zeroed.contiguous(), dW, db, dX, 1.0)
    a.check()
    for k, chain in (("dW", dW), ("db", db), ("dX", dX)):
        assert_bitwise(o[k], chain, f"bad labels: fused {k} vs head_bwd on the zeroed dlogits")
        exact(o[k], getattr(m, k), f"bad labels: {k} vs the model")
    loss2, dl2, _ = _ce(ops, o["logits"].cpu(), bad, H.INV)
    assert torch.isnan(loss2).all()
    assert_bitwise(dl2, o["dl"], "bad labels: fused dlogits vs ce_fwd_bwd")
    # the feature phase: the bad rows contribute nothing to the momentum, and SGD applies none of them
    p, pm = _phase(ops, c, bad, H.INV), H.feature_model(c.X, c.W, c.b, bad, H.INV, H.LR)
    assert torch.isnan(p["loss"]).all()
    assert_bitwise(p["logits"], good["logits"], "bad labels: feature_phase logits")
    assert_bitwise(p["dl"], zeroed, "bad labels: feature_phase dlogits")
    assert_bitwise(p["buf"], torch.cat([dW.reshape(-1), db]), "bad labels: feature_phase momentum vs head_bwd on the zeroed dlogits")
    for k in ("buf", "W", "b"):
        exact(p[k], getattr(pm, k), f"bad labels: feature_phase {k} vs the model")


# ---- the QMF heads -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,shape", list(zip(H.MODS, H.TABLE)), ids=IDS)
def test_qmf_head_exact(ops, M, shape):
    B, D, C = shape
    lin = H.lin_case(B, D, C, M)
    Ws = [lin.W[:, m * D:(m + 1) * D].contiguous() for m in range(M)]
    bs = [torch.roll(H.lin_case(B, D, C).b, m) for m in range(M)]
    z64 = torch.stack([H.logits_model(lin.xs[m], Ws[m], bs[m]) for m in range(M)])
    a = Arena()
    z, out, conf = a.out(M, B, C, name="z"), a.out(B, C, name="out"), a.out(M, B, name="conf")
    ops.qmf_head_fwd(dev(lin.xs), dev(Ws), dev(bs), z, out, conf)
    a.check()
    exact(z, z64, "qmf_head_fwd LIN z")
    # the training call on the same inputs: z again
    n_data = B + 3
    a = Arena()
    assert ops.qmf_head_ws_elems(B, C, M) == 4 * 3 * 256 + 2 * M * B * C + B * C + B + M * B
    z, out, conf, ell, target, margin = (a.out(*s, name=n) for s, n in (((M, B, C), "z"), ((B, C), "out"), ((M, B), "conf"), ((M, B), "ell"),
                                                                         ((M, B), "target"), ((M, B), "margin")))
    losses = a.out(2 * M + 2, name="losses")
    dWs, dbs, dxs = ([a.out(*s, name=f"{n}{m}") for m in range(M)] for s, n in (((C, D), "dW"), ((C,), "db"), ((B, D), "dx")))
    ws = a.ws(ops.qmf_head_ws_elems(B, C, M), "qmf ws")
    corr = torch.zeros((M, n_data), dtype=torch.float64, device="cuda")
    ops.qmf_head_fwd_bwd(dev(lin.xs), dev(Ws), dev(bs), dev(H.uni_case(B, D, C).labels), torch.arange(B, device="cuda"), corr, torch.zeros_like(corr),
                         z, out, conf, ell, target, margin, losses, dWs, dbs, dxs, ws, 1.0, 0.1, 1.0 / B)
    a.check()
    exact(z, z64, "qmf_head_fwd_bwd LIN z")
    # SAT in every modality: E = max, conf = fl(max / 10)
    sats = [H.sat_case(B, D, C, 1, salt=m) for m in range(M)]
    z64 = torch.stack([H.logits_model(s.X, s.W, s.b) for s in sats])
    a = Arena()
    z, out, conf = a.out(M, B, C, name="z"), a.out(B, C, name="out"), a.out(M, B, name="conf")
    ops.qmf_head_fwd(dev([s.X for s in sats]), dev([s.W for s in sats]), dev([s.b for s in sats]), z, out, conf)
    a.check()
    exact(z, z64, "qmf_head_fwd SAT z")
    assert_bitwise(conf, H.exact32(z64.max(2).values) / torch.tensor(10.0), "qmf_head_fwd SAT conf = float32(max / 10)")
    terms = conf.double().cpu()[:, :, None] * z64
    err, bound = (out.double().cpu() - terms.sum(0)).abs(), (M + 1) * 2.0 ** -24 * terms.abs().sum(0)
    assert bool((err <= bound).all()), f"qmf_head_fwd SAT out: max excess {(err - bound).max().item():.3e}"


@pytest.mark.parametrize("shape", H.QMF_DENSE, ids=IDS)
def test_qmf_head_fwd_bwd_dense(ops, shape):
    """Two consecutive steps with the History carried on the device, against tests/qmf_model.py."""
    M, B, D, C, n_data = shape
    c = H.qmf_dense_case(*shape)
    Ws, bs = dev(c.Ws), dev(c.bs)
    corr = torch.zeros((M, n_data), dtype=torch.float64, device="cuda")
    conf_h = torch.zeros_like(corr)

    def rel(got, want, name):
        got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
        err, bound = (got - want).abs().max().item(), QMF_REL * want.abs().max().item()
        print(f"{name}: max|d| {err:.3e} bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound, f"{name}: max|d|={err:.3e} > {bound:.3e}"

    for s, st in enumerate(c.steps):
        a = Arena()
        z, out, conf, ell, target, margin = (a.out(*sh, name=n) for sh, n in (((M, B, C), "z"), ((B, C), "out"), ((M, B), "conf"), ((M, B), "ell"),
                                                                              ((M, B), "target"), ((M, B), "margin")))
        losses = a.out(2 * M + 2, name="losses")
        dWs, dbs, dxs = ([a.out(*sh, name=f"{n}{m}") for m in range(M)] for sh, n in (((C, D), "dW"), ((C,), "db"), ((B, D), "dx")))
        ws = a.ws(ops.qmf_head_ws_elems(B, C, M), "qmf ws")
        ops.qmf_head_fwd_bwd(dev(st.xs), Ws, bs, dev(st.labels), dev(st.idx), corr, conf_h, z, out, conf, ell, target, margin, losses, dWs, dbs,
                             dxs, ws, c.w_cml, c.w_crl, 1.0 / B)
        a.check()
        r, p = st.ref, f"step {s} "
        assert torch.equal(target.cpu().double(), r["target"]), p + "target"
        for k, t in (("z", z), ("out", out), ("conf", conf), ("ell", ell), ("margin", margin), ("loss", losses[0]), ("ce", losses[1:1 + M]),
                     ("rank", losses[1 + M:1 + 2 * M]), ("cml", losses[1 + 2 * M])):
            rel(t, r[k], p + k)
        for k, t in (("dW", dWs), ("db", dbs), ("dX", dxs)):
            rel(torch.stack(t), torch.stack(r[k]), p + k)
        rel(corr, st.hist[0], p + "History correctness")
        rel(conf_h, st.hist[1], p + "History confidence")
        assert np.array_equal(corr.cpu().numpy() != 0, st.hist[0] != 0), p + "History entries written"
