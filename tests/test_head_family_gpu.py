"""GPU: the head families (shared head, concat head, QMF heads, fused feature phase) are written on one set of device helpers
(csrc/head_common.h), so the quantities they have in common are equal bit for bit -- `torch.equal`, no tolerance:

  (a) logits: head_logits = head_ce_fwd_bwd = feature_phase = qmf_head_fwd z[m]; concat_head_fwd out_m[m] at zero bias = head_logits
      on the column block W[:, mD:(m+1)D] at zero bias;
  (b) shared head: the fused head_ce_fwd_bwd = head_logits -> ce_fwd_bwd -> head_bwd(scale = 1);
  (c) concat head: the fused concat_head_ce_fwd_bwd = concat_head_fwd -> ce_fwd_bwd -> concat_head_bwd(scale = 1), and loss_m[m] is
      ce_fwd_bwd's loss of out_m[m].

Shapes: B = 70 crosses the 64-row stride of the bias-gradient and loss sums; D = 70 is no multiple of 64 or 4, D = 320 more than one
256-column block; C = 3, 64, 65, 128: one softmax slot, the slot boundary, the second slot, the limit.  Labels are valid, except in
the two bad-label cases of (b) and (c): labels -1 and C at rows 0 and B - 1 of BAD_SHAPE give a NaN loss on both sides and, with the
zero dlogits rows every family writes for them, the same gradients bit for bit."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402

SHAPES = [(B, D, C) for B in (1, 5, 70) for D in (70, 320) for C in (3, 64, 65, 128)]
BAD_SHAPE = (70, 70, 65)
F32 = dict(device="cuda", dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _inputs(B, D, C):
    """Three modalities' features and heads, one label vector; made once per shape and never written to."""
    seed = 1000 * B + 10 * D + C
    xs = [O.portable_normal(seed + m, (B, D), stream=31, mean=0.3, std=0.7).cuda() for m in range(3)]
    heads = [O.make_head_params(D, C, seed + 10 + m) for m in range(3)]
    Ws, bs = [h["weight"].cuda() for h in heads], [h["bias"].cuda() for h in heads]
    Wcat = {M: O.make_head_params(M * D, C, seed + 20 + M)["weight"].cuda() for M in (2, 3)}
    return xs, Ws, bs, Wcat, bs[0], O.portable_labels(seed, B, C).cuda()


def _head_logits(X, W, b):
    from mla_hip import ops
    out = torch.empty((X.shape[0], W.shape[0]), **F32)
    ops.head_logits(X, W, b, out)
    return out


def _ce(logits, labels):
    """ce_fwd_bwd: (loss, dlogits)"""
    from mla_hip import ops
    B = logits.shape[0]
    loss, dl, ws = torch.empty(1, **F32), torch.empty_like(logits), torch.empty(B, **F32)
    ops.ce_fwd_bwd(logits, labels, loss, dl, ws, 1.0 / B)
    return loss, dl


def _bad_labels(labels, C):
    bad = labels.clone()
    bad[0], bad[-1] = -1, C
    return bad


def _same(a, b, what):
    assert torch.equal(a, b), f"{what}: not bit-equal (max |difference| {(a - b).abs().max().item():.3g})"


@pytest.mark.parametrize("B,D,C", SHAPES)
def test_logits_agree_across_families(B, D, C):
    from mla_hip import ops
    xs, Ws, bs, Wcat, _, labels = _inputs(B, D, C)
    X, W, b = xs[0], Ws[0], bs[0]
    ref = _head_logits(X, W, b)

    logits, loss, dW, db, dX = (torch.empty(s, **F32) for s in ((B, C), (1,), (C, D), (C,), (B, D)))
    ops.head_ce_fwd_bwd(X, W, b, labels, logits, loss, dW, db, dX, torch.empty(ops.head_ws_elems(B, C), **F32), 1.0 / B)
    _same(logits, ref, "head_ce_fwd_bwd logits vs head_logits")

    flat = torch.cat([W.reshape(-1), b])                                  # the phase updates its head in place: a private copy
    buf, plog, ploss = torch.zeros_like(flat), torch.empty((B, C), **F32), torch.empty(1, **F32)
    ops.feature_phase(X, labels, flat[:C * D].view(C, D), flat[C * D:], buf, None, plog, ploss,
                      torch.empty(ops.feature_ws_elems(B, D, C), **F32), 1.0 / B, False, 0.1, 1e-3, 0.9, 1e-4, True)
    _same(plog, ref, "feature_phase logits vs head_logits")

    for M in (2, 3):
        z, out, conf = torch.empty((M, B, C), **F32), torch.empty((B, C), **F32), torch.empty((M, B), **F32)
        ops.qmf_head_fwd(xs[:M], Ws[:M], bs[:M], z, out, conf)
        for m in range(M):
            _same(z[m], ref if m == 0 else _head_logits(xs[m], Ws[m], bs[m]), f"qmf_head_fwd z[{m}] (M = {M}) vs head_logits")
        zero = torch.zeros(C, **F32)
        out, out_m = torch.empty((B, C), **F32), torch.empty((M, B, C), **F32)
        ops.concat_head_fwd(xs[:M], Wcat[M], zero, out, out_m)
        for m in range(M):
            _same(out_m[m], _head_logits(xs[m], Wcat[M][:, m * D:(m + 1) * D].contiguous(), zero),
                  f"concat_head_fwd out_m[{m}] (M = {M}) vs head_logits on its column block")
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,D,C", SHAPES)
def test_shared_head_fused_equals_split(B, D, C):
    _shared_head_fused_equals_split(B, D, C, _inputs(B, D, C)[5], bad=False)


def test_shared_head_fused_equals_split_bad_labels():
    B, D, C = BAD_SHAPE
    _shared_head_fused_equals_split(B, D, C, _bad_labels(_inputs(B, D, C)[5], C), bad=True)


def _shared_head_fused_equals_split(B, D, C, labels, bad):
    from mla_hip import ops
    xs, Ws, bs = _inputs(B, D, C)[:3]
    X, W, b = xs[0], Ws[0], bs[0]
    logits, loss, dW, db, dX = (torch.empty(s, **F32) for s in ((B, C), (1,), (C, D), (C,), (B, D)))
    ops.head_ce_fwd_bwd(X, W, b, labels, logits, loss, dW, db, dX, torch.empty(ops.head_ws_elems(B, C), **F32), 1.0 / B)
    loss2, dl = _ce(_head_logits(X, W, b), labels)
    dW2, db2, dX2 = torch.empty_like(dW), torch.empty_like(db), torch.empty_like(dX)
    ops.head_bwd(X, W, dl, dW2, db2, dX2, 1.0)
    if bad:
        assert torch.isnan(loss).all() and torch.isnan(loss2).all() and bool((dl[0] == 0).all()) and bool((dl[-1] == 0).all())
        assert torch.isfinite(dW).all() and torch.isfinite(db).all() and torch.isfinite(dX).all()
    for name, a, c in (("loss", loss, loss2), ("dW", dW, dW2), ("db", db, db2), ("dX", dX, dX2)):
        if not (bad and name == "loss"):
            _same(a, c, f"head_ce_fwd_bwd {name} vs head_logits -> ce_fwd_bwd -> head_bwd")


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("B,D,C", SHAPES)
def test_concat_head_fused_equals_split(B, D, C, M):
    _concat_head_fused_equals_split(B, D, C, M, _inputs(B, D, C)[5], bad=False)


def test_concat_head_fused_equals_split_bad_labels():
    B, D, C = BAD_SHAPE
    _concat_head_fused_equals_split(B, D, C, 3, _bad_labels(_inputs(B, D, C)[5], C), bad=True)


def _concat_head_fused_equals_split(B, D, C, M, labels, bad):
    from mla_hip import ops
    xs, _, _, Wcat, b, _ = _inputs(B, D, C)
    xs, W = xs[:M], Wcat[M]
    out, out_m, loss, loss_m, dW, db = (torch.empty(s, **F32) for s in ((B, C), (M, B, C), (1,), (M,), (C, M * D), (C,)))
    dxs = [torch.empty((B, D), **F32) for _ in range(M)]
    ops.concat_head_ce_fwd_bwd(xs, W, b, labels, out, out_m, loss, loss_m, dW, db, dxs,
                               torch.empty(ops.concat_head_ws_elems(B, C, M), **F32), 1.0 / B)
    out2, out_m2 = torch.empty_like(out), torch.empty_like(out_m)
    ops.concat_head_fwd(xs, W, b, out2, out_m2)
    loss2, dl = _ce(out2, labels)
    dW2, db2, dxs2 = torch.empty_like(dW), torch.empty_like(db), [torch.empty_like(t) for t in dxs]
    ops.concat_head_bwd(xs, W, dl, dW2, db2, dxs2, 1.0)
    pairs = [("out", out, out2), ("out_m", out_m, out_m2), ("loss", loss, loss2), ("dW", dW, dW2), ("db", db, db2)]
    pairs += [(f"dx[{m}]", dxs[m], dxs2[m]) for m in range(M)]
    if bad:
        assert torch.isnan(loss).all() and torch.isnan(loss2).all() and torch.isnan(loss_m).all()
        assert bool((dl[0] == 0).all()) and bool((dl[-1] == 0).all()) and torch.isfinite(dW).all() and torch.isfinite(db).all()
        pairs = [p for p in pairs if p[0] != "loss"]
    for name, a, c in pairs:
        _same(a, c, f"concat_head_ce_fwd_bwd {name} vs concat_head_fwd -> ce_fwd_bwd -> concat_head_bwd")
    for m in range(M):
        lm = _ce(out_m2[m].contiguous(), labels)[0]
        if bad:
            assert torch.isnan(lm).all()
        else:
            _same(loss_m[m:m + 1], lm, f"loss_m[{m}] vs ce_fwd_bwd(out_m[{m}])")
