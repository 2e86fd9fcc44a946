"""CPU: the transformer encoder's launch wiring, recorded instead of launched.  `ops._call` is replaced by a recorder, so one
forward and one backward_from_pooled of a small encoder run through on the CPU without the library; the tests then check that
every Linear of the layout is launched once per direction, on its own weight / image / gradient views and dims, through the
entry points of the encoder's arithmetic -- for the 4 kinds x 3 arithmetics -- and that grads_as_reference() is the registered
gradient views, copied."""
import pytest
import torch

from mla_hip import m3ae, ops
from mla_hip.m3ae import M3AEEncoder

DEPTH, D, B = 2, 128, 2
ENTRY = {"f32": ("mla_linear_fwd", "mla_linear_dgrad", "mla_linear_wgrad"),
         "split": ("mla_linear_fwd_split", "mla_linear_dgrad_split", "mla_linear_wgrad_split_bias"),
         "bf16": ("mla_linear_fwd_bf16", "mla_linear_dgrad_bf16", "mla_linear_wgrad_bias_bf16")}
LINEAR_ENTRIES = {e for es in ENTRY.values() for e in es} | {"mla_linear_wgrad_split", "mla_linear_wgrad_bf16"}


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(ops, "_call", lambda name, *args: rec.append((name, args)))
    monkeypatch.setattr(ops, "_p", lambda t, dtype=torch.float32: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "cur_stream", lambda: 0)
    monkeypatch.setattr(ops, "linear_wgrad_ws_bytes", lambda *a: 4096)
    monkeypatch.setattr(ops, "colreduce_ws_elems", lambda M, C: 1024)
    monkeypatch.setattr(ops, "tokens_assemble_bwd_ws_bytes", lambda B_, L, D_: 4096)
    monkeypatch.setattr(m3ae, "FUSE_BIAS_GRAD", True)
    return rec


def _encoder(kind, math):
    return M3AEEncoder(kind, device="cpu", depth=DEPTH, emb_dim=D, num_heads=2, text_vocab_size=50, seed=3, conv_math=math)


def _inputs(kind):
    g = torch.Generator().manual_seed(0)
    if kind == "text":
        return torch.randint(0, 50, (B, 1, 16), generator=g), (torch.rand((B, 1, 16), generator=g) < 0.3).float()
    shape = {"image": (B, 3, 64, 64), "audio": (B, 1024, 128), "cav_visual": (B, 3, 224, 224)}[kind]
    return torch.randn(shape, generator=g), None


# positions in the C argument lists (ops.linear_fwd / linear_dgrad / linear_wgrad / colsum_rows)
def _fwd(a): return dict(w=a[1], b=a[2], K=a[-3], N=a[-2])
def _dgrad(a): return dict(w=a[1], K=a[-3], N=a[-2])
def _wgrad(a, f32): return dict(dw=a[2], db=None if f32 else a[3], K=a[-5], N=a[-4])


@pytest.mark.parametrize("math", ["f32", "split", "bf16"])
@pytest.mark.parametrize("kind", ["text", "image", "audio", "cav_visual"])
def test_every_linear_is_launched_once_per_direction_on_its_own_operands(calls, kind, math):
    enc = _encoder(kind, math)
    inp, pm = _inputs(kind)
    enc.forward(inp, pm)
    enc.backward_from_pooled(torch.ones((B, D)))
    f32 = math == "f32"
    e_fwd, e_dgrad, e_wgrad = ENTRY[math]
    names = [n for n, _a in calls]
    assert {n for n in names if n in LINEAR_ENTRIES} == set(ENTRY[math])                  # no Linear call of another arithmetic

    weights = [k for k, (_o, shp) in enc.layout.items() if len(shp) == 2 and k.endswith(".weight") and k != "text_embedding.weight"]
    embed = [w for w in weights if not w.startswith("encoder.blocks.")]
    assert len(weights) == DEPTH * 4 + len(embed) and len(embed) == (0 if kind == "text" else 1)
    assert names.count(e_fwd) == len(weights) and names.count(e_wgrad) == len(weights) and names.count(e_dgrad) == DEPTH * 4
    assert names.count("mla_colsum_rows") == (DEPTH * 4 if f32 else 0) + 1 + len(embed)

    for W in weights:
        K, N = enc.layout[W][1]
        bias = W[:-len("weight")] + "bias"
        img_fwd, img_dgrad = (enc.p[W], enc.p[W]) if f32 else enc.wsp[W]
        fwd = [_fwd(a) for n, a in calls if n == e_fwd and _fwd(a)["w"] == img_fwd.data_ptr()]
        assert fwd == [dict(w=img_fwd.data_ptr(), b=enc.p[bias].data_ptr(), K=K, N=N)], W
        at = [i for i, (n, a) in enumerate(calls) if n == e_wgrad and _wgrad(a, f32)["dw"] == enc.g[W].data_ptr()]
        assert len(at) == 1, W
        wg = _wgrad(calls[at[0]][1], f32)
        assert (wg["K"], wg["N"]) == (K, N), W
        dgrad = [_dgrad(a) for n, a in calls if n == e_dgrad and _dgrad(a)["w"] == img_dgrad.data_ptr()]
        if W in embed:   # the input projection: no input gradient, and its bias gradient is not the weight-gradient kernel's
            assert dgrad == [] and wg["db"] is None, W
            continue
        assert dgrad == [dict(w=img_dgrad.data_ptr(), K=K, N=N)], W
        if f32:      # the bias gradient: a column reduction over the same dy, launched immediately before the weight gradient
            n_prev, a_prev = calls[at[0] - 1]
            assert n_prev == "mla_colsum_rows" and a_prev[1] == enc.g[bias].data_ptr() and a_prev[4] == N, W
            assert a_prev[0] == calls[at[0]][1][1], W
        else:        # ... or out of the weight-gradient kernel's own pass
            assert wg["db"] == enc.g[bias].data_ptr(), W


@pytest.mark.parametrize("kind", ["text", "image", "audio", "cav_visual"])
def test_grads_as_reference_copies_the_registered_gradient_views(kind):
    enc = _encoder(kind, "f32")
    enc.grad.copy_(torch.arange(enc.numel, dtype=torch.float32))
    got = enc.grads_as_reference()
    assert set(got) == {name for name, _p, _gv in enc._entries}
    assert len(got) == len(enc._entries) == len(enc.layout)
    for name, p, gv in enc._entries:
        g = got[name]
        assert g.shape == gv.shape == p.shape and torch.equal(g, gv), name
        assert g.is_contiguous(), name
        assert g.untyped_storage().data_ptr() != enc.grad.untyped_storage().data_ptr(), name
