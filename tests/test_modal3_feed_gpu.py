"""GPU: mla_modal3_assemble (csrc/modal3.hip) bit for bit -- present rows equal their sources, absent rows have every bit clear
whatever their source held, nothing outside the batch is written -- and the Modal3Batcher -> DeviceFeeder path against the
reference's expressions (Pillow's transform, then `x * mask`) and into MLATrainer(Modal3Classifier)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jitter_model as J  # noqa: E402
from mla_hip import DeviceFeeder, M3AEBatcher, Modal3Batcher, ops  # noqa: E402
from mla_hip.frames import make_lut  # noqa: E402
from test_modal3_feed_cpu import ALL_ROWS, SIZES, _write_modal3_dataset  # noqa: E402

GUARD_ROWS = 2
INT64_MIN = -(1 << 63)
SHAPES = {"tile": (5, 40, 64 * 16, 256),          # B, S, T*F, L: 1200 + 256 + 128 + 64 units per sample, more than one block
          "ragged": (5, 36, 24 * 4, 12)}          # 972 + 24 + 6 + 3 units: no range is a multiple of the 256-thread block
PATTERNS = {"all": ([[1, 1, 1]] * 5, [0, 1, 2, 3, 4]),
            "no_image": ([[1, 0, 1], [0, 0, 1], [1, 0, 0], [1, 0, 1], [0, 0, 1]], [-1] * 5),
            # every non-zero row within two launches of five, the slots not in batch order
            "mixed_a": (ALL_ROWS[:5], [-1, 1, -1, 0, -1]),
            "mixed_b": ([ALL_ROWS[5], ALL_ROWS[6], ALL_ROWS[1], ALL_ROWS[0], ALL_ROWS[3]], [2, 0, 3, -1, 1])}


def _case(shape, pattern, seed=0):
    """Device buffers with GUARD_ROWS guard rows behind row B (and behind row P of the compact images), the rows of absent
    modalities pre-filled with NaN / INT64_MIN, and host copies of everything as it is before the launch."""
    B, S, TF, L = SHAPES[shape]
    rows, slots = PATTERNS[pattern]
    table = torch.tensor([r + [s] for r, s in zip(rows, slots)], dtype=torch.int64)
    P = sum(r[1] for r in rows)
    g = torch.Generator().manual_seed(seed)
    compact = torch.randn((P + GUARD_ROWS, 3, S, S), generator=g)
    compact[0, 0, 0, :4] = torch.tensor([-0.0, float("inf"), -1e-45, 3.0]) if P else compact[0, 0, 0, :4]
    spec = torch.randn((B + GUARD_ROWS, TF), generator=g)
    token = torch.randint(-5, 30000, (B + GUARD_ROWS, L), generator=g)
    pm = (torch.rand((B + GUARD_ROWS, L), generator=g) < 0.5).float()
    for b, r in enumerate(rows):
        if not r[0]:
            spec[b] = float("nan")
        if not r[2]:
            token[b] = INT64_MIN
            pm[b] = float("nan")
    out = torch.full((B + GUARD_ROWS, 3, S, S), float("nan"))
    host = dict(compact=compact, spec=spec, token=token, pm=pm, out=out)
    return table, P, host


def _launch(table, P, host, via_op=False):
    B = table.shape[0]
    dev = {k: v.cuda() for k, v in host.items()}
    if via_op:
        import mla_hip  # noqa: F401  registers torch.ops.mla_hip
        S = host["out"].shape[-1]
        image = torch.ops.mla_hip.modal3_assemble(dev["compact"][:P], dev["spec"][:B], dev["token"][:B], dev["pm"][:B], table, S)
        dev["out"][:B] = image
    else:
        ops.modal3_assemble(dev["compact"][:P] if P else None, dev["spec"][:B], dev["token"][:B], dev["pm"][:B], table.cuda(), table,
                            dev["out"][:B])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dev.items()}


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.int64 else torch.int32)


@pytest.fixture(scope="module")
def runs():
    """Every (shape, pattern) once: (table, P, host tensors before, host tensors after)."""
    out = {}
    for shape in SHAPES:
        for pattern in PATTERNS:
            table, P, host = _case(shape, pattern)
            out[shape, pattern] = (table, P, host, _launch(table, P, host))
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_present_rows_are_their_sources_and_absent_rows_are_all_bits_clear(runs, shape, pattern):
    table, P, before, after = runs[shape, pattern]
    B = table.shape[0]
    assert torch.equal(_bits(after["compact"]), _bits(before["compact"]))                    # the input images are only read
    for b, (a, i, t, slot) in enumerate(table.tolist()):
        if i:
            assert torch.equal(_bits(after["out"][b]), _bits(before["compact"][slot])), b    # -0.0, Inf and denormals included
        else:
            assert not _bits(after["out"][b]).any(), b
        for present, keys in ((a, ("spec",)), (t, ("token", "pm"))):
            for k in keys:
                if present:
                    assert torch.equal(_bits(after[k][b]), _bits(before[k][b])), (k, b)
                else:
                    assert not _bits(after[k][b]).any(), (k, b)
    for k in ("spec", "token", "pm", "out"):                                                 # guard rows behind row B
        assert torch.equal(_bits(after[k][B:]), _bits(before[k][B:])), k
    assert {tuple(r) for p in ("mixed_a", "mixed_b") for r in PATTERNS[p][0]} == {tuple(r) for r in ALL_ROWS}


def test_rerun_is_bit_identical_and_the_torch_op_gives_the_launchers_bits(runs):
    for key in (("tile", "mixed_b"), ("ragged", "mixed_a"), ("ragged", "no_image")):
        table, P, before, after = runs[key]
        again, op = _launch(table, P, before), _launch(table, P, before, via_op=True)
        for k in after:
            assert torch.equal(_bits(after[k]), _bits(again[k])) and torch.equal(_bits(after[k]), _bits(op[k])), (key, k)
    table, P, before, _ = runs["tile", "all"]
    with pytest.raises(NotImplementedError):                        # no CPU implementation is registered
        torch.ops.mla_hip.modal3_assemble(before["compact"][:P], before["spec"][:5], before["token"][:5], before["pm"][:5], table, 40)


# ---- the batcher through DeviceFeeder ----------------------------------------------------------------------------------------
OUT = 40
LABELS = [3, 2, 1, 0, 3, 2, 1]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return _write_modal3_dataset(str(tmp_path_factory.mktemp("modal3")), 7, SIZES)


def _lut_of(u8_hwc, lut):
    idx = torch.as_tensor(np.ascontiguousarray(u8_hwc)).long().permute(2, 0, 1)
    return torch.stack([lut[c][idx[c]] for c in range(3)])


def _fed(dataset, mask, train, **kw):
    names, text, audio, visual, _flat = dataset
    kw = dict(dict(seed=4, pin=True, out_size=OUT, threads=2), **kw)
    fb = Modal3Batcher(names, LABELS, 3, text, audio, visual_feature_path=visual, train=train, mask=mask, **kw)
    got = [tuple(t.cpu() for t in batch) for batch in DeviceFeeder(fb, depth=3)]
    torch.cuda.synchronize()
    fb.close()
    return got


@pytest.fixture(scope="module")
def fed(dataset):
    """The 7-sample dataset under the mask of all 7 non-zero rows, train and eval, once."""
    return {train: _fed(dataset, np.array(ALL_ROWS), train) for train in (True, False)}


@pytest.mark.parametrize("train", [True, False])
def test_fed_batches_equal_the_reference_expressions(dataset, fed, train):
    """image = lut[Pillow's transform of the sample's own draws] * mask[:, 1], spec = the raw fbank * mask[:, 0], token and
    padding mask * mask[:, 2] (dataset.py:794-801), with torch.equal: -0.0 == +0.0."""
    names, text, audio, visual, _flat = dataset
    mask = np.array(ALL_ROWS)
    lut = make_lut()
    host = Modal3Batcher(names, LABELS, 3, text, audio, visual_feature_path=visual, train=train, mask=np.ones((7, 3), dtype=np.int64),
                         seed=4, pin=False, out_size=OUT, threads=2)
    seen = 0
    for (h_token, h_pm, h_spec, frames, desc, jdesc, _md, _l, _i), (token, pm, image, spec, label, idx) in zip(host, fed[train]):
        n = label.shape[0]
        assert image.shape == (n, 3, OUT, OUT) and spec.shape == (n, 1024, 128) and token.shape == (n, 1, 256) and idx.shape == (n, 1)
        assert token.dtype == torch.int64 and pm.dtype == image.dtype == spec.dtype == torch.float32
        assert label.tolist() == LABELS[seen:seen + n] and idx[:, 0].tolist() == list(range(seen, seen + n))
        for j in range(n):
            m = torch.from_numpy(mask[seen + j])
            off, H, W = (int(v) for v in desc[j, :3])
            pil = J.augment_pil(frames[off:off + H * W * 3].numpy().reshape(H, W, 3), desc[j].numpy(), jdesc[j].numpy(), OUT, OUT)
            assert torch.equal(image[j], _lut_of(pil, lut) * m[1]), (seen + j, "image")
            assert torch.equal(spec[j], h_spec[j] * m[0]), (seen + j, "spec")
            assert torch.equal(token[j], h_token[j] * m[2]) and torch.equal(pm[j], h_pm[j] * m[2]), (seen + j, "text")
            if not m[1]:
                assert not image[j].view(torch.int32).any()
        seen += n
    host.close()
    assert seen == 7


def test_all_ones_mask_equals_the_m3ae_batcher(dataset):
    names, text, audio, _visual, flat = dataset
    got = _fed(dataset, np.ones((7, 3), dtype=np.int64), True)
    fb = M3AEBatcher(names, LABELS, 3, text, visual_feature_path=flat, train=True, seed=4, pin=True, out_size=OUT, threads=2)
    want = [tuple(t.cpu() for t in batch) for batch in DeviceFeeder(fb, depth=3)]
    fb.close()
    assert len(got) == len(want) == 3
    for (token, pm, image, spec, label, idx), (w_token, w_pm, w_image, w_label, w_idx) in zip(got, want):
        assert torch.equal(image.view(torch.int32), w_image.view(torch.int32)) and torch.equal(token, w_token) and torch.equal(pm, w_pm)
        assert torch.equal(label, w_label) and torch.equal(idx, w_idx)
        for j, i in enumerate(idx[:, 0].tolist()):
            assert np.array_equal(spec[j].numpy(), np.load(os.path.join(audio, names[i] + ".npy")))


def test_batches_do_not_depend_on_threads_or_ring_depth(dataset, fed):
    for kw in (dict(threads=1, ring=2), dict(threads=4, ring=4)):
        for got, want in zip(_fed(dataset, np.array(ALL_ROWS), True, **kw), fed[True]):
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want)), kw


def test_modal3_batcher_through_device_feeder_into_the_trainer(tmp_path):
    """One MLA step of the three-encoder model at the real 256 / 1024 x 128 shapes, fed at a mask rate of 0.5."""
    from mla_hip import MLATrainer, Modal3Classifier
    names, text, audio, visual, _flat = _write_modal3_dataset(str(tmp_path), 4, [(90, 120), (150, 100)], n_frames=2)

    class Args:
        fusion_method, dataset, gs_flag, modulation, modal3 = "concat", "IEMOCAP", True, "Normal", True
    model = Modal3Classifier(Args(), depth=1, text_vocab_size=64, seed=0)
    tr = MLATrainer(model)
    tr.keep_debug = False
    before = {tag: enc.flat.clone() for tag, _g, enc in model.mla_encoders()}
    fb = Modal3Batcher(names, [0, 1, 2, 3], 4, text, audio, visual_feature_path=visual, mask_percent=0.5, mask_seed=0, seed=1, pin=True)
    assert fb.mask.sum() == 6 and (fb.mask.sum(axis=1) >= 1).all()
    steps = 0
    for token, pm, image, spec, label, idx in DeviceFeeder(fb, depth=3):
        assert image.shape == (4, 3, 256, 256) and spec.shape == (4, 1024, 128) and token.shape == (4, 1, 256)
        absent = torch.from_numpy(fb.mask == 0)
        assert not image[absent[:, 1]].view(torch.int32).any() and not spec[absent[:, 0]].view(torch.int32).any()
        assert not token[absent[:, 2]].any() and not pm[absent[:, 2]].view(torch.int32).any()
        losses = tr.train_step(token, pm, image, spec, label, 0, 1)
        steps += 1
    tr.join()
    torch.cuda.synchronize()
    fb.close()
    assert steps == 1 and set(losses) == {"loss", "loss_a", "loss_v", "loss_t"}
    for k in ("loss_a", "loss_v", "loss_t"):
        assert torch.isfinite(losses[k]).all(), (k, losses[k])
    assert set(before) == {"a", "v", "t"}
    for tag, _g, enc in model.mla_encoders():
        assert torch.isfinite(enc.flat).all() and not torch.equal(enc.flat, before[tag]), tag
