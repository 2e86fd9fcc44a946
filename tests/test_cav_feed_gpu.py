"""GPU: the CAV-MAE batch feed's two kernels -- mla_image_resample (csrc/frames.hip) against PIL's BICUBIC resize + crop and
torchvision's ToTensor / Normalize torch ops, mla_fbank_augment (csrc/fbank.hip) against the reference's literal torch CPU
expressions with the uniforms of a numpy Philox4x32-10 -- all bit for bit, and the CAVBatcher -> DeviceFeeder path into MLATrainer."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_cav_feed_cpu import _write_dataset, pil_window  # noqa: E402

BICUBIC, BILINEAR = 1, 0


def _run(frames_u8, desc, B, T, OH, OW, filt=BICUBIC, lut=None):
    from mla_hip import ops
    from mla_hip.frames import make_lut
    lut = make_lut() if lut is None else lut
    desc_host = torch.as_tensor(np.ascontiguousarray(desc), dtype=torch.int64)
    out = torch.full((B, 3, T, OH, OW), float("nan"), device="cuda")
    ops.image_resample(torch.as_tensor(frames_u8).cuda(), desc_host.cuda(), desc_host, lut.cuda(), out, T, filt)
    torch.cuda.synchronize()
    return out.cpu()


def _lut_of(u8_hwc, lut):
    idx = torch.as_tensor(np.ascontiguousarray(u8_hwc)).long().permute(2, 0, 1)
    return torch.stack([lut[c][idx[c]] for c in range(3)])


def _cpu_pipeline(frame, row, size):
    """The reference's transform on the host: PIL crop, BICUBIC resize, window (+ flip), then torch ToTensor and Normalize."""
    from mla_hip.frames import MEAN, STD
    u8 = pil_window(frame, *[int(v) for v in row[3:]], size, size)
    t = torch.from_numpy(np.array(u8, np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(dtype=torch.float32).div(255)
    return t.sub_(torch.as_tensor(MEAN)[:, None, None]).div_(torch.as_tensor(STD)[:, None, None])


def test_bicubic_equals_lut_of_pil_on_the_fixture(golden_dir):
    from mla_hip.frames import make_lut
    fx = np.load(os.path.join(golden_dir, "cav_feed_small.npz"))
    lut = make_lut()
    for g in ("w32", "w224"):
        desc, want = fx[f"desc_{g}"], fx[f"out_{g}"]
        N, OH, OW = want.shape[:3]
        out = _run(fx["frames"], desc, N, 1, OH, OW, BICUBIC, lut)
        for n in range(N):
            assert torch.equal(out[n, :, 0], _lut_of(want[n], lut)), (g, n, desc[n])


def test_bicubic_bitwise_vs_live_pil_mixed_sizes_one_launch():
    pytest.importorskip("PIL")
    from mla_hip import image_descriptors, resize_center_crop
    rng = np.random.default_rng(12)
    B, T = 3, 2
    shapes = [(360, 480), (480, 360), (224, 300), (37, 23), (225, 500), (97, 131)]
    frames = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in shapes]
    yy, xx = np.mgrid[0:97, 0:131]
    frames[5] = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)          # all 0 / 255
    boxes = [(0, 0, H, W, 0) for (H, W) in shapes]
    boxes[1] = (0, 0, 480, 360, 1)                                                                   # flipped
    boxes[4] = (3, 17, 210, 401, 0)                                                                  # a non-trivial crop box
    desc, nbytes = image_descriptors(shapes, boxes, [resize_center_crop(b[2], b[3], 224) for b in boxes])
    packed = np.concatenate([f.reshape(-1) for f in frames])
    assert packed.size == nbytes
    out = _run(packed, desc, B, T, 224, 224)
    assert not torch.isnan(out).any()
    for n in range(B * T):
        assert torch.equal(out[n // T, :, n % T], _cpu_pipeline(frames[n], desc[n], 224)), (n, shapes[n], boxes[n])


def test_bilinear_through_the_new_entry_point_equals_frames_resample():
    from mla_hip import frame_descriptors, ops
    from mla_hip.frames import make_lut
    rng = np.random.default_rng(6)
    shapes = [(120, 90), (50, 70), (224, 224), (300, 410)]
    boxes = [(0, 0, 120, 90, 0), (3, 4, 40, 50, 1), (0, 0, 224, 224, 1), (20, 10, 260, 333, 0)]
    frames = torch.from_numpy(np.concatenate([rng.integers(0, 256, size=s + (3,), dtype=np.uint8).reshape(-1) for s in shapes])).cuda()
    d8, _ = frame_descriptors(shapes, boxes)
    lut = make_lut().cuda()
    for OH, OW in ((224, 224), (33, 48)):
        d12 = np.concatenate([d8, np.tile(np.array([[OH, OW, 0, 0]], dtype=np.int64), (4, 1))], axis=1)
        h8, h12 = torch.from_numpy(d8), torch.from_numpy(np.ascontiguousarray(d12))
        want = ops.frames_resample(frames, h8.cuda(), h8, lut, torch.full((2, 3, 2, OH, OW), float("nan"), device="cuda"), 2)
        got = ops.image_resample(frames, h12.cuda(), h12, lut, torch.full((2, 3, 2, OH, OW), float("nan"), device="cuda"), 2, BILINEAR)
        torch.cuda.synchronize()
        assert not torch.isnan(want).any() and torch.equal(got, want), (OH, OW)


def test_bicubic_large_downscale_halves_the_band():
    """(1080, 1920) -> 224: 21 taps per pass and about 97 source rows per 16-row band do not fit the LDS, so the planner halves
    the band; the result still equals PIL."""
    pytest.importorskip("PIL")
    from mla_hip import image_descriptors, resize_center_crop
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, size=(1080, 1920, 3), dtype=np.uint8)
    desc, _ = image_descriptors([(1080, 1920)], [(0, 0, 1080, 1920, 0)], [resize_center_crop(1080, 1920, 224)])
    out = _run(frame.reshape(-1), desc, 1, 1, 224, 224)
    assert torch.equal(out[0, :, 0], _cpu_pipeline(frame, desc[0], 224))


# ---- the spectrogram kernel --------------------------------------------------------------------------------------------------
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, stream_id, seed):
    """Philox4x32-10 on a uint64 array of counters: four uint32 arrays (the words of each block)."""
    c = [counter & M32, counter >> np.uint64(32), np.full_like(counter, stream_id & 0xFFFFFFFF), np.full_like(counter, stream_id >> 32)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def uniforms(T, F, stream_id, seed):
    """u(b, i) of include/mla_hip.h as a (T, F) fp32 tensor: word i % 4 of block i / 4, top 24 bits * 2^-24."""
    i = np.arange(T * F, dtype=np.uint64)
    words = np.stack(philox4x32_10(i >> np.uint64(2), stream_id, seed))              # (4, T*F)
    r = words[(i & np.uint64(3)).astype(np.int64), np.arange(T * F)]
    u = (r >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy(u.reshape(T, F))


def test_philox_restatement_known_answer():
    """Random123's known-answer vectors for philox4x32-10, so that the restatement the kernel is held to is itself pinned."""
    ff = 0xFFFFFFFFFFFFFFFF
    got = [int(w[0]) for w in philox4x32_10(np.array([ff], dtype=np.uint64), ff, ff)]
    assert got == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    got = [int(w[0]) for w in philox4x32_10(np.array([0], dtype=np.uint64), 0, 0)]
    assert got == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def reference_fbank(x, row, mean, std, seed):
    """dataset.py:281-294, 303-321 with torch CPU ops on one (T, F) sample; the uniforms stand in for torch.rand(T, F)."""
    flags, f0, fw, t0, tw, roll, bits, sid = (int(v) for v in row)
    fbank = x.clone()
    if flags:
        fmask = (torch.arange(x.shape[1]) >= f0) & (torch.arange(x.shape[1]) < f0 + fw)
        tmask = (torch.arange(x.shape[0]) >= t0) & (torch.arange(x.shape[0]) < t0 + tw)
        fbank = fbank.masked_fill(fmask[None, :], 0.0).masked_fill(tmask[:, None], 0.0)
    fbank = (fbank - mean) / (std)
    if flags:
        s = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])        # np.random.rand(), already representable in fp32
        fbank = fbank + uniforms(x.shape[0], x.shape[1], sid, seed) * s / 10
        fbank = torch.roll(fbank, roll, 0)
    return fbank


@pytest.mark.parametrize("shape", [(4, 64, 16), (2, 1024, 128), (8, 13, 12)])
def test_fbank_augment_equals_the_reference_expressions(shape):
    from mla_hip import fbank_descriptors, ops
    B, T, F = shape
    g = torch.Generator().manual_seed(B * T)
    x = torch.randn(shape, generator=g) * 4.5 - 5.0
    mean, std, seed = -5.081, 4.4849, 0x1234567890ABCDEF
    fq, tq = max(F // 4, 1), max(T // 4, 1)
    full = [None,                                            # flags = 0: only normalised
            (F - fq, fq, T - tq, tq, 0.37, 0),               # roll = 0, masks ending exactly at F / T
            (0, fq, 0, tq, 0.999, -T),                       # roll = -T (the same shift as 0)
            (2, 0, 3, tq, 0.5, -(T // 3)),                   # negative roll, fw = 0
            (1, fq, 2, tq, 0.0625, T // 2 + 1),              # positive roll
            (0, F, 0, 0, 0.25, T - 1),                       # every bin masked, tw = 0
            (1, 1, 1, 1, 1e-3, -1),
            (0, 0, 0, 0, 0.75, 1)]                           # no mask at all: noise and roll only
    # (4, 64, 16) holds the first four; (2, 1024, 128) a positive and a negative roll at the reference's mask parameters, one
    # mask ending exactly at F / T; (8, 13, 12) all eight in one launch (odd T, F no power of two)
    draws = full[:B] if B >= 4 else [(F - 48, 48, T - 192, 192, 0.61, 517), (3, 17, 100, 150, 0.123, -1000)]
    desc = fbank_descriptors(draws, [(1 << 40) + 7 * b for b in range(B)])
    dh = torch.from_numpy(desc)
    out = torch.full(shape, float("nan"), device="cuda")
    ops.fbank_augment(x.cuda(), out, dh.cuda(), dh, mean, std, seed)
    torch.cuda.synchronize()
    out = out.cpu()
    assert not torch.isnan(out).any()
    for b in range(B):
        want = reference_fbank(x[b], desc[b], mean, std, seed)
        assert torch.equal(out[b], want), (b, draws[b], (out[b] != want).sum().item())


def test_torch_ops_match_the_launchers():
    import mla_hip  # noqa: F401  registers torch.ops.mla_hip
    from mla_hip import fbank_descriptors, image_descriptors, ops, resize_center_crop
    from mla_hip.frames import make_lut
    rng = np.random.default_rng(2)
    shapes = [(50, 70), (80, 33)]
    frames = np.concatenate([rng.integers(0, 256, size=s + (3,), dtype=np.uint8).reshape(-1) for s in shapes])
    boxes = [(3, 4, 40, 50, 1), (0, 0, 80, 33, 0)]
    desc, _ = image_descriptors(shapes, boxes, [resize_center_crop(b[2], b[3], 24) for b in boxes])
    got = torch.ops.mla_hip.image_resample(torch.from_numpy(frames).cuda(), torch.from_numpy(desc), make_lut().cuda(), 2, 24, 24)
    assert got.shape == (1, 3, 2, 24, 24) and torch.equal(got.cpu(), _run(frames, desc, 1, 2, 24, 24))
    x = torch.randn((2, 64, 16), generator=torch.Generator().manual_seed(1)).cuda()
    fd = torch.from_numpy(fbank_descriptors([(2, 3, 10, 20, 0.5, -9), None], [5, 6]))
    got = torch.ops.mla_hip.fbank_augment(x, fd, -5.081, 4.4849, 77)
    want = ops.fbank_augment(x, torch.full_like(x, float("nan")), fd.cuda(), fd, -5.081, 4.4849, 77)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and not torch.isnan(got).any()
    with pytest.raises(NotImplementedError):                        # no CPU implementation is registered
        torch.ops.mla_hip.fbank_augment(x.cpu(), fd, -5.081, 4.4849, 77)


def _cav_trainer():
    from mla_hip import CAVClassifier, MLATrainer

    class Args:
        fusion_method, dataset, gs_flag, modulation, lorb = "concat", "CREMAD", True, "Normal", "large"
    tr = MLATrainer(CAVClassifier(Args(), depth=2, seed=0), lr=1e-3)         # the reduced depth of test_cav_gpu.py
    tr.keep_debug = False
    return tr


def test_cav_batcher_through_device_feeder_into_the_trainer(tmp_path):
    """Train batcher with --cav_augnois, pinned ring of 2, feeder depth 3, a short last batch: every fed batch equals, bit for
    bit, the two ops run on the batcher's host tuple, and two MLA steps on them give finite losses."""
    pytest.importorskip("PIL")
    import mla_hip
    from mla_hip import CAVBatcher, DeviceFeeder
    from mla_hip.frames import make_lut
    names, audio, visual = _write_dataset(str(tmp_path), 5, [(90, 120), (150, 100), (72, 96)])
    labels = [i % 6 for i in range(5)]
    kw = dict(visual_feature_path=visual, train=True, augnois=True, seed=3, threads=4, ring=2, pin=True)
    want, lut = [], make_lut().cuda()
    for spec, frames, desc, fdesc, label, idx in CAVBatcher(names, labels, 2, audio, **kw):
        image = torch.ops.mla_hip.image_resample(frames.cuda(), desc.clone(), lut, 1, 224, 224, 1)
        sp = torch.ops.mla_hip.fbank_augment(spec.cuda(), fdesc.clone(), -5.081, 4.4849, 3)
        want.append((sp.cpu(), image[:, :, 0].cpu(), label.clone(), idx.clone()))
        assert bool((fdesc[:, 0] == 1).all())
    fb = CAVBatcher(names, labels, 2, audio, **kw)
    tr, got, losses = _cav_trainer(), [], []
    for s, (spec, image, label, idx) in enumerate(DeviceFeeder(fb, depth=3)):
        assert image.shape[1:] == (3, 224, 224) and image.dtype == torch.float32 and spec.shape[1:] == (1024, 128)
        got.append((spec.cpu(), image.cpu(), label.cpu(), idx.cpu()))
        if s < 2:
            assert label.shape[0] == 2
            losses.append(tr.train_step(spec, image, label, s, 3))
    tr.join()
    torch.cuda.synchronize()
    fb.close()
    assert len(got) == len(want) == 3 and got[-1][2].shape[0] == 1
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert torch.equal(a, b)
    for l in losses:
        assert all(torch.isfinite(l[k]).all() for k in ("loss", "loss_a", "loss_v"))
    assert torch.isfinite(tr.model.mae_a.flat).all() and torch.isfinite(tr.model.mae_v.flat).all()


def test_eval_batcher_equals_the_pillow_pipeline_end_to_end(tmp_path):
    """train=False (augnois set, and ignored): image = PIL BICUBIC Resize + CenterCrop + ToTensor + Normalize of the middle
    frame, spectrogram = (fbank - mean) / std with torch CPU ops; from the JPEGs and from the decoded cache."""
    pytest.importorskip("PIL")
    from mla_hip import CAVBatcher, DeviceFeeder, decode_middle_frames, pick_middle_frame, resize_center_crop
    from mla_hip.frames import decode_jpeg
    names, audio, visual = _write_dataset(str(tmp_path), 3, [(90, 120), (150, 100)])
    cache = str(tmp_path / "cache")
    decode_middle_frames(visual, cache, names)
    for source in ({"visual_feature_path": visual}, {"frame_cache": cache}):
        fb = CAVBatcher(names, [0, 1, 2], 2, audio, train=False, augnois=True, seed=1, ring=2, pin=True, **source)
        n = 0
        for spec, image, label, idx in DeviceFeeder(fb, depth=3):
            for j, i in enumerate(idx[:, 0].tolist()):
                d = os.path.join(visual, names[i])
                frame = decode_jpeg(os.path.join(d, pick_middle_frame(d)))
                H, W = frame.shape[:2]
                row = [0, H, W, 0, 0, H, W, 0] + list(resize_center_crop(H, W, 224))
                assert torch.equal(image[j].cpu(), _cpu_pipeline(frame, row, 224)), (source, i)
                fbank = torch.tensor(np.load(os.path.join(audio, names[i] + ".npy")))
                assert torch.equal(spec[j].cpu(), (fbank - (-5.081)) / (4.4849)), (source, i)
                assert label[j].item() == i
                n += 1
        assert n == 3
        fb.close()
