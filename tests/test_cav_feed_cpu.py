"""CPU: the CAV-MAE batch feed's host side (mla_hip.cav_feed) -- Pillow's 8-bit bicubic resample + CenterCrop window restated in
numpy and pinned bit for bit to PIL, torchvision's Resize / CenterCrop size arithmetic, the torchaudio mask_along_axis
restatement and the other spectrogram draws, descriptor packing, the launch checks of mla_image_check / mla_fbank_check, and
CAVBatcher's host tuples."""
import os

import numpy as np
import pytest
import torch

PRECISION = 22


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _coeffs(inp, out, first, count):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc (bicubic, box = the whole input) of output indices first .. first+count."""
    scale = inp / out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    res = []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), inp) - xmin
        ws = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in ws:
            ww += w
        ks = []
        for w in ws:
            w = w / ww if ww != 0.0 else w
            ks.append(int(-0.5 + w * (1 << PRECISION)) if w < 0 else int(0.5 + w * (1 << PRECISION)))
        res.append((xmin, np.array(ks, dtype=np.int64)))
    return res


def _pass(img, coeffs, axis):
    src = img.astype(np.int64)
    outs = []
    for xmin, k in coeffs:
        sl = src[xmin:xmin + len(k)] if axis == 0 else src[:, xmin:xmin + len(k)]
        acc = (1 << (PRECISION - 1)) + np.tensordot(k, sl, axes=([0], [axis]))
        outs.append(np.clip(acc >> PRECISION, 0, 255).astype(np.uint8))
    return np.stack(outs, axis=axis)


def resample_np(frame, top, left, h, w, flip, full_h, full_w, win_top, win_left, OH, OW):
    """PIL crop(box).resize((full_w, full_h), BICUBIC).crop(window) [.transpose(FLIP_LEFT_RIGHT)] in numpy: only the window's
    coefficients are formed; horizontal first, uint8 clip in between."""
    crop = frame[top:top + h, left:left + w]
    res = _pass(_pass(crop, _coeffs(w, full_w, win_left, OW), 1), _coeffs(h, full_h, win_top, OH), 0)
    return res[:, ::-1] if flip else res


def pil_window(frame, top, left, h, w, flip, full_h, full_w, win_top, win_left, OH, OW):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(frame)).crop((left, top, left + w, top + h)).resize((full_w, full_h), Image.BICUBIC)
    im = im.crop((win_left, win_top, win_left + OW, win_top + OH))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "cav_feed_small.npz")))


def _frame(fx, d):
    off, H, W = int(d[0]), int(d[1]), int(d[2])
    return fx["frames"][off:off + H * W * 3].reshape(H, W, 3)


def test_numpy_bicubic_matches_the_pil_fixture(fixture):
    for g in ("w32", "w224"):
        desc, want = fixture[f"desc_{g}"], fixture[f"out_{g}"]
        assert desc.shape[1] == 12
        OH, OW = want.shape[1:3]
        for d, ref in zip(desc, want):
            got = resample_np(_frame(fixture, d), *[int(v) for v in d[3:]], OH, OW)
            assert np.array_equal(got, ref), (g, d)


def test_fixture_descriptors_follow_resize_center_crop(fixture):
    from mla_hip import resize_center_crop
    for g, size in (("w32", 32), ("w224", 224)):
        for d in fixture[f"desc_{g}"]:
            assert tuple(int(v) for v in d[8:]) == resize_center_crop(int(d[5]), int(d[6]), size), (g, d)


def test_numpy_bicubic_matches_live_pil():
    pytest.importorskip("PIL.Image")
    from mla_hip import resize_center_crop
    rng = np.random.default_rng(4)
    cases = [((37, 23), 224, "noise"),          # upscale
             ((64, 64), 48, "noise"),           # H == W
             ((224, 300), 224, "noise"),        # short side already equal to size
             ((97, 131), 64, "checker"),        # all 0 / 255
             ((360, 480), 224, "noise"), ((480, 360), 224, "noise"), ((225, 500), 224, "noise")]
    for _ in range(5):
        cases.append(((int(rng.integers(8, 300)), int(rng.integers(8, 300))), int(rng.integers(4, 200)), "noise"))
    for (H, W), size, kind in cases:
        if kind == "checker":
            yy, xx = np.mgrid[0:H, 0:W]
            frame = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
        else:
            frame = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        win = resize_center_crop(H, W, size)
        args = (0, 0, H, W, 0) + win + (size, size)
        assert np.array_equal(resample_np(frame, *args), pil_window(frame, *args)), (H, W, size)
    # a crop box and a flip
    frame = rng.integers(0, 256, size=(120, 90, 3), dtype=np.uint8)
    args = (7, 9, 100, 60, 1) + resize_center_crop(100, 60, 32) + (32, 32)
    assert np.array_equal(resample_np(frame, *args), pil_window(frame, *args))


def test_resize_center_crop_hand_computed():
    from mla_hip import resize_center_crop
    assert resize_center_crop(360, 480, 224) == (224, 298, 0, 37)        # ow = int(224 * 480 / 360) = 298, left = round(37.0)
    assert resize_center_crop(480, 360, 224) == (298, 224, 37, 0)        # portrait
    assert resize_center_crop(224, 224, 224) == (224, 224, 0, 0)
    assert resize_center_crop(224, 225, 224) == (224, 225, 0, 0)         # full - size = 1: round(0.5) = 0
    assert resize_center_crop(224, 227, 224) == (224, 227, 0, 2)         # full - size = 3: round(1.5) = 2
    assert resize_center_crop(448, 450, 224) == (224, 225, 0, 0)
    assert resize_center_crop(37, 23, 224) == (360, 224, 68, 0)          # upscale: oh = int(224 * 37 / 23) = 360
    assert resize_center_crop(384, 512, 256) == (256, 341, 0, 42)        # the M3AE eval transform: round(42.5) = 42


def _mask_along_axis_literal(specgram, mask_param, axis, g):
    """torchaudio.functional.mask_along_axis (mask_value 0.0) with its draws taken from `g`."""
    value = torch.rand(1, generator=g) * mask_param
    min_value = torch.rand(1, generator=g) * (specgram.size(axis) - value)
    mask_start = (min_value.long()).squeeze()
    mask_end = (min_value.long() + value.long()).squeeze()
    mask = torch.arange(0, specgram.shape[axis])
    mask = (mask >= mask_start) & (mask < mask_end)
    if axis == 1:
        mask = mask.unsqueeze(-1)
    return specgram.masked_fill(mask, 0.0)


def test_sample_fbank_aug_invariants_determinism_and_torchaudio_transcription():
    from mla_hip import sample_fbank_aug, sample_generator
    seen = set()
    for i in range(300):
        f0, fw, t0, tw, s, roll = sample_fbank_aug(sample_generator(3, 1, i))
        assert 0 <= f0 and f0 + fw <= 128 and 0 <= fw <= 48
        assert 0 <= t0 and t0 + tw <= 1024 and 0 <= tw <= 192
        assert 0.0 <= s < 1.0 and -1024 <= roll < 1024
        seen.add((f0, fw, t0, tw, roll))
    assert len(seen) > 290
    a = sample_fbank_aug(sample_generator(5, 2, 17))
    assert a == sample_fbank_aug(sample_generator(5, 2, 17))
    assert a != sample_fbank_aug(sample_generator(5, 3, 17)) and a != sample_fbank_aug(sample_generator(5, 2, 18))
    # fbank_aug (dataset.py:281-294) on a generator in the same state: transpose to (1, 128, 1024), freq mask on axis 1, time on 2
    for i in range(20):
        f0, fw, t0, tw, _s, _r = sample_fbank_aug(sample_generator(9, 0, i))
        g = sample_generator(9, 0, i)
        fbank = torch.ones(1024, 128).transpose(0, 1).unsqueeze(0)
        fbank = _mask_along_axis_literal(fbank, 48, 1, g)
        fbank = _mask_along_axis_literal(fbank, 192, 2, g)
        got = fbank.squeeze(0).transpose(0, 1)
        want = torch.ones(1024, 128)
        want[:, f0:f0 + fw] = 0
        want[t0:t0 + tw, :] = 0
        assert torch.equal(got, want), i
    # other sizes: the roll stays within +-T
    for i in range(50):
        f0, fw, t0, tw, s, roll = sample_fbank_aug(sample_generator(1, 0, i), T=64, F=16, freqm=6, timem=12)
        assert f0 + fw <= 16 and fw <= 6 and t0 + tw <= 64 and tw <= 12 and -64 <= roll < 64


def test_descriptor_packing():
    from mla_hip import fbank_descriptors, image_descriptors
    desc, total = image_descriptors([(4, 5), (6, 7)], [(0, 0, 4, 5, 0), (1, 2, 5, 5, 1)], [(8, 10, 0, 1), (9, 9, 2, 3)])
    assert desc.dtype == np.int64 and total == (20 + 42) * 3
    assert desc.tolist() == [[0, 4, 5, 0, 0, 4, 5, 0, 8, 10, 0, 1], [60, 6, 7, 1, 2, 5, 5, 1, 9, 9, 2, 3]]
    fd = fbank_descriptors([(3, 4, 5, 6, 0.25, -7), None], [11, 12])
    assert fd.dtype == np.int64 and fd.tolist() == [[1, 3, 4, 5, 6, -7, 0x3E800000, 11], [0, 0, 0, 0, 0, 0, 0, 12]]


def test_image_check_accepts_and_refuses():
    from mla_hip import MLAHipError, image_descriptors, ops, resize_center_crop
    shapes = [(40, 50), (60, 70), (30, 30)]
    boxes = [(0, 0, 40, 50, 0), (1, 2, 50, 50, 1), (0, 0, 30, 30, 0)]
    desc, total = image_descriptors(shapes, boxes, [resize_center_crop(b[2], b[3], 16) for b in boxes])
    ok = torch.from_numpy(desc)
    for filt in (0, 1):
        ops.image_check(ok, 3, 1, total, 16, 16, filt)
    ops.image_check(ok, 1, 3, total, 16, 16)
    big, n = image_descriptors([(1080, 1920)], [(0, 0, 1080, 1920, 0)], [resize_center_crop(1080, 1920, 224)])
    ops.image_check(torch.from_numpy(big), 1, 1, n)                  # fits once the planner has halved the band

    def bad(col, val, match, filt=1, B=3, T=1, nbytes=total, oh=16, ow=16):
        d = ok.clone()
        if col is not None:
            d[0, col] = val
        with pytest.raises(MLAHipError, match=match):
            ops.image_check(d, B, T, nbytes, oh, ow, filt)
    bad(10, 1, "window")                     # win_top + out_h > full_h (frame 0 is 16 x 20 resized)
    bad(11, 5, "window")                     # win_left + out_w > full_w
    bad(10, -1, "window")
    bad(11, -1, "window")
    bad(None, None, "window", oh=17)         # a window taller than the resized image
    bad(8, 0, "resized size")
    bad(9, -4, "resized size")
    bad(5, 0, "empty crop")
    bad(6, 0, "empty crop")
    bad(1, 0, "out of range")
    bad(3, 1, "leaves")                      # crop top + h > H
    bad(7, 2, "flip")
    bad(0, total, "outside")
    bad(None, None, "outside", nbytes=total - 1)
    bad(None, None, "B\\*T", B=2)
    bad(None, None, "out of range", oh=0)
    bad(None, None, "unknown filter", filt=2)
    bad(None, None, "unknown filter", filt=-1)
    with pytest.raises(MLAHipError, match="LDS"):                     # a 60000-row crop squeezed into 2 output rows
        ops.image_check(torch.tensor([[0, 60000, 8, 0, 0, 60000, 8, 0, 2, 8, 0, 0]]), 1, 1, 60000 * 8 * 3, 2, 8)
    with pytest.raises(MLAHipError, match="int64"):
        ops.image_check(ok.int(), 3, 1, total, 16, 16)
    with pytest.raises(MLAHipError, match=r"\(N, 12\)"):
        ops.image_check(ok[:, :8].contiguous(), 3, 1, total, 16, 16)


def test_fbank_check_accepts_and_refuses():
    from mla_hip import MLAHipError, fbank_descriptors, ops
    T, F = 64, 16
    ok = torch.from_numpy(fbank_descriptors([(2, 3, 10, 20, 0.5, -64), (13, 3, 44, 20, 0.25, 64), None, (0, 0, 0, 0, 0.0, 0)], [1, 2, 3, 4]))
    ops.fbank_check(ok, T, F)
    ops.fbank_check(torch.from_numpy(fbank_descriptors([(80, 48, 832, 192, 0.9, -1024)], [7])))       # the defaults: 1024 x 128

    def bad(col, val, match):
        d = ok.clone()
        d[0, col] = val
        with pytest.raises(MLAHipError, match=match):
            ops.fbank_check(d, T, F)
    bad(1, 14, "frequency mask")             # f0 + fw > F
    bad(1, -1, "frequency mask")
    bad(3, 45, "time mask")                  # t0 + tw > T
    bad(2, -1, "negative mask width")
    bad(4, -2, "negative mask width")
    bad(5, 65, "roll")
    bad(5, -65, "roll")
    bad(0, 2, "flags")
    bad(6, 1 << 32, "bit pattern")
    with pytest.raises(MLAHipError, match="std"):
        ops.fbank_check(ok, T, F, std=0.0)
    with pytest.raises(MLAHipError, match="must be > 0"):
        ops.fbank_check(ok, 0, F)
    with pytest.raises(MLAHipError, match="multiple of 4"):
        ops.fbank_check(torch.from_numpy(fbank_descriptors([None], [0])), T, 18)
    with pytest.raises(MLAHipError, match=r"\(N, 8\)"):
        ops.fbank_check(ok[:, :7].contiguous(), T, F)


def test_fbank_augment_refuses_zero_std_before_any_launch():
    """The C entry point validates before it launches: with std == 0 it returns the error without touching its pointers."""
    import ctypes
    from mla_hip import _lib, fbank_descriptors
    lib = _lib.load()
    d = np.ascontiguousarray(fbank_descriptors([None], [0]))
    fake = 0x1000
    assert lib.mla_fbank_augment(fake, fake + (1 << 20), fake, d.ctypes.data_as(ctypes.c_void_p), 1, 64, 16, -5.081, 0.0, 0, None) == -1
    assert b"std" in lib.mla_last_error()
    assert lib.mla_fbank_augment(fake, fake + 64, fake, d.ctypes.data_as(ctypes.c_void_p), 1, 64, 16, -5.081, 4.4849, 0, None) == -1
    assert b"overlap" in lib.mla_last_error()


def test_middle_frame_follows_listdir(tmp_path, monkeypatch):
    from mla_hip import MLAHipError, pick_middle_frame
    for n, want in ((1, 0), (2, 1), (3, 1), (6, 3), (7, 3)):
        d = tmp_path / f"s{n}"
        d.mkdir()
        names = [f"f{i:03d}.jpg" for i in range(n)]
        listing = list(reversed(names))                 # any listdir order is used as it comes: not sorted
        monkeypatch.setattr(os, "listdir", lambda p, _l=listing: list(_l))
        assert pick_middle_frame(str(d)) == listing[want], n
        monkeypatch.undo()
    (tmp_path / "empty").mkdir()
    with pytest.raises(MLAHipError, match="no frames"):
        pick_middle_frame(str(tmp_path / "empty"))


def _write_dataset(root, n_samples, sizes, seed=0):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(seed)
    audio, visual = os.path.join(root, "audio"), os.path.join(root, "visual")
    os.makedirs(audio)
    names = [f"clip{i}" for i in range(n_samples)]
    for i, name in enumerate(names):
        np.save(os.path.join(audio, name + ".npy"), rng.standard_normal((1024, 128)).astype(np.float32))
        d = os.path.join(visual, name)
        os.makedirs(d)
        H, W = sizes[i % len(sizes)]
        for f in range(3 + i % 3):
            yy, xx = np.mgrid[0:H, 0:W]
            img = np.stack([(xx * 3 + f * 40) % 256, (yy * 2 + i * 30) % 256, (xx + yy + f * 17) % 256], -1).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, f"frame_{f:05d}.jpg"), quality=90)
    return names, audio, visual


def test_cav_batcher_host_tuples(tmp_path):
    from mla_hip import CAVBatcher, decode_middle_frames, pick_middle_frame, resize_center_crop
    from mla_hip.cav_feed import fbank_stream_id
    from mla_hip.frames import decode_jpeg
    names, audio, visual = _write_dataset(str(tmp_path), 5, [(60, 80), (72, 50)])
    cache = str(tmp_path / "cache")
    assert decode_middle_frames(visual, cache, names, threads=3) == 5
    labels = [4, 3, 2, 1, 0]
    for train, augnois in ((True, True), (True, False), (False, True)):
        kw = dict(train=train, augnois=augnois, seed=4, pin=False, out_size=32)
        a = [tuple(t.clone() for t in b) for b in CAVBatcher(names, labels, 2, audio, visual_feature_path=visual, threads=3, **kw)]
        c = [tuple(t.clone() for t in b) for b in CAVBatcher(names, labels, 2, audio, frame_cache=cache, threads=1, **kw)]
        assert len(a) == len(c) == 3
        seen = 0
        for x, y in zip(a, c):
            spec, frames, desc, fdesc, label, idx = x
            b = label.shape[0]
            assert b == (2 if seen < 4 else 1)                               # the last batch is short
            assert spec.shape == (b, 1024, 128) and spec.dtype == torch.float32 and frames.dtype == torch.uint8
            assert desc.shape == (b, 12) and fdesc.shape == (b, 8) and idx.shape == (b, 1)
            assert idx[:, 0].tolist() == list(range(seen, seen + b)) and label.tolist() == labels[seen:seen + b]
            nbytes = int(desc[-1, 0] + desc[-1, 1] * desc[-1, 2] * 3)
            assert torch.equal(desc, y[2]) and torch.equal(fdesc, y[3]) and torch.equal(frames[:nbytes], y[1][:nbytes])     # cache == JPEG source
            for u, v in zip((spec, label, idx), (y[0], y[4], y[5])):
                assert torch.equal(u, v)
            for j in range(b):
                i = seen + j
                d = os.path.join(visual, names[i])
                want = decode_jpeg(os.path.join(d, pick_middle_frame(d)))     # the middle frame, as it comes
                off, H, W = (int(v) for v in desc[j, :3])
                assert (H, W) == want.shape[:2] and np.array_equal(frames[off:off + H * W * 3].numpy().reshape(H, W, 3), want)
                assert desc[j, 3:].tolist() == [0, 0, H, W, 0] + list(resize_center_crop(H, W, 32))
                assert torch.equal(spec[j], torch.from_numpy(np.load(os.path.join(audio, names[i] + ".npy"))))     # raw: normalised on the device
                assert int(fdesc[j, 7]) == fbank_stream_id(4, 0, i)
            assert bool((fdesc[:, 0] == int(train and augnois)).all())
            if not (train and augnois):
                assert bool((fdesc[:, :7] == 0).all())
            seen += b
    assert len(list(CAVBatcher(names, labels, 2, audio, frame_cache=cache, drop_last=True, pin=False))) == 2
    assert len(CAVBatcher(names, labels, 2, audio, frame_cache=cache, drop_last=True, pin=False)) == 2
    with pytest.raises(ValueError):
        CAVBatcher(names, labels, 2, audio)


def test_cav_batches_do_not_depend_on_threads_or_batching(tmp_path):
    from mla_hip import CAVBatcher
    names, audio, visual = _write_dataset(str(tmp_path), 4, [(40, 64)])
    rows = lambda fb: torch.cat([b[3].clone() for b in fb])
    kw = dict(visual_feature_path=visual, augnois=True, seed=9, pin=False)
    a = rows(CAVBatcher(names, [0] * 4, 4, audio, threads=1, **kw))
    b = rows(CAVBatcher(names, [0] * 4, 3, audio, threads=4, **kw))
    assert torch.equal(a, b)
    fb = CAVBatcher(names, [0] * 4, 4, audio, **kw)
    fb.set_epoch(1)
    c = rows(fb)
    assert not torch.equal(c[:, :7], a[:, :7]) and not torch.equal(c[:, 7], a[:, 7])
