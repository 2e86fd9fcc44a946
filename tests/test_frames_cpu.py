"""CPU: the CREMA-D frame pipeline's host side (mla_hip.frames) -- Pillow's 8-bit bilinear resample restated in numpy and
pinned bit for bit to PIL, the normalisation LUT, the RandomResizedCrop / RandomHorizontalFlip restatement, the reference's
frame choice, descriptor packing and the launch checks of mla_frames_check, and the decoded-frame cache."""
import math
import os

import numpy as np
import pytest
import torch

PRECISION = 22


def _coeffs(inp, out):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc (bilinear, box = the whole input)."""
    scale = inp / out
    fs = max(scale, 1.0)
    support, ss = fs, 1.0 / fs
    res = []
    for xx in range(out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), inp) - xmin
        ws = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for w in ws:
            ww += w
        res.append((xmin, np.array([int(0.5 + (w / ww) * (1 << PRECISION)) for w in ws], dtype=np.int64)))
    return res


def _pass(img, coeffs, axis):
    """one separable pass over `axis` (0 = rows, 1 = columns) of an (H, W, 3) uint8 image, uint8 result"""
    src = img.astype(np.int64)
    outs = []
    for xmin, k in coeffs:
        sl = src[xmin:xmin + len(k)] if axis == 0 else src[:, xmin:xmin + len(k)]
        acc = (1 << (PRECISION - 1)) + np.tensordot(k, sl, axes=([0], [axis]))
        outs.append(np.clip(acc >> PRECISION, 0, 255).astype(np.uint8))
    return np.stack(outs, axis=axis)


def resample_np(frame, top, left, h, w, flip, OH, OW):
    """PIL crop((left, top, left+w, top+h)).resize((OW, OH), BILINEAR) [.transpose(FLIP_LEFT_RIGHT)] in numpy."""
    crop = frame[top:top + h, left:left + w]
    res = _pass(_pass(crop, _coeffs(w, OW), 1), _coeffs(h, OH), 0)       # horizontal first, uint8 clip in between
    return res[:, ::-1] if flip else res


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "frames_small.npz")))


def _frame(fx, d):
    off, H, W = int(d[0]), int(d[1]), int(d[2])
    return fx["frames"][off:off + H * W * 3].reshape(H, W, 3)


def test_numpy_resample_matches_the_pil_fixture(fixture):
    for g in ("g64", "g224"):
        desc, want = fixture[f"desc_{g}"], fixture[f"out_{g}"]
        OH, OW = want.shape[1:3]
        for d, ref in zip(desc, want):
            got = resample_np(_frame(fixture, d), *[int(v) for v in d[3:]], OH, OW)
            assert np.array_equal(got, ref), (g, d)


def test_numpy_resample_matches_live_pil_on_random_boxes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    for trial in range(12):
        H, W = int(rng.integers(8, 400)), int(rng.integers(8, 400))
        frame = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        OH, OW = (224, 224) if trial % 2 else (int(rng.integers(1, 300)), int(rng.integers(1, 300)))
        flip = trial % 3 == 0
        im = Image.fromarray(frame).crop((left, top, left + w, top + h)).resize((OW, OH), Image.BILINEAR)
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        assert np.array_equal(resample_np(frame, top, left, h, w, flip, OH, OW), np.asarray(im)), (H, W, top, left, h, w, OH, OW)


def test_lut_equals_totensor_normalize_torch_ops():
    from mla_hip.frames import MEAN, STD, make_lut
    lut = make_lut()
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    img = torch.arange(256, dtype=torch.uint8).reshape(16, 16, 1).expand(16, 16, 3).contiguous()
    t = img.permute(2, 0, 1).contiguous().to(dtype=torch.float32).div(255)                   # ToTensor
    t = t.sub_(torch.as_tensor(MEAN)[:, None, None]).div_(torch.as_tensor(STD)[:, None, None])   # Normalize
    for c in range(3):
        assert torch.equal(lut[c], t[c].reshape(256)), c


def test_sampler_invariants_and_fallback():
    from mla_hip.frames import sample_crop, sample_flip, sample_generator
    g = torch.Generator().manual_seed(0)
    central = 0
    for _ in range(2000):
        H, W = int(torch.randint(1, 600, (1,), generator=g)), int(torch.randint(1, 600, (1,), generator=g))
        top, left, h, w = sample_crop(H, W, g)
        assert 0 <= top and 0 <= left and 0 < h and 0 < w and top + h <= H and left + w <= W
        if (top, left) == ((H - h) // 2, (W - w) // 2) and (h == H or w == W):
            central += 1                                               # possibly the fallback: no range guarantee
            continue
        frac, ratio = h * w / (H * W), w / h
        # rounding of w and h to integers moves area and ratio slightly off the sampled values
        assert 0.08 * (1 - 2 / min(h, w)) - 1e-9 <= frac <= 1.0 + 1e-9
        assert 3 / 4 * (1 - 1 / h) / (1 + 1 / w) <= ratio <= 4 / 3 * (1 + 1 / w) / (1 - 1 / h) if h > 1 else True
    assert central < 2000
    assert sample_crop(1, 1000, g) == (0, 499, 1, 1)                   # too wide: h = H, w = round(H * 4/3)
    assert sample_crop(1000, 1, g) == (499, 0, 1, 1)                   # too tall: w = W, h = round(W / (3/4))
    a = sample_generator(5, 2, 17)
    b = sample_generator(5, 2, 17)
    draws_a = [sample_crop(360, 480, a) + (sample_flip(a),) for _ in range(5)]
    draws_b = [sample_crop(360, 480, b) + (sample_flip(b),) for _ in range(5)]
    assert draws_a == draws_b
    c = sample_generator(5, 3, 17)
    assert [sample_crop(360, 480, c) + (sample_flip(c),) for _ in range(5)] != draws_a
    g = torch.Generator().manual_seed(1)
    rate = sum(sample_flip(g) for _ in range(10000)) / 10000
    assert abs(rate - 0.5) < 0.02


def test_sampler_matches_torchvision_algorithm_statistics():
    """Area fraction drawn from U(0.08, 1) and log-ratio from U(log 3/4, log 4/3) on a big square frame: boxes that do not fit
    (large area at an extreme ratio) are redrawn, which lowers the mean area below 0.54 and keeps the log-ratio symmetric."""
    from mla_hip.frames import sample_crop
    g = torch.Generator().manual_seed(7)
    fr, lr = [], []
    for _ in range(4000):
        top, left, h, w = sample_crop(2000, 2000, g)
        fr.append(h * w / 4e6)
        lr.append(math.log(w / h))
    assert 0.44 < np.mean(fr) < 0.52 and abs(np.mean(lr)) < 0.01
    assert min(fr) > 0.079 and max(fr) <= 1.0 and min(lr) > math.log(3 / 4) - 0.01 and max(lr) < math.log(4 / 3) + 0.01


def test_eval_mode_takes_the_whole_frame_without_draws():
    from mla_hip.frames import sample_augment
    assert sample_augment([(360, 480), (10, 20)], None, False) == [(0, 0, 360, 480, 0), (0, 0, 10, 20, 0)]


def test_frame_choice_follows_listdir(tmp_path, monkeypatch):
    from mla_hip import MLAHipError
    from mla_hip.frames import pick_frames
    for n, want in ((1, [0, 0, 0]), (2, [0, 0, 0]), (3, [0, 1, 2]), (7, [0, 2, 4])):
        d = tmp_path / f"s{n}"
        d.mkdir()
        names = [f"f{i:03d}.jpg" for i in range(n)]
        for f in names:
            (d / f).write_bytes(b"")
        listing = list(reversed(names))                 # any listdir order is used as it comes: not sorted
        monkeypatch.setattr(os, "listdir", lambda p, _l=listing: list(_l))
        assert pick_frames(str(d)) == [listing[i] for i in want], n
        monkeypatch.undo()
    (tmp_path / "empty").mkdir()
    with pytest.raises(MLAHipError, match="no frames"):
        pick_frames(str(tmp_path / "empty"))


def test_descriptor_packing_and_launch_checks():
    from mla_hip import MLAHipError, ops
    from mla_hip.frames import frame_descriptors
    shapes = [(4, 5), (6, 7), (3, 3)]
    boxes = [(0, 0, 4, 5, 0), (1, 2, 5, 5, 1), (0, 0, 3, 3, 0)]
    desc, total = frame_descriptors(shapes, boxes)
    assert desc.dtype == np.int64 and desc.shape == (3, 8) and total == (20 + 42 + 9) * 3
    assert desc.tolist() == [[0, 4, 5, 0, 0, 4, 5, 0], [60, 6, 7, 1, 2, 5, 5, 1], [186, 3, 3, 0, 0, 3, 3, 0]]
    ok = torch.from_numpy(desc)
    ops.frames_check(ok, 3, 1, total)
    ops.frames_check(ok, 1, 3, total, 224, 224)

    def bad(col, val, match, B=3, T=1, nbytes=total):
        d = ok.clone()
        if col is not None:
            d[1, col] = val
        with pytest.raises(MLAHipError, match=match):
            ops.frames_check(d, B, T, nbytes)
    bad(3, 2, "leaves")                      # top + h > H
    bad(4, 3, "leaves")                      # left + w > W
    bad(3, -1, "leaves")
    bad(5, 0, "empty crop")
    bad(6, 0, "empty crop")
    bad(1, 0, "out of range")
    bad(2, -3, "out of range")
    bad(7, 2, "flip")
    bad(0, total, "outside")                 # offset + H*W*3 past the buffer
    bad(None, None, "outside", nbytes=total - 1)
    bad(None, None, "B\\*T", B=2, T=1)       # N != B*T
    with pytest.raises(MLAHipError, match="outside"):
        ops.frames_check(ok, 3, 1, total - 1)
    with pytest.raises(MLAHipError, match="LDS"):                     # a 60000-row crop squeezed into 2 output rows
        ops.frames_check(torch.tensor([[0, 60000, 8, 0, 0, 60000, 8, 0]]), 1, 1, 60000 * 8 * 3, 2, 8)
    with pytest.raises(MLAHipError, match="int64"):
        ops.frames_check(ok.int(), 3, 1, total)


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
        for f in range(4 + i % 3):
            yy, xx = np.mgrid[0:H, 0:W]
            img = np.stack([(xx * 3 + f * 20) % 256, (yy * 2 + i * 30) % 256, (xx + yy) % 256], -1).astype(np.uint8)
            img = np.clip(img.astype(np.int16) + rng.integers(-20, 20, size=img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, f"frame_{f:05d}.jpg"), quality=90)
    return names, audio, visual


def test_cache_and_jpeg_sources_give_identical_batches(tmp_path):
    from mla_hip import FrameBatcher, decode_frames
    from mla_hip.frames import load_cached_frame
    names, audio, visual = _write_dataset(str(tmp_path), 5, [(60, 80), (72, 50)])
    cache = str(tmp_path / "cache")
    assert decode_frames(visual, cache, names, threads=3) == 15
    labels = list(range(5))
    for train in (True, False):
        a = list(FrameBatcher(names, labels, 2, audio, visual_feature_path=visual, train=train, seed=4, threads=3, pin=False))
        b = list(FrameBatcher(names, labels, 2, audio, frame_cache=cache, train=train, seed=4, threads=1, pin=False))
        assert len(a) == len(b) == 3
        for x, y in zip(a, b):
            spec, frames, desc, label, idx = x
            assert spec.shape[0] == label.shape[0] == idx.shape[0] and desc.shape == (3 * label.shape[0], 8)
            nbytes = int(desc[-1, 0] + desc[-1, 1] * desc[-1, 2] * 3)
            assert torch.equal(desc, y[2]) and torch.equal(frames[:nbytes], y[1][:nbytes])
            for u, v in zip((spec, label, idx), (y[0], y[3], y[4])):
                assert torch.equal(u, v)
        if not train:
            assert all((x[2][:, 3:5] == 0).all() and (x[2][:, 7] == 0).all() for x in a)
    np.save(os.path.join(cache, names[0], "1.npy"), np.zeros((4, 4), np.uint8))
    from mla_hip import MLAHipError
    with pytest.raises(MLAHipError, match="1.npy"):
        load_cached_frame(cache, names[0], 1)


def test_batches_do_not_depend_on_threads_or_batching(tmp_path):
    """The draws are a function of (seed, epoch, index): thread count and batch boundaries do not move them; epochs do."""
    from mla_hip import FrameBatcher
    names, audio, visual = _write_dataset(str(tmp_path), 4, [(40, 64)])
    rows = lambda fb: torch.cat([b[2][:, 3:] for b in fb])
    a = rows(FrameBatcher(names, [0] * 4, 4, audio, visual_feature_path=visual, seed=9, threads=1, pin=False))
    b = rows(FrameBatcher(names, [0] * 4, 3, audio, visual_feature_path=visual, seed=9, threads=4, pin=False))
    assert torch.equal(a, b)
    fb = FrameBatcher(names, [0] * 4, 4, audio, visual_feature_path=visual, seed=9, pin=False)
    fb.set_epoch(1)
    assert not torch.equal(rows(fb), a)
