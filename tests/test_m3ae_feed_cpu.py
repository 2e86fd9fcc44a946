"""CPU: the M3AE batch feed's host side (mla_hip.m3ae_feed) -- Pillow's ImageEnhance restated in numpy (tests/jitter_model.py) and
pinned bit for bit to live PIL and to the Pillow-made fixture, torchvision's ColorJitter draws, descriptor packing, the launch
checks of mla_image_augment_check, and M3AEBatcher's host tuples."""
import itertools
import os

import numpy as np
import pytest
import torch

import jitter_model as J
from mla_hip import M3AEBatcher, MLAHipError, decode_images, jitter_descriptors, ops, sample_generator, sample_jitter

OUT = 40


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "m3ae_feed_small.npz")))


def _frame(fx, d):
    off, H, W = int(d[0]), int(d[1]), int(d[2])
    return fx["frames"][off:off + H * W * 3].reshape(H, W, 3)


def test_numpy_model_matches_the_pillow_fixture(fixture):
    assert fixture["desc"].shape[1] == 12 and fixture["jit"].shape[1] == 7 and fixture["out"].shape[1:] == (OUT, OUT, 3)
    for d, j, want, label in zip(fixture["desc"], fixture["jit"], fixture["out"], fixture["labels"]):
        assert np.array_equal(J.augment_np(_frame(fixture, d), d, j, OUT, OUT), want), label


def test_fixture_covers_the_cases(fixture):
    jit = fixture["jit"]
    orders = {tuple(r[1:4]) for r in jit if r[0] == 3}
    assert orders == set(itertools.permutations((0, 1, 2)))
    assert {tuple(r[1:2]) for r in jit if r[0] == 1} == {(0,), (1,), (2,)} and any(r[0] == 0 for r in jit)
    factors = np.concatenate([np.asarray(r[4 + r[1]:5 + r[1]]) for r in jit if r[0] == 1]).astype(np.uint32).view(np.float32)
    assert {0.0, 1.0, 2.0} <= set(factors.tolist()) and any(0 < f < 1 for f in factors) and any(1 < f < 2 for f in factors)
    d = fixture["desc"]
    assert bool((d[:, 7] == 1).any()) and bool((d[:, 7] == 0).any())
    assert bool(((d[:, 5] == 5) & (d[:, 6] == 7)).any()) and bool(((d[:, 5] == OUT) & (d[:, 6] == OUT)).any()) and bool((d[:, 5] > OUT).any())
    # identity-size crops pass through the bicubic resize unchanged
    for r, j, label in zip(d, jit, fixture["labels"]):
        if r[5] == OUT and r[6] == OUT and j[0] == 0:
            f = _frame(fixture, r)[r[3]:r[3] + OUT, r[4]:r[4] + OUT]
            assert np.array_equal(J.augment_np(_frame(fixture, r), r, j, OUT, OUT), f[:, ::-1] if r[7] else f), label
    half = [i for i, l in enumerate(fixture["labels"]) if str(l).startswith("halfgrey")]
    assert len(half) == 3
    f = _frame(fixture, d[half[0]])
    S, n = int(J.luma(f).sum()), OUT * OUT
    assert 2 * S % (2 * n) == n and J.contrast_mean(f) == S // n + 1              # the mean is exactly k + 0.5 and rounds up


def test_numpy_model_matches_live_pil():
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    imgs = [rng.integers(0, 256, size=(23, 31, 3), dtype=np.uint8), np.full((8, 9, 3), 255, np.uint8), np.zeros((5, 5, 3), np.uint8),
            (rng.integers(0, 2, size=(16, 16, 3)) * 255).astype(np.uint8), np.broadcast_to(np.array([7, 250, 99], np.uint8), (6, 4, 3)).copy()]
    for img in imgs:
        for order in [p for k in range(4) for p in itertools.permutations((0, 1, 2), k)]:
            for fac in ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), (0.5, 1.5, 0.25), tuple(float(np.float32(v)) for v in rng.uniform(0, 2, 3))):
                assert np.array_equal(J.jitter_np(img, order, fac), J.jitter_pil(img, order, fac)), (img.shape, order, fac)
    # with the crop, the resize and the flip in front
    frame = rng.integers(0, 256, size=(70, 55, 3), dtype=np.uint8)
    d = (0, 70, 55, 4, 6, 50, 44, 1, OUT, OUT, 0, 0)
    j = jitter_descriptors([((2, 1, 0), (1.4, 0.6, 1.9))])[0]
    assert np.array_equal(J.augment_np(frame, d, j, OUT, OUT), J.augment_pil(frame, d, j, OUT, OUT))


def test_sample_jitter_orders_factors_and_determinism():
    n = 3000
    counts, lo, hi = {}, 2.0, 0.0
    for i in range(n):
        order, fac = sample_jitter(sample_generator(11, 0, i))
        assert sorted(order) == [0, 1, 2] and len(fac) == 3
        assert all(0.0 <= f <= 2.0 and float(np.float32(f)) == f for f in fac)                # fp32 values in [0, 2]
        counts[order] = counts.get(order, 0) + 1
        lo, hi = min(lo, *fac), max(hi, *fac)
    # 6 orders, each Binomial(3000, 1/6): mean 500, sd 20.4; 5 sd
    assert len(counts) == 6 and all(abs(c - n / 6) < 5 * (n * (1 / 6) * (5 / 6)) ** 0.5 for c in counts.values()), counts
    assert lo < 0.05 and hi > 1.95
    a = sample_jitter(sample_generator(5, 2, 17))
    assert a == sample_jitter(sample_generator(5, 2, 17))
    assert a != sample_jitter(sample_generator(5, 3, 17)) and a != sample_jitter(sample_generator(5, 2, 18)) \
        and a != sample_jitter(sample_generator(6, 2, 17))


def test_sample_jitter_is_torchvisions_draw_sequence_and_drops_zero_strengths():
    g, h = sample_generator(1, 2, 3), sample_generator(1, 2, 3)
    order, fac = sample_jitter(g, 0.4, 1.0, 0.2)
    perm = torch.randperm(4, generator=h).tolist()
    b = torch.empty(1).uniform_(0.6, 1.4, generator=h).item()
    c = torch.empty(1).uniform_(0.0, 2.0, generator=h).item()
    s = torch.empty(1).uniform_(0.8, 1.2, generator=h).item()
    assert order == tuple(p for p in perm if p != 3) and fac == (b, c, s)
    assert torch.equal(torch.rand(1, generator=g), torch.rand(1, generator=h))              # nothing else was drawn
    for i in range(50):
        order, fac = sample_jitter(sample_generator(0, 0, i), 1.0, 0.0, 1.0)
        assert sorted(order) == [0, 2] and fac[1] == 1.0
        assert sample_jitter(sample_generator(0, 0, i), 0.0, 0.0, 0.0) == ((), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        sample_jitter(sample_generator(0, 0, 0), -1.0)


def test_jitter_descriptor_packing():
    d = jitter_descriptors([((2, 0, 1), (0.5, 2.0, 0.25)), ((1,), (1.0, 1.5, 1.0)), ((), (1.0, 1.0, 1.0))])
    assert d.dtype == np.int64 and d.tolist() == [[3, 2, 0, 1, 0x3F000000, 0x40000000, 0x3E800000],
                                                   [1, 1, -1, -1, 0x3F800000, 0x3FC00000, 0x3F800000],
                                                   [0, -1, -1, -1, 0x3F800000, 0x3F800000, 0x3F800000]]
    assert J.unpack_jitter(d[0]) == ((2, 0, 1), (0.5, 2.0, 0.25))


def _ok_tables():
    from mla_hip import image_descriptors
    shapes = [(40, 50), (60, 70), (30, 30)]
    boxes = [(0, 0, 40, 50, 0), (1, 2, 50, 50, 1), (0, 0, 30, 30, 0)]
    desc, total = image_descriptors(shapes, boxes, [(OUT, OUT, 0, 0)] * 3)
    jit = jitter_descriptors([((0, 1, 2), (0.5, 1.5, 2.0)), ((1,), (1.0, 0.0, 1.0)), ((), (1.0, 1.0, 1.0))])
    return torch.from_numpy(desc), torch.from_numpy(jit), total


def test_image_augment_check_accepts_and_refuses_jitter_and_buffers():
    ok, jit, total = _ok_tables()
    ops.image_augment_check(ok, jit, total, OUT, OUT)
    ops.image_augment_check(ok, jit, total, OUT, OUT, 3 * OUT * OUT * 3, 3 * 3)               # exactly enough: three 16-row bands per image

    def bad(col, val, match, row=0, **kw):
        j = jit.clone()
        if col is not None:
            j[row, col] = val
        with pytest.raises(MLAHipError, match=match):
            ops.image_augment_check(ok, j, total, OUT, OUT, **kw)
    nan, neg, inf = (int(np.float32(v).view(np.uint32)) for v in (np.nan, -0.5, np.inf))
    bad(2, 0, "repeated")                         # brightness twice
    bad(3, 1, "repeated")
    bad(1, 3, "unknown operation")                # hue is not built
    bad(2, -1, "unknown operation")
    bad(0, 4, "operations")
    bad(0, -1, "operations")
    for col in (4, 5, 6):
        bad(col, nan, "finite")
        bad(col, neg, "finite")
        bad(col, inf, "finite")
        bad(col, 1 << 32, "bit pattern")
        bad(col, -1, "bit pattern")
    bad(6, nan, "finite", row=2)                  # factors are checked even where no operation uses them
    bad(None, None, "staging", staging_bytes=3 * OUT * OUT * 3 - 1)
    bad(None, None, "partials", partials_count=3 * 3 - 1)
    j = jit.clone()
    j[1, 1:4] = torch.tensor([1, 7, 7])           # slots beyond n_ops are ignored
    ops.image_augment_check(ok, j, total, OUT, OUT)
    with pytest.raises(MLAHipError, match="jitter descriptors"):
        ops.image_augment_check(ok, jit[:2].contiguous(), total, OUT, OUT)
    with pytest.raises(MLAHipError, match=r"\(N, 7\)"):
        ops.image_augment_check(ok, jit[:, :6].contiguous(), total, OUT, OUT)
    with pytest.raises(MLAHipError, match="int64"):
        ops.image_augment_check(ok, jit.int(), total, OUT, OUT)


def test_image_augment_check_refuses_what_image_check_refuses():
    ok, jit, total = _ok_tables()

    def bad(col, val, match, nbytes=total, oh=OUT, ow=OUT):
        d = ok.clone()
        if col is not None:
            d[0, col] = val
        with pytest.raises(MLAHipError, match=match):
            ops.image_augment_check(d, jit, nbytes, oh, ow)
    bad(10, 1, "window")
    bad(11, 5, "window")
    bad(10, -1, "window")
    bad(11, -1, "window")
    bad(None, None, "window", oh=OUT + 1)
    bad(8, 0, "resized size")
    bad(9, -4, "resized size")
    bad(5, 0, "empty crop")
    bad(6, 0, "empty crop")
    bad(1, 0, "out of range")
    bad(3, 1, "leaves")
    bad(7, 2, "flip")
    bad(0, total, "outside")
    bad(None, None, "outside", nbytes=total - 1)
    bad(None, None, "out of range", oh=0)
    one = torch.tensor([[0, 60000, 8, 0, 0, 60000, 8, 0, 2, 8, 0, 0]])
    with pytest.raises(MLAHipError, match="LDS"):
        ops.image_augment_check(one, jit[:1].contiguous(), 60000 * 8 * 3, 2, 8)
    with pytest.raises(MLAHipError, match="int64"):
        ops.image_augment_check(ok.int(), jit, total, OUT, OUT)
    with pytest.raises(MLAHipError, match=r"\(N, 12\)"):
        ops.image_augment_check(ok[:, :8].contiguous(), jit, total, OUT, OUT)
    # a large downscale halves the band: more partial sums per image than out_h / 16
    from mla_hip import image_descriptors
    big, n = image_descriptors([(1080, 1920)], [(0, 0, 1080, 1920, 0)], [(224, 224, 0, 0)])
    ops.image_augment_check(torch.from_numpy(big), jit[:1].contiguous(), n, 224, 224)
    with pytest.raises(MLAHipError, match="partials"):
        ops.image_augment_check(torch.from_numpy(big), jit[:1].contiguous(), n, 224, 224, partials_count=14)


def test_image_augment_refuses_overlapping_buffers_before_any_launch():
    """The C entry point validates before it launches: with overlapping buffers it returns the error without touching them."""
    import ctypes
    from mla_hip import _lib
    lib = _lib.load()
    ok, jit, total = _ok_tables()
    d, j = ok.numpy(), jit.numpy()
    dp, jp = d.ctypes.data_as(ctypes.c_void_p), j.ctypes.data_as(ctypes.c_void_p)
    out_bytes, st_bytes, out = 3 * 3 * OUT * OUT * 4, 3 * OUT * OUT * 3, 0x100000
    call = lambda staging, partials: lib.mla_image_augment(0x1000, total, 0x1000, dp, 0x1000, jp, 0x1000, out, staging, st_bytes, partials, 9,
                                                           3, OUT, OUT, None)
    for staging, partials in ((out + out_bytes - 1, 0x800000), (0x800000, out - 9 * 8 + 8), (0x800000, 0x800000 + st_bytes - 8)):
        assert call(staging, partials) == -1
        assert b"overlap" in lib.mla_last_error()
    assert call(0x800000, 0x900004) == -1 and b"aligned" in lib.mla_last_error()
    assert lib.mla_image_augment(0x1000, total, 0x1000, dp, 0x1000, jp, 0x1000, out, None, st_bytes, 0x900000, 9, 3, OUT, OUT, None) == -1
    assert b"null" in lib.mla_last_error()


def _write_dataset(root, n_samples, sizes, seed=0):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(seed)
    text, visual = os.path.join(root, "text"), os.path.join(root, "visual")
    os.makedirs(text)
    os.makedirs(visual)
    names = [f"img{i}" for i in range(n_samples)]
    for i, name in enumerate(names):
        n_tok = 5 + 3 * i
        token = np.zeros((1, 256), dtype=np.int64)
        token[0, :n_tok] = rng.integers(1, 64, n_tok)
        pm = np.ones((1, 256), dtype=np.float32)
        pm[0, :n_tok] = 0.0
        np.save(os.path.join(text, name + "_token.npy"), token)
        np.save(os.path.join(text, name + "_pm.npy"), pm)
        H, W = sizes[i % len(sizes)]
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.stack([(xx * 3 + i * 40) % 256, (yy * 2 + i * 30) % 256, (xx + yy + i * 17) % 256], -1).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(visual, name + ".jpg"), quality=90)
    return names, text, visual


def _clone(fb):
    out = []
    for b in fb:
        nbytes = int(b[3][-1, 0] + b[3][-1, 1] * b[3][-1, 2] * 3)
        out.append(tuple(t[:nbytes].clone() if k == 2 else t.clone() for k, t in enumerate(b)))
    fb.close()
    return out


def test_m3ae_batcher_host_tuples_do_not_depend_on_threads_or_source(tmp_path):
    from mla_hip import resize_center_crop, sample_crop, sample_flip
    from mla_hip.frames import decode_jpeg
    names, text, visual = _write_dataset(str(tmp_path), 5, [(60, 80), (72, 50)])
    cache = str(tmp_path / "cache")
    assert decode_images(visual, cache, names, threads=3) == 5
    labels = [4, 3, 2, 1, 0]
    for train in (True, False):
        kw = dict(train=train, seed=4, pin=False, out_size=32)
        a = _clone(M3AEBatcher(names, labels, 2, text, visual_feature_path=visual, threads=1, **kw))
        b = _clone(M3AEBatcher(names, labels, 2, text, visual_feature_path=visual, threads=4, ring=2, **kw))
        c = _clone(M3AEBatcher(names, labels, 2, text, frame_cache=cache, threads=1, **kw))
        assert len(a) == len(b) == len(c) == 3
        for x, y, z in zip(a, b, c):
            assert len(x) == 7 and all(torch.equal(u, v) and torch.equal(u, w) for u, v, w in zip(x, y, z))
        seen = 0
        for token, pm, frames, desc, jdesc, label, idx in a:
            n = label.shape[0]
            assert n == (2 if seen < 4 else 1)
            assert token.shape == (n, 1, 256) and token.dtype == torch.int64 and pm.shape == (n, 1, 256) and pm.dtype == torch.float32
            assert desc.shape == (n, 12) and jdesc.shape == (n, 7) and idx[:, 0].tolist() == list(range(seen, seen + n))
            assert label.tolist() == labels[seen:seen + n]
            for j in range(n):
                i = seen + j
                want = decode_jpeg(os.path.join(visual, names[i] + ".jpg"))
                off, H, W = (int(v) for v in desc[j, :3])
                assert (H, W) == want.shape[:2] and np.array_equal(frames[off:off + H * W * 3].numpy().reshape(H, W, 3), want)
                assert np.array_equal(token[j].numpy(), np.load(os.path.join(text, names[i] + "_token.npy")))
                assert np.array_equal(pm[j].numpy(), np.load(os.path.join(text, names[i] + "_pm.npy")))
                if train:                                   # crop, flip, jitter, in that order on the sample's generator
                    g = sample_generator(4, 0, i)
                    box = sample_crop(H, W, g)
                    flip = int(sample_flip(g))
                    assert desc[j, 3:].tolist() == list(box) + [flip, 32, 32, 0, 0]
                    assert np.array_equal(jdesc[j].numpy(), jitter_descriptors([sample_jitter(g)])[0])
                else:
                    assert desc[j, 3:].tolist() == [0, 0, H, W, 0] + list(resize_center_crop(H, W, 32))
                    assert jdesc[j].tolist() == [0, -1, -1, -1] + [0x3F800000] * 3
            ops.image_augment_check(desc.clone(), jdesc.clone(), frames.numel(), 32, 32)
            seen += n
    fb = M3AEBatcher(names, labels, 2, text, frame_cache=cache, seed=4, pin=False, out_size=32)
    e0 = _clone(fb)
    fb.set_epoch(1)
    e1 = _clone(fb)
    assert not torch.equal(e1[0][4], e0[0][4]) and not torch.equal(e1[0][3], e0[0][3])          # set_epoch reseeds the draws
    assert len(M3AEBatcher(names, labels, 2, text, frame_cache=cache, drop_last=True, pin=False)) == 2
    nojit = _clone(M3AEBatcher(names, labels, 5, text, frame_cache=cache, color_jitter=(1.0, 0.0, 0.0), seed=4, pin=False, out_size=32))
    assert nojit[0][4][:, 0].tolist() == [1] * 5 and nojit[0][4][:, 1].tolist() == [0] * 5
    with pytest.raises(ValueError):
        M3AEBatcher(names, labels, 2, text)
    with pytest.raises(ValueError):
        M3AEBatcher(names, labels, 2, text, frame_cache=cache, color_jitter=(1.0, 1.0))
