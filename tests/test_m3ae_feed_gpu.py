"""GPU: mla_image_augment (csrc/frames.hip) against Pillow's own crop / BICUBIC resize / flip / ImageEnhance results
(tests/golden/m3ae_feed_small.npz, made by make_golden_m3ae_feed.py) and the M3AEBatcher -> DeviceFeeder path into MLATrainer --
everything bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jitter_model as J  # noqa: E402
from mla_hip import M3AEBatcher, decode_images, jitter_descriptors, ops  # noqa: E402
from mla_hip.frames import make_lut  # noqa: E402
from test_m3ae_feed_cpu import _write_dataset  # noqa: E402

OUT, GUARD = 40, 256


def _lut_of(u8_hwc, lut):
    idx = torch.as_tensor(np.ascontiguousarray(u8_hwc)).long().permute(2, 0, 1)
    return torch.stack([lut[c][idx[c]] for c in range(3)])


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _run_guarded(frames_u8, desc, jit, OH, OW, bands):
    """One launch with out, staging and partials of exactly the required size inside guard zones; returns out on the host after
    checking that no guard element changed."""
    N = desc.shape[0]
    dh, jh = torch.as_tensor(np.ascontiguousarray(desc), dtype=torch.int64), torch.as_tensor(np.ascontiguousarray(jit), dtype=torch.int64)
    obuf, out = _guarded(N * 3 * OH * OW, torch.float32, -777.0)
    sbuf, staging = _guarded(N * OH * OW * 3, torch.uint8, 0xA5)
    pbuf, partials = _guarded(N * bands, torch.int64, -0x0123456789ABCDEF)
    ops.image_augment(torch.as_tensor(frames_u8).cuda(), dh.cuda(), dh, jh.cuda(), jh, make_lut().cuda(), out.view(N, 3, 1, OH, OW),
                      staging, partials)
    torch.cuda.synchronize()
    for buf, fill in ((obuf, -777.0), (sbuf, 0xA5), (pbuf, -0x0123456789ABCDEF)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())
    assert not bool((out == -777.0).any())
    return out.view(N, 3, OH, OW).cpu(), staging.cpu(), partials.cpu()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "m3ae_feed_small.npz")))


@pytest.fixture(scope="module")
def golden_run(fixture):
    """Every case of the fixture in one launch: 42 images x three bands (two of 16 rows, one of 8)."""
    return _run_guarded(fixture["frames"], fixture["desc"], fixture["jit"], OUT, OUT, 3)


def test_output_equals_lut_of_pillow_on_every_fixture_case(fixture, golden_run):
    """All 6 orders, each single operation and none, factors 0 / 1 / 2 / (0, 1) / (1, 2), noise / constant / pure 0-255 images,
    downscale / 5 x 7 upscale / identity crops flipped and not, contrast first / middle / last on the high-saturation image, and
    the half-grey image whose mean luma is exactly k + 0.5 (see make_golden_m3ae_feed.py)."""
    out, _, _ = golden_run
    lut = make_lut()
    bad = [str(label) for n, label in enumerate(fixture["labels"]) if not torch.equal(out[n], _lut_of(fixture["out"][n], lut))]
    assert not bad, bad


def test_staging_holds_the_image_before_contrast_and_partials_its_luma_sums(fixture, golden_run):
    _, staging, partials = golden_run
    staging, partials = staging.numpy().reshape(-1, OUT, OUT, 3), partials.numpy().reshape(-1, 3)
    for n, (d, j) in enumerate(zip(fixture["desc"], fixture["jit"])):
        off, H, W = int(d[0]), int(d[1]), int(d[2])
        order, fac = J.unpack_jitter(j)
        pre = order[:order.index(J.CONTRAST)] if J.CONTRAST in order else order
        jpre = jitter_descriptors([(pre, fac)])[0]
        want = J.augment_np(fixture["frames"][off:off + H * W * 3].reshape(H, W, 3), d, jpre, OUT, OUT)
        assert np.array_equal(staging[n], want), fixture["labels"][n]
        L = J.luma(want)
        assert partials[n].tolist() == [int(L[0:16].sum()), int(L[16:32].sum()), int(L[32:40].sum())], fixture["labels"][n]


def test_rerun_is_bit_identical(fixture, golden_run):
    again = _run_guarded(fixture["frames"], fixture["desc"], fixture["jit"], OUT, OUT, 3)
    for a, b in zip(golden_run, again):
        assert torch.equal(a, b)


def test_sizes_off_the_tile_and_more_than_one_block_vs_numpy_model():
    """33 x 47 outputs (odd, a short last band, a pixel count that is no multiple of the 256-thread block) and a 256 x 256 output
    (the training size: 16 bands, 256 blocks per image in the second launch), mixed source sizes in one launch."""
    from mla_hip import image_descriptors
    rng = np.random.default_rng(5)
    for (OH, OW), shapes in (((33, 47), [(50, 70), (20, 20), (64, 31)]), ((256, 256), [(300, 280), (97, 131)])):
        frames = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in shapes]
        boxes = [(1, 2, H - 3, W - 4, n % 2) for n, (H, W) in enumerate(shapes)]
        desc, nbytes = image_descriptors(shapes, boxes, [(OH, OW, 0, 0)] * len(shapes))
        jit = jitter_descriptors([((2, 1, 0), (1.7, 0.3, 1.1)), ((0, 1), (0.6, 1.9, 1.0)), ((1, 2, 0), (1.2, 1.4, 0.2))][:len(shapes)])
        out, _, _ = _run_guarded(np.concatenate([f.reshape(-1) for f in frames]), desc, jit, OH, OW, (OH + 15) // 16)
        lut = make_lut()
        for n, f in enumerate(frames):
            assert torch.equal(out[n], _lut_of(J.augment_np(f, desc[n], jit[n], OH, OW), lut)), (OH, OW, n)


def test_torch_op_matches_the_launcher(fixture, golden_run):
    import mla_hip  # noqa: F401  registers torch.ops.mla_hip
    got = torch.ops.mla_hip.image_augment(torch.from_numpy(fixture["frames"]).cuda(), torch.from_numpy(fixture["desc"]),
                                          torch.from_numpy(fixture["jit"]), make_lut().cuda(), OUT, OUT)
    assert got.shape == (fixture["desc"].shape[0], 3, 1, OUT, OUT) and torch.equal(got[:, :, 0].cpu(), golden_run[0])
    with pytest.raises(NotImplementedError):                        # no CPU implementation is registered
        torch.ops.mla_hip.image_augment(torch.from_numpy(fixture["frames"]), torch.from_numpy(fixture["desc"]),
                                        torch.from_numpy(fixture["jit"]), make_lut(), OUT, OUT)


def test_eval_batcher_equals_cav_batcher_at_256(tmp_path):
    """train=False: the image equals CAVBatcher(out_size=256, train=False)'s for the same decoded file, bit for bit."""
    from mla_hip import CAVBatcher, DeviceFeeder
    names, text, visual = _write_dataset(str(tmp_path), 3, [(300, 400), (500, 350), (256, 256)])
    cache, audio = str(tmp_path / "cache"), str(tmp_path / "audio")
    decode_images(visual, cache, names)
    os.makedirs(audio)
    for name in names:
        np.save(os.path.join(audio, name + ".npy"), np.zeros((1024, 128), dtype=np.float32))
    labels = [0, 1, 2]
    cav = CAVBatcher(names, labels, 2, audio, frame_cache=cache, train=False, out_size=256, pin=True)
    want = [image.cpu() for _, image, _, _ in DeviceFeeder(cav, depth=3)]
    cav.close()
    for source in ({"frame_cache": cache}, {"visual_feature_path": visual}):
        fb = M3AEBatcher(names, labels, 2, text, train=False, pin=True, **source)
        got = [(token.cpu(), image.cpu(), label.cpu()) for token, pm, image, label, idx in DeviceFeeder(fb, depth=3)]
        fb.close()
        assert [g[1].shape for g in got] == [(2, 3, 256, 256), (1, 3, 256, 256)]
        assert all(torch.equal(g[1], w) for g, w in zip(got, want)), source
        assert torch.cat([g[2] for g in got]).tolist() == labels
        assert np.array_equal(got[0][0][1].numpy(), np.load(os.path.join(text, names[1] + "_token.npy")))


def _trainer():
    from mla_hip import M3AEClassifier, MLATrainer

    class Args:
        fusion_method, dataset, gs_flag, modulation = "concat", "Food101", True, "Normal"
    tr = MLATrainer(M3AEClassifier(Args(), depth=2, text_vocab_size=1000, seed=0))        # the reduced model of test_m3ae_gpu.py
    tr.keep_debug = False
    return tr


def test_m3ae_batcher_through_device_feeder_into_the_trainer(tmp_path):
    """Train batcher, pinned ring of 2, feeder depth 3: every fed image equals lut[Pillow's transform] of the batcher's own host
    descriptors, and two MLA steps on the fed batches give exactly the losses of the same steps fed from the CPU-built batch."""
    pytest.importorskip("PIL")
    from mla_hip import DeviceFeeder
    names, text, visual = _write_dataset(str(tmp_path), 4, [(90, 120), (150, 100), (72, 96)])
    labels = [i % 101 for i in (3, 50, 100, 7)]
    kw = dict(visual_feature_path=visual, train=True, seed=3, threads=4, ring=2, pin=True)
    lut, cpu = make_lut(), []
    fb = M3AEBatcher(names, labels, 2, text, **kw)
    for token, pm, frames, desc, jdesc, label, idx in fb:
        imgs = []
        for d, j in zip(desc.numpy(), jdesc.numpy()):
            off, H, W = int(d[0]), int(d[1]), int(d[2])
            imgs.append(_lut_of(J.augment_pil(frames[off:off + H * W * 3].numpy().reshape(H, W, 3), d, j, 256, 256), lut))
        assert bool((jdesc[:, 0] == 3).all())
        cpu.append((token.clone(), pm.clone(), torch.stack(imgs), label.clone(), idx.clone()))
    fb.close()
    assert len(cpu) == 2
    ref, want = _trainer(), []
    for s, (token, pm, image, label, idx) in enumerate(cpu):
        want.append(ref.train_step(token.cuda(), pm.cuda(), image.cuda(), label.cuda(), s, 3))
    ref.join()
    torch.cuda.synchronize()
    fb = M3AEBatcher(names, labels, 2, text, **kw)
    tr, got = _trainer(), []
    for s, batch in enumerate(DeviceFeeder(fb, depth=3)):
        token, pm, image, label, idx = batch
        assert image.shape == (2, 3, 256, 256) and image.dtype == torch.float32 and token.dtype == torch.int64
        for a, b in zip(batch, cpu[s]):
            assert torch.equal(a.cpu(), b), s
        got.append(tr.train_step(token, pm, image, label, s, 3))
    tr.join()
    torch.cuda.synchronize()
    fb.close()
    assert len(got) == 2
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in g:
            assert torch.isfinite(g[k]).all() and torch.equal(g[k], w[k]), (k, g[k], w[k])
