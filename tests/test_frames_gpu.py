"""GPU: the CREMA-D frame augmentation kernel (csrc/frames.hip) against PIL + torchvision's ToTensor/Normalize, bit for bit,
and the FrameBatcher -> DeviceFeeder path into MLATrainer."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(frames_u8, desc, B, T, OH, OW, lut=None):
    from mla_hip import ops
    from mla_hip.frames import make_lut
    lut = make_lut() if lut is None else lut
    desc_host = torch.as_tensor(np.ascontiguousarray(desc), dtype=torch.int64)
    out = torch.full((B, 3, T, OH, OW), float("nan"), device="cuda")
    ops.frames_resample(torch.as_tensor(frames_u8).cuda(), desc_host.cuda(), desc_host, lut.cuda(), out, T)
    torch.cuda.synchronize()
    return out.cpu()


def _lut_of(u8_hwc, lut):
    """LUT[c][PIL result] as (3, H, W)."""
    idx = torch.as_tensor(np.ascontiguousarray(u8_hwc)).long().permute(2, 0, 1)
    return torch.stack([lut[c][idx[c]] for c in range(3)])


def _cpu_pipeline(frame, box, OH=224, OW=224):
    """The reference's transform on the host: PIL crop + resize (+ flip), then torch ToTensor and Normalize."""
    from PIL import Image
    from mla_hip.frames import MEAN, STD
    top, left, h, w, flip = box
    im = Image.fromarray(np.ascontiguousarray(frame)).crop((left, top, left + w, top + h)).resize((OW, OH), Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    t = torch.from_numpy(np.array(im, np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(dtype=torch.float32).div(255)
    return t.sub_(torch.as_tensor(MEAN)[:, None, None]).div_(torch.as_tensor(STD)[:, None, None])


def test_kernel_equals_lut_of_pil_on_the_fixture(golden_dir):
    from mla_hip.frames import make_lut
    fx = np.load(os.path.join(golden_dir, "frames_small.npz"))
    lut = make_lut()
    for g in ("g64", "g224"):
        desc, want = fx[f"desc_{g}"], fx[f"out_{g}"]
        N, OH, OW = want.shape[:3]
        out = _run(fx["frames"], desc, N, 1, OH, OW, lut)
        for n in range(N):
            assert torch.equal(out[n, :, 0], _lut_of(want[n], lut)), (g, n, desc[n])


def test_kernel_bitwise_vs_live_pil_mixed_sizes_one_launch():
    pytest.importorskip("PIL")
    from mla_hip.frames import frame_descriptors
    rng = np.random.default_rng(11)
    B, T = 4, 3
    frames, shapes, boxes = [], [], []
    for n in range(B * T):
        H, W = int(rng.integers(16, 500)), int(rng.integers(16, 500))
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        frames.append(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
        shapes.append((H, W))
        boxes.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w, n % 2))
    desc, nbytes = frame_descriptors(shapes, boxes)
    packed = np.concatenate([f.reshape(-1) for f in frames])
    assert packed.size == nbytes
    out = _run(packed, desc, B, T, 224, 224)
    for n in range(B * T):
        assert torch.equal(out[n // T, :, n % T], _cpu_pipeline(frames[n], boxes[n])), (n, shapes[n], boxes[n])


def test_eval_mode_and_output_layout():
    """Resize((224, 224)) boxes (the whole frame, no flip), T = 3 per sample: frame n lands at [n // T, :, n % T]."""
    pytest.importorskip("PIL")
    from mla_hip.frames import frame_descriptors, sample_augment
    rng = np.random.default_rng(5)
    shapes = [(360, 480), (120, 90), (224, 224), (500, 300), (360, 480), (60, 40)]
    frames = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in shapes]
    boxes = sample_augment(shapes, None, train=False)
    desc, _ = frame_descriptors(shapes, boxes)
    out = _run(np.concatenate([f.reshape(-1) for f in frames]), desc, 2, 3, 224, 224)
    assert out.shape == (2, 3, 3, 224, 224) and not torch.isnan(out).any()
    for n in range(6):
        assert torch.equal(out[n // 3, :, n % 3], _cpu_pipeline(frames[n], boxes[n])), n


def test_torch_op_matches_the_launcher():
    import mla_hip  # noqa: F401  registers torch.ops.mla_hip
    from mla_hip.frames import frame_descriptors, make_lut
    rng = np.random.default_rng(2)
    shapes = [(50, 70), (80, 33)]
    frames = np.concatenate([rng.integers(0, 256, size=s + (3,), dtype=np.uint8).reshape(-1) for s in shapes])
    desc, _ = frame_descriptors(shapes, [(3, 4, 40, 50, 1), (0, 0, 80, 33, 0)])
    got = torch.ops.mla_hip.frames_resample(torch.from_numpy(frames).cuda(), torch.from_numpy(desc), make_lut().cuda(), 2, 32, 48)
    assert torch.equal(got.cpu(), _run(frames, desc, 1, 2, 32, 48))


def _dataset(root, n, sizes):
    from PIL import Image
    rng = np.random.default_rng(1)
    audio, visual = os.path.join(root, "audio"), os.path.join(root, "visual")
    os.makedirs(audio)
    names = [f"clip{i}" for i in range(n)]
    for i, name in enumerate(names):
        np.save(os.path.join(audio, name + ".npy"), (rng.standard_normal((1024, 128)) * 4.5 - 5.0).astype(np.float32))
        d = os.path.join(visual, name)
        os.makedirs(d)
        H, W = sizes[i % len(sizes)]
        for f in range(3 + i % 4):
            Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(os.path.join(d, f"{f:04d}.jpg"), quality=85)
    return names, audio, visual


def _cpu_batches(fb):
    """(spec, image, label, idx) per batch made on the CPU from the same frames and the same sampled boxes."""
    out = []
    for b0 in range(0, len(fb.names), fb.B):
        ids = range(b0, min(b0 + fb.B, len(fb.names)))
        imgs, specs = [], []
        for i in ids:
            frames = [np.asarray(f) for f in fb.sample_frames(i)]
            boxes = fb.sample_boxes(i, [f.shape[:2] for f in frames])
            imgs.append(torch.stack([_cpu_pipeline(f, bx) for f, bx in zip(frames, boxes)], 1))       # (3, T, 224, 224)
            specs.append(torch.from_numpy(np.load(os.path.join(fb.audio, fb.names[i] + ".npy"))))
        out.append((torch.stack(specs), torch.stack(imgs), torch.tensor([fb.labels[i] for i in ids]),
                    torch.tensor(list(ids)).view(-1, 1)))
    return out


def test_frame_batcher_through_device_feeder_equals_cpu_pipeline(tmp_path):
    """Pinned ring of 2, feeder depth 3, mixed frame sizes (staging grows), a short last batch: every batch equals, bit for
    bit, the reference's CPU transform with the same boxes; the batch tuple is the reference's (spec, image, label, idx)."""
    pytest.importorskip("PIL")
    from mla_hip import DeviceFeeder, FrameBatcher
    names, audio, visual = _dataset(str(tmp_path), 7, [(90, 120), (150, 200), (72, 96)])
    fb = FrameBatcher(names, [i % 6 for i in range(7)], 2, audio, visual_feature_path=visual, seed=3, threads=4, ring=2, pin=True)
    want = _cpu_batches(fb)
    got = []
    for spec, image, label, idx in DeviceFeeder(fb, depth=3):
        assert image.shape[1:] == (3, 3, 224, 224) and image.dtype == torch.float32 and spec.shape[1:] == (1024, 128)
        got.append((spec.cpu(), image.cpu(), label.cpu(), idx.cpu()))
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert torch.equal(a, b)
    fb.close()


def _model(sd=None):
    from mla_hip import AVClassifier, MLATrainer

    class Args:
        fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", True, "Normal"
    model = AVClassifier(Args(), seed=0)
    if sd is not None:
        model.load_state_dict(sd)
    tr = MLATrainer(model)
    tr.keep_debug = False
    return model, tr


def test_trainer_fed_by_frame_batcher_equals_cpu_fed_steps(tmp_path):
    """MLATrainer fed from FrameBatcher + DeviceFeeder (pinned ring, depth 3, JPEG source and decoded-frame cache, no host
    sync between steps, stream pipeline on) ends bitwise where the serialized trainer fed the CPU-made tensors ends."""
    pytest.importorskip("PIL")
    from mla_hip import DeviceFeeder, FrameBatcher, decode_frames
    names, audio, visual = _dataset(str(tmp_path), 6, [(96, 128)])
    labels = [i % 6 for i in range(6)]
    cache = str(tmp_path / "cache")
    decode_frames(visual, cache, names)
    fb = FrameBatcher(names, labels, 2, audio, visual_feature_path=visual, seed=8, ring=2, pin=True)
    want = _cpu_batches(fb)
    model_s, tr_s = _model()
    sd0 = {k: v.clone() for k, v in model_s.state_dict().items()}
    tr_s.set_overlap(False)
    for s, (spec, image, label, _idx) in enumerate(want):
        tr_s.train_step(spec.cuda(), image.cuda(), label.cuda(), s, len(want))
    torch.cuda.synchronize()
    for source in ({"visual_feature_path": visual}, {"frame_cache": cache}):
        fb = FrameBatcher(names, labels, 2, audio, seed=8, ring=2, pin=True, **source)
        model_f, tr_f = _model(sd0)
        assert tr_f.overlap_forward
        for s, (spec, image, label, _idx) in enumerate(DeviceFeeder(fb, depth=3)):
            tr_f.train_step(spec, image, label, s, len(want))          # no .item(), no synchronize between steps
        tr_f.join()
        torch.cuda.synchronize()
        for a, b in ((model_s.audio_net.flat, model_f.audio_net.flat), (model_s.visual_net.flat, model_f.visual_net.flat),
                     (model_s.fusion_module.fc_out.flat, model_f.fusion_module.fc_out.flat),
                     (tr_s.gs_plugin.Pl, tr_f.gs_plugin.Pl)):
            assert torch.equal(a, b), source
        fb.close()
