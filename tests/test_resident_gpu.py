"""GPU: the HBM-resident CREMA-D feed (csrc/resident.hip, mla_hip/resident_feed.py).  The device draw against its restatement
(tests/resident_model.py) row for row, the pixels against the PIL-pinned mla_frames_resample kernel and against live PIL, eval
batches against FrameBatcher + DeviceFeeder, the feed's semantics, its ring, and MLATrainer fed by it.

The dataset is that of tests/test_frames_gpu.py::_dataset: 7 clips of T = 3 frames, sizes (36, 48), (50, 40), (8, 200), (90, 120) mixed,
batch 3 (a short last batch of 1), out_size 40 (bands of 16 + 16 + 8 rows) where the trainer is not involved."""
import os
import wave

import numpy as np
import pytest
import torch

import resident_model as M
from test_frames_gpu import _cpu_pipeline, _dataset, _model

pytestmark = pytest.mark.gpu

OUT, B, SEED = 40, 3, M.GPU_SEED
LABELS = [i % 6 for i in range(M.GPU_N)]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The dataset on disk (JPEGs, decode_frames cache, fbank .npy), its decoded frames, and ONE store shared by the tests."""
    pytest.importorskip("PIL")
    from mla_hip import ResidentStore, decode_frames
    from mla_hip.frames import load_cached_frame
    root = str(tmp_path_factory.mktemp("resident"))
    names, audio, visual = _dataset(root, M.GPU_N, M.GPU_SIZES)
    cache = os.path.join(root, "cache")
    decode_frames(visual, cache, names)
    frames = [[load_cached_frame(cache, n, t) for t in range(M.GPU_T)] for n in names]
    specs = [np.load(os.path.join(audio, n + ".npy")) for n in names]
    store = ResidentStore(names, LABELS, frame_cache=cache, audio_feature_path=audio, staging_bytes=1 << 16)   # several staging rounds
    return dict(names=names, audio=audio, visual=visual, cache=cache, frames=frames, specs=specs, store=store)


def _batcher(data, **kw):
    from mla_hip import ResidentFrameBatcher
    kw = dict(dict(store=data["store"], seed=SEED, out_size=OUT), **kw)
    return ResidentFrameBatcher(data["names"], LABELS, kw.pop("batch_size", B), **kw)


def _epoch(rb, epoch):
    """Every batch of one epoch, read back: (spec, image, label, idx, desc) on the host."""
    rb.set_epoch(epoch)
    out = []
    for spec, image, label, idx in rb:
        out.append(tuple(t.cpu() for t in (spec, image, label, idx, rb.last_desc)))
    return out


@pytest.fixture(scope="module")
def shuffled(data):
    """Epochs 0 and 1 of the shuffled train feed, computed once and shared."""
    rb = _batcher(data, shuffle=True)
    return {e: _epoch(rb, e) for e in M.GPU_EPOCHS}


def test_store_holds_the_dataset(data):
    st = data["store"]
    assert st.frames.dtype == torch.uint8 and st.table.dtype == torch.int64 and tuple(st.table.shape) == (M.GPU_N * M.GPU_T, 3)
    assert torch.equal(st.table.cpu(), st.table_host) and st.labels.cpu().tolist() == LABELS
    assert st.nbytes == st.frames.numel() + st.spec.numel() * 4 + st.table.numel() * 8 + st.labels.numel() * 8
    want = np.concatenate([f.reshape(-1) for fs in data["frames"] for f in fs])
    assert np.array_equal(st.frames.cpu().numpy(), want)
    assert np.array_equal(st.spec.cpu().numpy(), np.stack(data["specs"]))


def test_draws_equal_the_restatement_row_for_row(data, shuffled):
    from mla_hip import epoch_permutation
    table = data["store"].table_host.numpy()
    for e in M.GPU_EPOCHS:
        order = epoch_permutation(M.GPU_N, True, SEED, e).tolist()
        assert [len(b[2]) for b in shuffled[e]] == [3, 3, 1]
        for k, (_spec, _image, _label, idx, desc) in enumerate(shuffled[e]):
            ids = order[k * B:(k + 1) * B]
            assert idx.view(-1).tolist() == ids and tuple(desc.shape) == (len(ids) * M.GPU_T, 8)
            for j, i in enumerate(ids):
                for t in range(M.GPU_T):
                    off, H, W = (int(v) for v in table[i * M.GPU_T + t])
                    assert (H, W) == M.GPU_SIZES[i % 4]
                    assert tuple(desc[j * M.GPU_T + t].tolist()) == M.desc_row(off, H, W, SEED, e, i, t), (e, i, t)


def test_pixels_equal_frames_resample_and_live_pil(data, shuffled):
    from mla_hip import ops
    from mla_hip.frames import make_lut
    st = data["store"]
    lut = make_lut().cuda()
    for e in M.GPU_EPOCHS:
        for _spec, image, _label, idx, desc in shuffled[e]:
            b = idx.shape[0]
            assert not torch.isnan(image).any()
            # the PIL-pinned kernel on the read-back descriptors, over the resident buffer itself
            want = torch.full((b, 3, M.GPU_T, OUT, OUT), float("nan"), device="cuda")
            ops.frames_resample(st.frames, desc.cuda(), desc.contiguous(), lut, want, M.GPU_T)
            assert torch.equal(image, want.cpu())
            # ... and repacked: only this batch's frames, back to back, in another buffer
            packed, rows, off = [], desc.clone(), 0
            for n in range(b * M.GPU_T):
                o, H, W = (int(v) for v in desc[n, :3])
                packed.append(st.frames[o:o + H * W * 3])
                rows[n, 0] = off
                off += H * W * 3
            want.fill_(float("nan"))
            ops.frames_resample(torch.cat(packed), rows.cuda(), rows, lut, want, M.GPU_T)
            assert torch.equal(image, want.cpu())
            # live PIL: crop -> resize(BILINEAR) -> flip -> ToTensor + Normalize
            for j, i in enumerate(idx.view(-1).tolist()):
                for t in range(M.GPU_T):
                    box = tuple(int(v) for v in desc[j * M.GPU_T + t, 3:])
                    assert torch.equal(image[j, :, t], _cpu_pipeline(data["frames"][i][t], box, OUT, OUT)), (e, i, t, box)


def test_eval_equals_frame_batcher_through_device_feeder(data):
    from mla_hip import DeviceFeeder, FrameBatcher
    rb = _batcher(data, train=False)
    assert rb.shuffle is False
    fb = FrameBatcher(data["names"], LABELS, B, data["audio"], frame_cache=data["cache"], train=False, out_size=OUT, threads=1, ring=2)
    n = 0
    for got, want in zip(rb, DeviceFeeder(fb, depth=3)):
        assert len(got) == len(want) == 4
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b)
        d = rb.last_desc.cpu()
        assert torch.equal(d[:, 3:5], torch.zeros_like(d[:, 3:5])) and torch.equal(d[:, 5:7], d[:, 1:3]) and not d[:, 7].any()
        n += 1
    assert n == len(rb) == 3
    fb.close()


def test_feed_semantics(data, shuffled):
    e0, e1 = shuffled[0], shuffled[1]
    for ep in (e0, e1):
        ids = torch.cat([b[3].view(-1) for b in ep]).tolist()
        assert sorted(ids) == list(range(M.GPU_N))                           # every index exactly once per epoch
        for spec, _image, label, idx, _desc in ep:                           # spec / label / idx belong to the drawn index
            assert tuple(idx.shape) == (len(label), 1) and label.dtype == torch.int64
            for j, i in enumerate(idx.view(-1).tolist()):
                assert label[j].item() == LABELS[i] and np.array_equal(spec[j].numpy(), data["specs"][i])
    assert torch.cat([b[3] for b in e0]).tolist() != torch.cat([b[3] for b in e1]).tolist()      # two epochs: another order ...
    by0 = {i: b[1][j] for b in e0 for j, i in enumerate(b[3].view(-1).tolist())}
    by1 = {i: b[1][j] for b in e1 for j, i in enumerate(b[3].view(-1).tolist())}
    assert all(not torch.equal(by0[i], by1[i]) for i in range(M.GPU_N))                          # ... and other crops
    again = _epoch(_batcher(data, shuffle=True), 0)                                              # the same (seed, epoch) reproduces
    assert all(torch.equal(a, b) for x, y in zip(again, e0) for a, b in zip(x, y))
    for kw in (dict(batch_size=4, shuffle=True), dict(shuffle=False), dict(batch_size=4, shuffle=False, drop_last=True)):
        other = _epoch(_batcher(data, **kw), 0)                              # sample i: the same bits under another batch size / order
        assert len(other) == (1 if kw.get("drop_last") else -(-M.GPU_N // kw.get("batch_size", B)))
        for _spec, image, _label, idx, _desc in other:
            for j, i in enumerate(idx.view(-1).tolist()):
                assert torch.equal(image[j], by0[i]), (kw, i)
    other_seed = _epoch(_batcher(data, shuffle=False, seed=SEED + 1), 0)
    assert not torch.equal(other_seed[0][1][0], by0[0])


def test_iterating_before_set_epoch_uses_epoch_0(data, shuffled):
    rb = _batcher(data, shuffle=True)
    first = next(iter(rb))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(first, shuffled[0][0]))


def test_jpeg_source_equals_cache_source(data, shuffled):
    from mla_hip import ResidentStore
    st = ResidentStore(data["names"], LABELS, visual_feature_path=data["visual"], audio_feature_path=data["audio"], threads=4)
    assert torch.equal(st.frames, data["store"].frames) and torch.equal(st.table_host, data["store"].table_host)
    got = _epoch(_batcher(data, store=st, shuffle=True), 1)
    assert all(torch.equal(a, b) for x, y in zip(got, shuffled[1]) for a, b in zip(x, y))


def test_audio_wav_path_gives_the_bits_of_wav_fbank(data, tmp_path):
    from mla_hip import ResidentFrameBatcher, wav_feed
    rng = np.random.default_rng(4)
    clips = [(rng.standard_normal(int(n)) * 3000).astype(np.int16) for n in rng.integers(4000, 30000, size=M.GPU_N)]
    for name, c in zip(data["names"], clips):
        with wave.open(str(tmp_path / (name + ".wav")), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(c.tobytes())
    want = wav_feed.wav_fbank(clips, 1024, "cuda").cpu()
    rb = ResidentFrameBatcher(data["names"], LABELS, B, frame_cache=data["cache"], audio_wav_path=str(tmp_path), shuffle=True, seed=SEED,
                              out_size=OUT)
    assert torch.equal(rb.store.spec.cpu(), want)
    for spec, _image, _label, idx in rb:
        assert torch.equal(spec.cpu(), want[idx.view(-1).cpu()])


def test_ring_keeps_a_batch_until_depth_further_batches(data):
    """depth = 2: a batch's tensors are untouched after one further batch has been yielded, and are refilled by the second."""
    rb = _batcher(data, shuffle=True, depth=2)
    rb.set_epoch(0)
    it = iter(rb)
    first = next(it)
    clones = [t.clone() for t in first]
    second = next(it)
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(first, second))
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(first, clones))
    third = next(it)                                                          # the short batch, into the first slot
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(first, third)) and third[0].shape[0] == 1
    assert not torch.equal(first[3][:1], clones[3][:1])


def test_trainer_fed_by_resident_batcher_equals_serialized_steps_on_clones(tmp_path):
    """MLATrainer with the stream pipeline on, fed by the resident batcher (depth 2) for three steps without host sync, ends bitwise
    where the serialized trainer fed clones of the same batches ends."""
    pytest.importorskip("PIL")
    from mla_hip import ResidentFrameBatcher, decode_frames
    names, audio, visual = _dataset(str(tmp_path), 6, [(96, 128)])
    labels = [i % 6 for i in range(6)]
    cache = str(tmp_path / "cache")
    decode_frames(visual, cache, names)
    rb = ResidentFrameBatcher(names, labels, 2, frame_cache=cache, audio_feature_path=audio, shuffle=True, seed=8, out_size=224, depth=2)
    rb.set_epoch(2)
    want = [tuple(t.clone() for t in batch) for batch in rb]
    assert len(want) == 3
    model_s, tr_s = _model()
    sd0 = {k: v.clone() for k, v in model_s.state_dict().items()}
    tr_s.set_overlap(False)
    for s, (spec, image, label, _idx) in enumerate(want):
        tr_s.train_step(spec, image, label, s, len(want))
    torch.cuda.synchronize()
    model_f, tr_f = _model(sd0)
    assert tr_f.overlap_forward
    for s, (spec, image, label, _idx) in enumerate(rb):
        tr_f.train_step(spec, image, label, s, len(want))                    # no .item(), no synchronize between steps
    tr_f.join()
    torch.cuda.synchronize()
    for a, b in ((model_s.audio_net.flat, model_f.audio_net.flat), (model_s.visual_net.flat, model_f.visual_net.flat),
                 (model_s.fusion_module.fc_out.flat, model_f.fusion_module.fc_out.flat), (tr_s.gs_plugin.Pl, tr_f.gs_plugin.Pl)):
        assert torch.equal(a, b)


def test_torch_op_matches_the_launcher(data, shuffled):
    import mla_hip  # noqa: F401  registers torch.ops.mla_hip
    from mla_hip import epoch_permutation
    from mla_hip.frames import make_lut
    st = data["store"]
    order = epoch_permutation(M.GPU_N, True, SEED, 1).cuda()
    got = torch.ops.mla_hip.resident_batch(st.frames, st.table, st.spec, st.labels, order, M.GPU_T, B, B, SEED, 1, True, make_lut().cuda(), OUT,
                                           OUT)
    assert len(got) == 5 and all(torch.equal(a.cpu(), b) for a, b in zip(got, shuffled[1][1]))
    none = torch.ops.mla_hip.resident_batch(st.frames, st.table, None, st.labels, order, M.GPU_T, B, B, SEED, 1, True, make_lut().cuda(), OUT, OUT)
    assert tuple(none[0].shape) == (0, 1024, 128) and torch.equal(none[1].cpu(), shuffled[1][1][1])
    with pytest.raises(NotImplementedError):
        torch.ops.mla_hip.resident_batch(st.frames.cpu(), st.table.cpu(), None, st.labels.cpu(), order.cpu(), M.GPU_T, 0, B, SEED, 1, True,
                                         make_lut(), OUT, OUT)
