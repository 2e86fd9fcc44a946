"""GPU: mla_wav_fbank (csrc/wav_fbank.hip).  Exact structure (floor, frame counts, cut, zero rows), independence of neighbours,
offset and batch size, accuracy against the fp64 restatement of torchaudio 0.8.1's kaldi.fbank (tests/fbank_model.py) element by
element under the FFT's error model, and the three batchers and extract_fbank through the .wav path."""
import math
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fbank_model as M  # noqa: E402
from mla_hip import CAVBatcher, DeviceFeeder, FrameBatcher, Modal3Batcher, extract_fbank, ops, wav_feed  # noqa: E402
from mla_hip.cav_feed import NORM_MEAN, NORM_STD, fbank_descriptors  # noqa: E402

LOG_EPS = float(np.float32(math.log(2.0 ** -23)))          # log(eps), correctly rounded to fp32
KERNEL_FACTOR = 4.0                                      # the kernel may need 4 times the constant of the fp32 CPU restatement
NEAR_FLOOR_SHARE = 0.01
# share of the elements above the floor whose tolerance at the kernel's constant is below 1e-3, over the six signals together.
# 0.99 does not hold for this bound: measured 0.93 (noise 1.000, tone on noise 0.952, chirp on noise 0.696, quiet noise 1.000,
# burst 1.000, full scale 1.000): the chirp puts most of a frame's energy into a few banks while delta scales with the whole
# frame, so its quiet banks get a wide tolerance.  The shares follow c, which depends on the host's FFT; with the chirp's at 0.1
# the share would still be 0.81 (the burst has few elements above the floor and hardly counts).
BITE_SHARE = 0.8


def run(clips, target_length=8, pad_front=0):
    """ops.wav_fbank on int16 clips packed back to back behind `pad_front` samples of garbage, into a NaN-poisoned buffer."""
    desc, total = wav_feed.clip_descriptors(clips)
    desc[:, 0] += pad_front
    wav = np.full(total + pad_front, 12345, dtype=np.int16)
    for d, c in zip(desc, clips):
        if c is not None:
            wav[d[0]:d[0] + d[1]] = c
    desc_host = torch.from_numpy(desc)
    out = torch.full((len(clips), target_length, 128), float("nan"), device="cuda")
    ops.wav_fbank(torch.from_numpy(wav).cuda(), desc_host.cuda(), desc_host, wav_feed.device_tables("cuda"), out)
    torch.cuda.synchronize()
    return out.cpu()


def noise(n, seed):
    return np.random.default_rng(seed).integers(-20000, 20000, n).astype(np.int16)


def is_plus_zero(t):
    return bool((t.view(torch.int32) == 0).all())


# ---- 1. exact structure ----------------------------------------------------------------------------------------------------------
def test_zero_and_constant_clips_sit_exactly_on_the_floor():
    n = 400 + 160 * 4
    out = run([np.zeros(n, np.int16), np.full(n, 1234, np.int16)])
    assert (out[:, :5] == LOG_EPS).all() and not torch.isnan(out).any()
    assert is_plus_zero(out[:, 5:])


def test_frame_counts_and_the_cut():
    lengths = (400, 559, 560, 400 + 160 * 7, 400 + 160 * 8)
    clips = [noise(n, i) for i, n in enumerate(lengths)]
    out = run(clips)
    for b, (n, rows) in enumerate(zip(lengths, (1, 1, 2, 8, 8))):
        assert M.num_frames(n) >= rows and not torch.isnan(out[b]).any()
        assert (out[b, :rows].abs().sum(dim=1) > 0).all() and is_plus_zero(out[b, rows:]), (n, rows)
    longer = run(clips[4:], target_length=16)
    assert torch.equal(out[4], longer[0, :8]) and (longer[0, 8].abs().sum() > 0) and is_plus_zero(longer[0, 9:])


def test_absent_clip_is_plus_zero():
    out = run([noise(560, 0), None, noise(400, 1)])
    assert is_plus_zero(out[1]) and (out[0, :2].abs().sum(dim=1) > 0).all() and (out[2, 0].abs().sum() > 0)
    assert is_plus_zero(run([None], target_length=5))


def test_one_second_at_the_training_length():
    out = run([noise(16000, 3)], target_length=1024)
    assert not torch.isnan(out).any() and (out[0, :98].abs().sum(dim=1) > 0).all() and is_plus_zero(out[0, 98:])


# ---- 2. independence and determinism ----------------------------------------------------------------------------------------------
def test_a_clip_depends_on_nothing_but_itself():
    clip, a, b = noise(400 + 160 * 9 + 77, 5), noise(559, 6), noise(1001, 7)          # 10 frames: more than one workgroup at 12 rows
    alone = run([clip], target_length=12)
    assert not torch.isnan(alone).any() and is_plus_zero(alone[0, 10:])
    assert torch.equal(run([clip], target_length=12), alone)                          # two runs, the same bits
    assert torch.equal(run([clip], target_length=12, pad_front=1), alone)             # odd offset
    assert torch.equal(run([clip], target_length=12, pad_front=2), alone)             # even offset
    assert torch.equal(run([clip, a, b], target_length=12)[0:1], alone)
    assert torch.equal(run([a, clip, b], target_length=12)[1:2], alone)               # behind 559 samples: odd offset again
    assert torch.equal(run([a, None, clip], target_length=12)[2:3], alone)
    import mla_hip  # noqa: F401  registers torch.ops.mla_hip
    desc = torch.tensor([[0, clip.shape[0], int(clip.sum(dtype=np.int64)), 0]])
    assert torch.equal(torch.ops.mla_hip.wav_fbank(torch.from_numpy(clip).cuda(), desc, 12).cpu(), alone)


# ---- 3. accuracy against fp64 under the FFT's error model -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy():
    """Per signal: the fp64 reference with the terms of its bound, the constant c the fp32 CPU restatement needs (measured here, on
    these inputs), and the kernel's output.  One launch for the six signals."""
    sig = M.signals()
    out = run(list(sig.values()), target_length=M.num_frames(2 * M.SAMPLE_RATE)).numpy()
    nonempty = M.mel_banks(np.float64).sum(axis=1) > 0
    res = {}
    for k, (name, s) in enumerate(sig.items()):
        ref, x, absX, E = M.fbank(s, np.float64, parts=True)
        terms = M.tolerance_terms(x, absX, E)
        c_cpu = M.smallest_c(M.error(M.fbank(s, np.float32), ref, E), terms)
        res[name] = dict(ref=ref, E=E, terms=terms, c_cpu=c_cpu, out=out[k], nonempty=nonempty,
                         torchaudio=M.fbank(s, np.float32, torchaudio_weights=True))
    return res


SIGNALS = ["noise", "tone440_on_noise", "chirp_on_noise", "quiet_noise", "burst", "full_scale"]


@pytest.mark.parametrize("name", SIGNALS)
def test_accuracy_against_fp64_element_by_element(accuracy, name):
    """|out - ref| <= tol element by element, tol = (2 d sum_k w_k |X_k| + d^2 sum_k w_k) / max(E, eps) + 4u |log max(E, eps)| + 300u
    with d = c * 9u * |x|_2 and c = 4 times the smallest c the fp32 CPU restatement needs on the same signal.  Where the fp64
    energy is within a factor 2 of eps either side of the floor is accepted.
    The kernel and the fp32 restatement both carry the fp64 mel weights rounded once (with torchaudio's fp32 weights, 1.4e-5 off,
    the restatement would need c = 7 to 400, which says nothing about an FFT).  Measured c of the fp32 CPU restatement / of the
    kernel, on the MI355X host: noise 0.468 / 0.290, tone on noise 0.851 / 0.613, chirp on noise 1.481 / 1.015, quiet noise
    0.517 / 0.229, burst 0.579 / 0.097, full scale 0.486 / 0.397.  Worst error / tol: 0.12 to 0.29.
    The restatement's c is that of the host's fp32 FFT (torch.fft.rfft on the CPU) and so depends on the host, by up to a factor 2
    where it was seen; the kernel's does not.  A signal whose restatement the flat part alone covers has c = 0 and holds the kernel
    to the flat part alone; none of the six does where this was measured (smallest c 0.27)."""
    r = accuracy[name]
    err = M.error(r["out"], r["ref"], r["E"])
    c_kernel = M.smallest_c(err, r["terms"])
    tol = M.tolerance(r["terms"], KERNEL_FACTOR * r["c_cpu"])
    print(f"{name}: c of the fp32 CPU restatement {r['c_cpu']:.4g}, c of the kernel {c_kernel:.4g}, max error {err.max():.3g}, "
          f"median error {np.median(err):.3g}, worst error / tol {np.max(err / tol):.3g}")
    loud = r["E"] >= 1e-6 * r["E"].max(axis=1, keepdims=True)                          # where fp32 itself is accurate
    away = np.abs(r["out"].astype(np.float64) - r["torchaudio"])[loud & (r["E"] >= 4.0 * M.EPS)]
    print(f"{name}: from the fp32 restatement with torchaudio's own fp32 mel weights, elements within 60 dB of the frame's largest: "
          f"max {away.max():.3g}, median {np.median(away):.3g}")
    assert 0 <= r["c_cpu"] < math.inf                                                  # 0: the flat part alone covers the restatement
    assert not np.isnan(r["out"]).any()
    assert (err <= tol).all(), (c_kernel, r["c_cpu"])
    empty = ~r["nonempty"]
    assert (r["out"][:, empty] == LOG_EPS).all()                                       # a bank without bins: exactly the floor


@pytest.mark.parametrize("name", SIGNALS)
def test_few_elements_are_near_the_floor(accuracy, name):
    """Under 1 % of a signal's non-empty-bank elements may take the either-side-of-the-floor rule of the accuracy test."""
    r = accuracy[name]
    share = M.near_floor(r["E"])[:, r["nonempty"]].mean()
    print(f"{name}: {share:.4f} of the non-empty-bank elements within a factor 2 of eps")
    assert share < NEAR_FLOOR_SHARE


def test_the_bound_bites(accuracy):
    below = total = 0
    for name, r in accuracy.items():
        above = r["E"] >= 2.0 * M.EPS
        tol = M.tolerance(r["terms"], KERNEL_FACTOR * r["c_cpu"])
        print(f"{name}: {np.mean(tol[above] < 1e-3):.4f} of the elements above the floor have tol < 1e-3")
        below += int((tol[above] < 1e-3).sum())
        total += int(above.sum())
    assert below / total >= BITE_SHARE


# ---- 4. through the feed ----------------------------------------------------------------------------------------------------------
def _write_wav(path, samples):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(samples.tobytes())


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """Three clips (1 frame, 23 frames, 2 s) as .wav, a synthetic frame cache and token files; the clips' filterbanks through
    ops.wav_fbank, the .npy files extract_fbank writes from the .wav files."""
    root = str(tmp_path_factory.mktemp("wav_feed"))
    wav, cache, text, npy = (os.path.join(root, d) for d in ("wav", "cache", "text", "npy"))
    for d in (wav, cache, text):
        os.makedirs(d)
    names = ["a", "b", "c"]
    clips = [noise(n, 10 + i) for i, n in enumerate((559, 4001, 32000))]
    rng = np.random.default_rng(0)
    for name, clip in zip(names, clips):
        _write_wav(os.path.join(wav, name + ".wav"), clip)
        os.makedirs(os.path.join(cache, name))
        for t in range(3):
            np.save(os.path.join(cache, name, f"{t}.npy"), rng.integers(0, 256, (20, 24, 3)).astype(np.uint8))
        np.save(os.path.join(text, name + "_token.npy"), rng.integers(1, 64, (1, 256)).astype(np.int64))
        np.save(os.path.join(text, name + "_pm.npy"), np.zeros((1, 256), np.float32))
    spec = wav_feed.wav_fbank(clips, 1024, "cuda")
    assert extract_fbank(wav, npy, names, batch_size=2) == 3
    return dict(names=names, wav=wav, cache=cache, text=text, npy=npy, spec=spec)


def _batches(batcher):
    out = [tuple(t.clone() for t in batch) for batch in DeviceFeeder(batcher)]
    torch.cuda.synchronize()
    batcher.close()
    return out


def test_frame_batcher_wav_path_equals_the_op_and_the_npy_path(dataset):
    d = dataset
    kw = dict(frame_cache=d["cache"], train=False, threads=2, out_size=16)
    (w1, w2), (n1, n2) = (_batches(FrameBatcher(d["names"], [0, 1, 2], 2, **src, **kw))
                          for src in ({"audio_wav_path": d["wav"]}, {"audio_feature_path": d["npy"]}))
    assert torch.equal(torch.cat([w1[0], w2[0]]), d["spec"]) and w1[0].shape == (2, 1024, 128)
    assert torch.equal(torch.cat([n1[0], n2[0]]), d["spec"])                           # extract_fbank's files hold the same bits
    for a, b in zip(w1 + w2, n1 + n2):
        assert torch.equal(a, b)
    assert is_plus_zero(d["spec"][0, 1:].cpu()) and is_plus_zero(d["spec"][2, 198:].cpu())


def test_cav_batcher_wav_path_normalises_the_op_result(dataset):
    d = dataset
    (batch,) = _batches(CAVBatcher(d["names"], [0, 1, 2], 3, audio_wav_path=d["wav"], frame_cache=d["cache"], train=False, out_size=16))
    fdesc = torch.from_numpy(fbank_descriptors([None] * 3, [0] * 3))
    want = ops.fbank_augment(d["spec"], torch.empty_like(d["spec"]), fdesc.cuda(), fdesc, NORM_MEAN, NORM_STD, 0)
    assert torch.equal(batch[0], want)
    assert torch.equal(want.cpu(), (d["spec"].cpu() - NORM_MEAN) / NORM_STD)


def test_modal3_batcher_wav_path_zeroes_the_absent_clip(dataset):
    d = dataset
    mask = [[1, 1, 1], [0, 1, 1], [1, 0, 1]]
    os.rename(os.path.join(d["wav"], "b.wav"), os.path.join(d["wav"], "b.away"))       # the absent clip's file is not opened
    try:
        (batch,) = _batches(Modal3Batcher(d["names"], [0, 1, 2], 3, d["text"], audio_wav_path=d["wav"], frame_cache=d["cache"],
                                          train=False, mask=mask, out_size=16))
    finally:
        os.rename(os.path.join(d["wav"], "b.away"), os.path.join(d["wav"], "b.wav"))
    spec = batch[3]
    assert spec.shape == (3, 1024, 128) and is_plus_zero(spec[1].cpu())
    assert torch.equal(spec[0], d["spec"][0]) and torch.equal(spec[2], d["spec"][2])
