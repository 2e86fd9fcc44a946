"""CPU: the host side of the .wav feed (mla_hip/wav_feed.py): the kernel's constant tables against the fp64 restatement of
torchaudio 0.8.1 (tests/fbank_model.py), read_wav, WavPart's packing, the batchers' tuple orders with audio_wav_path, and the
wrapper's refusals through the C ABI (which launch nothing, so they need no GPU)."""
import ctypes
import wave

import numpy as np
import pytest
import torch

import fbank_model as M
from mla_hip import CAVBatcher, FrameBatcher, MLAHipError, Modal3Batcher, _lib, ops, wav_feed


def write_wav(path, samples, rate=16000, channels=1, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.asarray(samples).tobytes())


@pytest.fixture(scope="module")
def tables():
    return wav_feed.fbank_tables()


# ---- fbank_tables() against the fp64 restatement ------------------------------------------------------------------------------
def test_window_within_one_ulp_of_fp64(tables):
    """The window is torch.hann_window(400, periodic=False) evaluated in fp64 and rounded once, against 0.5 - 0.5 cos(2 pi n / 399)
    in fp64.  (torch's fp32 evaluation would miss this: max |w32 - w64| = 1.94e-7, 619 ulp of the value at n = 1, 188 of the 400
    values beyond 1 ulp.)"""
    w32, w64 = tables.window.numpy(), M.window(np.float64)
    assert tables.window.dtype == torch.float32 and w32.shape == (400,)
    ulp = np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64)
    worst = np.max(np.abs(w32.astype(np.float64) - w64) / ulp)
    print("window: max error in ulp", worst, "max abs", np.abs(w32 - w64).max())
    assert worst <= 1.0


def test_mel_weights_within_2_pow_minus_20_of_fp64(tables):
    """The mel matrix (torchaudio's order of operations, evaluated in fp64 and rounded once) against the fp64 restatement.
    (An fp32 evaluation would miss this: max |w32 - w64| = 1.375e-5 at bank 116, bin 195.  The weights are quotients
    (mel - left) / (center - left) of mel values up to 2840, whose fp32 spacing is 2.4e-4, over center - left = 21.8: half a
    spacing in each of the two terms is already 1.1e-5.)"""
    w32, w64 = tables.mel.numpy().astype(np.float64), M.mel_banks(np.float64)
    worst = np.abs(w32 - w64).max()
    print("mel weights: max abs error", worst)
    assert worst <= 2.0 ** -20


def test_sparse_mel_expands_to_the_dense_matrix_bit_for_bit(tables):
    start, length, weight = tables.mel_start_host.numpy(), tables.mel_len_host.numpy(), tables.mel_weight.numpy()
    assert start.dtype == np.int32 and length.dtype == np.int32 and weight.dtype == np.float32
    dense, o = np.zeros((128, 256), np.float32), 0
    for i in range(128):
        dense[i, start[i]:start[i] + length[i]] = weight[o:o + length[i]]
        o += length[i]
    assert o == weight.shape[0]
    assert np.array_equal(dense.view(np.uint32), tables.mel.numpy().view(np.uint32))
    assert (start >= 0).all() and (start + length <= 256).all() and (weight > 0).all()      # one contiguous run of positive weights


def test_empty_banks_equal_the_fp64_models(tables):
    """The lowest banks are narrower than one 31.25 Hz FFT bin, so some cover none."""
    empty64 = np.flatnonzero((M.mel_banks(np.float64) > 0).sum(axis=1) == 0)
    assert empty64.size > 0
    assert np.array_equal(np.flatnonzero(tables.mel_len_host.numpy() == 0), empty64)
    assert np.array_equal(np.flatnonzero((tables.mel.numpy() > 0).sum(axis=1) == 0), empty64)


def test_twiddles_are_fp64_rounded_once(tables):
    j = np.arange(512, dtype=np.float64)
    want = np.stack([np.cos(2 * np.pi * j / 512), -np.sin(2 * np.pi * j / 512)], axis=1).astype(np.float32)
    assert np.array_equal(tables.twiddle.numpy(), want)
    assert tuple(tables.twiddle[0]) == (1.0, 0.0) and tables.twiddle[128, 1] == -1.0 and tables.twiddle[256, 0] == -1.0


def test_distance_to_torchaudios_own_fp32_weights_is_the_weights_relative_error():
    """What the fp64 table costs in parity: the fp32 restatement with the table's weights against the same with torchaudio's own
    fp32 weights w' (what torchaudio returns).  Both weigh the same fp32 power spectrum P, so E' / E = sum w' P / sum w P lies within
    1 -+ r of 1 with r = max_k |w'_k - w_k| / w_k over the bank's bins, and |log E' - log E| <= -log(1 - r); a bank of one bin
    attains it.  fp32 slack: the two dot products (at most 10 terms) and the two logs (1 ulp = 2u |log E| each): 64u + 4u |log E|.
    Measured here: r at most 1.6e-3 (one bank above 1e-3), median 1.5e-5; the distance at most 4.9e-5 to 2.2e-4 by signal, median
    2.9e-6.  Banks whose fp32 run of bins differs from the table's would have no such bound; there were none."""
    w = M.mel_banks(np.float64).astype(np.float32).astype(np.float64)
    wt = M.mel_banks(np.float32).astype(np.float64)
    same = ((w > 0) == (wt > 0)).all(axis=1)
    assert same.sum() >= 120
    r = (np.abs(wt - w) / np.where(w > 0, w, 1.0) * (w > 0)).max(axis=1)
    print("relative weight error by bank: max", r.max(), "median", np.median(r), "banks with another run of bins", (~same).sum())
    assert r[same].max() < 0.01
    for name, s in M.signals().items():
        E = M.fbank(s, np.float64, parts=True)[3]
        ours, theirs = M.fbank(s, np.float32).astype(np.float64), M.fbank(s, np.float32, torchaudio_weights=True).astype(np.float64)
        ok = (E >= 4.0 * M.EPS) & same[None, :]          # clear of the floor in both
        d = np.abs(ours - theirs)
        bound = -np.log1p(-r)[None, :] + 64.0 * M.U + 4.0 * M.U * np.abs(np.log(np.maximum(E, M.EPS)))
        print(f"{name}: distance max {d[ok].max():.3g}, median {np.median(d[ok]):.3g}, worst distance / bound {(d / bound)[ok].max():.3g}")
        assert (d <= bound)[ok].all()


# ---- read_wav --------------------------------------------------------------------------------------------------------------------
def test_read_wav_round_trips_int16(tmp_path):
    s = np.random.default_rng(0).integers(-32768, 32768, 1601).astype(np.int16)
    s[:2] = (-32768, 32767)
    write_wav(tmp_path / "a.wav", s)
    got = wav_feed.read_wav(str(tmp_path / "a.wav"))
    assert got.dtype == np.int16 and np.array_equal(got, s)


def test_read_wav_refuses_other_formats(tmp_path):
    s = np.zeros(800, np.int16)
    write_wav(tmp_path / "r8k.wav", s, rate=8000)
    write_wav(tmp_path / "stereo.wav", s, channels=2)
    write_wav(tmp_path / "u8.wav", np.zeros(800, np.uint8), width=1)
    (tmp_path / "junk.wav").write_bytes(b"not a wav file")
    for name, text in (("r8k", "8000 Hz"), ("stereo", "2 channel"), ("u8", "8-bit"), ("junk", "cannot read"), ("missing", "cannot read")):
        with pytest.raises(MLAHipError, match=text):
            wav_feed.read_wav(str(tmp_path / (name + ".wav")))


# ---- WavPart.pack ----------------------------------------------------------------------------------------------------------------
class Ring:
    """What frames.Batcher hands a part: a slot dict and an allocator."""
    def __init__(self, part, B):
        self.st = {k: torch.zeros((B * rows,) + tuple(shape), dtype=dtype) for k, (rows, shape, dtype) in part.tensors.items()}

    @staticmethod
    def empty(shape, dtype):
        return torch.empty(shape, dtype=dtype)


def test_pack_offsets_lengths_and_sums(tmp_path):
    rng = np.random.default_rng(1)
    lengths = (559, 400, 560, 16001)                    # 559 first: every later clip starts at an odd offset
    clips = [rng.integers(-32768, 32768, n).astype(np.int16) for n in lengths]
    for i, c in enumerate(clips):
        write_wav(tmp_path / f"c{i}.wav", c)
    part = wav_feed.WavPart(str(tmp_path))
    recs = [part.load(f"c{i}", None) for i in range(4)]
    ring = Ring(part, 4)
    host = part.pack(ring.st, recs, 4, ring.empty)
    for j, r in enumerate(recs):
        part.fill(ring.st, j, r)
    assert sorted(host) == ["wav", "wdesc"] and host["wav"].dtype == torch.int16 and host["wav"].numel() == 1 << 19
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    want = np.stack([offsets, lengths, [int(c.astype(np.int64).sum()) for c in clips], np.zeros(4)], axis=1).astype(np.int64)
    assert np.array_equal(host["wdesc"].numpy(), want) and offsets[1] % 2 == 1
    buf = host["wav"].numpy()
    for o, c in zip(offsets, clips):
        assert np.array_equal(buf[o:o + c.shape[0]], c)
    ops.wav_fbank_check(host["wdesc"], host["wav"].numel(), wav_feed.fbank_tables(), 1024)     # the wrapper's host checks accept it
    assert [wav_feed.num_frames(n) for n in lengths] == [1, 1, 2, 98]


def test_pack_grows_the_buffer_in_mib_steps(tmp_path):
    part = wav_feed.WavPart(str(tmp_path))
    ring = Ring(part, 2)
    small = wav_feed.Wav(np.ones(400, np.int16), 400, [0])
    big = wav_feed.Wav(np.ones((1 << 19) + 1, np.int16), (1 << 19) + 1, [0])
    assert part.pack(ring.st, [small, None], 2, ring.empty)["wav"].numel() == 1 << 19
    assert part.pack(ring.st, [small, big], 2, ring.empty)["wav"].numel() == 1 << 20
    assert big.offset == [400]
    assert part.pack(ring.st, [small, None], 2, ring.empty)["wav"].numel() == 1 << 20            # never shrinks


def test_present_mask_opens_no_file(tmp_path):
    write_wav(tmp_path / "here.wav", np.arange(-200, 360, dtype=np.int16))
    names = ["gone0", "here", "gone1"]                  # the audio-absent names have no .wav: opening one would raise
    text, cache = tmp_path / "text", tmp_path / "cache"
    text.mkdir()
    (cache / "gone1").mkdir(parents=True)
    np.save(text / "gone0_token.npy", np.ones((1, 256), np.int64))                   # gone0 has text only, gone1 an image only
    np.save(text / "gone0_pm.npy", np.zeros((1, 256), np.float32))
    np.save(cache / "gone1" / "0.npy", np.full((9, 12, 3), 7, np.uint8))
    b = Modal3Batcher(names, [0, 1, 2], 3, str(text), audio_wav_path=str(tmp_path), frame_cache=str(cache),
                      mask=[[0, 0, 1], [1, 0, 0], [0, 1, 0]], train=False, threads=1, pin=False, out_size=8)
    part = b.parts[2]
    assert isinstance(part, wav_feed.WavPart) and list(part.present) == [False, True, False]
    try:
        (batch,) = list(b)                               # the batcher's own loop decides what is loaded
    finally:
        b.close()
    host = dict(zip(b.host_fields, batch))
    assert host["wdesc"].tolist() == [[0, 0, 0, 0], [0, 560, int(np.arange(-200, 360).sum()), 0], [560, 0, 0, 0]]
    assert np.array_equal(host["wav"][:560].numpy(), np.arange(-200, 360, dtype=np.int16))
    with pytest.raises(MLAHipError, match="gone0.wav"):
        part.load("gone0", None)


def test_short_clip_is_refused(tmp_path):
    write_wav(tmp_path / "short.wav", np.zeros(399, np.int16))
    with pytest.raises(MLAHipError, match="399 samples"):
        wav_feed.WavPart(str(tmp_path)).load("short", None)
    with pytest.raises(MLAHipError, match="neither 0 nor >= 400"):
        ops.wav_fbank_check(torch.tensor([[0, 399, 0, 0]]), 1000, wav_feed.fbank_tables())


# ---- batchers --------------------------------------------------------------------------------------------------------------------
BATCHERS = {
    "frames": (FrameBatcher, {}, ("wav", "wdesc", "frames", "desc", "label", "idx"), ("spec", "image", "label", "idx")),
    "cav": (CAVBatcher, {}, ("wav", "wdesc", "frames", "desc", "fdesc", "label", "idx"), ("spec", "image", "label", "idx")),
    "modal3": (Modal3Batcher, {"text_feature_path": "text"}, ("token", "pm", "wav", "wdesc", "frames", "desc", "jdesc", "mdesc", "label", "idx"),
               ("token", "pm", "image", "spec", "label", "idx")),
}


@pytest.mark.parametrize("kind", sorted(BATCHERS))
def test_batcher_field_order_with_audio_wav_path(kind):
    cls, extra, host, device = BATCHERS[kind]
    b = cls(["a"], [0], 1, audio_wav_path="wav", frame_cache="cache", **extra)
    assert b.host_fields == host and b.device_fields == device
    old = cls(["a"], [0], 1, audio_feature_path="npy", frame_cache="cache", **extra)
    assert old.host_fields == tuple("spec" if f == "wav" else f for f in host if f != "wdesc") and old.device_fields == device


@pytest.mark.parametrize("kind", sorted(BATCHERS))
def test_batcher_wants_exactly_one_audio_source(kind):
    cls, extra, _, _ = BATCHERS[kind]
    with pytest.raises(ValueError, match="exactly one of audio_feature_path"):
        cls(["a"], [0], 1, audio_feature_path="npy", audio_wav_path="wav", frame_cache="cache", **extra)
    with pytest.raises(ValueError, match="exactly one of audio_feature_path"):
        cls(["a"], [0], 1, frame_cache="cache", **extra)


# ---- wrapper refusals through the C ABI: none of them launches anything -----------------------------------------------------------
def test_wrapper_refusals_through_the_c_abi(tables):
    lib = _lib.load()
    fake = 0x1000                                       # non-null, 16-byte aligned, never dereferenced: validation fails first
    start, length = tables.mel_start_host, tables.mel_len_host

    def call(desc_rows, wav_samples=2000, out=fake, target_length=8, mel_start=start):
        d = torch.tensor(desc_rows, dtype=torch.int64)
        return lib.mla_wav_fbank(fake, wav_samples, fake, d.data_ptr(), fake, fake, fake, fake, mel_start.data_ptr(), length.data_ptr(), fake,
                                 tables.mel_weight.numel(), out, d.shape[0], target_length, None)

    def refused(rc, text):
        assert rc == -1 and b"mla_wav_fbank" in lib.mla_last_error() and text in lib.mla_last_error(), lib.mla_last_error()
    refused(call([[0, 400, 0, 0], [2001, 0, 0, 0]]), b"leave the buffer")             # an offset past the buffer
    refused(call([[1601, 400, 0, 0]]), b"leave the buffer")
    refused(call([[0, 399, 0, 0]]), b"neither 0 nor >= 400")
    refused(call([[0, 400, 0, 0]], out=fake + 4), b"16-byte aligned")
    refused(call([[0, 400, 0, 0]], target_length=-8), b"target_length > 0")
    refused(call([[0, 400, 0, 0]], target_length=1 << 24), b"fit an int")
    bad = start.clone()
    bad[127] = 250
    refused(call([[0, 400, 0, 0]], mel_start=bad), b"outside [0, 256)")
    assert lib.mla_wav_fbank_check(torch.tensor([[0, 400, 0, 0]]).data_ptr(), 1, 400, 8, start.data_ptr(), length.data_ptr(),
                                   tables.mel_weight.numel()) == 0
    assert ctypes.c_int(lib.mla_abi_version()).value == 3


def test_new_names_are_exported():
    import mla_hip
    from mla_hip import torch_ops
    for name in ("WavPart", "wav_part", "read_wav", "fbank_tables", "extract_fbank"):
        assert hasattr(mla_hip, name)
    assert "wav_fbank" in torch_ops.op_names()
