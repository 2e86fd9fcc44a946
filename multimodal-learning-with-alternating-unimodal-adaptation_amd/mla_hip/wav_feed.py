"""16 kHz mono PCM16 .wav files -> the (1024, 128) log-mel filterbank every audio model here takes, on the device.

The reference makes its fbank .npy files offline with torchaudio 0.8.1 (data/extract_fbank.py:8-54, again from
data/preprocess_iemo.py):

    waveform, sr = torchaudio.load(filename);  waveform = waveform - waveform.mean()
    fbank = torchaudio.compliance.kaldi.fbank(waveform, htk_compat=True, sample_frequency=sr, use_energy=False,
                                              window_type='hanning', num_mel_bins=128, dither=0.0, frame_shift=10)
    pad with zeros / cut to 1024 rows

Here the host reads the samples (stdlib `wave`), sums them as integers and packs int16 clips plus one descriptor row per clip;
csrc/wav_fbank.hip's mla_wav_fbank does the rest in one launch behind the batch's copies.  A clip's samples are 2.5 to 5 times
smaller than its fbank (5 s: 160 KB against 512 KB), so the staged and copied bytes per batch go down.

    read_wav        the clip as int16; anything but PCM16 / 1 channel / 16 000 Hz is an error
    fbank_tables    the constants of the kernel: Hann window, sparse mel matrix (torch CPU ops in torchaudio's order of
                    operations), twiddles; each evaluated in fp64 and rounded once
    WavPart         the frames.Part that stands where fbank_part stands: "wav" + "wdesc" on the host, "spec" on the device
    extract_fbank   <out>/<name>.npy for every name: the GPU counterpart of the reference script, as decode_frames is for JPEGs

torchaudio is restated (tests/fbank_model.py holds the restatement the kernel is tested against), as frames.py restates
torchvision.  Out of scope: the mixup branch of wav2fbank (nothing calls it), resampling and other sample rates (all three datasets
are 16 kHz), stereo or float WAV, the log-STFT of data/extract_spec.py (no dataset class reads it), dither.
"""
from __future__ import annotations

import functools
import math
import os
import wave
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import MLAHipError
from .data import FBANK_SHAPE, batch_ids
from .frames import MAX_THREADS, Part, SampleKey, fbank_part, slot_buffer

SAMPLE_RATE = 16000
WINDOW, SHIFT, PADDED = 400, 160, 512            # 25 ms, 10 ms, round_to_power_of_two(400)
NUM_MEL, LOW_FREQ = 128, 20.0


def num_frames(n_samples: int) -> int:
    """Rows kaldi.fbank gives for n_samples with snip_edges=True."""
    return 0 if n_samples < WINDOW else 1 + (n_samples - WINDOW) // SHIFT


def read_wav(path: str) -> np.ndarray:
    """The samples of a mono 16 kHz PCM16 .wav as int16 (n,); torchaudio.load's waveform is this / 32768."""
    try:
        with wave.open(path, "rb") as w:
            fmt = (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getcomptype())
            raw = w.readframes(w.getnframes()) if fmt == (1, 2, SAMPLE_RATE, "NONE") else None
    except (OSError, EOFError, wave.Error) as e:
        raise MLAHipError(f"{path}: cannot read ({e})") from e
    if raw is None:
        raise MLAHipError(f"{path}: expected 1 channel of 16-bit PCM at {SAMPLE_RATE} Hz, found {fmt[0]} channel(s) of {8 * fmt[1]}-bit "
                          f"{fmt[3]} at {fmt[2]} Hz")
    return np.frombuffer(raw, dtype="<i2").astype(np.int16, copy=False)


class FbankTables(NamedTuple):
    """Host constants of mla_wav_fbank.  Bank i weighs the FFT bins [mel_start[i], mel_start[i] + mel_len[i]) with the next
    mel_len[i] entries of mel_weight; `mel` is the dense (128, 256) matrix they were cut from."""
    window: torch.Tensor          # fp32 (400,)
    twiddle: torch.Tensor         # fp32 (512, 2): (cos, -sin)(2 pi j / 512)
    mel: torch.Tensor             # fp32 (128, 256)
    mel_start_host: torch.Tensor  # int32 (128,)
    mel_len_host: torch.Tensor    # int32 (128,)
    mel_weight: torch.Tensor      # fp32 (sum of mel_len,)


class DeviceTables(NamedTuple):
    """FbankTables as ops.wav_fbank takes them: the constants on the device, the mel runs also on the host."""
    window: torch.Tensor
    twiddle: torch.Tensor
    mel_start: torch.Tensor
    mel_len: torch.Tensor
    mel_weight: torch.Tensor
    mel_start_host: torch.Tensor
    mel_len_host: torch.Tensor


def mel_banks() -> torch.Tensor:
    """torchaudio.compliance.kaldi.get_mel_banks(128, 512, 16000.0, 20.0, 0.0, 100.0, -500.0, 1.0) in its order of operations with
    torch CPU tensors, evaluated in fp64 and rounded once: fp32 (128, 256), before the zero Nyquist column is added.  torchaudio
    evaluates it in fp32, where a weight is (mel - left) / (center - left) of mel values up to 2840 (spacing 2.4e-4) over 21.8: that
    is up to 1.4e-5 from the weight it means, and one ulp of the host's fp32 log moves it by 1.1e-5, so two hosts would not agree."""
    num_fft_bins = PADDED / 2
    high_freq = 0.5 * SAMPLE_RATE
    fft_bin_width = SAMPLE_RATE / PADDED
    mel_low_freq = 1127.0 * math.log(1.0 + LOW_FREQ / 700.0)
    mel_high_freq = 1127.0 * math.log(1.0 + high_freq / 700.0)
    mel_freq_delta = (mel_high_freq - mel_low_freq) / (NUM_MEL + 1)
    bin = torch.arange(NUM_MEL, dtype=torch.float64).unsqueeze(1)
    left_mel = mel_low_freq + bin * mel_freq_delta
    center_mel = mel_low_freq + (bin + 1.0) * mel_freq_delta
    right_mel = mel_low_freq + (bin + 2.0) * mel_freq_delta
    mel = (1127.0 * (1.0 + (fft_bin_width * torch.arange(num_fft_bins, dtype=torch.float64)) / 700.0).log()).unsqueeze(0)
    up_slope = (mel - left_mel) / (center_mel - left_mel)
    down_slope = (right_mel - mel) / (right_mel - center_mel)
    return torch.max(torch.zeros(1, dtype=torch.float64), torch.min(up_slope, down_slope)).float()


@functools.lru_cache(maxsize=None)
def fbank_tables() -> FbankTables:
    # torch.hann_window(400, periodic=False) evaluated in fp64 and rounded once: the fp32 evaluation torchaudio gets is up to 1.9e-7
    # (3 ulp of 1, hundreds of ulp of the small values at the ends) away from the window it means, and not symmetric
    window = torch.hann_window(WINDOW, periodic=False, dtype=torch.float64).float()
    mel = mel_banks()
    assert mel.dtype == torch.float32 and tuple(mel.shape) == (NUM_MEL, PADDED // 2)
    start, length, weight = np.zeros(NUM_MEL, np.int32), np.zeros(NUM_MEL, np.int32), []
    for i, row in enumerate(mel.numpy()):
        nz = np.flatnonzero(row)
        if nz.size:                                  # a bank narrower than one FFT bin may cover none: an empty run
            start[i], length[i] = nz[0], nz[-1] - nz[0] + 1
            weight.append(row[nz[0]:nz[-1] + 1])
    angle = 2.0 * np.pi * np.arange(PADDED, dtype=np.float64) / PADDED
    twiddle = np.stack([np.cos(angle), -np.sin(angle)], axis=1).astype(np.float32)
    return FbankTables(window, torch.from_numpy(twiddle), mel, torch.from_numpy(start), torch.from_numpy(length),
                       torch.from_numpy(np.concatenate(weight).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def _device_tables(device: torch.device) -> DeviceTables:
    t = fbank_tables()
    return DeviceTables(t.window.to(device), t.twiddle.to(device), t.mel_start_host.to(device), t.mel_len_host.to(device),
                        t.mel_weight.to(device), t.mel_start_host, t.mel_len_host)


def device_tables(device) -> DeviceTables:
    """fbank_tables() on `device`, copied there once."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    return _device_tables(device)


def clip_descriptors(clips: Sequence[Optional[np.ndarray]]) -> tuple:
    """Pack clips back to back: int64 (B, 4) rows (offset_samples, n_samples, sample_sum, 0) and the total sample count.  A clip of
    None is absent: n_samples = 0, which the kernel turns into zero rows.  The sum is the exact integer sum of the samples."""
    desc = np.zeros((len(clips), 4), dtype=np.int64)
    off = 0
    for b, c in enumerate(clips):
        n = 0 if c is None else int(c.shape[0])
        desc[b] = (off, n, 0 if c is None else int(c.sum(dtype=np.int64)), 0)
        off += n
    return desc, off


def wav_fbank(clips: Sequence[Optional[np.ndarray]], target_length: int = FBANK_SHAPE[0], device="cuda") -> torch.Tensor:
    """fp32 (B, target_length, 128) on `device`: the filterbank of each int16 clip (None: zero rows) through ops.wav_fbank."""
    desc, total = clip_descriptors(clips)
    wav = np.zeros(total, dtype=np.int16)
    for d, c in zip(desc, clips):
        if c is not None:
            wav[d[0]:d[0] + d[1]] = np.asarray(c, dtype=np.int16)
    desc_host = torch.from_numpy(desc)
    out = torch.empty((len(clips), int(target_length), NUM_MEL), dtype=torch.float32, device=device)
    return ops.wav_fbank(torch.from_numpy(wav).to(out.device), desc_host.to(out.device), desc_host, device_tables(out.device), out)


class Wav(NamedTuple):
    samples: np.ndarray                              # int16 (n,)
    total: int                                       # the exact integer sum of the samples
    offset: list                                     # [sample offset in the packed buffer]; WavPart.pack sets it


class WavPart(Part):
    """<path>/<name>.wav as packed int16 samples: "wav" (capacity,), one descriptor row per sample of the batch in "wdesc" (B, 4);
    the device step turns them into "spec", fp32 (B, target_length, 128), in the slot's own buffer.  A sample that `present`
    leaves out gets n_samples = 0 and a zero spectrogram; no file is opened for it."""
    tensors = {"wdesc": (1, (4,), torch.int64)}

    def __init__(self, path: str, present=None, target_length: int = FBANK_SHAPE[0]):
        self.path, self.present, self.target_length = path, present, int(target_length)

    def load(self, name: str, key: SampleKey) -> Wav:
        file = os.path.join(self.path, name + ".wav")
        samples = read_wav(file)
        if samples.shape[0] < WINDOW:
            raise MLAHipError(f"{file}: {samples.shape[0]} samples are less than one {WINDOW}-sample frame")
        return Wav(samples, int(samples.sum(dtype=np.int64)), [0])

    def pack(self, st: dict, recs: Sequence[Optional[Wav]], b: int, empty) -> dict:
        desc, total = clip_descriptors([None if r is None else r.samples for r in recs])
        buf = st.get("wav")
        if buf is None or buf.numel() < total:                             # grows with the largest batch seen, in MiB steps
            cap = max(total, 1, (buf.numel() * 5 // 4) if buf is not None else 0)
            buf = st["wav"] = empty(((2 * cap + (1 << 20) - 1) >> 20) << 19, torch.int16)
        st["wdesc"][:b].numpy()[...] = desc
        for r, d in zip(recs, desc):
            if r is not None:
                r.offset[0] = int(d[0])
        return {"wav": buf, "wdesc": st["wdesc"][:b]}

    def fill(self, st: dict, j: int, rec: Wav) -> None:
        o, n = rec.offset[0], rec.samples.shape[0]
        np.copyto(st["wav"].numpy()[o:o + n], rec.samples)

    def device(self, host: dict, dev: dict, scratch: dict, out: dict, B: int) -> None:
        wdesc = dev["wdesc"]
        buf = slot_buffer(scratch, "wav_spec", wdesc.shape[0], B, (self.target_length, NUM_MEL), torch.float32, wdesc.device)
        out["spec"] = ops.wav_fbank(dev["wav"], wdesc, host["wdesc"], device_tables(wdesc.device), buf)


def wav_part(path: str, present=None) -> WavPart:
    """<path>/<name>.wav -> "spec" fp32 (B, 1024, 128), raw: what frames.fbank_part leaves from <name>.npy."""
    return WavPart(path, present)


def audio_part(audio_feature_path: Optional[str], audio_wav_path: Optional[str], present=None) -> Part:
    """The audio part of a batcher and its host fields: fbank .npy files ("spec") or .wav files ("wav", "wdesc")."""
    if (audio_feature_path is None) == (audio_wav_path is None):
        raise ValueError("give exactly one of audio_feature_path (fbank .npy files) and audio_wav_path (.wav files)")
    return fbank_part(audio_feature_path, present) if audio_wav_path is None else wav_part(audio_wav_path, present)


def audio_fields(fields: Sequence[str], audio_wav_path: Optional[str]) -> tuple:
    """A batcher's host tuple order: with .wav files "wav", "wdesc" stand where "spec" stood."""
    if audio_wav_path is None:
        return tuple(fields)
    return tuple(g for f in fields for g in (("wav", "wdesc") if f == "spec" else (f,)))


def extract_fbank(audio_wav_path: str, out_path: str, names: Sequence[str], batch_size: int = 64, device="cuda") -> int:
    """Write <out_path>/<name>.npy, fp32 (1024, 128), for every <audio_wav_path>/<name>.wav: the files data.load_fbank reads, with
    the bits the .wav path of the batchers gives.  Returns the number of files written."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(out_path, exist_ok=True)
    part = WavPart(audio_wav_path)
    written = 0
    with ThreadPoolExecutor(MAX_THREADS) as pool:
        for ids in batch_ids(len(names), int(batch_size), False):
            recs = list(pool.map(lambda i: part.load(names[i], None), ids))
            spec = wav_fbank([r.samples for r in recs], FBANK_SHAPE[0], device).cpu().numpy()
            for i, row in zip(ids, spec):
                np.save(os.path.join(out_path, names[i] + ".npy"), row)
                written += 1
    return written
