"""torchaudio 0.8.1's compliance/kaldi.py fbank, restated in numpy for the one call the reference makes (data/extract_fbank.py:8-54):

    waveform = waveform - waveform.mean()
    kaldi.fbank(waveform, htk_compat=True, sample_frequency=16000, use_energy=False, window_type='hanning', num_mel_bins=128,
                dither=0.0, frame_shift=10)

with every other argument at its default (frame_length=25, snip_edges, remove_dc_offset, preemphasis 0.97, round_to_power_of_two,
low_freq=20, high_freq=0, no VTLN warp, use_log_fbank, use_power), then padded with zeros or cut to target_length rows.  torchaudio is
not installed where these tests run, so this restatement is the pin, as tests/cav_model.py is for timm.  It runs in fp64 (the
reference of the accuracy test) and in fp32 (the arithmetic torchaudio itself does: elementwise fp32 ops in torchaudio's order, the
FFT through torch on the CPU; the mel weights are the fp64 ones rounded once, see `fbank`), and `tolerance` is the element-wise
bound that the FFT's error model gives.
"""
import math

import numpy as np
import torch

SAMPLE_RATE, WINDOW, SHIFT, PADDED, NUM_MEL = 16000, 400, 160, 512, 128
LOW_FREQ, PREEMPHASIS = 20.0, 0.97
EPS = float(np.finfo(np.float32).eps)                  # torch.finfo(torch.float).eps = 2^-23
U = 2.0 ** -24                                         # fp32 unit roundoff


def num_frames(n):
    return 0 if n < WINDOW else 1 + (n - WINDOW) // SHIFT


def window(dtype):
    """torch.hann_window(400, periodic=False)."""
    if dtype == np.float32:
        return torch.hann_window(WINDOW, periodic=False, dtype=torch.float32).numpy()
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WINDOW, dtype=np.float64) / (WINDOW - 1))


def mel_banks(dtype):
    """get_mel_banks(128, 512, 16000, 20, 0, 100, -500, 1.0): (128, 256).  In fp64 it is written out in closed form in numpy, on its
    own, so that the tables of mla_hip.wav_feed are not compared with a copy of their code.  In fp32 it follows torchaudio line by
    line (the scalars Python doubles, the arrays torch CPU tensors): a weight is (mel - left) / (center - left) with mel values up to 2840
    (spacing 2.4e-4) over center - left = 21.8, so one ulp of the fp32 log, which numpy and torch do not round alike, moves a weight
    by 1.1e-5.  The kernel's table is the fp64 one rounded once, and `fbank` uses that in fp32 too; the fp32 matrix here is what
    torchaudio itself gets, kept for comparison."""
    if dtype != np.float32:
        # fp64, in closed form and in numpy: bank i is the triangle over the mel points e[i], e[i+1], e[i+2] of 130 equally spaced
        # ones from mel(20 Hz) to mel(8000 Hz), evaluated at the mel value of each FFT bin's frequency
        mel_of = lambda hz: 1127.0 * np.log1p(np.asarray(hz, dtype=np.float64) / 700.0)
        e = np.linspace(mel_of(LOW_FREQ), mel_of(SAMPLE_RATE / 2), NUM_MEL + 2)
        m = mel_of(np.arange(PADDED // 2) * (SAMPLE_RATE / PADDED))[None, :]
        lo, mid, hi = e[:-2, None], e[1:-1, None], e[2:, None]
        return np.clip(np.minimum((m - lo) / (mid - lo), (hi - m) / (hi - mid)), 0.0, None)
    high_freq = 0.5 * SAMPLE_RATE
    fft_bin_width = SAMPLE_RATE / PADDED
    mel_low = 1127.0 * math.log(1.0 + LOW_FREQ / 700.0)
    mel_high = 1127.0 * math.log(1.0 + high_freq / 700.0)
    delta = (mel_high - mel_low) / (NUM_MEL + 1)
    t = torch.float32
    bin = torch.arange(NUM_MEL, dtype=t).unsqueeze(1)
    left = mel_low + bin * delta
    center = mel_low + (bin + 1.0) * delta
    right = mel_low + (bin + 2.0) * delta
    mel = (1127.0 * (1.0 + (fft_bin_width * torch.arange(PADDED // 2, dtype=t)) / 700.0).log()).unsqueeze(0)
    up = (mel - left) / (center - left)
    down = (right - mel) / (right - center)
    return torch.max(torch.zeros(1, dtype=t), torch.min(up, down)).numpy()


def frames(samples, dtype=np.float64):
    """The windowed, zero-padded frames (m, 512) of an int16 clip: _get_window."""
    f = dtype
    x = np.asarray(samples, dtype=np.int16).astype(f) / f(32768.0)          # torchaudio.load
    x = x - x.mean(dtype=f)
    m = num_frames(x.shape[0])
    fr = np.stack([x[r * SHIFT:r * SHIFT + WINDOW] for r in range(m)]) if m else np.zeros((0, WINDOW), f)
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=f)                        # remove_dc_offset
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)                   # replicate padding on the left
    fr = fr - f(PREEMPHASIS) * prev
    fr = fr * window(f)[None, :]
    return np.concatenate([fr, np.zeros((m, PADDED - WINDOW), f)], axis=1).astype(f)


def fbank(samples, dtype=np.float64, target_length=None, parts=False, torchaudio_weights=False):
    """(m or target_length, 128) log-mel filterbank of an int16 clip in `dtype`.  parts=True also returns what `tolerance` needs:
    the frames x, |X| over the bins 0..255 and the mel energies E.  torchaudio_weights=True makes the fp32 run carry torchaudio's
    own fp32 mel weights: what torchaudio itself returns, up to the host's fp32 log and FFT."""
    f = dtype
    x = frames(samples, f)
    if f == np.float32:
        spec = torch.fft.rfft(torch.from_numpy(x)).abs().pow(2.0).numpy()
    else:
        spec = np.abs(np.fft.rfft(x, axis=1)) ** 2.0
    # the fp32 run carries the fp64 weights rounded once, as the kernel does: torchaudio's fp32 weights are up to 1.4e-5 off, which
    # is no FFT error, yet it would set the constant the FFT's error model is given (c = 7 to 400 in place of 0 to 1)
    weights = mel_banks(np.float32) if torchaudio_weights and f == np.float32 else mel_banks(np.float64).astype(f)
    mel = np.concatenate([weights, np.zeros((NUM_MEL, 1), f)], axis=1)                           # the Nyquist bin has weight 0
    E = (spec @ mel.T).astype(f)
    out = np.log(np.maximum(E, f(EPS)))
    if target_length is not None:
        out = np.concatenate([out, np.zeros((max(target_length - out.shape[0], 0), NUM_MEL), f)])[:target_length]
    return (out, x, np.sqrt(spec[:, :PADDED // 2]), E) if parts else out


def tolerance_terms(x, absX, E):
    """What the bound is made of, from the fp64 model (x (m, 512), |X| (m, 256), E (m, 128)): with delta = c * 9u * |x|_2 the
    error of every FFT output,
        tol(c) = (c * lin + c^2 * quad) / max(E, eps) + flat,   lin = 2 * 9u|x| * sum_k w_k |X_k|,  quad = (9u|x|)^2 * sum_k w_k,
        flat = 4u * |log max(E, eps)| + 300u.
    Returns (lin / max(E, eps), quad / max(E, eps), flat), each (m, 128)."""
    w = mel_banks(np.float64)
    d1 = (9.0 * U * np.linalg.norm(x, axis=1))[:, None]
    floor = np.maximum(E, EPS)
    return 2.0 * d1 * (absX @ w.T) / floor, d1 ** 2 * w.sum(axis=1)[None, :] / floor, 4.0 * U * np.abs(np.log(floor)) + 300.0 * U


def tolerance(terms, c):
    lin, quad, flat = terms
    return c * lin + c * c * quad + flat


def error(out, ref, E):
    """|out - ref|; where the fp64 energy is within a factor 2 of eps the output may land on either side of the floor, so there
    the smaller of |out - ref| and |out - log(eps)|."""
    err = np.abs(out.astype(np.float64) - ref)
    near = near_floor(E)
    return np.where(near, np.minimum(err, np.abs(out.astype(np.float64) - math.log(EPS))), err)


def near_floor(E):
    return (E > EPS / 2.0) & (E < EPS * 2.0)


def smallest_c(err, terms):
    """The smallest c with err <= tol(c) everywhere (0 when the flat part alone covers every error)."""
    lin, quad, flat = terms
    r = err - flat
    need = r > 0
    if not need.any():
        return 0.0
    a, b, r = quad[need], lin[need], r[need]
    if (a == 0).any():
        return math.inf                                 # an error in a bank without weights: no c explains it
    return float(np.max((-b + np.sqrt(b * b + 4.0 * a * r)) / (2.0 * a)))


def signals(n=2 * SAMPLE_RATE, seed=0):
    """The six 2 s test signals as int16: uniform noise, a 440 Hz tone on a noise bed, a 100 -> 7300 Hz chirp on a noise bed, quiet
    noise, a 400-sample burst in silence, full-scale int16 noise.  Each keeps fewer than 1 % of its elements within a factor 2 of
    the floor, where the test accepts either side of it.  That is why the tone lies on uniform noise of amplitude 2^-9 and the
    chirp on 2^-6 (alone, the int16 rounding noise of a pure tone puts a mel energy of about 1e-7 = eps into every bank away from
    the tone: a fifth of the elements; the chirp on 2^-9 still has 2.6 %, on 2^-7 0.8 %), and why the quiet noise has amplitude
    2^-6, not 1e-3: pre-emphasis takes 60 dB off the lowest banks, which at 1e-3 puts 5.6 % of the elements there (0.9 % at 8e-3)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SAMPLE_RATE
    q = lambda v: np.clip(np.round(v * 32768.0), -32768, 32767).astype(np.int16)
    burst = np.zeros(n)
    burst[n // 2:n // 2 + WINDOW] = rng.uniform(-0.5, 0.5, WINDOW)
    return {
        "noise": q(rng.uniform(-0.5, 0.5, n)),
        "tone440_on_noise": q(0.5 * np.sin(2 * np.pi * 440.0 * t) + rng.uniform(-2.0 ** -9, 2.0 ** -9, n)),
        "chirp_on_noise": q(0.5 * np.sin(2 * np.pi * (100.0 * t + (7300.0 - 100.0) / (2 * t[-1]) * t * t)) + rng.uniform(-2.0 ** -6, 2.0 ** -6, n)),
        "quiet_noise": q(rng.uniform(-2.0 ** -6, 2.0 ** -6, n)),
        "burst": q(burst),
        "full_scale": rng.integers(-32768, 32768, n).astype(np.int16),
    }
