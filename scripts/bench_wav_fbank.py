"""mla_wav_fbank on one MI355X (numbers go to DESIGN.md section 9; no pass/fail threshold):
  kernel time at B = 64 for 250-frame (2.5 s) and 1024-frame (10.25 s) clips, device events around REPS launches after WARMUP;
  mla_fbank_augment (normalise only) on the same (64, 1024, 128) output in the same process: an existing streaming kernel that
  writes the same bytes;
  the host rate of read_wav against np.load of the .npy, one thread, files in the page cache."""
import os, sys, tempfile, time, wave
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import numpy as np
import torch
from mla_hip import load_fbank, ops, read_wav, wav_feed
from mla_hip.cav_feed import NORM_MEAN, NORM_STD, fbank_descriptors

B, T = int(os.environ.get("B", "64")), 1024
WARMUP, REPS, ROUNDS = int(os.environ.get("WARMUP", "20")), int(os.environ.get("REPS", "200")), int(os.environ.get("ROUNDS", "5"))


def timed(fn):
    """Median and spread over ROUNDS of the mean device time of REPS launches, in microseconds."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / REPS)
    return float(np.median(times)), min(times), max(times)


def main():
    assert torch.cuda.is_available(), "bench_wav_fbank needs a GPU"
    rng = np.random.default_rng(0)
    tables = wav_feed.device_tables("cuda")
    out = torch.empty((B, T, 128), device="cuda")
    for frames in (250, 1024):
        n = 400 + 160 * (frames - 1)
        clips = [rng.integers(-20000, 20000, n).astype(np.int16) for _ in range(B)]
        desc, total = wav_feed.clip_descriptors(clips)
        wav, desc_host = torch.from_numpy(np.concatenate(clips)).cuda(), torch.from_numpy(desc)
        desc_dev = desc_host.cuda()
        med, lo, hi = timed(lambda: ops.wav_fbank(wav, desc_dev, desc_host, tables, out))
        flop = B * frames * (5 * 256 * 8 + 10 * 400 + 2 * 504 + 8 * 256)            # FFT 5 N log2 N, framing, mel, post-pass
        print(f"wav_fbank B={B} {frames}-frame clips: {med:.1f} us (min {lo:.1f}, max {hi:.1f}); reads {total * 2 / 1e6:.1f} MB, writes "
              f"{out.numel() * 4 / 1e6:.1f} MB -> {(total * 2 + out.numel() * 4) / med / 1e3:.0f} GB/s, {flop / med / 1e3:.0f} GFLOP/s")
    fdesc = torch.from_numpy(fbank_descriptors([None] * B, [0] * B))
    fdesc_dev, aug = fdesc.cuda(), torch.empty_like(out)
    med, lo, hi = timed(lambda: ops.fbank_augment(out, aug, fdesc_dev, fdesc, NORM_MEAN, NORM_STD, 0))
    print(f"fbank_augment (normalise only) on ({B}, {T}, 128): {med:.1f} us (min {lo:.1f}, max {hi:.1f}); reads and writes "
          f"{out.numel() * 4 / 1e6:.1f} MB each -> {2 * out.numel() * 4 / med / 1e3:.0f} GB/s")

    with tempfile.TemporaryDirectory() as d:
        n = 16000 * 5
        for i in range(32):
            with wave.open(os.path.join(d, f"{i}.wav"), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(rng.integers(-20000, 20000, n).astype(np.int16).tobytes())
            np.save(os.path.join(d, f"{i}.npy"), rng.standard_normal((1024, 128)).astype(np.float32))
        stage = np.empty((1024, 128), np.float32)

        def host(fn, rounds=20):
            fn(0)
            t0 = time.perf_counter()
            for r in range(rounds):
                for i in range(32):
                    fn(i)
            return (time.perf_counter() - t0) / (32 * rounds)
        t_wav = host(lambda i: int(read_wav(os.path.join(d, f"{i}.wav")).sum(dtype=np.int64)))
        t_npy = host(lambda i: np.copyto(stage, load_fbank(d, str(i))))
        print(f"host, one thread, page cache: read_wav + integer sum of a 5 s clip (160 KB) {t_wav * 1e6:.0f} us = {1 / t_wav:.0f} clips/s; "
              f"np.load + copy of its (1024, 128) .npy (512 KB) {t_npy * 1e6:.0f} us = {1 / t_npy:.0f} clips/s")


if __name__ == "__main__":
    main()
