"""Fused attention, fp32-MFMA kernels (math "f32") against the split-bf16 kernels (math "split"), at the shapes of
scripts/bench_attention.py.  Both arithmetics alternate inside one process: three runs of each per shape, every run printed as us and
TFLOP/s executed (products incl. the backward's recomputation), then the median and (max - min) / median per arithmetic, and the
ratio split / f32 of the medians of forward + backward."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import statistics
import torch
from mla_hip import ops

MATHS = ("f32", "split")
RUNS = 3


def timeit(fn, rep=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(rep): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / rep * 1e3


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


for B, H, n, masked in ((64, 12, 257, True), (64, 12, 257, False), (64, 12, 256, True), (64, 12, 256, False), (64, 12, 288, False), (64, 12, 258, False), (32, 12, 512, False)):
    D = H * 64
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn((B, n, 3 * D), device="cuda", generator=g) * 0.7
    do = torch.randn((B, n, D), device="cuda", generator=g)
    pm = None
    if masked:
        lens = torch.randint(8, n, (B,), device="cuda", generator=g)
        pm = (torch.arange(n, device="cuda")[None, :] >= lens[:, None]).float().contiguous()
        pm[:, 0] = 0
    o, lse = torch.empty((B, n, D), device="cuda"), torch.empty((B, H, n), device="cuda")
    dqkv, dvec = torch.empty_like(qkv), torch.empty((B, H, n), device="cuda")
    unit = 2.0 * B * H * n * n * 64 / 1e9
    t = {m: {"fwd": [], "bwd": [], "sum": []} for m in MATHS}
    print(f"B={B} H={H} n={n} masked={masked}")
    for run in range(RUNS):
        for m in MATHS:
            tf = timeit(lambda: ops.attention_fwd(qkv, pm, o, lse, B, H, n, 64, math=m))
            tb = timeit(lambda: ops.attention_bwd(do, qkv, o, lse, pm, dqkv, dvec, B, H, n, 64, math=m))
            t[m]["fwd"].append(tf); t[m]["bwd"].append(tb); t[m]["sum"].append(tf + tb)
            print(f"  run {run} {m:5s}: fwd {tf:7.1f} us ({2 * unit / tf * 1e3:5.1f} TF) | bwd {tb:7.1f} us ({7 * unit / tb * 1e3:5.1f} TF executed)", flush=True)
    for m in MATHS:
        print(f"  {m:5s} median: " + " | ".join(f"{k} {statistics.median(v):7.1f} us, (max - min) / median {spread(v):.3f}" for k, v in t[m].items()))
    ratio = statistics.median(t["split"]["sum"]) / statistics.median(t["f32"]["sum"])
    worst = max(spread(t[m]["sum"]) for m in MATHS)
    verdict = "split faster" if ratio < 1 - worst else ("split slower" if ratio > 1 + worst else "within the spread")
    print(f"  split / f32 (fwd + bwd): {ratio:.3f}; fwd {statistics.median(t['split']['fwd']) / statistics.median(t['f32']['fwd']):.3f}, "
          f"bwd {statistics.median(t['split']['bwd']) / statistics.median(t['f32']['bwd']):.3f}; larger spread {worst:.3f} -> {verdict}", flush=True)
