"""`--lorb large` (CREMA-D, CAVClassifier: two CAV-MAE ViT-B encoders, audio 512 tokens + visual 196 tokens) on one MI355X:
samples/s of the batch-64 MLA step under FusedSGD and under FusedAdam with the reference's --cav_opti groups, and the Adam launch
alone on an encoder-sized flat buffer against its memory bound (4 reads + 3 writes of 4 B per element = 28 B/element at the HBM
rates of MI355X_MICROARCH.md: 8.0 TB/s peak, 6.29 TB/s measured for a float4 copy).  Not the headline bench line; numbers go to
DESIGN.md."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import torch
from mla_hip import CAVClassifier, MLATrainer, cav_param_groups, ops

B = int(os.environ.get("B", "64")); steps = int(os.environ.get("STEPS", "5")); depth = int(os.environ.get("DEPTH", "12"))
math_ = os.environ.get("MATH", "split"); launches = int(os.environ.get("LAUNCHES", "200"))
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
assert torch.cuda.is_available(), "bench_cav.py measures on the GPU"
class Args: fusion_method, dataset, gs_flag, modulation, lorb = "concat", "CREMAD", True, "Normal", "large"
g = torch.Generator(device="cuda").manual_seed(0)
spec = torch.randn((B, 1024, 128), device="cuda", generator=g) * 4.4849 - 5.081
image = torch.randn((B, 3, 224, 224), device="cuda", generator=g)
label = torch.randint(0, 6, (B,), device="cuda", generator=g)
result = {"batch": B, "depth": depth, "conv_math": math_}
for name in ("sgd", "adam"):
    model = CAVClassifier(Args(), depth=depth, seed=1, conv_math=math_)
    if name == "adam":
        tr = MLATrainer(model, optimizer="adam", betas=(0.95, 0.999), weight_decay=5e-7, param_groups=cav_param_groups(model, 1e-3))
    else:
        tr = MLATrainer(model, lr=1e-3)
    for s in range(2):
        tr.train_step(spec, image, label, s, 100)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        tr.train_step(spec, image, label, s + 2, 100)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    print(f"CAV MLA step ({name}, {math_}): B={B} depth={depth}: {dt*1e3:.1f} ms/step, {B/dt:.1f} samples/s, loss {tr.losses['loss'].item():.4f}")
    result[name] = {"ms_per_step": dt * 1e3, "samples_per_s": B / dt}
    n = model.mae_a.numel
    del model, tr
    torch.cuda.empty_cache()
# ---- the Adam launch alone: one encoder's flat buffer (p, g, m, v far larger than the 256 MiB Infinity Cache together)
p, gr = torch.randn(n, device="cuda", generator=g), torch.randn(n, device="cuda", generator=g) * 1e-2
m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
for s in range(3):
    ops.adam_step(p, gr, m, v, 1e-4, 0.95, 0.999, 1e-8, 5e-7, s + 1)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for s in range(launches):
    ops.adam_step(p, gr, m, v, 1e-4, 0.95, 0.999, 1e-8, 5e-7, s + 4)
e1.record()
torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 1e3 / launches          # back-to-back launches on one stream: kernel time + the boundary between two
rate = 28.0 * n / (us * 1e-6)
print(f"mla_adam_step: n={n} ({28 * n / 1e9:.2f} GB per launch): {us:.1f} us, {rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f} % of "
      f"the 8.0 TB/s peak, {100 * rate / HBM_COPY:.0f} % of the 6.29 TB/s float4-copy rate")
result["adam_launch"] = {"n": n, "us": us, "TBps": rate / 1e12, "of_peak": rate / HBM_PEAK, "of_copy_rate": rate / HBM_COPY}
print(json.dumps(result))
