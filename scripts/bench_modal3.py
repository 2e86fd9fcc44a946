"""Config 5 of BASELINE.json (IEMOCAP, --modal3: CAV-MAE audio + M3AE image + M3AE text, 3-way alternation), per-GPU batch 32,
on one MI355X: samples/s of the MLA step.  Not the headline bench line; numbers go to DESIGN.md.

--mask-percent R zero-fills the inputs per a random_mask(3, B, R) matrix, as Modal3Batcher leaves the absent modalities;
--present on hands that matrix to train_step(present=) (each encoder on the rows that have its modality plus one zero row),
--present both runs the two forms alternately in this one process, --runs of --steps steps each, and reports per form the median
and (max - min) / median of the runs.  Without arguments: one run on unmasked inputs, as before.  B, STEPS, DEPTH and MATH in the
environment set the defaults of --batch, --steps, --depth and --math."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import numpy as np
import torch
from mla_hip import Modal3Classifier, MLATrainer, random_mask

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=int(os.environ.get("B", "32")))
ap.add_argument("--steps", type=int, default=int(os.environ.get("STEPS", "5")))
ap.add_argument("--depth", type=int, default=int(os.environ.get("DEPTH", "12")))
ap.add_argument("--math", default=os.environ.get("MATH", "f32"))
ap.add_argument("--mask-percent", type=float, nargs="+", default=[0.0])
ap.add_argument("--mask-seed", type=int, default=0)
ap.add_argument("--present", choices=("off", "on", "both"), default="off")
ap.add_argument("--runs", type=int, default=1)
ap.add_argument("--warmup-steps", type=int, default=0, help="untimed steps on the unmasked inputs before the first run (DESIGN section 9: "
                "the first passes of a process are slower whatever feeds them)")
a = ap.parse_args()
B, steps, depth, math_ = a.batch, a.steps, a.depth, a.math

class Args: fusion_method, dataset, gs_flag, modulation, modal3 = "concat", "IEMOCAP", True, "Normal", True
model = Modal3Classifier(Args(), depth=depth, seed=1, conv_math=math_)
tr = MLATrainer(model)
g = torch.Generator(device="cuda").manual_seed(0)
token = torch.randint(0, 30522, (B, 1, 256), device="cuda", generator=g)
lens = torch.randint(8, 257, (B,), device="cuda", generator=g)
pm = (torch.arange(256, device="cuda")[None, :] >= lens[:, None]).float().view(B, 1, 256)
image = torch.randn((B, 3, 256, 256), device="cuda", generator=g)
spec = torch.randn((B, 1024, 128), device="cuda", generator=g) * 4.4849 - 5.081
label = torch.randint(0, 4, (B,), device="cuda", generator=g)
step = 0


def run(inputs, present):
    """ms per step of `steps` steps behind two untimed ones."""
    global step
    kw = {} if present is None else {"present": present}
    for timed in (2, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(timed):
            tr.train_step(*inputs, label, step, 100, **kw)
            step += 1
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


for _ in range(a.warmup_steps):
    tr.train_step(token, pm, image, spec, label, step, 100)
    step += 1
for rate in a.mask_percent:
    mask = random_mask(3, B, rate, np.random.RandomState(a.mask_seed))           # columns (audio, image, text)
    m = torch.from_numpy(mask).cuda()
    inputs = (token * m[:, 2].view(B, 1, 1), pm * m[:, 2].view(B, 1, 1), image * m[:, 1].view(B, 1, 1, 1), spec * m[:, 0].view(B, 1, 1))
    present = torch.from_numpy(mask != 0)
    forms = {"off": [("all rows", None)], "on": [("present", present)], "both": [("all rows", None), ("present", present)]}[a.present]
    ms = {name: [] for name, _p in forms}
    for _ in range(a.runs):
        for name, p in forms:                                                    # the forms alternate, run by run
            ms[name].append(run(inputs, p))
    rows = "/".join(str(int(c)) for c in mask.sum(axis=0))
    for name, v in ms.items():
        med = statistics.median(v)
        print(f"Modal3 MLA step ({math_}): B={B} depth={depth} mask={rate:g} (present a/v/t {rows}) {name}: {med:.1f} ms/step, "
              f"{B / med * 1e3:.1f} samples/s, spread {(max(v) - min(v)) / med:.3f} over {len(v)} run(s) of {steps} steps "
              f"[{', '.join(f'{x:.1f}' for x in v)}], loss {tr.losses['loss'].item():.4f}")
