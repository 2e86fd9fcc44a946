"""Evaluation of one batch on one MI355X: the published chain (M mla_head_logits launches + one mla_eval_fuse, --dynamic) against the
one mla_eval_head call (per-sample gating, mode 1), from the same features to the same counter layout.  The two alternate in one
process: warm-up, then three timed windows each, every window at least WINDOW_S of back-to-back calls on one stream ended by a
device synchronise (host clock: launch overhead is what the fusion is about).  The figure is the median window, the spread
(max - min) / median.  Also the CLIPClassifier evaluation loop (Evaluator.update over a synthetic feature table, Food-101's test
size), one row per launch form.  The two forms compute different gating rules by design; this times them, tests/ compares them.
Not the headline bench line; numbers go to DESIGN.md section 9, the README and INTEGRATION.md."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import torch  # noqa: E402
from mla_hip import CLIPClassifier, Evaluator, ops  # noqa: E402
from _windows import WINDOW_S, summary, verdict, windows  # noqa: E402

SHAPES = [(2, 64, 512, 101), (2, 64, 512, 6), (2, 64, 768, 101), (3, 32, 768, 4)]            # (M, B, D, C)
N_TABLE = int(os.environ.get("N", "22714"))                                                  # Food-101 test samples
assert torch.cuda.is_available(), "bench_eval.py measures on the GPU"
f32 = dict(device="cuda", dtype=torch.float32)


result = {"window_s": WINDOW_S, "shapes": [], "clip_loop": {}}
for M, B, D, C in SHAPES:
    g = torch.Generator(device="cpu").manual_seed(1000 + D + C)
    feats = [torch.randn((B, D), generator=g).cuda() for _ in range(M)]
    W, b = (torch.randn((C, D), generator=g) * 0.05).cuda(), (torch.randn((C,), generator=g) * 0.1).cuda()
    label = torch.randint(0, C, (B,), generator=g).cuda()
    alphas = [0.5, 0.5] if M == 2 else [0.35, 0.25, 0.4]
    outs = [torch.empty((B, C), **f32) for _ in range(M)]
    counts_c, w_c = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32), torch.zeros(3, **f32)
    logits, fused, wts = torch.empty((M, B, C), **f32), torch.empty((B, C), **f32), torch.empty((B, M), **f32)
    pred, counts_f = torch.empty((B, 1 + M), device="cuda", dtype=torch.int32), torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)

    def chain():
        for f, o in zip(feats, outs):
            ops.head_logits(f, W, b, o)
        ops.eval_fuse(outs, label, counts_c, w_c, True, alphas)

    def one():
        ops.eval_head(feats, W, b, label, counts_f, logits, mode=1, alphas=alphas, fused_out=fused, weights_out=wts, pred_out=pred)

    w = windows({"chain": (chain, 1), "eval_head": (one, 1)})
    row = {"M": M, "B": B, "D": D, "C": C, "chain": summary(w["chain"]), "eval_head": summary(w["eval_head"])}
    row["verdict"] = verdict(row["chain"], row["eval_head"], what="the chain's spread")
    result["shapes"].append(row)
    print(f"M={M} B={B} D={D} C={C}: chain ({M + 1} launches) {row['chain']['us']:.1f} us (spread {row['chain']['spread']:.1%}), "
          f"eval_head (1 launch) {row['eval_head']['us']:.1f} us (spread {row['eval_head']['spread']:.1%}): {row['verdict']}")


# ---- the CLIPClassifier evaluation loop: Evaluator.update over a device-resident synthetic table, Food-101's test size
class Args:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "Food101", True, "Normal", True


B, D, C = 64, 512, 101
g = torch.Generator(device="cpu").manual_seed(7)
tok, img = torch.randn((N_TABLE, 1, D), generator=g).cuda(), torch.randn((N_TABLE, 1, D), generator=g).cuda()
lab = torch.randint(0, C, (N_TABLE,), generator=g).cuda()
model = CLIPClassifier(Args(), seed=1, feat_dim=D)
evs = {"chain": Evaluator(model, dynamic=True), "eval_head": Evaluator(model, dynamic=True, dynamic_mode="sample")}
batches = [(tok[o:o + B], img[o:o + B], lab[o:o + B]) for o in range(0, N_TABLE, B)]


def loop(ev):
    def run():
        ev.reset()
        for t, i, l in batches:
            ev.update(t, i, l)
    return run


w = windows({k: (loop(ev), len(batches)) for k, ev in evs.items()})
for k, ev in evs.items():
    result["clip_loop"][k] = dict(summary(w[k]), acc=ev.result()[0])
result["clip_loop"]["batches"], result["clip_loop"]["N"] = len(batches), N_TABLE
result["clip_loop"]["verdict"] = verdict(result["clip_loop"]["chain"], result["clip_loop"]["eval_head"], what="the chain's spread")
for k in evs:
    r = result["clip_loop"][k]
    print(f"CLIP valid loop ({k}): N={N_TABLE} B={B} D={D} C={C}: {r['us']:.1f} us/batch (spread {r['spread']:.1%}), "
          f"{r['us'] * len(batches) / 1e3:.2f} ms per pass")
print("CLIP valid loop:", result["clip_loop"]["verdict"])
print(json.dumps(result))
