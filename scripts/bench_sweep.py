"""Fusion-weight search on one MI355X: the one mla_fusion_sweep launch that scores a whole grid of fusion weights on a batch's kept
logits, against what the library offered for the same answer before it -- G calls of ops.eval_fuse on those logits, one per grid
row -- and what sweep= adds to the CLIPClassifier evaluation loop.  Timed the way bench_eval.py / bench_metrics.py time: the forms
alternate in one process, warm-up, then three windows each of at least WINDOW_S of back-to-back calls ended by a device synchronise
(host clock); the figure is the median window, the spread (max - min) / median.  The larger claim -- one evaluation pass instead of G
passes through the encoders -- needs no measurement beyond the pass time printed beside it.  Not the headline bench line; numbers go
to DESIGN.md section 9 and profiles/."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import torch  # noqa: E402
from mla_hip import CLIPClassifier, Evaluator, fusion_grid, ops  # noqa: E402
from _windows import WINDOW_S, summary, verdict, windows  # noqa: E402

SHAPES = [(2, 64, 6, 100), (2, 64, 101, 100), (3, 32, 4, 20), (3, 32, 4, 80)]       # (M, B, C, steps): G = 101, 101, 231, 3 321
assert torch.cuda.is_available(), "bench_sweep.py measures on the GPU"


result = {"window_s": WINDOW_S, "shapes": [], "clip_loop": {}}
for M, B, C, steps in SHAPES:
    gen = torch.Generator(device="cpu").manual_seed(100 * M + C)
    outs = [(torch.randn((B, C), generator=gen) * 2).cuda() for _ in range(M)]
    label = torch.randint(0, C, (B,), generator=gen).cuda()
    grid_host = fusion_grid(M, steps)
    G = grid_host.shape[0]
    grid = grid_host.cuda()
    rows = [[float(v) for v in r] for r in grid_host]
    tp, pp = (torch.zeros((G, C), device="cuda", dtype=torch.int32) for _ in range(2))
    num = torch.zeros(C, device="cuda", dtype=torch.int32)
    counts = torch.zeros((G, C * (2 + M)), device="cuda", dtype=torch.int32)

    def one_launch():
        ops.fusion_sweep(outs, label, grid, tp, pp, num=num)

    def g_fuse_launches():                                   # the same answer before the sweep: one fusion launch per grid row
        for g in range(G):
            ops.eval_fuse(outs, label, counts[g], None, False, rows[g])

    tp.zero_(), pp.zero_(), counts.zero_()
    one_launch()
    g_fuse_launches()
    same = bool(torch.equal(tp, counts[:, C:2 * C]))         # the fused-correct counters of the G launches are the sweep's tp
    w = windows({"sweep": (one_launch, 1, 50), "g_fuse": (g_fuse_launches, 1, 1)}, warmup=3)       # back-to-back launches on both sides
    row = {"M": M, "B": B, "C": C, "G": G, "sweep": summary(w["sweep"]), "g_fuse": summary(w["g_fuse"]), "same_counts": same}
    row["verdict"] = verdict(row["g_fuse"], row["sweep"], both=True)
    result["shapes"].append(row)
    print(f"(M, B, C, G) = ({M}, {B}, {C}, {G}): one sweep launch {row['sweep']['us']:.1f} us (spread {row['sweep']['spread']:.1%}) vs "
          f"{G} eval_fuse launches {row['g_fuse']['us']:.1f} us (spread {row['g_fuse']['spread']:.1%}): {row['verdict']}; "
          f"same counts: {same}")


# ---- the CLIPClassifier evaluation loop of bench_eval.py, with sweep off and on
class Args:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "Food101", True, "Normal", True


N_TABLE, B, D, C = int(os.environ.get("N", "22714")), 64, 512, 101
gen = torch.Generator(device="cpu").manual_seed(7)
tok, img = torch.randn((N_TABLE, 1, D), generator=gen).cuda(), torch.randn((N_TABLE, 1, D), generator=gen).cuda()
lab = torch.randint(0, C, (N_TABLE,), generator=gen).cuda()
model = CLIPClassifier(Args(), seed=1, feat_dim=D)
grid = fusion_grid(2, 100)
evs = {"chain": Evaluator(model, av_alpha=0.55),
       "chain+sweep": Evaluator(model, av_alpha=0.55, sweep=grid),
       "eval_head": Evaluator(model, dynamic=True, dynamic_mode="sample"),
       "eval_head+sweep": Evaluator(model, dynamic=True, dynamic_mode="sample", sweep=grid)}
table = [(tok[o:o + B], img[o:o + B], lab[o:o + B]) for o in range(0, N_TABLE, B)]


def loop(ev):
    def run():
        ev.reset()
        for t, i, l in table:
            ev.update(t, i, l)
    return run


w = windows({k: (loop(ev), len(table), 1) for k, ev in evs.items()}, warmup=3)
for k, ev in evs.items():
    result["clip_loop"][k] = dict(summary(w[k]), acc=ev.result()[0])
    r = result["clip_loop"][k]
    print(f"CLIP valid loop ({k}): N={N_TABLE} B={B} D={D} C={C} G={grid.shape[0]}: {r['us']:.1f} us/batch (spread {r['spread']:.1%}), "
          f"{r['us'] * len(table) / 1e3:.2f} ms per pass")
for k in ("chain", "eval_head"):
    result["clip_loop"][k + "_verdict"] = verdict(result["clip_loop"][k], result["clip_loop"][k + "+sweep"], both=True)
    print(f"CLIP valid loop, {k} with sweep= against without:", result["clip_loop"][k + "_verdict"])
s = evs["chain+sweep"].sweep_result()
at = 55                                                      # grid row 55 = (0.55, 1.0 - 0.55): the evaluator's own alphas
result["clip_loop"]["own_row_matches"] = bool(s.acc[at] == evs["chain"].result()[0])
one, passes = result["clip_loop"]["chain"]["us"] * len(table) / 1e3, grid.shape[0]
print(f"one pass with sweep= answers what {passes} passes of {one:.2f} ms answer without it ({passes * one:.0f} ms); grid row {at} equals "
      f"the evaluator's own accuracy: {result['clip_loop']['own_row_matches']}; best of the grid {s.best('acc')[1]:.4f} at row {s.best('acc')[2]}")
print(json.dumps(result))
