"""Gate search on one MI355X: the one mla_gate_sweep launch that scores a whole grid of gates (a, beta) on a batch's kept logits -- at
each row tile the kernel is instantiated at, 1, 2 and 4 -- against what the library offers for the same answer without it, G calls of
ops.eval_head_gated on identity-head features, one per gate; and what gate_sweep= adds to the CLIPClassifier evaluation loop.  Timed
the way bench_sweep.py times (scripts/_windows.py): the forms alternate in one process, warm-up, then three windows each of at least
WINDOW_S of back-to-back calls ended by a device synchronise (host clock); the figure is the median window, the spread
(max - min) / median.  Not the headline bench line; numbers go to DESIGN.md section 9 and profiles/."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import torch  # noqa: E402
from mla_hip import CLIPClassifier, Evaluator, gate_grid, ops  # noqa: E402
from _windows import WINDOW_S, summary, verdict, windows  # noqa: E402

SHAPES = [(2, 64, 6, 100), (2, 64, 101, 100), (3, 32, 4, 20), (3, 32, 4, 80)]       # bench_sweep.py's: G = 101, 101, 231, 3 321
TILES = (1, 2, 4)
BETA = 2.0
assert torch.cuda.is_available(), "bench_gate_sweep.py measures on the GPU"


result = {"window_s": WINDOW_S, "shapes": [], "clip_loop": {}}
for M, B, C, steps in SHAPES:
    gen = torch.Generator(device="cpu").manual_seed(100 * M + C)
    outs = [(torch.randn((B, C), generator=gen) * 2).cuda() for _ in range(M)]
    label = torch.randint(0, C, (B,), generator=gen).cuda()
    grid_host = gate_grid(M, betas=(BETA,), steps=steps)
    G = grid_host.shape[0]
    grid = grid_host.cuda()
    rows = [[float(v) for v in r] for r in grid_host]
    tp, pp = (torch.zeros((G, C), device="cuda", dtype=torch.int32) for _ in range(2))
    num = torch.zeros(C, device="cuda", dtype=torch.int32)
    counts = torch.zeros((G, C * (2 + M)), device="cuda", dtype=torch.int32)
    eye, zero = torch.eye(C, device="cuda"), torch.zeros(C, device="cuda")           # the identity head: the features are the logits
    logits = torch.empty((M, B, C), device="cuda")

    def one_launch(tile):
        def run():
            ops.gate_sweep_tile(tile)
            ops.gate_sweep(outs, label, grid, tp, pp, num=num)
        return run

    def g_gated_launches():                                  # the same answer without the sweep: one apply launch per gate
        for g in range(G):
            ops.eval_head_gated(outs, eye, zero, label, counts[g], logits, prior=rows[g][:M], beta=rows[g][M])

    tp.zero_(), pp.zero_(), counts.zero_()
    one_launch(1)()
    g_gated_launches()
    same = bool(torch.equal(tp, counts[:, C:2 * C]))         # the fused-correct counters of the G launches are the sweep's tp
    forms = {f"sweep_tile{t}": (one_launch(t), 1, 50) for t in TILES}
    forms["g_gated"] = (g_gated_launches, 1, 1)
    w = windows(forms, warmup=3)
    ops.gate_sweep_tile(1)
    row = {"M": M, "B": B, "C": C, "G": G, "same_counts": same, "g_gated": summary(w["g_gated"])}
    for t in TILES:
        row[f"sweep_tile{t}"] = summary(w[f"sweep_tile{t}"])
    row["verdict"] = verdict(row["g_gated"], row["sweep_tile1"], both=True)
    for t in TILES[1:]:
        row[f"tile{t}_vs_tile1"] = verdict(row["sweep_tile1"], row[f"sweep_tile{t}"], both=True)
    result["shapes"].append(row)
    print(f"(M, B, C, G) = ({M}, {B}, {C}, {G}): one gate_sweep launch " +
          ", ".join(f"tile {t}: {row[f'sweep_tile{t}']['us']:.1f} us (spread {row[f'sweep_tile{t}']['spread']:.1%})" for t in TILES) +
          f" vs {G} eval_head_gated launches {row['g_gated']['us']:.1f} us (spread {row['g_gated']['spread']:.1%}): {row['verdict']}; "
          f"same counts: {same}")
    for t in TILES[1:]:
        print(f"    tile {t} against tile 1: {row[f'tile{t}_vs_tile1']}")


# ---- the CLIPClassifier evaluation loop of bench_eval.py, with gate_sweep off and on
class Args:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "Food101", True, "Normal", True


N_TABLE, B, D, C = int(os.environ.get("N", "22714")), 64, 512, 101
gen = torch.Generator(device="cpu").manual_seed(7)
tok, img = torch.randn((N_TABLE, 1, D), generator=gen).cuda(), torch.randn((N_TABLE, 1, D), generator=gen).cuda()
lab = torch.randint(0, C, (N_TABLE,), generator=gen).cuda()
model = CLIPClassifier(Args(), seed=1, feat_dim=D)
grid = gate_grid(2)                                          # 6 betas x 21 priors = 126 gates
evs = {"chain": Evaluator(model, av_alpha=0.55),
       "chain+gate_sweep": Evaluator(model, av_alpha=0.55, gate_sweep=grid),
       "eval_head": Evaluator(model, dynamic=True, dynamic_mode="sample"),
       "eval_head+gate_sweep": Evaluator(model, dynamic=True, dynamic_mode="sample", gate_sweep=grid),
       "eval_head_gated": Evaluator(model, dynamic=True, dynamic_mode="sample", gate_prior=[0.55, 0.45], gate_beta=2.0)}
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
    result["clip_loop"][k + "_verdict"] = verdict(result["clip_loop"][k], result["clip_loop"][k + "+gate_sweep"], both=True)
    print(f"CLIP valid loop, {k} with gate_sweep= against without:", result["clip_loop"][k + "_verdict"])
result["clip_loop"]["gated_verdict"] = verdict(result["clip_loop"]["eval_head"], result["clip_loop"]["eval_head_gated"], both=True)
print("CLIP valid loop, eval_head_gated against eval_head (mode 1):", result["clip_loop"]["gated_verdict"])
s = evs["eval_head+gate_sweep"].gate_sweep_result()
at = 11                                                      # beta = 0, priors (0.55, 1.0 - 0.55): the fixed fusion of the chain
result["clip_loop"]["fixed_row_matches"] = bool(s.acc[at] == evs["chain"].result()[0])
prior, beta, value, g = s.best("acc")
print(f"one pass with gate_sweep= scores {grid.shape[0]} gates; grid row {at} equals the fixed-weight evaluator's accuracy: "
      f"{result['clip_loop']['fixed_row_matches']}; best of the grid {value:.4f} at row {g}: prior {prior.tolist()}, beta {beta}")
print(json.dumps(result))
