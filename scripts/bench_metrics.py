"""Evaluation metrics on one MI355X: what metrics=True costs per batch (one mla_scores_append launch) and what
average_precision() costs at result time, each against the host route a user takes without it -- copy every batch's logits and
labels out, keep them, softmax and average precision in numpy / sklearn.  Timed the way bench_eval.py times: the forms alternate in
one process, warm-up, then three windows each of at least WINDOW_S of back-to-back calls ended by a device synchronise (host clock);
the figure is the median window, the spread (max - min) / median.  Also the CLIPClassifier evaluation loop of bench_eval.py with and
without metrics=True.  Not the headline bench line; numbers go to DESIGN.md section 9 and profiles/."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mla_hip import CLIPClassifier, Evaluator, ScoreStore  # noqa: E402
from _windows import WINDOW_S, summary, verdict, windows  # noqa: E402

try:
    from sklearn.metrics import average_precision_score
except ImportError:
    average_precision_score = None

SETS = [("CREMA-D test", 744, 6), ("Food-101 test", int(os.environ.get("N", "22716")), 101)]     # (name, N, C)
M, B = 2, 64
assert torch.cuda.is_available(), "bench_metrics.py measures on the GPU"
f32 = dict(device="cuda", dtype=torch.float32)


def host_ap(probs, labels, C):
    """The host route at result time: per head and class, sklearn's average_precision_score (numpy's sort-based sweep without it)."""
    out = np.full((len(probs), C), np.nan)
    for h, p in enumerate(probs):
        for c in range(C):
            pos = labels == c
            if not pos.any():
                continue
            if average_precision_score is not None:
                out[h, c] = average_precision_score(pos, p[:, c])
            else:
                order = np.argsort(-p[:, c], kind="stable")
                s, hit = p[order, c], pos[order]
                last = np.r_[s[1:] != s[:-1], True]                           # the end of each tie group
                tp, cnt = np.cumsum(hit)[last], (np.flatnonzero(last) + 1)
                out[h, c] = float(np.sum(np.diff(np.r_[0, tp]) / pos.sum() * tp / cnt))
    return out


result = {"window_s": WINDOW_S, "host_ap": "sklearn" if average_precision_score is not None else "numpy", "sets": [], "clip_loop": {}}
for name, N, C in SETS:
    g = torch.Generator(device="cpu").manual_seed(100 + C)
    logits = [(torch.randn((N, C), generator=g) * 2).cuda() for _ in range(M)]
    label = torch.randint(0, C, (N,), generator=g).cuda()
    weights = torch.tensor([0.5, 0.5, 0.0], **f32)
    store = ScoreStore(1 + M, C, N, "cuda")
    batches = [(o, min(B, N - o)) for o in range(0, N, B)]
    host = {"i": 0, "kept": [None] * len(batches)}
    dev = {"i": 0}

    def append_device():
        if dev["i"] == 0:
            store.reset()
        o, b = batches[dev["i"]]
        store.append([None] + [l[o:o + b] for l in logits], label[o:o + b], weights)
        dev["i"] = (dev["i"] + 1) % len(batches)

    def append_host():                                       # copy the batch's logits and labels out and keep them
        o, b = batches[host["i"]]
        host["kept"][host["i"]] = ([l[o:o + b].cpu() for l in logits], label[o:o + b].cpu())
        host["i"] = (host["i"] + 1) % len(batches)

    w = windows({"append": (append_device, 1), "host_copy": (append_host, 1)})
    row = {"set": name, "N": N, "C": C, "M": M, "B": B, "append": summary(w["append"]), "host_copy": summary(w["host_copy"])}

    dev["i"] = 0                                             # a full store, and the host route's kept copies of the same logits
    for _ in batches:
        append_device()
    host_logits = [l.cpu().numpy() for l in logits]
    host_labels = label.cpu().numpy()

    def ap_device():
        return store.average_precision()

    def ap_host():
        fused = 0.5 * host_logits[0] + 0.5 * host_logits[1]
        probs = []
        for x in [fused] + host_logits:
            e = np.exp(x - x.max(axis=1, keepdims=True))
            probs.append(e / e.sum(axis=1, keepdims=True))
        return host_ap(probs, host_labels, C)

    got, want = ap_device(), ap_host()
    row["ap_max_abs_diff_vs_host"] = float(np.nanmax(np.abs(got - want)))
    row["mAP"] = [float(np.nanmean(r)) for r in got]
    w = windows({"average_precision": (ap_device, 1, 1), "host_ap": (ap_host, 1, 1)})
    row["average_precision"], row["host_ap"] = summary(w["average_precision"]), summary(w["host_ap"])
    result["sets"].append(row)
    print(f"{name} N={N} C={C} H={1 + M}: append {row['append']['us']:.1f} us/batch (spread {row['append']['spread']:.1%}) vs copying "
          f"the logits out {row['host_copy']['us']:.1f} us/batch (spread {row['host_copy']['spread']:.1%}); average_precision() "
          f"{row['average_precision']['us'] / 1e3:.3f} ms (spread {row['average_precision']['spread']:.1%}) vs host "
          f"{result['host_ap']} {row['host_ap']['us'] / 1e3:.1f} ms (spread {row['host_ap']['spread']:.1%}); the two differ by "
          f"{row['ap_max_abs_diff_vs_host']:.2g}")


# ---- the CLIPClassifier evaluation loop of bench_eval.py, with and without metrics=True
class Args:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "Food101", True, "Normal", True


N_TABLE, D, C = SETS[1][1], 512, 101
g = torch.Generator(device="cpu").manual_seed(7)
tok, img = torch.randn((N_TABLE, 1, D), generator=g).cuda(), torch.randn((N_TABLE, 1, D), generator=g).cuda()
lab = torch.randint(0, C, (N_TABLE,), generator=g).cuda()
model = CLIPClassifier(Args(), seed=1, feat_dim=D)
evs = {"chain": Evaluator(model, dynamic=True),
       "chain+metrics": Evaluator(model, dynamic=True, metrics=True, capacity=N_TABLE),
       "eval_head": Evaluator(model, dynamic=True, dynamic_mode="sample"),
       "eval_head+metrics": Evaluator(model, dynamic=True, dynamic_mode="sample", metrics=True, capacity=N_TABLE)}
table = [(tok[o:o + B], img[o:o + B], lab[o:o + B]) for o in range(0, N_TABLE, B)]


def loop(ev):
    def run():
        ev.reset()
        for t, i, l in table:
            ev.update(t, i, l)
    return run


w = windows({k: (loop(ev), len(table)) for k, ev in evs.items()})
for k, ev in evs.items():
    result["clip_loop"][k] = dict(summary(w[k]), acc=ev.result()[0])
    r = result["clip_loop"][k]
    print(f"CLIP valid loop ({k}): N={N_TABLE} B={B} D={D} C={C}: {r['us']:.1f} us/batch (spread {r['spread']:.1%}), "
          f"{r['us'] * len(table) / 1e3:.2f} ms per pass")
for k in ("chain", "eval_head"):
    result["clip_loop"][k + "_verdict"] = verdict(result["clip_loop"][k], result["clip_loop"][k + "+metrics"])
    print(f"CLIP valid loop, {k} with metrics=True against without:", result["clip_loop"][k + "_verdict"])
print(json.dumps(result))
