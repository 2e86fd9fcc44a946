#!/usr/bin/env python3
"""SHA-256 of every output buffer of the four evaluation entry points -- mla_eval_fuse, mla_eval_head, mla_scores_append,
mla_fusion_sweep -- on the tests' own inputs, for scripts/head_isa.py --digests:

    MLA_HIP_LIB=<parent's libmla_hip.so> python scripts/eval_digests.py parent.json
    python scripts/eval_digests.py here.json                  (a fresh process per library)

Inputs: tests/tail_model.py's eval cases (exact ties, the 256-thread stride), eval_model.SAMPLE_DENSE (dense normal logits),
metrics_model.near_tie_case (fused values within two ulps: the rounding of the sum decides) and sweep_model.exact_case.  Every set of
logits goes through every entry point that takes its shape: fixed and gated fusion, with and without missing modalities and bad labels."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import eval_model as E  # noqa: E402
import metrics_model as MM  # noqa: E402
import sweep_model as SM  # noqa: E402
import tail_model as T  # noqa: E402
from mla_hip import fusion_grid, ops  # noqa: E402

ALPHAS = {2: (0.55, 0.45), 3: (0.35, 0.25, 0.4)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run(outs, label, alphas, grid=None):
    """{buffer: sha256} of one set of logits through the four entry points"""
    M, (B, C) = len(outs), outs[0].shape
    d_outs, out = [dev(o) for o in outs], {}
    holes = label.copy()                                     # bad labels and missing modalities, rows 1 .. of a batch that has them
    holes[1::5] = -1
    holes[2::7] = C
    present = E.every_pattern(B, M)
    present[3::11] = 0
    i32 = dict(device="cuda", dtype=torch.int32)
    for lname, lab in (("", dev(label)), ("holes.", dev(holes))):
        for dynamic in (False, True):
            counts, w = torch.zeros(C * (2 + M), **i32), torch.zeros(3, device="cuda")
            ops.eval_fuse(d_outs, lab, counts, w, dynamic, list(alphas))
            tag = f"{lname}fuse.{'dyn' if dynamic else 'fixed'}."
            out[tag + "counts"], out[tag + "weights"] = sha(counts), sha(w)
            if C > 128 or lname:                             # the row softmax of the other three holds at most 128 classes
                continue
            store = [torch.zeros((1 + M, C, B + 3), device="cuda"), torch.zeros((1 + M, B + 3), **i32), torch.zeros(B + 3, **i32)]
            ops.scores_append([None] + d_outs, lab, *store, 2, weights=w)
            for name, t in zip(("scores", "pred", "labels"), store):
                out[tag + "append." + name] = sha(t)
        if C > 128:
            continue
        Wi, bi = (dev(a) for a in E.identity_head(C))
        for mode in (0, 1):
            for pname, have in (("", None), ("present.", dev(present))):
                bufs = {"counts": torch.zeros(C * (2 + M), **i32), "logits": torch.zeros((M, B, C), device="cuda"),
                        "fused": torch.zeros((B, C), device="cuda"), "weights": torch.zeros((B, M), device="cuda"),
                        "pred": torch.zeros((B, 1 + M), **i32)}
                ops.eval_head(d_outs, Wi, bi, lab, bufs["counts"], bufs["logits"], mode=mode, alphas=list(alphas), present=have,
                              fused_out=bufs["fused"], weights_out=bufs["weights"], pred_out=bufs["pred"])
                for name, t in bufs.items():
                    out[f"{lname}head.mode{mode}.{pname}{name}"] = sha(t)
        g = dev(fusion_grid(M, 20).numpy() if grid is None else grid)
        for pname, have in (("", None), ("present.", dev(present))):
            tp, pp, num = torch.zeros((g.shape[0], C), **i32), torch.zeros((g.shape[0], C), **i32), torch.zeros(C, **i32)
            ops.fusion_sweep(d_outs, lab, g, tp, pp, num=num, present=have)
            for name, t in (("tp", tp), ("pp", pp), ("num", num)):
                out[f"{lname}sweep.{pname}{name}"] = sha(t)
    return out


def main(path):
    cases = {}
    for M, B, C in T.EVAL_FIXED_SHAPES:
        cases[f"tail.fixed.M{M}.B{B}.C{C}"] = run(*T.eval_fixed_case(M, B, C), T.EVAL_ALPHAS[M])
    for M, B, C in T.EVAL_DYN_SMALL:
        cases[f"tail.small.M{M}.B{B}.C{C}"] = run(*T.eval_small_case(M, B, C), ALPHAS[M])
    for B, C in T.EVAL_DYN_STRIDE:
        cases[f"tail.stride.B{B}.C{C}"] = run(*T.eval_stride_case(B, C), ALPHAS[2])
    for M, B, C in E.SAMPLE_DENSE:
        cases[f"dense.M{M}.B{B}.C{C}"] = run(*E.sample_dense_case(M, B, C), ALPHAS[M])
    for M, alphas in ((2, (0.35, 0.65)), (3, (0.35, 0.25, 0.4))):
        for B, C in ((512, 6), (130, 101)):
            outs, labels, w = MM.near_tie_case(M, B, C, alphas)
            cases[f"near_tie.M{M}.B{B}.C{C}"] = run(outs, labels, alphas, grid=np.stack([w, w[::-1].copy()]))
    for M, C, B, G in ((2, 6, 64, 64), (3, 64, 65, 65), (2, 65, 257, 256), (3, 101, 64, 257), (2, 128, 257, 861), (3, 3, 7, 4096)):
        outs, labels, grid = SM.exact_case(M, B, C, G, seed=1000 * M + 7 * C + B + G)
        cases[f"exact.M{M}.C{C}.B{B}.G{G}"] = run(list(outs), labels, ALPHAS[M], grid=grid)
    with open(path, "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d buffers -> %s (%s)" % (len(cases), sum(len(c) for c in cases.values()), path, os.environ.get("MLA_HIP_LIB", "this build")))


if __name__ == "__main__":
    main(sys.argv[1])
