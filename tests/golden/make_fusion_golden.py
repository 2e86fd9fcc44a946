"""Writes tests/golden/fusion_small.npz: the reference's own SumFusion, FiLM (x_film True / False) and GatedFusion (x_gate True / False),
imported unmodified from a reference checkout by path, run in fp64 at B = 5, D = dim = 128, C = 6 with mean-reduced cross entropy:
inputs, parameters, `out` and every gradient.  Generation time only; the tests read the .npz.

    python tests/golden/make_fusion_golden.py /path/to/reference

Before writing, the restatement tests/fusion_model.py is held to the reference to 1e-12 on every stored array."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import fusion_model as F  # noqa: E402

B, D, C = 5, 128, 6
CASES = [("sum", True), ("film", True), ("film", False), ("gated", True), ("gated", False)]


def key(method, flag):
    return method if method == "sum" else f"{method}_{int(flag)}"


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_fusion_modules", os.path.join(ref_root, "models", "fusion_modules.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for method, flag in CASES:
        c = F.dense_case(method, B, D, C)
        if method == "sum":
            mod = ref.SumFusion(D, C)
        elif method == "film":
            mod = ref.FiLM(D, D, C, x_film=flag)
        else:
            mod = ref.GatedFusion(D, D, C, x_gate=flag)
        mod = mod.double()
        with torch.no_grad():
            for n, p in mod.named_parameters():
                p.copy_(c.params[n].double())
        x, y = c.x.double().requires_grad_(True), c.y.double().requires_grad_(True)
        logits = mod(x, y)[2]
        logits.retain_grad()
        loss = torch.nn.CrossEntropyLoss()(logits, c.labels)
        loss.backward()
        got = {"out": logits.detach(), "loss": loss.detach(), "dlogits": logits.grad, "dx": x.grad, "dy": y.grad}
        got.update({"d" + n: p.grad for n, p in mod.named_parameters()})
        mine = F.run(method, c.x, c.y, c.params, c.labels, flag)
        k = key(method, flag)
        for n, v in got.items():
            err = (mine[n] - v).abs().max().item()
            assert err <= 1e-12, (k, n, err)
            # the (2 D, D) / (D, D) hidden weight gradients would take the file past 1 MB in fp64: stored rounded to fp32
            out[f"{k}/{n}"] = v.numpy() if v.numel() <= 4096 else v.float().numpy()
        out[f"{k}/x"], out[f"{k}/y"], out[f"{k}/labels"] = c.x.numpy(), c.y.numpy(), c.labels.numpy()
        for n, v in c.params.items():
            out[f"{method}/p/{n}"] = v.numpy()                    # the same parameters for both values of x_film / x_gate
    path = os.path.join(HERE, "fusion_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
