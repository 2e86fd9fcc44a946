"""Regenerate tests/golden/modal3_mask_small.npz: the matrices the reference's `random_mask` (dataset/dataset.py:596-640) returns
on numpy's global legacy stream, for the restated mla_hip.random_mask to be compared with.

    python tests/golden/make_golden_modal3.py /path/to/reference

The reference module cannot be imported where timm and torchaudio are absent, so the one function definition is taken out of the
parsed file and executed with what it names: numpy, sklearn's OneHotEncoder and numpy.random.randint.  For every case the global
stream is seeded with np.random.seed(seed) and the function called once.  Only (n, rate, seed) and the resulting matrices are
stored: no reference text.  Cases: n in {40, 400}, missing rates {0, 0.1, 0.3, 0.5, 0.6, 0.7, 0.8}, seeds {0, 1, 7} -- the
one-modality regime (rates 0.7 and 0.8: 1 - rate <= 1/3), the all-ones regime (rate 0) and the rejection loop (the others).
"""
import ast
import os
import sys

import numpy as np

NS = (40, 400)
RATES = (0.0, 0.1, 0.3, 0.5, 0.6, 0.7, 0.8)
SEEDS = (0, 1, 7)


def reference_random_mask(reference_root):
    from numpy.random import randint
    from sklearn.preprocessing import OneHotEncoder
    path = os.path.join(reference_root, "dataset", "dataset.py")
    tree = ast.parse(open(path).read(), path)
    fn = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "random_mask"]
    assert len(fn) == 1, f"{path}: expected one random_mask, found {len(fn)}"
    env = {"np": np, "OneHotEncoder": OneHotEncoder, "randint": randint}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), env)
    return env["random_mask"]


def main():
    ref = reference_random_mask(sys.argv[1])
    cases, out = [], {}
    for n in NS:
        for rate in RATES:
            for seed in SEEDS:
                np.random.seed(seed)
                m = np.asarray(ref(3, n, rate))
                assert m.shape == (n, 3) and np.isin(m, (0, 1)).all()
                out[f"mask_{len(cases)}"] = m.astype(np.int8)
                cases.append((n, rate, seed))
    out["n"] = np.array([c[0] for c in cases], dtype=np.int64)
    out["rate"] = np.array([c[1] for c in cases], dtype=np.float64)
    out["seed"] = np.array([c[2] for c in cases], dtype=np.int64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "modal3_mask_small.npz")
    np.savez_compressed(path, **out)
    print(path, len(cases), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
