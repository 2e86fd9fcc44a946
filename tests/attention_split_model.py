"""Inputs of the exact tests of the split-arithmetic attention kernels (csrc/attention_split.hip), shared by
tests/test_attention_split_cpu.py (which pins them on the CPU) and tests/test_attention_split_gpu.py.

One case = (class of tests/exact.py, length n): B = n batch rows, H = 1, and a padding mask that lets batch row b attend key b
only, so the attended key visits every position of every 32-key tile and, at n = 97, the remainder key.  q rows are drawn from the
class's operand A kind, k rows from its operand B kind (the sparse kinds over the 64 head dims), v from dense18 (all three bf16 planes
non-zero), dO from int7.  With one attended key p = 1 exactly, so
    lse[b, 0, q] = (q[b, q] . k[b, b]) / 8,   o[b, q] = v[b, b],   dV[b, b] = sum_q dO[b, q],   dV[b, other keys] = 0
hold bit for bit for a kernel whose products are exact."""
import functools

import torch

import exact as X

HD = 64
EXACT_N = (64, 97)          # two full tiles; three tiles + one remainder row (the TAIL = 1 instantiations)


@functools.lru_cache(maxsize=None)
def exact_case(cls, n):
    ka, kb, unit = X.SPEC[cls]
    B, seed = n, 4 * (1000 * X.CLASSES.index(cls) + n)
    shape = (B, n, HD)
    q = X.operand(ka, shape, seed + 1, sparse_axis=(2,))
    k = X.operand(kb, shape, seed + 2, sparse_axis=(2,))
    v = X.operand("dense18", shape, seed + 3)
    dO = X.operand("int7", shape, seed + 4)
    pm = torch.ones(B, n) - torch.eye(n)                              # row b: every key but b padded
    k_att = k[torch.arange(B), torch.arange(B)]                       # (B, 64): key b of batch row b
    return {"q": q, "k": k, "v": v, "dO": dO, "pm": pm, "k_att": k_att, "unit": unit,
            "qkv": torch.stack((q, k, v), dim=2).reshape(B, n, 3 * HD).contiguous()}


def attended_scores(case, dtype=torch.float32):
    """(B, n): q[b, q] . k[b, b], unscaled, contracted in `dtype`."""
    return torch.matmul(case["q"].to(dtype), case["k_att"].to(dtype).unsqueeze(-1)).squeeze(-1)


def six_term_scores(case, drop=None):
    """The kernels' product set on those scores in fp64 (exact.six_term), optionally with one product dropped."""
    return X.six_term(case["q"], case["k_att"].unsqueeze(-1), drop=drop).squeeze(-1)
