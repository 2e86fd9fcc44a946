"""Inputs and fp64 / exact models for the step-tail kernels: OGM / OGM-GE modulation and coefficients (csrc/modulation.hip), SGD,
scale_by_device_scalar, colsum, bn_invstd, the GS projection (csrc/head_gs_sgd.hip) and the evaluation fusion (csrc/eval_head.hip).

Everything here is numpy / CPU torch.  tests/test_tail_cpu.py proves that the inputs meet the conditions the tolerances rest on and that
the models agree with oracle/mla_oracle.py; tests/test_tail_gpu.py holds the kernels to the models.  Where a result is exactly
representable (the OGM scaling, SGD on the 2^-4 grid, colsum on integers, the fixed-weight fusion on integers) the kernel must match
bit for bit; elsewhere the bound is derived next to the case that uses it."""
import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import torch

from oracle import mla_oracle as O
from resident_model import philox4x32_10

F32, F64 = np.float32, np.float64


def ulp32(x):
    """fp32 unit in the last place at |x| (fp64 in, fp64 out)."""
    return np.spacing(np.abs(np.asarray(x, dtype=F64)).astype(F32)).astype(F64)


def _ints(seed, n, lo, hi, stream=0):
    """n integers uniform in [lo, hi] (int64), a pure function of (seed, stream)."""
    u = O.portable_uniform(seed, n, stream)
    return np.minimum((u * (hi - lo + 1)).astype(np.int64), hi - lo) + lo


# ---- 1. OGM modulation ---------------------------------------------------------------------------------------------------------------
OGM_CHUNK = 16384                      # csrc/modulation.hip: OGM_CHUNK (ops.ogm_chunk_elems() on the device side)
OGM_EPS = F32(1e-8)                    # main.py:399: std().item() + 1e-8


def u01(x):
    """csrc/modulation.hip: u01, in fp32: (float)(x >> 8) + 0.5f needs 25 bits and rounds (RNE), so u01(0xFFFFFFFF) is exactly 1."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(F32) + F32(0.5)) * F32(1.0 / 16777216.0)


def ogm_noise(n, s, step, seed):
    """z[0..n) of segment `s` (its index in the table) at call `step`: a restatement of ogm_apply_kernel.  Element i of the SEGMENT draws
    from Philox counter i // 4, stream id (step << 16) | s; words 0, 1 feed elements 4k (r cos) and 4k + 1 (r sin), words 2, 3 feed
    4k + 2 and 4k + 3.  u01 and the angle 6.2831853f * u are fp32; log, sqrt, sin and cos are fp64."""
    k = np.arange((n + 3) // 4, dtype=np.uint64)
    w = [np.broadcast_to(np.asarray(x, dtype=np.uint64), k.shape) for x in philox4x32_10(k, (step << 16) | s, seed)]
    u = [u01(x) for x in w]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0].astype(F64))), np.sqrt(-2.0 * np.log(u[2].astype(F64)))
    a0, a1 = (F32(6.28318530717958647692) * u[1]).astype(F64), (F32(6.28318530717958647692) * u[3]).astype(F64)
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1).reshape(-1)[:n]


def ogm_family(kind, n, seed):
    """Gradient values of one segment (fp32, all exactly representable) and the integer grid they live on: values = k / den."""
    if kind == "grid":                 # small integers times 2^-6
        k, den = _ints(seed, n, -7, 7), 64
    elif kind == "int":
        k, den = _ints(seed, n, -7, 7), 1
    elif kind == "bigmean":            # 1000 + k 2^-6: an fp32 or a naive accumulation of sum^2 loses the variance entirely
        k, den = 64000 + _ints(seed, n, -64, 64), 64
    elif kind == "const":
        k, den = np.full(n, 16, dtype=np.int64), 64
    else:
        raise ValueError(kind)
    return (k.astype(F64) / den).astype(F32), k, den


def exact_var(k, den):
    """Unbiased variance of k / den in exact integer arithmetic, rounded once to fp64 (NaN for fewer than two elements)."""
    n = len(k)
    if n < 2:
        return float("nan")
    S, Q = int(k.sum()), int((k * k).sum())
    return float(Fraction(Q * n - S * S, n * (n - 1) * den * den))


def sentinel(n):
    """The pattern between the segments: negative, far from every family, different at neighbouring positions."""
    return (-(2048.0 + (np.arange(n) % 251))).astype(F32)


def ogm_table(spec, seed, lead=3):
    """One flat buffer and its segment table.  spec: (n, family) per segment; the gaps between segments cycle through 1 .. 5 floats
    of sentinel, `lead` floats stand in front and 7 behind."""
    offs, off = [], lead
    for i, (n, _kind) in enumerate(spec):
        offs.append(off)
        off += n + 1 + i % 5
    total = off + 7
    buf = sentinel(total)
    inside = np.zeros(total, dtype=bool)
    vals, grids = [], []
    for i, ((n, kind), o) in enumerate(zip(spec, offs)):
        v, k, den = ogm_family(kind, n, seed + 17 * i)
        buf[o:o + n] = v
        inside[o:o + n] = True
        vals.append(v)
        grids.append((k, den))
    chunks = [(n + OGM_CHUNK - 1) // OGM_CHUNK for n, _ in spec]
    first_chunk = np.concatenate([[0], np.cumsum(chunks)]).astype(np.int32)
    seg = np.array([[o, n] for o, (n, _k) in zip(offs, spec)], dtype=np.int64)
    var = [exact_var(k, den) for k, den in grids]
    stdv = [F32(np.sqrt(v)) for v in var]
    return SimpleNamespace(spec=spec, buf=buf, inside=inside, seg=seg, first_chunk=first_chunk, n_seg=len(spec),
                           total_chunks=int(first_chunk[-1]), vals=vals, grids=grids, var=var, stdv=stdv)


# offsets of every residue mod 4 and the lengths 2, 5, one less than / exactly / one more than a chunk, two chunks + 3, a zero-length
# segment in the middle (the first_chunk scan must skip it), and the statistics families
OGM_MAIN_SPEC = ((5, "grid"), (16383, "grid"), (2, "int"), (16384, "bigmean"), (0, "grid"), (16385, "int"), (2 * 16384 + 3, "grid"),
                 (300, "const"), (20001, "bigmean"))
OGM_ONE_SPEC = ((4, "grid"), (1, "grid"), (6, "grid"))                      # n = 1: torch's std is NaN
OGM_X = (1003, "grid")                                                        # the segment whose noise must not depend on geometry
OGM_GEOM_A = ((5, "grid"), OGM_X, OGM_X)                                      # ... at s = 1 behind a 5-element segment (and again at s = 2)
OGM_GEOM_B = ((2 * 16384 + 3, "grid"), OGM_X)                                 # ... at s = 1 behind a 3-chunk segment
OGM_SEEDS = (0, (1 << 40) + 3)                                                # the second one exercises the high key word
OGM_STEPS = (0, 5)


@functools.lru_cache(maxsize=None)
def ogm_main():
    return ogm_table(OGM_MAIN_SPEC, seed=100)


@functools.lru_cache(maxsize=None)
def ogm_one():
    return ogm_table(OGM_ONE_SPEC, seed=200, lead=2)


@functools.lru_cache(maxsize=None)
def ogm_geom(which):
    """Tables A and B: segment s = 1 (and s = 2 of A) hold the SAME values (the family seed is set by hand, not by position)."""
    t = ogm_table(OGM_GEOM_A if which == "A" else OGM_GEOM_B, seed=300 if which == "A" else 400, lead=1 if which == "A" else 2)
    x, k, den = ogm_family(OGM_X[1], OGM_X[0], 777)
    for s in range(1, t.n_seg):
        o = int(t.seg[s, 0])
        t.buf[o:o + len(x)] = x
        t.vals[s], t.grids[s], t.var[s] = x, (k, den), exact_var(k, den)
        t.stdv[s] = F32(np.sqrt(t.var[s]))
    return t


def ogm_scaled(t, coeff):
    """OGM mode in fp64: g * coeff inside the segments, the buffer elsewhere."""
    out = t.buf.astype(F64)
    out[t.inside] *= coeff
    return out


# ---- 2. OGM coefficients ------------------------------------------------------------------------------------------------------------
COEFF_SHAPES = [(M, B, C) for M in (2, 3) for B in (1, 5, 70) for C in (2, 6, 101, 300)]
COEFF_FAMILIES = ("normal", "range", "same")
COEFF_BRANCH_SHAPES = [(5, 6), (70, 101)]
COEFF_BRANCHES = ("visual", "text", "neither")
COEFF_ALPHA = 0.3


def _boost(outs, label):
    """Modality m's row m % B gets its label as the arg-max, 1 / (1 + m) above the row's maximum: every score stays away from 0, and
    the modalities' scores differ even where every other softmax term underflows (B = 1, the 'range' family)."""
    B = outs[0].shape[0]
    for m, o in enumerate(outs):
        r = m % B
        o[r, label[r]] = o[r].max() + 1.0 / (1 + m)
    return outs


def coeff_case(M, B, C, family):
    """(outs [M x (B, C) fp32], label (B) int64).  'normal': unit normal logits.  'range': rows offset by +-1e4 with an in-row spread
    of 200 (exp underflows for the classes far from the maximum; modality 1 has such a class in every row).  'same': modalities 0 and 1 hold identical logits (ratio_v == 1
    exactly: the else branch must modulate modality 0)."""
    seed = 1000 * M + 10 * B + C
    label = O.portable_labels(seed, B, C)
    outs = []
    for m in range(M):
        if family == "range":
            u = torch.from_numpy(O.portable_uniform(seed + m, B * C, 50)).float().view(B, C)
            sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0).view(B, 1)
            o = sign * 1e4 + (u - 0.5) * 200.0
            if m % 2:        # modality 1, every row: a class whose exp underflows to 0 (with C = 2 its score is then exactly B)
                o[torch.arange(B), (label + 1) % C] = o[torch.arange(B), label] - 190.0
            outs.append(o)
        else:
            outs.append(O.portable_normal(seed + m, (B, C), stream=51))
    outs = _boost(outs, label)
    if family == "same":
        outs[1] = outs[0].clone()
    return [o.float().contiguous() for o in outs], label


def coeff_branch_case(B, C, branch):
    """Three modalities, one case per branch of main.py:323-337: the dominant modality's logits are scaled up at the label (its score
    is about B), the others stay unit normal (about B / C each)."""
    seed = 5000 + 10 * B + C
    label = O.portable_labels(seed, B, C)
    outs = _boost([O.portable_normal(seed + m, (B, C), stream=52) for m in range(3)], label)
    dom = {"visual": 1, "text": 2, "neither": None}[branch]
    if dom is not None:
        outs[dom][torch.arange(B), label] += 12.0
    return [o.float().contiguous() for o in outs], label


def coeff_ref(outs, label, alpha=COEFF_ALPHA):
    """O.ogm_coefficients on doubles -> (coeffs, scores, ratios) as fp64 arrays."""
    c, s, r = O.ogm_coefficients([o.double() for o in outs], label, alpha)
    return (np.array([float(x) for x in c]), np.array([float(x) for x in s]), np.array([float(x) for x in r]))


def coeff_score_rtol(B):
    """The ordered fp32 sum of B terms plus a few ulp of expf and the division."""
    return (B + 8) * 2.0 ** -23


# ---- 3. SGD ------------------------------------------------------------------------------------------------------------------------------
SGD_LR, SGD_MOM, SGD_WD = 2.0 ** -3, 0.5, 2.0 ** -4
SGD_SIZES = [1, 2, 3, 4, 5, 1023, 1027, 4096 * 256 * 4 + 7]            # the last: a second trip of the 4096-block grid-stride loop + tail
SGD_SMALL = SGD_SIZES[:-1]


SGD_PMAX = 4      # |p| <= 4/16: see sgd_case


def _grid16(seed, n, stream, kmax=7):
    return (_ints(seed, n, -kmax, kmax, stream).astype(F64) / 16.0).astype(F32)


def sgd_case(n, seed=0, wide=False):
    """buf and two gradients: integers in [-7, 7] times 2^-4 (fp32); p: integers in [-4, 4] times 2^-4.  Steps: (first, g0),
    (steady, g1), (steady, None).  The grids: d1 2^-8, p1 2^-11, d2 and b2 2^-15, p2 2^-18, b3 2^-22, p3 2^-25.  p3 fits fp32's 24
    bits only while |p3| < 1/2; the three steps move p by less than 0.2 (|b| <= 0.47, 0.71, 0.39, times lr), so |p0| <= 1/4 keeps
    every element exact.  (With |p0| up to 7/16 a few elements per thousand end above 1/2 and round.)
    wide: p spans [-7, 7] times 2^-4 as well, and the case stops after the second step (p2 on the 2^-18 grid, |p2| < 1)."""
    s = 9000 + n % 9973 + seed
    if wide:
        return SimpleNamespace(p=_grid16(s, n, 5), buf=_grid16(s, n, 2), gs=[_grid16(s, n, 3), _grid16(s, n, 4)])
    return SimpleNamespace(p=_grid16(s, n, 1, SGD_PMAX), buf=_grid16(s, n, 2), gs=[_grid16(s, n, 3), _grid16(s, n, 4), None])


def sgd_model(p, g, buf, first, dtype=F64, lr=SGD_LR, mom=SGD_MOM, wd=SGD_WD):
    """torch.optim.SGD (dampening 0, no nesterov) on arrays of `dtype`, one rounding per operation: (p_new, buf_new)."""
    p, buf = p.astype(dtype), buf.astype(dtype)
    g = np.zeros_like(p) if g is None else g.astype(dtype)
    d = g + dtype(wd) * p
    b = d if first else dtype(mom) * buf + d
    return p - dtype(lr) * b, b


def sgd_run(c, dtype=F64):
    """The three steps of a case -> [(p, buf) after each]."""
    p, buf, out = c.p, c.buf, []
    for k, g in enumerate(c.gs):
        p, buf = sgd_model(p, g, buf, k == 0, dtype)
        out.append((p, buf))
    return out


def sgd_random_case(n, seed=3):
    """Non-exact inputs (every product rounds): shows that an element's result does not depend on where the range starts."""
    return SimpleNamespace(p=O.portable_normal(seed, (n,), stream=7).numpy(), buf=np.zeros(n, dtype=F32),
                           gs=[O.portable_normal(seed, (n,), stream=8 + k, std=0.37).numpy() for k in range(2)])


HEAD_D, HEAD_C = 70, 3                 # C * D = 210: the bias starts 8 bytes off a 16-byte boundary


def head_case():
    """SharedHead(70, 3) on the 2^-4 grid: weight, bias and three steps of gradients (None = that parameter's .grad is None)."""
    mk = lambda shape, st, kmax=7: torch.from_numpy(_grid16(77, int(np.prod(shape)), st, kmax)).view(shape)
    W, b = mk((HEAD_C, HEAD_D), 1, SGD_PMAX), mk((HEAD_C,), 2, SGD_PMAX)
    steps = [(mk(W.shape, 3), None), (mk(W.shape, 4), mk(b.shape, 5)), (None, mk(b.shape, 6))]
    return W, b, steps


def head_run(dtype=torch.float64):
    """O.sgd_step per parameter under torch's rule (a parameter whose .grad is None is skipped; its first step comes later)."""
    W, b, steps = head_case()
    st = {"weight": [W.to(dtype), None], "bias": [b.to(dtype), None]}
    out = []
    for gW, gb in steps:
        for name, g in (("weight", gW), ("bias", gb)):
            if g is not None:
                st[name] = list(O.sgd_step(st[name][0], g.to(dtype), st[name][1], SGD_LR, SGD_MOM, SGD_WD))
        out.append((st["weight"][0].clone(), st["bias"][0].clone()))
    return out


# ---- 4. scale_by_device_scalar, colsum, bn_invstd -----------------------------------------------------------------------------------------
SCALE_SIZES = [0, 1, 255, 2048 * 256 + 3]           # the last crosses the 2048-block cap
SCALE_SCALARS = [0.5, 0.3]
COLSUM_SHAPES = [(1, 1), (70, 255), (5, 256), (70, 257)]
COLSUM_SCALE = 0.25
INVSTD_SIZES = [1, 255, 256, 257, 1000]
INVSTD_EPS = 1e-5


def scale_case(n):
    return O.portable_normal(31, (max(n, 1),), stream=3).numpy()[:n]


def colsum_case(B, D):
    return _ints(40 + B + D, B * D, -7, 7).astype(F32).reshape(B, D)


def invstd_case(n):
    """var log-uniform in [1e-6, 1e3] (fp32) and 1 / sqrt(var + eps) in fp64, eps as the fp32 the ABI carries."""
    u = O.portable_uniform(50 + n, n, 4)
    var = (10.0 ** (u * 9.0 - 6.0)).astype(F32)
    return var, 1.0 / np.sqrt(var.astype(F64) + F64(F32(INVSTD_EPS)))


# ---- 5. GS projection --------------------------------------------------------------------------------------------------------------------
GS_CASES = [(4, 1), (63, 3), (64, 4), (65, 5), (70, 3), (257, 101), (70, 130), (64, 101), (257, 1), (4, 130)]
GS_ALPHA = 1.0
GS_RTOL = 2e-5                         # of max |want|: the project's GS tolerance (tests/test_ops_gpu.py, tests/test_clip_gpu.py)


def gs_ref(Pl, r, G, alpha=GS_ALPHA):
    """utils/utils.py:34-41 on doubles with r and alpha given: (Pl_new, G_new, min |alpha + k_i r_j|)."""
    Pl, r, G = Pl.double(), r.double().view(1, -1), G.double()
    k = Pl @ r.t()
    den = alpha + k @ r
    Pl = Pl - (k @ k.t()) / den
    Pl = Pl / torch.linalg.norm(Pl)
    return Pl, G @ Pl.t(), den.abs().min().item()


@functools.lru_cache(maxsize=None)
def gs_case(D, C):
    """Identity Pl, two feature means with sum r^2 = 0.4 < 0.5 (alpha = 1: every first-call denominator is 1 + r_i r_j >= 0.6), G
    unit normal; the fp64 references of the two consecutive calls (the second starts from a non-identity Pl)."""
    rs = []
    for call in range(2):
        r = O.portable_normal(600 + D + C, (D,), stream=20 + call).double()
        rs.append((r * (0.4 ** 0.5) / r.norm()).float())
    G = O.portable_normal(600 + D + C, (C, D), stream=22)
    Pl1, G1, m1 = gs_ref(torch.eye(D), rs[0], G)
    Pl2, G2, m2 = gs_ref(Pl1.float(), rs[1], G1.float())
    return SimpleNamespace(D=D, C=C, rs=rs, G=G, want=[(Pl1, G1), (Pl2, G2)], min_den=[m1, m2])


# ---- 6. evaluation fusion ------------------------------------------------------------------------------------------------------------------
EVAL_FIXED_SHAPES = [(M, B, C) for M in (2, 3) for B in (1, 255, 256, 257, 600) for C in (2, 6, 101)]
EVAL_ALPHAS = {2: (0.5, 0.5), 3: (0.5, 0.25, 0.25)}
EVAL_DYN_SMALL = [(2, 32, 6), (3, 7, 8), (2, 1, 3), (3, 32, 8)]
EVAL_DYN_STRIDE = [(257, 6), (8, 257), (257, 300)]
EVAL_MARGIN = 1e-4
EVAL_BAD_ROW = 200


def eval_counts(outs, label, weights):
    """main.py:640-676 for one batch on fp64 arrays, arg-max = first maximum (numpy.argmax): counts (2 + M, C) int64.  Rows whose
    label lies outside [0, C) are counted nowhere."""
    outs = [np.asarray(o, dtype=F64) for o in outs]
    C = outs[0].shape[1]
    fused = sum(F64(w) * o for w, o in zip(weights, outs))
    counts = np.zeros((2 + len(outs), C), dtype=np.int64)
    preds = [fused.argmax(1)] + [o.argmax(1) for o in outs]
    for i, lab in enumerate(np.asarray(label)):
        if not 0 <= lab < C:
            continue
        counts[0, lab] += 1
        for k, pr in enumerate(preds):
            counts[1 + k, lab] += int(pr[i] == lab)
    return counts


def entropies(outs):
    """main.py:65-70 on fp64: per modality, - sum p log p with p = softmax over the BATCH axis, summed over the whole tensor."""
    ent = []
    for o in outs:
        lp = torch.log_softmax(torch.as_tensor(o).double(), dim=0)
        ent.append(float(-(lp.exp() * lp).sum()))
    return np.array(ent)


def gating(outs):
    """main.py:72-106 on fp64: (weights, entropies)."""
    ent = entropies(outs)
    w = np.exp(ent.max() - ent)
    return w / w.sum(), ent


def top2_margin(outs, weights):
    """Smallest gap between the largest and the second largest fused logit over the rows (fp64)."""
    fused = sum(F64(w) * np.asarray(o, dtype=F64) for w, o in zip(weights, outs))
    if fused.shape[1] < 2:
        return float("inf")
    top = np.sort(fused, axis=1)
    return float((top[:, -1] - top[:, -2]).min())


def eval_fixed_case(M, B, C):
    """Integer logits in [-3, 3] (with C = 101 nearly every row's maximum is tied; alphas 0.5 / 0.25 keep the fused values exact),
    plus forced ties: row 0 is constant in every modality (arg-max 0), and modality 0 of row B // 2 equals its own maximum at the
    last class too."""
    seed = 7000 + 100 * M + B + C
    outs = [_ints(seed + m, B * C, -3, 3, 60).astype(F32).reshape(B, C) for m in range(M)]
    for o in outs:
        o[0, :] = 2.0
    outs[0][B // 2, C - 1] = outs[0][B // 2].max()
    return outs, O.portable_labels(seed, B, C).numpy()


def eval_small_case(M, B, C):
    outs = [O.portable_normal(7500 + 10 * B + C + m, (B, C), stream=61, std=1.5).numpy() for m in range(M)]
    return outs, O.portable_labels(7500 + B + C, B, C).numpy()


# strength of the peaked part per stride-crossing shape: keeps the fp64 weights inside (0.05, 0.95)
_PEAK = {(257, 6): 4.0, (8, 257): 3.0, (257, 300): 2.0}


def eval_stride_case(B, C):
    """Two modalities.  Modality 1 is modality 0 with every column's rows permuted: the entropy over the batch axis does not change.
    Only the part behind the 256-thread stride differs -- the columns c >= 256, or for C < 256 the rows r >= 256 -- where modality 0
    is peaked and modality 1 flat: the whole entropy difference sits where a kernel that stops at the stride never looks."""
    seed = 8000 + B + C
    a = O.portable_normal(seed, (B, C), stream=62).numpy().astype(F32)
    b = a.copy()
    rows = B if C > 256 else 256                      # rows taking part in the permutation
    for c in range(C):
        perm = np.argsort(O.portable_uniform(seed + 1, rows, 100 + c), kind="stable")
        b[:rows, c] = a[perm, c]
    t = F32(_PEAK[(B, C)])
    if C > 256:
        a[:, 256:] = 0.0
        b[:, 256:] = 0.0
        a[0, 256:] = t                                # one row holds most of the column's mass
    else:
        a[256:, :] = t                                # the rows behind the stride hold most of every column's mass
        b[256:, :] = 0.0
    label = O.portable_labels(seed, B, C).numpy()
    return [a, b], label


def dent_tol(B, ent):
    """Worst case of the kernel's serial fp32 sums: B terms per column, 256 + a few per modality, twice (both modalities)."""
    return 2 * (B + 264) * 2.0 ** -24 * float(np.max(ent))


def dent_of(weights):
    """Entropy differences to the lowest-entropy modality, recovered from the weights: -ln(w_m / w_max)."""
    w = np.asarray(weights, dtype=F64)
    return -np.log(w / w.max())
