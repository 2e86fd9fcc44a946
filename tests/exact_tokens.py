"""Case tables and input builders for the token-path kernels of csrc/transformer.hip: the embedding gradient, the strided batched
GEMM, the masked softmax, the LayerNorm forward, token assembly and patchify (test_tokens_exact_cpu.py proves the tables and the
inputs, test_tokens_exact_gpu.py runs the kernels).

Where the operation allows it the inputs are exactly summable (tests/exact.py): small integers or multiples of a power of two
whose sums stay below 2^24 units, so a correct kernel returns the int64 / fp64 result bit for bit whatever its summation order.
Each case is sized by the regime it proves, not by a workload."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from exact import SUM_BUDGET, assert_bitwise, assert_sum_budget, case_seed, rand_ints  # noqa: F401  (re-exported to the tests)

# ======================================================================================================================================
# 1. Embedding gradient
# ======================================================================================================================================
EMB_CHUNK, EMB_BLK = 16384, 32            # csrc/transformer.hip
EMB_INVALID = -1                          # census id of a position the sort pushed to the end (key 0xFFFFFFFF)
EMB_D = (4, 252, 256, 516, 768, 1024)     # D / 4 = 1, 63, 64, 129, 192, 256: each of the four float4 slots of a lane once partly, once fully used
EMB_N_EDGES = (1, 31, 32, 33, 63, 64, 65)


def _fill(total, first_id, pattern, step=1):
    """Runs (id, length) with increasing ids and lengths cycling through `pattern` until exactly `total` tokens are used."""
    runs, i, nid = [], 0, first_id
    while total > 0:
        ln = min(pattern[i % len(pattern)], total)
        runs.append((nid, ln))
        total -= ln
        nid += step
        i += 1
    return runs


def _regime_runs():
    """One chunk of 12 x 256 = 3072 tokens (npos = 4096) whose sorted key sequence is laid out by hand; positions in brackets.
    block 0: A [0, 10) closed; B [10, 101) open to the right, whole blocks 1 and 2, ends in block 3 at 5
    block 3: B's tail, C [101, 128) ends at position 31 and block 4 begins another id
    blocks 4-6: D [128, 224) = three whole blocks: starts a segment, middle, ends it (block 7 begins E)
    block 7: E [224, 244) closed, F [244, 264) open to the right
    block 8: F's tail [256, 264) open to the left, G [264, 274) closed, H [274, 292) open to the right: both partial slots live
    block 9: H's tail, then PAD [292, 2435): 28 + 66 whole blocks + 3
    then 600 single tokens and 37 ids out of range: the last valid position is 3034 (mid-block), blocks 95 ... 127 hold no valid id."""
    lens = [10, 91, 27, 96, 20, 20, 10, 18, 28 + 66 * 32 + 3]
    runs = [(3 + 2 * i, ln) for i, ln in enumerate(lens)]           # odd ids 3 ... 19: the even rows in between get no gradient
    runs += [(40 + i, 1) for i in range(600)]
    assert sum(ln for _, ln in runs) == 3072 - 37
    return runs, 37


def _emb_specs():
    """name -> (B, L, D, V, [per chunk: (runs, number of out-of-range ids)]).  Runs have distinct increasing ids within a chunk."""
    specs = {}
    rr, bad = _regime_runs()
    specs["regimes"] = (12, 256, 768, 700, [(rr, bad)])
    for i, n in enumerate(EMB_N_EDGES):                               # n tokens in one sequence: npos = 64, or 128 for n = 65
        if n == 64:
            runs = [(2, 10), (5, 54)]                                 # n == npos: the second run is open to the left and fills the last block
        else:
            runs = _fill(n - (1 if n > 2 else 0), 1, (max(1, n // 3), 1, 2, 40), step=2)
        specs[f"n{n}"] = (1, n, EMB_D[i % len(EMB_D)], 200, [(runs, n - sum(ln for _, ln in runs))])
    # n == npos again, but the run that reaches the chunk's end starts inside the last block: it goes straight to dtable and the combine
    # must leave that block alone whatever lies behind the sorted keys in the workspace
    specs["n64b"] = (1, 64, 64, 200, [([(2, 40), (5, 24)], 0)])
    for D in EMB_D:                                                   # every D on a case that uses both partial slots and the combine
        specs[f"d{D}"] = (2, 100, D, 64, [([(1, 5), (4, 40), (6, 70), (9, 33)] + _fill(49, 11, (1, 2, 3)), 3)])
    pat = (1, 2, 3, 31, 32, 33, 64, 65, 5, 96, 7, 130)
    # two chunks at L = 256: 64 sequences (n == npos == 16384) + 1 sequence (npos = 256); id 0 is [PAD]-like and occurs in both
    specs["chunks"] = (65, 256, 64, 3000, [([(0, 5000)] + _fill(16384 - 5000, 1, pat), 0), ([(0, 100)] + _fill(150, 7, (3, 40, 1)), 6)])
    # L = 77 does not divide 16384: 212 sequences = 16324 tokens (60 invalid tail positions) + 1 sequence of 77 tokens (npos = 128)
    specs["l77"] = (213, 77, 64, 3000, [([(0, 3000)] + _fill(16324 - 3000 - 9, 2, pat), 9), ([(0, 30), (5, 40)] + _fill(5, 9, (1,)), 2)])
    # the largest V the packed key allows, in a full chunk: the key of (V - 1, r = 16383) is 2^32 - 16385
    V = 262143
    head = _fill(16384 - 40 - 7, 0, pat, step=431)
    assert head[-1][0] < V - 2
    specs["vmax"] = (64, 256, 4, V, [(head + [(V - 2, 7), (V - 1, 40)], 0)])
    return specs


EMB_SPECS = _emb_specs()
EMB_CASES = list(EMB_SPECS)


def emb_ids(name):
    """ids (B, L) int64 of a case: each chunk's runs (in key order) scattered to the chunk's token positions by a seeded permutation;
    out-of-range tokens alternate between -1 and V.  'vmax' additionally puts a token of id V - 1 on the chunk's last position."""
    B, L, D, V, chunks = EMB_SPECS[name]
    rpc = EMB_CHUNK // L
    out = torch.empty(B * L, dtype=torch.int64)
    for c, (runs, bad) in enumerate(chunks):
        b0 = c * rpc
        n = min(rpc, B - b0) * L
        ids = [i for i, ln in runs for _ in range(ln)] + [(-1 if k % 2 == 0 else V) for k in range(bad)]
        assert len(ids) == n, f"{name}: chunk {c} describes {len(ids)} tokens, not {n}"
        assert all(a[0] < b[0] for a, b in zip(runs, runs[1:])) and 0 <= runs[0][0] and runs[-1][0] < V
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(case_seed(len(name), B, L, D, c)))
        chunk = torch.empty(n, dtype=torch.int64)
        chunk[perm] = torch.tensor(ids, dtype=torch.int64)
        if name == "vmax":
            j = int(torch.nonzero(chunk == V - 1)[0])
            chunk[j], chunk[n - 1] = chunk[n - 1].item(), V - 1
        out[b0 * L:b0 * L + n] = chunk
    assert len(chunks) == -(-B // rpc)
    return out.view(B, L)


def emb_census(ids, L, V):
    """Replays mla_tokens_assemble_bwd's host loop and what emb_segment_kernel / emb_combine_kernel do with every block of 32 sorted
    positions.  Returns one record per chunk: b0, nb, n, npos, sh, max_key, runs (the (id, length) runs of the valid sorted keys) and
    blocks, a list with the set of regimes of each block:
      a  a run closed inside the block (added straight to dtable)        b  a run starting mid-block, open to the right (part[w][1])
      c  a run open to the left that ends mid-block (part[w][0])         d  a whole-block run in the middle of a segment
      e  a whole-block run that starts a segment (slot 0)                f  a whole-block run that ends a segment, next block another id
      g  a closed run ending at position 31, next block another id       h  first run open to the left AND last run open to the right
      i  the last block of the chunk is a whole-block run open to the left (n == npos)
      j  a valid -> invalid transition inside the block                   J  a block without any valid position
      k  a run that starts here and touches at least 66 blocks
      L  the chunk's last position is valid (n == npos) and its run started inside the last block: closed, nothing to combine"""
    ids = torch.as_tensor(ids).reshape(-1, L)
    B = ids.shape[0]
    rpc = EMB_CHUNK // L
    out = []
    for b0 in range(0, B, rpc):
        nb = min(rpc, B - b0)
        n = nb * L
        npos, sh = 64, 6
        while npos < n:
            npos <<= 1
            sh += 1
        flat = ids[b0:b0 + nb].reshape(-1).numpy().astype(np.int64)
        ok = (flat >= 0) & (flat < V)
        keys = np.full(npos, 0xFFFFFFFF, dtype=np.int64)
        keys[:n][ok] = flat[ok] * npos + np.arange(n)[ok]
        assert keys[:n][ok].size == 0 or keys[:n][ok].max() < 0xFFFFFFFF, "a valid key collides with the invalid marker"
        max_key = int(keys[:n][ok].max()) if ok.any() else -1
        keys.sort()
        sid = np.where(keys == 0xFFFFFFFF, EMB_INVALID, keys >> sh)
        # runs over the whole chunk
        runs, start = [], 0
        for p in range(1, npos + 1):
            if p == npos or sid[p] != sid[start]:
                if sid[start] != EMB_INVALID:
                    runs.append((int(sid[start]), p - start, start))
                start = p
        long_starts = {s // EMB_BLK for _, ln, s in runs if (s + ln - 1) // EMB_BLK - s // EMB_BLK + 1 >= 66}
        blocks = []
        for w in range(npos // EMB_BLK):
            p0 = w * EMB_BLK
            blk = sid[p0:p0 + EMB_BLK]
            left = sid[p0 - 1] if p0 > 0 else -2
            right = sid[p0 + EMB_BLK] if p0 + EMB_BLK < npos else -2
            reg, s, slots = set(), 0, set()
            for e in range(1, EMB_BLK + 1):
                if e < EMB_BLK and blk[e] == blk[s]:
                    continue
                cur = blk[s]
                if cur != EMB_INVALID:
                    open_l, open_r = s == 0 and left == cur, e == EMB_BLK and right == cur
                    whole = s == 0 and e == EMB_BLK
                    other_next = right not in (cur, EMB_INVALID, -2)
                    if not open_l and not open_r:
                        reg.add("a")
                        if e == EMB_BLK and other_next:
                            reg.add("g")
                    elif whole:
                        reg.add("d" if open_l and open_r else "e" if open_r else "f" if other_next else "c")
                        if open_l and not open_r and p0 + EMB_BLK == npos:
                            reg.add("i")
                    elif open_r:
                        reg.add("b")
                        slots.add(1)
                    else:
                        reg.add("c")
                        slots.add(0)
                s = e
            if slots == {0, 1}:
                reg.add("h")
            if blk[0] != EMB_INVALID and blk[-1] == EMB_INVALID:
                reg.add("j")
            if blk[0] == EMB_INVALID:
                reg.add("J")
            if w in long_starts:
                reg.add("k")
            if p0 + EMB_BLK == npos and blk[-1] != EMB_INVALID and blk[0] != blk[-1]:
                reg.add("L")
            blocks.append(reg)
        out.append(SimpleNamespace(b0=b0, nb=nb, n=n, npos=npos, sh=sh, max_key=max_key, runs=[(i, ln) for i, ln, _ in runs], blocks=blocks))
    return out


def emb_case_build(name):
    """ids, integer dx0 (|v| <= 7, the [cls] rows included), an integer dtable prefill (|v| <= 3) and the int64 references.  The budget
    7 * (tokens of the most frequent id over all chunks) + 3 < 2^24 is asserted here, before anything could be launched."""
    B, L, D, V, _ = EMB_SPECS[name]
    seed = case_seed(len(name), B, L, D, V)
    ids = emb_ids(name)
    ok = (ids >= 0) & (ids < V)
    most = int(torch.bincount(ids[ok]).max())
    assert_sum_budget(torch.tensor(7 * most + 3), f"embedding gradient {name}")
    assert_sum_budget(torch.tensor(7 * B * (L + 1)), f"column totals {name}")
    dx0 = rand_ints((B, L + 1, D), -7, 7, seed, dtype=torch.int32)
    pre = rand_ints((V, D), -3, 3, seed + 1, dtype=torch.int32)
    dtable = pre.long().index_add_(0, ids[ok], dx0[:, 1:][ok].long())
    dcls = dx0[:, 0].long().sum(0)
    tot = dx0.long().sum((0, 1))
    touched = torch.zeros(V, dtype=torch.bool)
    touched[ids[ok]] = True
    return SimpleNamespace(name=name, B=B, L=L, D=D, V=V, ids=ids, dx0=dx0.float(), prefill=pre.float(), dtable=dtable.float(),
                           dcls=dcls.float(), tot=tot.float(), dtype=(tot - dcls).float(), touched=touched, most=most)


def emb_stale_key(ids, L, V):
    """A 32-bit word for the workspace's sorted-key area that a kernel reading behind its npos keys would take for a continuation of
    the last chunk's last run: that run's id in the key's id field (id 0 where the chunk ends with invalid positions)."""
    last = emb_census(ids, L, V)[-1]
    tail_valid = "J" not in last.blocks[-1] and "j" not in last.blocks[-1]
    return ((last.runs[-1][0] if tail_valid else 0) << last.sh) & 0xFFFFFFFF


@functools.lru_cache(maxsize=1)
def emb_case(name):
    return emb_case_build(name)


# ======================================================================================================================================
# 2. bgemm: class D operands, every instantiation, ragged and aligned shapes, generic strides, offsets, windows
# ======================================================================================================================================
BGEMM_K = (1, 31, 32, 33, 63, 64, 65, 96)
BGEMM_MN = (1, 31, 32, 33, 63, 64, 65, 129)
BGEMM_BH = ((1, 1), (1, 5), (3, 1), (2, 3))
# (layout of A, layout of B, M, N, K, B, H, alpha, option)
#   A: 'k' k-contiguous (a_k = 1) | 'i' i-contiguous (a_i = 1) | 'g' no unit stride (a_i = 3 K, a_k = 3)
#   B: 'j' j-contiguous (b_j = 1) | 'k' k-contiguous (b_k = 1) | 'g' no unit stride (b_k = 3 N, b_j = 3)
#   option: 'bh0' B shared by the heads (b_h = 0) | 'ab0' A shared by the batches (a_b = 0) | 'ct' transposed output (c_i = 1, c_j = M')
BGEMM_CASES = [
    ("k", "j", 64, 64, 64, 1, 1, 1.0, ""), ("k", "k", 64, 64, 32, 1, 1, 0.125, ""),            # aligned: whole tiles, whole K steps
    ("i", "j", 64, 128, 64, 1, 1, 1.0, ""), ("i", "k", 128, 64, 96, 1, 1, 0.125, ""),
    ("k", "j", 1, 129, 1, 1, 5, 1.0, ""), ("k", "k", 129, 1, 31, 3, 1, 0.125, ""),
    ("i", "j", 31, 33, 33, 2, 3, 0.125, ""), ("i", "k", 33, 31, 63, 2, 3, 1.0, ""),
    ("k", "j", 63, 65, 65, 1, 1, 0.125, ""), ("k", "k", 65, 63, 96, 1, 5, 1.0, ""),
    ("i", "j", 129, 32, 1, 3, 1, 1.0, ""), ("i", "k", 32, 129, 31, 1, 1, 0.125, ""),
    ("i", "k", 1, 129, 65, 1, 5, 1.0, ""), ("i", "k", 129, 1, 33, 3, 1, 0.125, ""),
    ("i", "k", 63, 65, 64, 2, 3, 1.0, ""), ("i", "k", 65, 33, 1, 1, 1, 0.125, ""),
    ("i", "k", 31, 63, 32, 1, 1, 1.0, ""), ("k", "k", 32, 64, 63, 1, 1, 1.0, ""),
    ("i", "j", 64, 31, 96, 1, 5, 0.125, ""), ("k", "j", 33, 32, 32, 2, 3, 1.0, ""),
    ("g", "j", 33, 65, 33, 2, 3, 1.0, ""), ("k", "g", 65, 33, 65, 1, 5, 0.125, ""),            # generic strides: the default maps
    ("g", "g", 31, 63, 63, 3, 1, 1.0, ""), ("i", "g", 63, 31, 64, 1, 1, 1.0, ""), ("g", "k", 32, 65, 31, 1, 1, 0.125, ""),
    ("i", "k", 33, 65, 33, 2, 3, 1.0, "bh0"), ("i", "k", 65, 31, 65, 2, 3, 0.125, "ab0"), ("k", "j", 31, 129, 64, 2, 3, 1.0, "ab0"),
    ("i", "k", 63, 33, 65, 2, 3, 0.125, "ct"), ("k", "j", 129, 65, 32, 1, 5, 1.0, "ct"),
]
BGEMM_OFFS = (3, 5, 7)                    # a_off, b_off, c_off in elements


def bgemm_instantiation(sa, sb):
    """mla_bgemm's selection rule recomputed from the stride tables: (AK, BJ)."""
    return (sa[3] == 1 or sa[2] != 1), (sb[3] == 1 or sb[2] != 1)


def bgemm_strides(case):
    """((a_b, a_h, a_i, a_k), (b_b, b_h, b_k, b_j), (c_b, c_h, c_i, c_j), element counts of the three buffers).  Rows are padded, the
    head and batch strides are larger than the matrices and differ from each other, so that every stride is distinguishable."""
    al, bl, M, N, K, B, H, alpha, opt = case

    def mat(R, C, generic=False):            # R rows of C elements -> (row stride, element stride, footprint in elements)
        if generic:
            return 3 * C, 3, 3 * C * (R - 1) + 3 * (C - 1) + 1
        return C + 2, 1, (C + 2) * (R - 1) + C
    if al == "i":
        a_k, a_i, fa = mat(K, M)
    else:
        a_i, a_k, fa = mat(M, K, al == "g")
    if bl == "k":
        b_j, b_k, fb = mat(N, K)
    else:
        b_k, b_j, fb = mat(K, N, bl == "g")
    if opt == "ct":
        c_j, c_i, fc = mat(N, M)
    else:
        c_i, c_j, fc = mat(M, N)
    a_h, b_h, c_h = fa + 5, fb + 9, fc + 3
    a_b, b_b, c_b = H * a_h + 11, H * b_h + 13, H * c_h + 7
    if opt == "bh0":
        b_h, b_b = 0, fb + 13
    if opt == "ab0":
        a_b = 0
    sa, sb, sc = (a_b, a_h, a_i, a_k), (b_b, b_h, b_k, b_j), (c_b, c_h, c_i, c_j)
    ext = lambda s, f, off: off + (B - 1) * s[0] + (H - 1) * s[1] + f + 17
    return sa, sb, sc, (ext(sa, fa, BGEMM_OFFS[0]), ext(sb, fb, BGEMM_OFFS[1]), ext(sc, fc, BGEMM_OFFS[2]))


def bgemm_case(case):
    """Integer buffers (|v| <= 7, the gaps between the matrices included), the strided views and the exact result: want is the whole C
    buffer, NaN outside the window, and window marks the cells the kernel must write."""
    al, bl, M, N, K, B, H, alpha, opt = case
    assert 49 * K < SUM_BUDGET
    sa, sb, sc, (na, nb, nc) = bgemm_strides(case)
    seed = case_seed(M, N, K, B, H, len(opt), ord(al), ord(bl))
    A, Bm = rand_ints((na,), -7, 7, seed).float(), rand_ints((nb,), -7, 7, seed + 1).float()
    Av = torch.as_strided(A, (B, H, M, K), sa, BGEMM_OFFS[0])
    Bv = torch.as_strided(Bm, (B, H, K, N), sb, BGEMM_OFFS[1])
    ref = (Av.long() @ Bv.long()).double() * alpha
    assert torch.equal(ref, Av.double() @ Bv.double() * alpha) and torch.equal(ref.float().double(), ref)
    want, window = torch.full((nc,), float("nan")), torch.zeros(nc, dtype=torch.bool)
    torch.as_strided(want, (B, H, M, N), sc, BGEMM_OFFS[2]).copy_(ref.float())
    torch.as_strided(window, (B, H, M, N), sc, BGEMM_OFFS[2]).fill_(True)
    assert int(window.sum()) == B * H * M * N, "the C windows of different (b, h) must not overlap"
    return SimpleNamespace(A=A, B=Bm, sa=sa, sb=sb, sc=sc, nc=nc, want=want, window=window, ref=ref, Av=Av, Bv=Bv, alpha=alpha,
                           dims=(B, H, M, N, K))


# ======================================================================================================================================
# 3. Softmax
# ======================================================================================================================================
SOFTMAX_N = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024)
SOFTMAX_BH = {1: (1, 3), 2: (3, 1), 63: (1, 1), 64: (1, 2), 65: (1, 3), 127: (1, 1), 128: (2, 1), 129: (1, 1), 1023: (1, 1), 1024: (1, 2)}
SOFTMAX_GUARD = 64
SOFTMAX_FAMILIES = ("normal", "wide", "equal", "spike", "low")
SOFTMAX_FWD_CASES = [(n, "normal", m) for n in SOFTMAX_N for m in (False, True)] + \
                    [(n, fam, m) for n in (65, 1024) for fam in SOFTMAX_FAMILIES[1:] for m in (False, True)]
SOFTMAX_FWD_BH = (2, 3)                   # B = 2 batch elements with different masks, H = 3: B * H * n is odd for odd n


def softmax_bwd_case(n):
    """P = multiples of 1/64 in [0, 1], dP = integers |g| <= 7: sum P g is exact in any order (7 n 64 < 2^24), g - dot is exact, and
    P (g - dot) is ONE rounding of an exact product: the result is float32(fp64 formula) bit for bit."""
    B, H = SOFTMAX_BH[n]
    seed = case_seed(n, B, H)
    assert_sum_budget(torch.tensor(7 * n * 64 + 7 * 64), f"softmax backward n={n}")
    P = (rand_ints((B, H, n, n), 0, 64, seed).double() / 64).float()
    g = rand_ints((B, H, n, n), -7, 7, seed + 1).float()
    dot = (P.double() * g.double()).sum(-1, keepdim=True)
    want = (P.double() * (g.double() - dot)).float()
    return SimpleNamespace(B=B, H=H, n=n, P=P, g=g, want=want)


def softmax_scores(n, family, seed, B=SOFTMAX_FWD_BH[0], H=SOFTMAX_FWD_BH[1]):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn((B, H, n, n), generator=g)
    if family == "wide":
        s = s * 30.0
    elif family == "equal":
        s = torch.full((B, H, n, n), 1.25)
    elif family == "spike":
        j = torch.randint(0, n, (B, H, n, 1), generator=g)
        s = s.scatter_add(-1, j, torch.full((B, H, n, 1), 1e4))
    elif family == "low":
        s = torch.rand((B, H, n, n), generator=g) - 1e4
    else:
        assert family == "normal"
    return s.float()


def softmax_mask(n, B=SOFTMAX_FWD_BH[0]):
    """(B, n) mask values: > 0 is masked (1.0 and 0.5), 0 and -1 are not.  Batch 0 masks a tail, batch 1 every other column from 1 on;
    column 0 always stays (so n = 1 masks nothing)."""
    pm = torch.zeros((B, n))
    pm[:, ::3] = -1.0
    t = max(1, n // 3) if n > 1 else 0
    if t:
        pm[0, n - t:] = 1.0
        pm[0, n - t::2] = 0.5
    pm[1:, 1::2] = 1.0
    pm[1:, 3::4] = 0.5
    pm[:, 0] = -1.0 if n % 2 else 0.0
    return pm


def softmax_ref(s, pm):
    """fp64 softmax of the same fp32 scores, masked like the kernel (pm > 0 -> -1e7)."""
    s = s.double()
    if pm is not None:
        s = torch.where(pm[:, None, None, :].expand(s.shape) > 0, torch.tensor(-1e7, dtype=torch.float64), s)
    return torch.softmax(s, dim=-1)


def softmax_tol(ref):
    return 2e-6 + 1e-5 * ref.abs().max().item()              # test_attention_pieces: atol 2e-6, rtol 1e-5 of max|ref|


# ======================================================================================================================================
# 4. LayerNorm forward
# ======================================================================================================================================
LNF_D = (512, 768, 1024)
LNF_M = (1, 2, 3, 4, 5, 17)
LNF_FAMILIES = ((0.3, 1.7), (1000.0, 1.0), (0.0, 1e-3), (-50.0, 20.0))
LNF_CASES = [(D, M, f) for D in LNF_D for M in LNF_M for f in range(len(LNF_FAMILIES))]
LN_EPS32 = torch.tensor(1e-5, dtype=torch.float32).double().item()
U24 = 2.0 ** -24


def lnf_case(D, M, fam):
    mean, std = LNF_FAMILIES[fam]
    g = torch.Generator().manual_seed(case_seed(D, M, fam))
    x = (torch.randn((M, D), generator=g, dtype=torch.float64) * std + mean).float()
    w = (torch.randn((D,), generator=g, dtype=torch.float64) * 0.2 + 1.0).float()
    b = (torch.randn((D,), generator=g, dtype=torch.float64) * 0.2).float()
    return SimpleNamespace(M=M, D=D, x=x, w=w, b=b)


def lnf_ref(x, w, b, eps=LN_EPS32):
    """fp64 LayerNorm of the fp32 inputs: y, mean, rstd."""
    xd = x.double()
    mean = xd.mean(1)
    var = ((xd - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (xd - mean[:, None]) * rstd[:, None] * w.double() + b.double(), mean, rstd


def lnf_bounds(x, w, b, y64, rstd64):
    """Error bounds from the kernel's summation depth, PER = D / 64 elements per lane.
    mean: PER sequential adds per lane + 6 butterfly levels + the divide, each relative to a partial sum of magnitude <= sum |x|:
          |mean - mean64| <= (PER + 7) 2^-24 mean|x|  =: mb.
    rstd: the sum of squares has PER + 6 adds of non-negative terms (relative error <= (PER + 6) u, in practice half of it since the
          terms are positive and the errors do not align), each term d * d carries 2 u + the error of mu, the divide, the add of eps, the
          square root and the reciprocal one u each; halved by the square root: |rstd / rstd64 - 1| <= (PER / 2 + 8) u.
          This is a bound for the TWO-PASS form (deviations from the computed mean).  The shift dm of that mean adds dm^2 to the
          variance, at most (mb / std)^2 relative: 8e-7 for mean 1000, std 1 if mb were reached, 1e-8 at the measured dm of 1e-4 --
          the mean's rounding errors do not align, so mb is a worst case never met by an order of magnitude.
    y:    (x - mu) carries mu's error mb (times rstd |w|); the three multiplies, the subtract and rstd's error are relative to
          |y64 - b|: (PER / 2 + 8 + 3) u; the final add rounds once relative to |y64|."""
    PER = x.shape[1] // 64
    mb = (PER + 7) * U24 * x.double().abs().mean(1)
    rb = (PER / 2 + 8) * U24
    yb = mb[:, None] * rstd64[:, None] * w.double().abs() + (PER / 2 + 11) * U24 * (y64 - b.double()).abs() + U24 * y64.abs()
    return mb, rb, yb


LNF_EXACT_K = (-3, 0, 2, 5)


def lnf_const_case(D, M=6):
    """Constant rows of a small integer c: mean == c and y == b bitwise, rstd = 1 / sqrt(eps)."""
    c = torch.tensor([-3.0, -1.0, 0.0, 1.0, 2.0, 7.0])[:M]
    s = lnf_case(D, M, 0)
    s.x = c[:, None].expand(M, D).contiguous()
    s.c = c
    return s


def lnf_pm_case(D):
    """eps = 0, row r = m_r +- 2^k_r, half of the columns each in a seeded order: every partial sum is a small multiple of 2^k (below
    2^24 of them), so mean == m_r bitwise, the variance is 4^k exactly and rstd = 2^-k."""
    M = len(LNF_EXACT_K)
    s = lnf_case(D, M, 0)
    m = torch.tensor([3.0, -2.0, 0.0, 5.0])
    k = torch.tensor(LNF_EXACT_K, dtype=torch.float64)
    sign = torch.ones(M, D, dtype=torch.float64)
    for r in range(M):
        sign[r, torch.randperm(D, generator=torch.Generator().manual_seed(D + r))[:D // 2]] = -1.0
    x = m.double()[:, None] + sign * (2.0 ** k)[:, None]
    assert float((x.abs() / (2.0 ** k)[:, None]).sum(1).max()) < SUM_BUDGET
    s.x, s.m, s.k = x.float(), m, k
    assert torch.equal(s.x.double(), x)
    return s


# ======================================================================================================================================
# 5. Token assembly and patchify
# ======================================================================================================================================
ASM_GRID_CAP, ASM_TPB = 8192, 256
# (B, L, D): every D once small; B = 43 / 44 at L = 256, D = 768 are past the 8192-block cap of the grid (see test_assemble_cases_cross_the_grid_cap)
ASM_CASES = [(3, 5, 4), (2, 7, 768), (2, 7, 1024), (43, 256, 768), (44, 256, 768)]
ASM_GUARD = 256


def grid256(shape, seed, lim=4):
    """Multiples of 2^-8 with |v| < lim."""
    return (rand_ints(shape, -(lim * 256 - 1), lim * 256 - 1, seed).double() / 256).float()


def asm_case(B, L, D):
    """All addends multiples of 2^-8 below 4: table + (pos + type) is exact in either association (|sum| < 12, 2^-8 grid)."""
    seed = case_seed(B, L, D)
    V = 37
    ids = rand_ints((B, L), 0, V - 1, seed)
    ids[0, min(2, L - 1)], ids[B - 1, L - 1] = -1, V                   # out of range: the forward poisons exactly these rows
    return SimpleNamespace(B=B, L=L, D=D, V=V, ids=ids, table=grid256((V, D), seed + 1), pos=grid256((L, D), seed + 2), type=grid256((D,), seed + 3),
                           cls=grid256((D,), seed + 4), lin=grid256((B, L, D), seed + 5))


PATCH_GRID_CAP = 16384
# (B, C, H, W, P, transposed)
PATCH_CASES = [(2, 3, 64, 48, 16, False), (1, 1, 16, 80, 16, False), (3, 3, 48, 16, 16, False), (2, 1, 5, 7, 1, False), (2, 3, 6, 10, 2, False),
               (2, 1, 64, 48, 16, True), (1, 1, 16, 80, 16, True), (3, 1, 6, 2, 2, True), (2, 1, 3, 4, 1, True),
               (1, 3, 1184, 1184, 16, False), (1, 1, 2064, 2048, 16, True)]            # the last two: just past the capped grid's first trip


def patch_image(case):
    B, C, H, W, P, tr = case
    n = B * C * H * W
    img = (torch.arange(n, dtype=torch.float64) % 8191 - 4095).float()                 # a copy kernel: any distinct-looking values will do
    return img.view(B, W, H) if tr else img.view(B, C, H, W)
