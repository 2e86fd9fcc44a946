"""The inputs and case tables of test_tokens_exact_gpu.py (tests/exact_tokens.py), checked without a GPU.

Two kinds of statement.  Conditions on the INPUTS: the 2^24 budgets hold, the int64 references equal fp64 / fp32 evaluations in more
than one order, and the bounds that are not bitwise are met by torch's own CPU fp32 kernels on every case.  Conditions on the TABLES: a
census replays the host-side chunking and the per-block decisions of the embedding-gradient kernels and must find every regime; the
bgemm table must reach every instantiation, edge size and stride pattern.  Removing a case from a table makes one of these fail."""
import pytest
import torch
import torch.nn.functional as F

import exact_tokens as T


# ---- 1. embedding gradient ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def census():
    return {name: T.emb_census(T.emb_ids(name), T.EMB_SPECS[name][1], T.EMB_SPECS[name][3]) for name in T.EMB_CASES}


def test_embedding_kernels_see_the_chosen_runs(census):
    """The sort key is id * npos + r: whatever the permutation, the sorted sequence consists of exactly the run lengths of the table."""
    for name in T.EMB_CASES:
        B, L, D, V, chunks = T.EMB_SPECS[name]
        assert len(census[name]) == len(chunks)
        for rec, (runs, bad) in zip(census[name], chunks):
            assert rec.runs == runs, f"{name}: the sorted keys do not form the runs of the table"
            assert rec.n - sum(ln for _, ln in runs) == bad and rec.npos >= max(rec.n, 64) and rec.npos == 1 << rec.sh
            assert rec.npos == 64 or rec.npos < 2 * rec.n


def test_embedding_census_finds_every_block_regime(census):
    union = set().union(*(reg for recs in census.values() for rec in recs for reg in rec.blocks))
    assert union >= set("abcdefghijJkL"), f"block regimes never reached: {sorted(set('abcdefghijJkL') - union)}"
    # the hand-laid case alone reaches all of them but (i), which needs n == npos
    reg = census["regimes"][0].blocks
    assert "a" in reg[0] and "b" in reg[0] and reg[1] == {"d"} and reg[2] == {"d"} and {"c", "g"} <= reg[3]
    assert reg[4] == {"e"} and reg[5] == {"d"} and reg[6] == {"f"} and {"a", "b"} <= reg[7] and {"a", "b", "c", "h"} <= reg[8]
    assert {"c", "b", "k"} <= reg[9] and all(r == {"d"} for r in reg[10:76]) and "c" in reg[76]
    assert "j" in reg[94] and all(r == {"J"} for r in reg[95:])
    # (i): a segment that runs to the end of the last block, in a small and in a full chunk
    assert "i" in census["n64"][0].blocks[-1] and census["n64"][0].n == census["n64"][0].npos == 64
    assert "i" in census["vmax"][0].blocks[-1] and census["vmax"][0].n == census["vmax"][0].npos == T.EMB_CHUNK
    # n == npos with a closed run at the very end: the stale-workspace word continues that run's id
    rec = census["n64b"][0]
    assert rec.blocks[-1] == {"c", "a", "L"} and rec.n == rec.npos and T.emb_stale_key(T.emb_ids("n64b"), 64, 200) >> rec.sh == rec.runs[-1][0] == 5
    assert T.emb_stale_key(T.emb_ids("vmax"), 256, 262143) >> 14 == 262142 and T.emb_stale_key(T.emb_ids("chunks"), 256, 3000) == 0
    # every D runs a case that uses both partial slots of one block and the combine
    for D in T.EMB_D:
        u = set().union(*census[f"d{D}"][0].blocks)
        assert u >= set("abcdh") and T.EMB_SPECS[f"d{D}"][2] == D


def test_embedding_cases_reach_every_host_regime(census):
    # (l) n on both sides of one and two blocks and of the 64-position minimum
    assert {census[f"n{n}"][0].n for n in T.EMB_N_EDGES} == set(T.EMB_N_EDGES)
    assert [census[f"n{n}"][0].npos for n in T.EMB_N_EDGES] == [64] * 6 + [128]
    # (m) two chunks, the second shorter with another npos, one id in both
    a, b = census["chunks"]
    assert T.EMB_SPECS["chunks"][:3] == (65, 256, 64) and a.n == a.npos == T.EMB_CHUNK and b.n == 256 == b.npos and a.sh != b.sh
    assert a.runs[0][0] == b.runs[0][0] == 0 and a.runs[0][1] >= 66 * 32
    # (n) L does not divide the chunk
    a, b = census["l77"]
    assert T.EMB_CHUNK % 77 and (a.nb, a.n, a.npos - a.n) == (212, 16324, 60) and (b.nb, b.n, b.npos) == (1, 77, 128)
    assert a.runs[0][0] == b.runs[0][0]
    # (o) ids -1 and V occur; some rows of dtable belong to no valid id
    for name in ("regimes", "l77", "chunks", "d4", "d1024"):
        ids, V = T.emb_ids(name), T.EMB_SPECS[name][3]
        assert (ids == -1).any() and (ids == V).any()
        assert not T.emb_case_build(name).touched.all()
    # (p) the largest V: (V + 1) * 16384 would overflow the packed key, and the largest key used is within 16384 of 2^32
    V = T.EMB_SPECS["vmax"][3]
    assert V == 262143 and V * T.EMB_CHUNK <= 2 ** 32 - 1 < (V + 1) * T.EMB_CHUNK
    assert T.EMB_SPECS["vmax"][:3] == (64, 256, 4) and 2 ** 32 - 16385 <= census["vmax"][0].max_key < 0xFFFFFFFF
    # (q) every D / 4: 1, 63, 64, 129, 192, 256
    assert sorted({T.EMB_SPECS[n][2] // 4 for n in T.EMB_CASES} & {1, 63, 64, 129, 192, 256}) == [1, 63, 64, 129, 192, 256]


@pytest.mark.parametrize("name", T.EMB_CASES)
def test_embedding_inputs_are_exactly_summable(name):
    c = T.emb_case_build(name)                                          # asserts the budgets
    assert c.dx0.abs().max() <= 7 and c.prefill.abs().max() <= 3 and (c.prefill != 0).any()
    assert 7 * c.most + 3 < T.SUM_BUDGET
    ok = (c.ids >= 0) & (c.ids < c.V)
    # fp32 index_add_ in two token orders gives the int64 result: the reference does not depend on the order
    rows, idx = c.dx0[:, 1:][ok], c.ids[ok]
    perm = torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(1))
    for p in (torch.arange(idx.numel()), perm):
        assert torch.equal(c.prefill.clone().index_add_(0, idx[p], rows[p]), c.dtable)
    assert torch.equal(c.dtable[~c.touched], c.prefill[~c.touched])
    assert torch.equal(c.dx0.sum((0, 1)), c.tot) and torch.equal(c.dx0.flip(0).sum((1, 0)), c.tot)
    assert torch.equal(c.tot - c.dcls, c.dtype) and torch.equal(c.dx0[:, 1:].double().sum((0, 1)).float(), c.dtype)


# ---- 2. bgemm -----------------------------------------------------------------------------------------------------------------------------
def test_bgemm_table_covers_the_cross_product():
    cases = T.BGEMM_CASES
    assert len(cases) == len(set(cases)) and 24 <= len(cases) <= 48
    inst = {}
    for c in cases:
        al, bl, M, N, K, B, H, alpha, opt = c
        sa, sb, sc, _ = T.bgemm_strides(c)
        ak, bj = T.bgemm_instantiation(sa, sb)
        # the rule sends k-contiguous and generic A to AK, i-contiguous A to !AK; likewise B
        assert ak == (al != "i") and bj == (bl != "k"), c
        assert (sa[3] == 1) == (al == "k") and (sa[2] == 1) == (al == "i") and (sb[3] == 1) == (bl == "j") and (sb[2] == 1) == (bl == "k")
        if al == "g":
            assert sa[2:] == (3 * K, 3)
        if bl == "g":
            assert sb[2:] == (3 * N, 3)
        aligned = M % 64 == 0 and N % 64 == 0 and K % 32 == 0
        inst.setdefault((ak, bj), set()).add(aligned)
        assert all(s[0] != s[1] for s in (sa, sb, sc)) and len({sa[:2], sb[:2], sc[:2]}) == 3, "batch and head strides must differ"
        assert all(s[1] > 0 and s[0] > s[1] * (H - 1) for s in (sa, sb, sc)) or opt in ("bh0", "ab0")
        assert 49 * K < T.SUM_BUDGET and alpha in (1.0, 0.125)
    assert inst == {(a, b): {True, False} for a in (True, False) for b in (True, False)}, "each instantiation: one aligned and one ragged shape"
    assert {c[4] for c in cases} == set(T.BGEMM_K)
    assert {c[2] for c in cases} - {128} == set(T.BGEMM_MN) == {c[3] for c in cases} - {128}       # 128: two whole tiles, aligned cases only
    assert any(c[2:4] == (1, 129) for c in cases) and any(c[2:4] == (129, 1) for c in cases)
    assert {c[5:7] for c in cases} == set(T.BGEMM_BH) and {c[7] for c in cases} == {1.0, 0.125}
    # the instantiation no caller uses sees every K and every (B, H)
    ff = [c for c in cases if c[0] == "i" and c[1] == "k"]
    assert {c[4] for c in ff} == set(T.BGEMM_K) and {c[5:7] for c in ff} == set(T.BGEMM_BH)
    # K steps: no prefetch (K <= 32), prefetch with a ragged last step, with a whole last step, more than two steps
    assert {1, 31, 32} <= {c[4] for c in cases} and any(c[4] > 64 for c in cases)
    kinds = {(c[0] == "g", c[1] == "g") for c in cases}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    assert {c[8] for c in cases} == {"", "bh0", "ab0", "ct"}
    for c in cases:
        sa, sb, sc, _ = T.bgemm_strides(c)
        if c[8] == "bh0":
            assert sb[1] == 0 and c[6] > 1
        if c[8] == "ab0":
            assert sa[0] == 0 and c[5] > 1
        if c[8] == "ct":
            assert sc[2] == 1 and sc[3] == c[2] + 2
    assert all(o > 0 for o in T.BGEMM_OFFS)


@pytest.mark.parametrize("case", T.BGEMM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_bgemm_inputs(case):
    c = T.bgemm_case(case)                                              # asserts the budget, int64 == fp64, the window's size
    B, H, M, N, K = c.dims
    assert torch.equal((c.Av @ c.Bv) * c.alpha, c.ref.float()), "a plain fp32 matmul is exact on these operands"
    assert torch.equal(torch.einsum("bhik,bhkj->bhij", c.Av.flip(3), c.Bv.flip(2)) * c.alpha, c.ref.float()), "... in another order too"
    assert torch.isnan(c.want[~c.window]).all() and not torch.isnan(c.want[c.window]).any()
    assert not c.window[:T.BGEMM_OFFS[2]].any() and not c.window[-17:].any()
    # the descriptor stays inside the buffers (what mla_bgemm checks before it launches)
    for s, dims, numel, off in ((c.sa, (B, H, M, K), c.A.numel(), T.BGEMM_OFFS[0]), (c.sb, (B, H, K, N), c.B.numel(), T.BGEMM_OFFS[1]),
                                (c.sc, (B, H, M, N), c.nc, T.BGEMM_OFFS[2])):
        assert off + sum(st * (d - 1) for st, d in zip(s, dims)) < numel


# ---- 3. softmax -----------------------------------------------------------------------------------------------------------------------------
def test_softmax_tables():
    assert set(T.SOFTMAX_N) == {1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024} == set(T.SOFTMAX_BH)
    for n in (1, 63, 65):
        B, H = T.SOFTMAX_BH[n]
        assert (B * H * n) % 4 != 0
    B, H = T.SOFTMAX_FWD_BH
    assert (B * H * 65) % 4 != 0 and B >= 2
    fams = {(n, f) for n, f, _ in T.SOFTMAX_FWD_CASES}
    assert fams >= {(n, f) for n in (65, 1024) for f in T.SOFTMAX_FAMILIES} | {(n, "normal") for n in T.SOFTMAX_N}
    assert all((n, f, m) in T.SOFTMAX_FWD_CASES for n, f in fams for m in (False, True))


@pytest.mark.parametrize("n", T.SOFTMAX_N)
def test_softmax_backward_inputs_are_exact(n):
    c = T.softmax_bwd_case(n)
    assert torch.equal(c.P * 64, (c.P * 64).round()) and 0 <= c.P.min() and c.P.max() <= 1 and c.g.abs().max() <= 7
    # fp32 throughout, in two summation orders (torch's blocked sum; a strictly sequential sum from the right): the same bits
    prod = c.P * c.g
    for dot in (prod.sum(-1, keepdim=True), prod.flip(-1).cumsum(-1)[..., -1:]):
        assert torch.equal(c.P * (c.g - dot), c.want), f"n={n}: the fp32 evaluation is not the rounded fp64 one"
    assert torch.equal(prod.double(), c.P.double() * c.g.double())


@pytest.mark.parametrize("n,family,masked", T.SOFTMAX_FWD_CASES)
def test_softmax_forward_tolerance_holds_for_torch(n, family, masked):
    s = T.softmax_scores(n, family, T.case_seed(n, len(family), masked))
    pm = T.softmax_mask(n) if masked else None
    ref = T.softmax_ref(s, pm)
    s32 = s if pm is None else torch.where(pm[:, None, None, :].expand(s.shape) > 0, torch.tensor(-1e7), s)
    got = torch.softmax(s32, dim=-1)
    err = (got.double() - ref).abs().max().item()
    assert err <= T.softmax_tol(ref), (err, T.softmax_tol(ref))
    if masked:
        cols = pm > 0
        assert (~cols).any(1).all() and (n == 1 or cols.any(1).all()), "every batch element keeps a column and (n > 1) masks one"
        assert (ref.transpose(1, 3)[cols.nonzero(as_tuple=True)[0], cols.nonzero(as_tuple=True)[1]] == 0).all(), "masked columns are exactly 0 in fp64 too"
        assert n < 4 or {0.5, 1.0, 0.0, -1.0} <= set(pm.unique().tolist())
    if family == "spike":
        assert ref.max().item() == 1.0
    if family == "low":
        assert s.max().item() <= -1e4 + 1 and s.min().item() >= -1e4


# ---- 4. LayerNorm forward -------------------------------------------------------------------------------------------------------------------
def test_layernorm_forward_table():
    assert {c[0] for c in T.LNF_CASES} == {512, 768, 1024} and {c[1] for c in T.LNF_CASES} == {1, 2, 3, 4, 5, 17}
    assert set(T.LNF_FAMILIES) == {(0.3, 1.7), (1000.0, 1.0), (0.0, 1e-3), (-50.0, 20.0)} and len(T.LNF_CASES) == 3 * 6 * 4


@pytest.mark.parametrize("D,M,fam", T.LNF_CASES)
def test_layernorm_forward_bounds_hold_for_torch(D, M, fam):
    """torch's CPU fp32 layer norm (another summation order: vectorised, blocked) and a plain fp32 mean stay inside the bounds.
    rstd: torch forms the variance in ONE pass (moments of blocks, merged), whose error grows with mean^2 / var -- at mean 1000, std 1 its
    rstd is 5 to 8 times the bound although its y is not.  The bound is derived for deviations from the computed mean, as the kernel forms
    them, so it is checked on that two-pass form in fp32, in two summation orders."""
    c = T.lnf_case(D, M, fam)
    y64, mean64, rstd64 = T.lnf_ref(c.x, c.w, c.b)
    mb, rb, yb = T.lnf_bounds(c.x, c.w, c.b, y64, rstd64)
    y, mean, _ = torch.native_layer_norm(c.x, (D,), c.w, c.b, 1e-5)
    assert torch.equal(y, F.layer_norm(c.x, (D,), c.w, c.b))
    ratios = [(mean.reshape(M).double() - mean64).abs() / mb, (c.x.mean(1).double() - mean64).abs() / mb, (y.double() - y64).abs() / yb]
    for order in (lambda t: t.sum(1), lambda t: t.view(M, D // 64, 64).cumsum(1)[:, -1].sum(1)):       # the second: per lane in sequence, then across lanes
        mu = order(c.x) / D
        d = c.x - mu[:, None]
        rs = 1.0 / torch.sqrt(order(d * d) / D + 1e-5)
        ratios += [(mu.double() - mean64).abs() / mb, (rs.double() / rstd64 - 1).abs() / rb,
                   ((d * rs[:, None] * c.w + c.b).double() - y64).abs() / yb]
    worst = max(r.max().item() for r in ratios)
    assert worst <= 1.0, f"error / bound = {worst:.3f}"
    if T.LNF_FAMILIES[fam][0] == 1000.0:
        assert (y.double() - y64).abs().max().item() > 1e-5, "the large-mean family is the one a flat 1e-5 cannot hold"


@pytest.mark.parametrize("D", T.LNF_D)
def test_layernorm_exact_rows(D):
    c = T.lnf_const_case(D)
    y, mean, rstd = T.lnf_ref(c.x, c.w, c.b)
    assert torch.equal(mean, c.c.double()) and torch.equal(y.float(), c.b.expand_as(y)) and torch.equal(c.x.sum(1) / D, c.c)
    p = T.lnf_pm_case(D)
    y, mean, rstd = T.lnf_ref(p.x, p.w, p.b, eps=0.0)
    assert torch.equal(mean, p.m.double()) and torch.equal(rstd, 2.0 ** -p.k)
    assert torch.equal(p.x.sum(1) / D, p.m) and torch.equal(p.x.flip(1).cumsum(1)[:, -1] / D, p.m), "fp32 sums in two orders are exact"


# ---- 5. assembly and patchify ---------------------------------------------------------------------------------------------------------------
def test_assemble_cases_cross_the_grid_cap():
    first = T.ASM_GRID_CAP * T.ASM_TPB                                  # float4 elements of the capped grid's first trip
    assert {c[2] for c in T.ASM_CASES} == {4, 768, 1024}
    B, L, D = T.ASM_CASES[3]
    assert first < B * (L + 1) * D // 4 < first + 65536                 # a second trip that is a short tail
    assert not first < (B - 1) * (L + 1) * D // 4, "the smallest such batch at L = 256, D = 768"
    # one sequence more: with [cls] the tail is just above 65536 float4, without [cls] (B, L, D) it is exactly 65536
    B, L, D = T.ASM_CASES[4]
    assert (B, L, D) == (44, 256, 768) and first + 65536 < B * (L + 1) * D // 4 < first + 2 * 65536 and B * L * D // 4 == first + 65536
    assert all(B * (L + 1) * D // 4 <= first for B, L, D in T.ASM_CASES[:3])


@pytest.mark.parametrize("B,L,D", T.ASM_CASES[:4])
def test_assemble_inputs_are_exact(B, L, D):
    c = T.asm_case(B, L, D)
    for t in (c.table, c.pos, c.type, c.cls, c.lin):
        assert torch.equal(t * 256, (t * 256).round()) and t.abs().max() < 4
    ids = c.ids.clamp(0, c.V - 1)
    a = F.embedding(ids, c.table) + (c.pos[None] + c.type)
    b = (F.embedding(ids, c.table) + c.pos[None]) + c.type
    assert torch.equal(a, b) and torch.equal(a.double(), F.embedding(ids, c.table).double() + c.pos.double()[None] + c.type.double())
    assert ((c.ids < 0) | (c.ids >= c.V)).sum() == 2


def test_patchify_table():
    cases = T.PATCH_CASES
    assert {c[4] for c in cases} == {1, 2, 16} and {c[1] for c in cases} == {1, 3}
    for tr in (False, True):
        sub = [c for c in cases if c[5] == tr]
        assert any(c[2] // c[4] == 1 and c[3] // c[4] > 1 for c in sub) and any(c[3] // c[4] == 1 and c[2] // c[4] > 1 for c in sub)
        assert any(c[2] != c[3] for c in sub) and {c[4] for c in sub} == {1, 2, 16}
        big = [c[0] * c[1] * c[2] * c[3] for c in sub if c[0] * c[1] * c[2] * c[3] > T.PATCH_GRID_CAP * 256]
        assert len(big) == 1 and big[0] < T.PATCH_GRID_CAP * 256 * 1.01, "one case just past the capped grid"
    assert all(c[1] == 1 for c in cases if c[5])
