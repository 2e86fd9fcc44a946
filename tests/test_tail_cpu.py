"""tests/tail_model.py without a GPU: the inputs meet the conditions that the tolerances of tests/test_tail_gpu.py rest on, and the
models agree with oracle/mla_oracle.py.  No case is excluded: a condition that fails here fails the test."""
import numpy as np
import pytest
import torch

import tail_model as T
from oracle import mla_oracle as O
from resident_model import philox4x32_10

F32, F64 = np.float32, np.float64


# ---- 1. OGM ------------------------------------------------------------------------------------------------------------------------------
def test_u01_is_fp32_and_rounds_at_25_bits():
    assert T.u01(0xFFFFFFFF).dtype == F32 and T.u01(0xFFFFFFFF) == F32(1.0)              # 16777215.5 rounds to even: 2^24
    assert T.u01(0) == F32(2.0 ** -25)
    assert T.u01((2 ** 23 + 1) << 8) == F32(8388610.0 / 16777216.0)                     # 8388609.5 -> 8388610 (RNE), not 8388609.5
    assert T.u01((2 ** 23 - 1) << 8) == F32(8388607.5 / 16777216.0)                     # below 2^23 the half is representable


def test_vectorised_philox_is_the_scalar_one():
    for seed in T.OGM_SEEDS:
        for stream in (0, (5 << 16) | 2):
            k = np.array([0, 1, 255, 4096, 2 ** 32 + 7], dtype=np.uint64)
            got = [np.broadcast_to(np.asarray(x, dtype=np.uint64), k.shape) for x in philox4x32_10(k, stream, seed)]
            for i, ki in enumerate(k.tolist()):
                assert [int(w[i]) for w in got] == philox4x32_10(ki, stream, seed)


def test_noise_model_is_standard_normal():
    """Mean, std, skew and kurtosis of N(0, 1) on 2^16 draws, each within 5 sigma of its estimator; |z| <= 5.9."""
    n = 1 << 16
    for seed, step, s in ((0, 0, 0), ((1 << 40) + 3, 5, 2)):
        z = T.ogm_noise(n, s, step, seed)
        assert z.shape == (n,) and np.isfinite(z).all() and np.abs(z).max() <= 5.9
        m, sd = z.mean(), z.std()
        u = (z - m) / sd
        assert abs(m) < 5 / n ** 0.5 and abs(sd - 1) < 5 / (2 * n) ** 0.5, (m, sd)
        assert abs((u ** 3).mean()) < 5 * (6 / n) ** 0.5 and abs((u ** 4).mean() - 3) < 5 * (24 / n) ** 0.5
    # the four words of one counter feed four consecutive elements; streams and steps are separate
    assert not np.array_equal(T.ogm_noise(64, 1, 0, 0), T.ogm_noise(64, 2, 0, 0))
    assert not np.array_equal(T.ogm_noise(64, 1, 0, 0), T.ogm_noise(64, 1, 5, 0))
    assert np.array_equal(T.ogm_noise(64, 1, 0, 0)[:13], T.ogm_noise(13, 1, 0, 0))


@pytest.mark.parametrize("table", [T.ogm_main, T.ogm_one, lambda: T.ogm_geom("A"), lambda: T.ogm_geom("B")])
def test_ogm_tables(table):
    """Gaps of 1 .. 5 sentinel floats, exactly representable families (fp32 value == k / den, scaling by a power of two exact), the
    statistics model against torch's std on doubles, the scaling against O.ogm_modulate."""
    t = table()
    ends = t.seg[:, 0] + t.seg[:, 1]
    gaps = t.seg[1:, 0] - ends[:-1]
    assert t.seg[0, 0] >= 1 and len(t.buf) - ends[-1] >= 1 and ((gaps >= 1) & (gaps <= 5)).all()
    assert t.inside.sum() == t.seg[:, 1].sum()
    assert (t.buf[~t.inside] == T.sentinel(len(t.buf))[~t.inside]).all() and (t.buf[~t.inside] < -2000).all()
    assert (np.diff(t.first_chunk) == -(-t.seg[:, 1] // T.OGM_CHUNK)).all() and t.first_chunk[0] == 0
    for s in range(t.n_seg):
        v, (k, den) = t.vals[s], t.grids[s]
        assert v.dtype == F32 and (v.astype(F64) * den == k).all()
        for cf in (0.5, 0.25, 1.0):
            assert ((v * F32(cf)).astype(F64) == v.astype(F64) * cf).all()              # fp32 result == fp64 result
        if len(v) > 1:
            want = torch.from_numpy(v).double().std().item()
            assert abs(np.sqrt(t.var[s]) - want) <= 1e-9 * max(want, 1e-3), (s, t.var[s], want)
        else:
            assert np.isnan(t.var[s])
        if len(v):
            g = torch.from_numpy(v).view(1, 1, 1, -1)
            got = O.ogm_modulate({"w": g, "b": g.view(-1)}, torch.tensor(0.5), "OGM")
            assert (got["w"].double().numpy().ravel() == T.ogm_scaled(t, 0.5)[t.seg[s, 0]:ends[s]]).all()
            assert got["b"] is not g and torch.equal(got["b"], g.view(-1))


def test_ogm_main_table_covers_the_cases():
    t = T.ogm_main()
    assert set((t.seg[t.seg[:, 1] > 0, 0] % 4).tolist()) == {0, 1, 2, 3}
    assert {2, 5, T.OGM_CHUNK - 1, T.OGM_CHUNK, T.OGM_CHUNK + 1, 2 * T.OGM_CHUNK + 3} <= set(t.seg[:, 1].tolist())
    zero = [s for s in range(t.n_seg) if t.seg[s, 1] == 0]
    assert zero and all(0 < s < t.n_seg - 1 for s in zero)                              # in the middle of the table
    assert 100000 <= len(t.buf) <= 130000
    const = [s for s, (_n, k) in enumerate(t.spec) if k == "const"]
    assert const and all(t.var[s] == 0.0 and t.stdv[s] == 0 for s in const)
    # the large-mean family defeats an fp32 accumulation of the one-pass formula: already over 4096 elements its variance is wrong
    # by more than the variance itself (the GPU test allows 1 ulp of the standard deviation)
    for s, (n, kind) in enumerate(t.spec):
        if kind == "bigmean":
            v = t.vals[s]
            sm, sq = F32(0), F32(0)
            for x in v[:4096]:
                sm, sq = F32(sm + x), F32(sq + x * x)
            naive = (float(sq) - float(sm) * float(sm) / 4096) / 4095
            assert abs(naive - T.exact_var(t.grids[s][0][:4096], 64)) > t.var[s]
    one = T.ogm_one()
    assert one.seg[1, 1] == 1 and np.isnan(one.stdv[1])


def test_ogm_geometry_tables_share_the_segment():
    a, b = T.ogm_geom("A"), T.ogm_geom("B")
    assert (a.first_chunk == [0, 1, 2, 3]).all() and (b.first_chunk == [0, 3, 4]).all()
    for t, s in ((a, 1), (a, 2), (b, 1)):
        o, n = t.seg[s]
        assert n == T.OGM_X[0] and (t.buf[o:o + n] == a.vals[1]).all() and t.stdv[s] == a.stdv[1]
    assert a.seg[1, 0] % 4 != b.seg[1, 0] % 4                                           # not even the same alignment


# ---- 2. OGM coefficients -------------------------------------------------------------------------------------------------------------------
def _label_is_argmax_somewhere(outs, label):
    return all(bool((o.argmax(1) == label).any()) for o in outs)


@pytest.mark.parametrize("M,B,C", T.COEFF_SHAPES)
def test_coeff_inputs(M, B, C):
    """Every modality has a row whose label is its arg-max, so the scores stay away from 0 and the ratios finite; outside the 'same'
    family no ratio that decides a branch is within 1e-3 of 1 (fp32 and fp64 then take the same branch)."""
    for fam in T.COEFF_FAMILIES:
        outs, label = T.coeff_case(M, B, C, fam)
        assert len(outs) == M and all(o.shape == (B, C) and o.dtype == torch.float32 for o in outs)
        assert _label_is_argmax_somewhere(outs, label), (fam, M, B, C)
        cf, sc, ra = T.coeff_ref(outs, label)
        assert (sc >= 1.0 / (C + 1)).all() and np.isfinite(ra).all() and np.isfinite(cf).all(), (fam, sc, ra)      # arg-max: p >= 1 / C
        if fam == "range":                               # expf(x) underflows to 0 below x = -104
            assert float((outs[1].max(1).values - outs[1].min(1).values).min()) > 104
            assert all(float(o.abs().min()) > 9000 for o in outs)
            assert C < 6 or B < 5 or all(float((o.max(1).values - o.min(1).values).max()) > 104 for o in outs)
        if fam == "same" and M == 2:
            assert sc[0] == sc[1] and ra[1] == 1.0 and cf[1] == 1.0 and cf[0] < 1.0            # else branch: modality 0
        elif fam == "same":
            assert sc[0] == sc[1]
            assert (np.abs(ra - 1) > 1e-3).all()
        else:
            decisive = ra[1:] if M == 3 else ra[1:2]
            assert (np.abs(decisive - 1) > 1e-3).all(), (fam, ra)


@pytest.mark.parametrize("B,C", T.COEFF_BRANCH_SHAPES)
def test_coeff_three_modality_branches(B, C):
    """One case per branch of main.py:323-337: exactly the expected modality is modulated."""
    for branch, which in zip(T.COEFF_BRANCHES, (1, 2, 0)):
        outs, label = T.coeff_branch_case(B, C, branch)
        assert _label_is_argmax_somewhere(outs, label)
        cf, sc, ra = T.coeff_ref(outs, label)
        assert (np.abs(ra[1:] - 1) > 0.05).all(), (branch, ra)
        assert cf[which] < 0.99 and all(cf[m] == 1.0 for m in range(3) if m != which), (branch, cf)


# ---- 3. SGD ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.SGD_SIZES)
def test_sgd_inputs_are_exact(n):
    """Every intermediate of the three steps is representable: numpy fp32, one rounding per operation, equals fp64."""
    c = T.sgd_case(n)
    for x, kmax in ((c.p, T.SGD_PMAX), (c.buf, 7), (c.gs[0], 7), (c.gs[1], 7)):
        assert x.dtype == F32 and x.shape == (n,) and (np.abs(x * 16) <= kmax).all() and (x * 16 == np.round(x * 16)).all()
    assert n < 1000 or all(np.abs(x * 16).max() == kmax for x, kmax in ((c.p, T.SGD_PMAX), (c.buf, 7), (c.gs[0], 7)))
    assert all(np.abs(p).max() < 0.5 for p, _b in T.sgd_run(c))                          # p3 lives on the 2^-25 grid: 24 bits below 1/2
    assert c.gs[2] is None and F32(T.SGD_LR) == T.SGD_LR and F32(T.SGD_WD) == T.SGD_WD
    for (p32, b32), (p64, b64) in zip(T.sgd_run(c, F32), T.sgd_run(c, F64)):
        assert p32.dtype == F32 and (p32.astype(F64) == p64).all() and (b32.astype(F64) == b64).all()
    w = T.sgd_case(n, wide=True)                                                         # p over [-7, 7] too: exact through two steps
    assert len(w.gs) == 2 and (np.abs(w.p * 16) <= 7).all() and (w.p * 16 == np.round(w.p * 16)).all() and (n < 1000 or np.abs(w.p * 16).max() == 7)
    for (p32, b32), (p64, b64) in zip(T.sgd_run(w, F32), T.sgd_run(w, F64)):
        assert (p32.astype(F64) == p64).all() and (b32.astype(F64) == b64).all()
    p64, b64 = T.sgd_run(c)[0]
    pt, bt = O.sgd_step(torch.from_numpy(c.p).double(), torch.from_numpy(c.gs[0]).double(), None, T.SGD_LR, T.SGD_MOM, T.SGD_WD)
    assert (pt.numpy() == p64).all() and (bt.numpy() == b64).all()


def test_sgd_head_case_is_exact_and_misaligned():
    assert (T.HEAD_C * T.HEAD_D) % 4 != 0                                               # the bias slice starts off a 16-byte boundary
    for (W32, b32), (W64, b64) in zip(T.head_run(torch.float32), T.head_run(torch.float64)):
        assert torch.equal(W32.double(), W64) and torch.equal(b32.double(), b64)
    _W, _b, steps = T.head_case()
    assert steps[0][1] is None and steps[1][0] is not None and steps[1][1] is not None and steps[2][0] is None


def test_sgd_random_case_rounds():
    c = T.sgd_random_case(1027)
    p32, _ = T.sgd_model(c.p, c.gs[0], c.buf, True, F32)
    p64, _ = T.sgd_model(c.p, c.gs[0], c.buf, True, F64)
    assert (p32.astype(F64) != p64).mean() > 0.5                                        # not an exact input


# ---- 4. scale, colsum, invstd -----------------------------------------------------------------------------------------------------------
def test_small_kernel_inputs():
    for n in T.SCALE_SIZES:
        assert T.scale_case(n).shape == (n,) and T.scale_case(n).dtype == F32
    assert T.SCALE_SIZES[-1] > 2048 * 256
    for B, D in T.COLSUM_SHAPES:
        x = T.colsum_case(B, D)
        assert x.dtype == F32 and (x == np.round(x)).all() and np.abs(x).sum(0).max() * 4 < 2 ** 24
        want = x.astype(F64).sum(0) * T.COLSUM_SCALE
        assert (want.astype(F32).astype(F64) == want).all()
        acc = np.zeros(D, dtype=F32)
        for r in range(B):
            acc = acc + x[r]
        assert ((acc * F32(T.COLSUM_SCALE)).astype(F64) == want).all()                   # fp32 result == fp64 result
    for n in T.INVSTD_SIZES:
        var, want = T.invstd_case(n)
        assert var.dtype == F32 and (var >= 1e-6).all() and (var <= 1e3).all() and np.isfinite(want).all()


# ---- 5. GS projection --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,C", T.GS_CASES)
def test_gs_inputs_and_model(D, C):
    """sum r^2 < 0.5 and min |alpha + k_i r_j| >= alpha / 2 at both calls; the model is O.gs_before_update's arithmetic."""
    c = T.gs_case(D, C)
    assert all(float((r.double() ** 2).sum()) < 0.5 for r in c.rs)
    assert all(m >= T.GS_ALPHA / 2 for m in c.min_den), c.min_den
    assert O.gs_alpha(-1, 1) == T.GS_ALPHA
    Pl, G = torch.eye(D, dtype=torch.float64), c.G.double()
    for call in range(2):
        Pl, G = O.gs_before_update(Pl, c.rs[call].double().view(1, -1), G, -1, 1, 1)
        wPl, wG = c.want[call]
        if call == 0:                                    # the second reference call starts from the fp32-rounded state, as the kernel does
            assert torch.allclose(Pl, wPl, rtol=0, atol=1e-14) and torch.allclose(G, wG, rtol=0, atol=1e-12)
        else:
            assert torch.allclose(Pl, wPl, rtol=0, atol=1e-7) and torch.allclose(G, wG, rtol=0, atol=1e-5)
        assert abs(float(torch.linalg.norm(wPl)) - 1) < 1e-12
    Pl1 = c.want[0][0]
    assert float((Pl1 - torch.diag(torch.diag(Pl1))).abs().max()) > 1e-4 * float(Pl1.abs().max())       # a non-identity start
    assert {d for d, _ in T.GS_CASES} == {4, 63, 64, 65, 70, 257} and {k for _, k in T.GS_CASES} == {1, 3, 4, 5, 101, 130}


# ---- 6. evaluation fusion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,B,C", T.EVAL_FIXED_SHAPES)
def test_eval_fixed_inputs(M, B, C):
    """Integer logits: the fused values are exact in fp32 in any order; ties between classes are present."""
    outs, label = T.eval_fixed_case(M, B, C)
    al = T.EVAL_ALPHAS[M]
    f32 = np.zeros((B, C), dtype=F32)
    for w, o in zip(al, outs):
        assert o.dtype == F32 and (o == np.round(o)).all()
        f32 = f32 + F32(w) * o
    f64 = sum(F64(w) * o.astype(F64) for w, o in zip(al, outs))
    assert (f32.astype(F64) == f64).all()
    assert ((f64 == f64.max(1, keepdims=True)).sum(1) > 1).any()                        # a tied maximum in the fused logits
    assert ((outs[0] == outs[0].max(1, keepdims=True)).sum(1) > 1).any()
    assert ((label >= 0) & (label < C)).all()
    counts = T.eval_counts(outs, label, al)
    assert counts[0].sum() == B and (counts[1:] <= counts[0]).all()


@pytest.mark.parametrize("M,B,C", T.EVAL_DYN_SMALL)
def test_eval_dynamic_small_inputs_and_model(M, B, C):
    """No row is excluded: the fp64 fused top-2 margin is above 1e-4 everywhere; weights and counts agree with O.valid_batch."""
    outs, label = T.eval_small_case(M, B, C)
    w, _ent = T.gating(outs)
    assert T.top2_margin(outs, w) > T.EVAL_MARGIN
    assert all(T.top2_margin([o], [1.0]) > 0 for o in outs)
    w_ref, c_ref = O.valid_batch([torch.from_numpy(o).double() for o in outs], torch.from_numpy(label), C, True, [])
    assert np.allclose(w, w_ref, rtol=0, atol=1e-12)
    assert (T.eval_counts(outs, label, w) == c_ref.numpy()).all()
    al = T.EVAL_ALPHAS[M]
    _w, c_fix = O.valid_batch([torch.from_numpy(o).double() for o in outs], torch.from_numpy(label), C, False, list(al))
    assert (T.eval_counts(outs, label, al) == c_fix.numpy()).all()


@pytest.mark.parametrize("B,C", T.EVAL_DYN_STRIDE)
def test_eval_stride_inputs(B, C):
    """The fp64 weights lie in (0.05, 0.95); the part before the 256 stride carries no entropy difference, the part behind it all of
    it, and that difference is many times the tolerance."""
    outs, _label = T.eval_stride_case(B, C)
    w, ent = T.gating(outs)
    assert ((w > 0.05) & (w < 0.95)).all(), w
    head = [o[:, :256] for o in outs] if C > 256 else [o[:256] for o in outs]
    ent_head = T.entropies(head)
    assert abs(ent_head[0] - ent_head[1]) < 1e-9 * ent_head.max()
    dent = abs(ent[0] - ent[1])
    assert dent > 0.3 and dent > 3 * T.dent_tol(B, ent), (dent, T.dent_tol(B, ent))
    assert np.allclose(T.dent_of(w), ent - ent.min(), rtol=0, atol=1e-9)
