"""The screened centroid probe's bound (csrc/kernels_probe_screen.hip: probe_bound; csrc/api.cpp: probe_screen_images), emulated on
the CPU: f16 images of (q - mu) 2^8 / |q - mu| and (c - mu) cscale with numpy float16, norms summed in center_normalize_f16_kernel's
order, the score in f64 and in f32, every f32 operation of the kernel's expression in numpy float32.  For every (query, centroid)
pair the reference-order f32 chain (src/ivf/index.rs:461-480: ((d0^2 + d1^2) + d2^2) + d3^2 per group of four, one running sum,
no FMA) must lie inside [lb, ub].  No GPU."""
import math

import numpy as np
import pytest

import probe_screen_cases as psc

F = np.float32
U = 2.0 ** -24
H = 2.0 ** -11


def _up(v):
    return np.nextafter(F(v), F(np.inf))


def sum_depth(dim):
    """center_normalize_f16_sum_depth (kernels_build.hip)"""
    per_lane = 8 * ((dim // 8 + 63) // 64) if (dim % 8 == 0 and dim <= 2048) else (dim + 63) // 64
    return per_lane + 6


def constants(dim, inv_cs):
    """probe_screen_images (api.cpp), line by line"""
    dim_p = (dim + 63) // 64 * 64
    hp = H + U + H * U
    sub = math.sqrt(dim) * 2.0 ** -25
    g = (sum_depth(dim) + 2) * U * 1.01
    cm = (dim // 4 + 8) * U
    return dict(
        fn=_up((1.0 + g) * 1.000001),
        e1=_up((2.0 * hp + hp * hp + 1.01 * 2.02 * dim_p * U + 1.01 * sub / 256.0 + 2.0e-6) * 1.001),
        e2s=_up(float(inv_cs) * sub * 1.02),
        kS=_up(1.01 * g + 16.0 * U),
        lo_f=np.nextafter(F(1.0 - cm - 1.0e-6), F(0)),
        hi_f=_up(1.0 + cm + 1.0e-6),
        inv_cs=F(inv_cs),
    )


def norms_like_kernel(v):
    """|row|^2 of every row of the f32 matrix v as center_normalize_f16_kernel sums it: fused multiply-adds along a lane, then the
    wave's xor tree (the products are exact in f64, so one rounding to f32 per step is the fused operation)"""
    n, dim = v.shape
    fast = dim % 8 == 0 and dim <= 2048
    lanes = np.zeros((n, 64), F)
    if fast:
        g8 = dim // 8
        for uu in range(4):
            for lane in range(64):
                g = lane + 64 * uu
                if g < g8:
                    for e in range(8):
                        x = v[:, g * 8 + e].astype(np.float64)
                        lanes[:, lane] = (x * x + lanes[:, lane].astype(np.float64)).astype(F)
    else:
        for e in range(dim):
            x = v[:, e].astype(np.float64)
            lanes[:, e % 64] = (x * x + lanes[:, e % 64].astype(np.float64)).astype(F)
    off = 32
    while off:
        lanes = (lanes + lanes[:, np.arange(64) ^ off]).astype(F)
        off //= 2
    return lanes[:, 0]


def images(q, c):
    """mu, the norms, cscale and the f16 images, as launch_col_mean / launch_center_normalize_f16 / probe_screen_images make them"""
    mu = (c.astype(np.float64).sum(0) / len(c)).astype(F)            # any fixed vector serves the bound
    a = (q - mu).astype(F)
    b = (c - mu).astype(F)
    an2, bn2 = norms_like_kernel(a), norms_like_kernel(b)
    mx = float(bn2.max())
    cscale = F(256.0 / (math.sqrt(mx) * 1.000001)) if mx > 0 else F(1.0)
    inv_cs = F(1.000001 / float(cscale))
    with np.errstate(divide="ignore", invalid="ignore"):
        sa = np.where(an2 > 0, F(256.0) / np.sqrt(an2, dtype=F), F(0)).astype(F)
    clamp = lambda x: np.minimum(np.maximum(x, F(-65504.0)), F(65504.0))
    q16 = clamp((a * sa[:, None]).astype(F)).astype(np.float16)
    c16 = clamp((b * cscale).astype(F)).astype(np.float16)
    return an2, bn2, q16, c16, inv_cs


def probe_bound(k, an2, bn2, s):
    """probe_bound (kernels_probe_screen.hip), f32 operation by f32 operation; an2 [nq, 1], bn2 [1, kc], s [nq, kc]"""
    an_ub = np.sqrt(an2, dtype=F) * k["fn"]
    bn_ub = np.sqrt(bn2, dtype=F) * k["fn"]
    est = (s * (np.sqrt(an2, dtype=F) * F(0.00390625))).astype(F) * k["inv_cs"]
    S = an2 + bn2
    mid = S - F(2.0) * est
    E = (k["kS"] * S + F(2.0) * an_ub * (bn_ub * k["e1"] + k["e2s"])) * F(1.00001) + F(1.0e-33)
    lo, hi = mid - E, mid + E
    inf = F(np.inf)
    with np.errstate(invalid="ignore"):
        finite = (np.abs(S) < inf) & (np.abs(est) < inf) & (np.abs(mid) < inf) & (E < inf) & (np.abs(lo) < inf) & (hi < F(3.0e38))
        # np.fmax is fmaxf: a NaN operand gives the OTHER operand (np.maximum would propagate it and hide what the kernel does)
        lb = np.where(finite, np.fmax(lo, F(0)) * k["lo_f"], F(0)).astype(F)
        ub = np.where(finite, np.fmax(hi, F(0)) * k["hi_f"] + F(1.0e-33), inf).astype(F)
    for x in (an_ub, bn_ub, est, S, mid, E, lb, ub):
        assert x.dtype == F
    return lb, ub


def reference_chain(q, c):
    """d_ref[i, j]: index.rs:461-480 in numpy float32"""
    nq, dim = q.shape
    total = np.zeros((nq, len(c)), F)
    for g in range(dim // 4):
        d = (q[:, None, 4 * g:4 * g + 4] - c[None, :, 4 * g:4 * g + 4]).astype(F)
        sq = (d * d).astype(F)
        t = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
        total = total + t
    assert total.dtype == F
    return total


def _sets(dim, rng):
    kc, nq = 48, 12
    uni_c, uni_q = rng.random((kc, dim), dtype=F), rng.random((nq, dim), dtype=F)
    yield "uniform", uni_q, uni_c
    yield "offset -1000 +- 0.01", (F(-1000) + F(0.01) * rng.standard_normal((nq, dim))).astype(F), \
        (F(-1000) + F(0.01) * rng.standard_normal((kc, dim))).astype(F)
    yield "scaled 1e-3", (uni_q * F(1e-3)).astype(F), (uni_c * F(1e-3)).astype(F)
    out = uni_c.copy()
    out[5] = F(1e15)
    yield "one 1e15 outlier centroid", uni_q, out
    eq = uni_q.copy()
    eq[0], eq[1] = uni_c[3], uni_c[kc - 1]
    yield "query equal to a centroid", eq, uni_c
    far = uni_q.copy()
    far[2] = far[2] * F(1e6)
    far[3] = F(-1e6) * far[3]
    yield "query 1e6 x outside the data", far, uni_c
    yield "all-equal centroids", uni_q, np.repeat(uni_c[:1], kc, axis=0)
    yield "all-equal centroids, query on them", np.repeat(uni_c[:1], nq, axis=0), np.repeat(uni_c[:1], kc, axis=0)
    # next to FLT_MAX: |q - mu|^2 and |c - mu|^2 in (1.7e38, 3e38) -- finite norms whose sum, and 2 est, overflow
    # (the centroids come in +- pairs: their mean is exactly zero, so the norms about the mean are the ones chosen here)
    big = np.sqrt(2.4e38 / dim)
    sgn = np.where(rng.random((kc // 2, dim)) < 0.85, 1.0, -1.0)
    half = (big * (0.9 + 0.2 * rng.random((kc // 2, 1))) * sgn).astype(F)
    hq = (big * (0.85 + 0.25 * rng.random((nq, 1))) * np.ones((nq, dim))).astype(F)
    hq[1] = (F(0.6) * hq[0]).astype(F)
    half[0] = F(0)
    half[7] = hq[1]
    yield "norms next to FLT_MAX", hq, np.concatenate([half, -half])


# 772 .. 3072: rows beyond one 768-dim slab of probe_resolve_kernel; 2048 is the last dim of center_normalize_f16_kernel's register
# path, 2052 (dim % 8 != 0) and 3072 take sum_depth's other branch
@pytest.mark.parametrize("dim", [4, 36, 100, 768, 772, 1536, 2048, 2052, 3072])
def test_bounds_enclose_the_reference_chain(dim):
    rng = np.random.default_rng(1000 + dim)
    for name, q, c in _sets(dim, rng):
        with np.errstate(over="ignore", invalid="ignore"):
            an2, bn2, q16, c16, inv_cs = images(q, c)
            d_ref = reference_chain(q, c)
        huge = name == "norms next to FLT_MAX"
        if huge:                     # what the kernels accept: finite query norms, a table whose norms are all <= 3e38
            assert (bn2 <= F(3.0e38)).all() and (an2 > 1.7e38).sum() >= 4 and (bn2 > 1.7e38).sum() >= 8, name
        assert np.isfinite(an2).all() and np.isfinite(bn2).all() and np.isfinite(inv_cs), name
        k = constants(dim, inv_cs)
        s64 = q16.astype(np.float64) @ c16.astype(np.float64).T
        # ... and accumulated in f32, one order (the products of two f16 values are exact in f32)
        s32 = np.zeros_like(s64, dtype=F)
        for i in range(q16.shape[1]):
            s32 = s32 + q16[:, i:i + 1].astype(F) * c16[None, :, i].astype(F)
        for label, s in (("f64 score", s64.astype(F)), ("f32 score", s32)):
            with np.errstate(over="ignore", invalid="ignore"):
                lb, ub = probe_bound(k, an2[:, None], bn2[None, :], s)
            # an overflowed intermediate must leave the pair unbounded, never NaN and never a made-up finite bound
            assert np.isfinite(lb).all() and not np.isnan(ub).any(), (name, label)
            assert huge or np.isfinite(ub).all(), (name, label)
            if huge:
                assert np.isinf(ub).any() and np.isfinite(ub).any(), (name, label)        # both kinds of pair are in the set
            bad = ~((lb <= d_ref) & (d_ref <= ub))
            assert not bad.any(), (name, label, dim, lb[bad][:3], d_ref[bad][:3], ub[bad][:3])


def test_bounds_are_tight_on_uniform_data():
    """On the flagship shape's data (uniform, 768 dims) the interval is a few thousandths of the distance wide: what makes the
    screen worth running.  Width <= 2 E (1 + cm) with E <= kS S + 2 |a||b| e1 (the subnormal term is nothing at this scale):
    kS <= 43 u, S <= 2.2 d here, e1 <= 1.2e-3, 2 |a||b| <= S  =>  width / d <= 2 * 2.2 * (43 u + 1.2e-3) * 1.01 < 6e-3."""
    rng = np.random.default_rng(7)
    q, c = rng.random((16, 768), dtype=F), rng.random((64, 768), dtype=F)
    an2, bn2, q16, c16, inv_cs = images(q, c)
    k = constants(768, inv_cs)
    s = (q16.astype(np.float64) @ c16.astype(np.float64).T).astype(F)
    lb, ub = probe_bound(k, an2[:, None], bn2[None, :], s)
    d_ref = reference_chain(q, c)
    assert (an2[:, None] + bn2[None, :] <= 2.2 * d_ref).all()
    assert ((ub - lb) <= 6e-3 * d_ref).all(), float(((ub - lb) / d_ref).max())


def contenders(queries, cent, n_probe):
    """per query the centroids probe_resolve_kernel keeps: lb <= T, T the n_probe-th smallest upper bound (the f64 score)"""
    an2, bn2, q16, c16, inv_cs = images(queries, cent)
    k = constants(queries.shape[1], inv_cs)
    s = (q16.astype(np.float64) @ c16.astype(np.float64).T).astype(F)
    lb, ub = probe_bound(k, an2[:, None], bn2[None, :], s)
    T = np.sort(ub, axis=1)[:, n_probe - 1]
    return (lb <= T[:, None]).sum(axis=1)


def test_sum_depth_takes_both_branches():
    assert sum_depth(2048) == 8 * 4 + 6 and sum_depth(2052) == 33 + 6 and sum_depth(3072) == 48 + 6 and sum_depth(772) == 13 + 6
    assert sum_depth(1536) == 8 * 3 + 6


@pytest.mark.parametrize("kc", psc.ALL_EQUAL_KC)
def test_all_equal_tables_leave_every_query_above_the_cap(kc):
    """The premise of tests/test_gpu_probe_screen.py::test_screened_probe_all_equal_table: every centroid is a contender of every
    query, more than PR_CAP of them."""
    _, cent, queries = psc.all_equal(kc)
    assert kc > psc.PR_CAP and (2 * kc <= 32 * 196) == (kc == 2304)          # parked / not parked (PR_R * PR_TW words of LDS)
    for n_probe in (1, 7, kc // 4):
        assert (contenders(queries, cent, n_probe) == kc).all(), n_probe


def test_split_table_leaves_2040_contenders():
    """The premise of test_screened_probe_2040_contenders: at nprobe 1 and 7 every query but FAR keeps exactly the 2040 copies --
    below the cap, 64 rounds of 32 with a last round of 24 --, FAR keeps a handful; nobody goes all-exact."""
    _, cent, queries = psc.split_2040()
    assert len(cent) == 2304 and len(np.unique(cent, axis=0)) == psc.N_FAR + 1
    near = np.arange(psc.NQ) != psc.FAR
    for n_probe in (1, 7):
        n = contenders(queries, cent, n_probe)
        assert (n[near] == psc.N_COPIES).all() and psc.N_COPIES <= psc.PR_CAP, (n_probe, n)
        assert n_probe <= n[psc.FAR] < psc.N_COPIES, (n_probe, n)
    assert contenders(queries, cent, len(cent) // 4)[psc.FAR] == len(cent) > psc.PR_CAP          # deeper, it is above the cap
    # psc.FAR_MAX: centroids no farther from FAR than the n_probe-th nearest + twice the widest interval (2 % to spare)
    an2, bn2, q16, c16, inv_cs = images(queries, cent)
    lb, ub = probe_bound(constants(psc.DIM, inv_cs), an2[:, None], bn2[None, :], (q16.astype(np.float64) @ c16.astype(np.float64).T).astype(F))
    d_far = reference_chain(queries, cent)[psc.FAR]
    width = float((ub - lb)[psc.FAR].max())
    for n_probe in (1, 7):
        assert (d_far <= np.sort(d_far)[n_probe - 1] + 2.02 * width).sum() <= psc.FAR_MAX[n_probe] < psc.N_COPIES - 1
    # the far query's nearest centroid is the one it was placed beside, 0.01 away
    d = np.sqrt(((cent.astype(np.float64) - queries[psc.FAR].astype(np.float64)) ** 2).sum(1))
    assert 0.009 < d.min() < 0.011 and (d < 1.0).sum() < psc.N_FAR


def test_refused_tables_have_a_norm_the_screen_cannot_hold():
    """The premise of test_screened_probe_refuses_the_table: probe_screen_images gives up where a centred norm is not <= 3e38 --
    the first table's is finite in every component and row norm of the centroids themselves, the second's is not a number."""
    tables = psc.refused_tables()
    for name, (_, cent) in tables.items():
        mu = (cent.astype(np.float64).sum(0) / len(cent)).astype(F)
        with np.errstate(over="ignore", invalid="ignore"):
            bn2 = norms_like_kernel((cent - mu).astype(F))
        assert not (bn2 <= F(3.0e38)).all(), name
    cent = tables["norm above 3e38"][1]
    assert np.isfinite(cent).all() and np.isfinite((cent.astype(np.float64) ** 2).sum(1).astype(F)).all()
    assert not np.isfinite(tables["inf component"][1]).all()
