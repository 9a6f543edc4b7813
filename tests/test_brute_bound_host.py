"""The bounds of the brute-force screen (csrc/kernels_brute.hip: normalize_i8_kernel, normalize_f16_kernel, brute_f16_kernel's exact
test and quick screen; csrc/api.cpp: pqv_brute_topk_impl's eps and eps_sum), restated in numpy with float32 wherever the kernels
compute in float32.  For every (query, row) pair, against the f64 cosine of the f32 inputs:
  * the pair estimate s~ is within the kernel's eps of the true cosine (int8: the per-pair eps; f16: the constant one);
  * the squared-L2 lower bound never exceeds the f64 distance;
  * a pair the exact test keeps at a threshold T also passes the quick screen -- T swept through the pair's own 1 - s~ -+ eps.
The component sums are taken in two different orders of the depth that eps_sum and the L2 bound's 1e-6 (|q|^2 + |v|^2) are sized
for -- 64 chains of dim / 64 additions and a 6-step tree: the wave's own, and one that shares no partial sum with it --, with and
without the fused multiply-add the compiler may form, so nothing here matches a wave bit for bit.  (One chain of 1536 additions is
outside both allowances -- 2e-6 of a norm, 1e-5 of a sum of equal components -- and no kernel sums that way.)  No GPU."""
import numpy as np
import pytest

F = np.float32
U = F(5.9604645e-08)          # 2^-24, as api.cpp writes it
INF = F(np.inf)


def fsum(a, order):
    """row sums of the f32 matrix a, every step rounded to f32: 64 chains of ceil(dim / 64) additions and a 6-step tree, the depth
    eps_sum is sized for.  "wave": lane l takes the components l, l + 64, ..; the tree pairs lanes 32, 16, .. 1 apart.
    "blocked": lane l takes a contiguous run, last component first; the tree pairs lanes 1, 2, .. 32 apart."""
    a = np.ascontiguousarray(a, F)
    m, d = a.shape
    per = (d + 63) // 64
    pad = np.zeros((m, per * 64), F)
    pad[:, :d] = a
    steps = pad.reshape(m, per, 64).transpose(1, 0, 2) if order == "wave" else pad.reshape(m, 64, per).transpose(2, 0, 1)[::-1]
    lanes = np.zeros((m, 64), F)
    for step in steps:
        lanes = (lanes + step).astype(F)
    for off in ((32, 16, 8, 4, 2, 1) if order == "wave" else (1, 2, 4, 8, 16, 32)):
        lanes = (lanes + lanes[:, np.arange(64) ^ off]).astype(F)
    return lanes[:, 0]


def rnorm(x, order):
    """launch_row_norms mode 0 (1 / |x|, 0 for a zero vector) and mode 1 (|x|^2)"""
    n2 = fsum(x * x, order)
    with np.errstate(all="ignore"):
        return np.where(n2 > 0, F(1) / np.sqrt(n2), F(0)).astype(F), n2


def image_i8(x, order, fused):
    """normalize_i8_kernel: (image [m, dim_p] int, sr = (1/S, r, b, sum), n, maxima = (A, B, C, E))"""
    m, dim = x.shape
    dim_p = (dim + 63) // 64 * 64
    with np.errstate(all="ignore"):
        rn, _ = rnorm(x, order)
        v = (x * rn[:, None]).astype(F)
        bad = ~(rn == rn) | (rn > F(3.0e38)) | ~(np.abs(v) <= F(3.0e38)).all(axis=1)
        mx = np.fmax.reduce(v, axis=1, initial=F(-3.0e38))
        mn = np.fmin.reduce(v, axis=1, initial=F(3.0e38))
        tot = fsum(v, order)
        b = np.where(bad, F(0), F(0.5) * (mx + mn)).astype(F)
        half = np.where(bad, F(0), np.maximum(mx - b, b - mn)).astype(F)
        S = np.where(half > 0, F(127) / np.where(half > 0, half, F(1)), F(0)).astype(F)
        invS = np.where(S > 0, F(1) / np.where(S > 0, S, F(1)), F(0)).astype(F)
        vp = np.zeros((m, dim_p), F)
        if fused:               # fma(p, rn, -b): the product is exact in f64
            vp[:, :dim] = (x.astype(np.float64) * rn[:, None].astype(np.float64) - b[:, None].astype(np.float64)).astype(F)
        else:
            vp[:, :dim] = v - b[:, None]
        vp[bad] = 0
        qf = np.clip(np.rint(vp * S[:, None]), F(-127), F(127)).astype(F)
        if fused:
            d = (vp.astype(np.float64) - qf.astype(np.float64) * invS[:, None].astype(np.float64)).astype(F)
        else:
            d = vp - (qf * invS[:, None]).astype(F)
        rr = (np.sqrt(fsum(d * d, order)) * F(1.0001) + F(1.0e-6)).astype(F)
        nn = (np.sqrt(fsum(vp * vp, order)) * F(1.0001) + F(1.0e-6)).astype(F)
        rr[bad] = INF
        nn[bad] = INF
        tot = np.where(bad, F(0), tot).astype(F)
        A = np.where(bad, INF, np.abs(tot - b * F(dim)) * F(1.00001)).astype(F)
        maxima = (A.max(), ((nn + F(3) * rr) * F(1.00001)).astype(F).max(), np.abs(b).max(), (rr * F(1.00001)).astype(F).max())
    return qf.astype(np.int64), (invS, rr, b, tot), nn, maxima, bad


def image_f16(x, order):
    """normalize_f16_kernel: the unit vector x 2^8, rounded to f16, zero-padded to a multiple of 32 values"""
    m, dim = x.shape
    rn, _ = rnorm(x, order)
    out = np.zeros((m, (dim + 31) // 32 * 32), np.float16)
    with np.errstate(all="ignore"):
        out[:, :dim] = np.clip(x * (rn * F(256))[:, None], F(-65504), F(65504)).astype(np.float16)
    return out


def true_cosine(q, v):
    """f64 cosine of the f32 inputs; 0 where a vector is zero (the library's distance 1)"""
    q64, v64 = q.astype(np.float64), v.astype(np.float64)
    with np.errstate(all="ignore"):
        s = (q64 @ v64.T) / (np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(v64, axis=1)[None, :])
    return np.where(np.isfinite(s), s, 0.0)


def eps_constants(dim, i8):
    """pqv_brute_topk_impl: f16_eps (a.eps) and eps_sum"""
    dim_p = (dim + 63) // 64 * 64 if i8 else (dim + 31) // 32 * 32
    if i8:
        eps = F(2.0) * F(dim_p) * U + F(4.0e-6)
    else:
        eps = F(1.01) * F(9.765625e-04) + F(2.0) * F(dim_p) * U + F(2.0e-6)
    eps_sum = (F(dim) / F(64) + F(8)) * U * np.sqrt(F(dim)) * F(1.01)
    return F(eps), F(eps_sum)


def l2_lower_bound(sc, eps, qaux, vaux):
    """brute_f16_kernel's exact test, squared L2"""
    with np.errstate(all="ignore"):
        qv = (np.sqrt(qaux)[:, None] * np.sqrt(vaux)[None, :] * F(1.000001)).astype(F)     # (|q| |v|: the product of the squares leaves f32's range)
        s = (qaux[:, None] + vaux[None, :]).astype(F)
        lb = ((s - F(2) * qv * sc) - F(2) * qv * eps - F(1.0e-6) * s).astype(F)
    return np.where(lb < 0, F(0), lb)


def thresholds(lb, eps):
    """thresholds around the place where the exact test starts to keep the pair (it keeps iff lb <= T)"""
    with np.errstate(all="ignore"):
        for t in (lb, np.nextafter(lb, INF), np.nextafter(lb, -INF), lb + eps, lb + F(2) * eps, lb + F(1.0e-3)):
            t = t.astype(F)
            yield np.where(np.isfinite(t), t, F(0.5)).astype(F)          # (the kernel screens with finite thresholds only)


def vectors(kind, m, dim, rng):
    if kind == "normal":
        return rng.standard_normal((m, dim)).astype(F)
    if kind == "uniform01":
        return rng.random((m, dim), dtype=F)
    x = rng.standard_normal((m, dim)).astype(F)
    if kind == "dominant":
        x[:, 3 % dim] += F(60)
    elif kind == "constant":                 # half = 0, S = 0: the image is zero and the mid-range term carries everything
        x[:] = rng.standard_normal((m, 1)).astype(F)
    elif kind == "tiny":
        x *= F(1e-12)
    elif kind == "huge":
        x *= F(1e12)
    elif kind == "mixed":                    # one of everything, a zero vector included
        x[0] = 0
        x[1] = F(0.37)
        x[2] *= F(1e-12)
        x[3] *= F(1e12)
        x[4, 5 % dim] += F(80)
        x[5] = np.abs(x[5])
    else:
        raise ValueError(kind)
    return x


KINDS = ["normal", "uniform01", "dominant", "constant", "tiny", "huge", "mixed"]
DIMS = [7, 50, 64, 100, 256, 1536]


@pytest.mark.parametrize("fused", [False, True], ids=["mul-sub", "fma"])
@pytest.mark.parametrize("order", ["wave", "blocked"])
@pytest.mark.parametrize("dim", DIMS)
def test_int8_pair_bound_and_quick_screen(dim, order, fused):
    rng = np.random.default_rng(1000 + dim)
    eps0, eps_sum = eps_constants(dim, True)
    for qkind in KINDS:
        q = vectors(qkind, 8, dim, rng)
        for vkind in KINDS:
            v = vectors(vkind, 48, dim, rng)
            if vkind == "normal":            # near-duplicates of the queries: the estimates that matter most
                v[:8] = q + F(1e-3) * np.abs(q).max() * rng.standard_normal(q.shape).astype(F)
            qi, (iq, rq, a, sq), nq_, _, _ = image_i8(q, order, fused)
            vi, (iv, rv, b, sv), nv, (mA, mB, mC, mE), _ = image_i8(v, order, fused)
            D = (qi @ vi.T).astype(F)                                          # exact in int32, and below 2^24 x 127: exact as a float sum
            assert np.abs(qi @ vi.T).max() < 2 ** 31
            with np.errstate(all="ignore"):
                sc = ((D * iq[:, None]) * iv[None, :] + (b[None, :] * sq[:, None] + a[:, None] * (sv - b * F(dim))[None, :])).astype(F)
                eps = ((nq_[:, None] * rv[None, :] + rq[:, None] * (nv + F(3) * rv)[None, :]) * F(1.00001) + eps0
                       + eps_sum * (np.abs(a)[:, None] + np.abs(b)[None, :])).astype(F)
            s = true_cosine(q, v)
            what = f"dim {dim}, queries {qkind}, rows {vkind}"
            assert (np.abs(sc.astype(np.float64) - s) <= eps.astype(np.float64)).all(), what
            # squared L2: the bound against the f64 distance
            _, q2 = rnorm(q, order)
            _, v2 = rnorm(v, order)
            lb2 = l2_lower_bound(sc, eps, q2, v2)
            q64, v64 = q.astype(np.float64), v.astype(np.float64)
            d2 = (q64 ** 2).sum(1)[:, None] + (v64 ** 2).sum(1)[None, :] - 2 * (q64 @ v64.T)
            assert (lb2.astype(np.float64) <= np.maximum(d2, 0)).all(), what
            # cosine: exact test and quick screen at thresholds around the pair's own bound
            lb = ((F(1) - sc) - eps).astype(F)
            with np.errstate(all="ignore"):
                K = ((rq * mB + nq_ * mE) * F(1.00002) + eps0 + eps_sum * (np.abs(a) + mC)).astype(F)
                slack = (F(1.0e-5) * (F(2) + np.abs(a) * mA + np.abs(sq) * mC)).astype(F)
                A, C = (sv - b * F(dim)).astype(F), b
                for T in thresholds(lb, eps):
                    keep = lb <= T
                    rhs = ((F(1) - T) - K[:, None] - slack[:, None]).astype(F)
                    k0, k1, k2 = (a / iq)[:, None], (sq / iq)[:, None], -(rhs / iq[:, None])
                    t = (k1.astype(np.float64) * C[None, :].astype(np.float64) + k2.astype(np.float64)).astype(F)   # fma chain: one rounding per step
                    t = (k0.astype(np.float64) * A[None, :].astype(np.float64) + t.astype(np.float64)).astype(F)
                    t = (D.astype(np.float64) * iv[None, :].astype(np.float64) + t.astype(np.float64)).astype(F)
                    passes = ~(t < 0)
                    assert (passes | ~keep).all(), what


@pytest.mark.parametrize("order", ["wave", "blocked"])
@pytest.mark.parametrize("dim", DIMS)
def test_f16_pair_bound_and_quick_screen(dim, order):
    rng = np.random.default_rng(2000 + dim)
    eps, _ = eps_constants(dim, False)
    for qkind in KINDS:
        q = vectors(qkind, 8, dim, rng)
        for vkind in KINDS:
            v = vectors(vkind, 48, dim, rng)
            if vkind == "normal":
                v[:8] = q + F(1e-3) * np.abs(q).max() * rng.standard_normal(q.shape).astype(F)
            qi, vi = image_f16(q, order), image_f16(v, order)
            # products of two f16 values are exact in f32; the matrix core accumulates them in f32, in an order of its own
            exact = qi.astype(np.float64) @ vi.astype(np.float64).T
            chain = np.cumsum(qi.astype(F)[:, None, :] * vi.astype(F)[None, :, :], axis=2, dtype=F)[:, :, -1]
            s = true_cosine(q, v)
            what = f"dim {dim}, queries {qkind}, rows {vkind}"
            _, q2 = rnorm(q, order)
            _, v2 = rnorm(v, order)
            q64, v64 = q.astype(np.float64), v.astype(np.float64)
            d2 = (q64 ** 2).sum(1)[:, None] + (v64 ** 2).sum(1)[None, :] - 2 * (q64 @ v64.T)
            for acc in (exact.astype(F), chain):
                sc = (acc * F(1.52587890625e-05)).astype(F)
                assert (np.abs(sc.astype(np.float64) - s) <= float(eps)).all(), what
                assert (l2_lower_bound(sc, eps, q2, v2).astype(np.float64) <= np.maximum(d2, 0)).all(), what
                lb = ((F(1) - sc) - eps).astype(F)
                for T in thresholds(lb, eps):
                    keep = lb <= T
                    cut = (((F(1) - T) - eps - F(4.0e-6)) * F(65536)).astype(F)
                    assert (~(acc < cut) | ~keep).all(), what


@pytest.mark.parametrize("dim", [7, 64, 100])
def test_a_non_finite_component_is_never_screened_out(dim):
    """normalize_i8_kernel gives such a vector r = n = +inf: its pairs pass the quick screen and the exact test at every threshold"""
    rng = np.random.default_rng(3000 + dim)
    eps0, eps_sum = eps_constants(dim, True)
    q = vectors("mixed", 8, dim, rng)
    v = vectors("normal", 16, dim, rng)
    v[2, 1] = np.inf
    v[5, dim - 1] = np.nan
    v[9, 0] = -np.inf
    qi, (iq, rq, a, sq), nq_, _, qbad = image_i8(q, "wave", False)
    vi, (iv, rv, b, sv), nv, (mA, mB, mC, mE), bad = image_i8(v, "wave", False)
    assert bad.tolist() == [i in (2, 5, 9) for i in range(16)] and not qbad.any()
    assert np.isposinf(rv[bad]).all() and np.isposinf(nv[bad]).all() and (vi[bad] == 0).all() and (sv[bad] == 0).all() and (b[bad] == 0).all()
    assert np.isposinf(mA) and np.isposinf(mB) and np.isposinf(mE) and np.isfinite(mC)
    D = (qi @ vi.T).astype(F)
    with np.errstate(all="ignore"):
        sc = ((D * iq[:, None]) * iv[None, :] + (b[None, :] * sq[:, None] + a[:, None] * (sv - b * F(dim))[None, :])).astype(F)
        eps = ((nq_[:, None] * rv[None, :] + rq[:, None] * (nv + F(3) * rv)[None, :]) * F(1.00001) + eps0
               + eps_sum * (np.abs(a)[:, None] + np.abs(b)[None, :])).astype(F)
        lb = ((F(1) - sc) - eps).astype(F)
        assert np.isneginf(lb[:, bad]).all()                     # below every threshold: kept
        K = ((rq * mB + nq_ * mE) * F(1.00002) + eps0 + eps_sum * (np.abs(a) + mC)).astype(F)
        slack = (F(1.0e-5) * (F(2) + np.abs(a) * mA + np.abs(sq) * mC)).astype(F)
        for T in (F(-1.0), F(0.0), F(1.0e-6), F(2.0)):
            rhs = ((F(1) - T) - K - slack).astype(F)
            k0, k1, k2 = (a / iq)[:, None], (sq / iq)[:, None], -(rhs / iq)[:, None]
            t = D * iv[None, :] + (k0 * (sv - b * F(dim))[None, :] + (k1 * b[None, :] + k2))
            assert (~(t < 0)).all()                              # one bad row sets the corpus maxima to +inf: every pair passes
