"""Per-query probe depths (pqv.h: pqv_topk_depth), host side: the numpy restatement of the depth rule (tests/depth_ref.py) on
hand-made cases, the ABI surface, and every check the C ABI and the Python wrapper make before any device use."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import depth_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pqv_topk_depth", "pqv_topk_depth_device")
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_ratio_rule_on_hand_made_distances():
    f = np.float32
    d2 = np.array([4, 6, 6, 8], f)
    assert depth_ref.ratio_count(d2, 1.5) == 3          # equality at the threshold decides: both tied lists are in
    assert depth_ref.ratio_count(d2, np.nextafter(f(1.5), f(0))) == 1
    assert depth_ref.ratio_count(d2, 1.0) == 1 and depth_ref.ratio_count(d2, 2.0) == 4 and depth_ref.ratio_count(d2, INF) == 4
    assert depth_ref.ratio_count(np.array([4, 4, 4, 9], f), 1.0) == 3       # ratio 1 with tied nearest centroids
    assert depth_ref.ratio_count(np.array([0, 0, 1, 2], f), 5.0) == 2       # d2_0 == 0: t == 0, only the zero distances
    assert depth_ref.ratio_count(np.array([0, 0, 1, 2], f), INF) == 0       # inf * 0 = NaN: nothing compares true
    assert depth_ref.ratio_count(np.array([1, np.nan, 2], f), 3.0) == 2     # a NaN distance is not counted
    # the product is ONE float32 multiplication: 3 * 0.1f rounds above the double product
    t = f(3.0) * f(0.1)
    assert depth_ref.ratio_count(np.array([f(0.1), t, np.nextafter(t, f(1))], f), 3.0) == 2
    big = f(3e38)
    assert depth_ref.ratio_count(np.array([big, big, f(3.3e38)], f), 2.0) == 3      # the product overflows to +inf


def test_clamps():
    c = depth_ref.clamp
    assert c(0, 2, 8, 16) == 2 and c(1, 2, 8, 16) == 2 and c(2, 2, 8, 16) == 2 and c(5, 2, 8, 16) == 5
    assert c(8, 2, 8, 16) == 8 and c(9, 2, 8, 16) == 8 and c(2 ** 32 - 1, 2, 8, 16) == 8
    assert c(0, 20, 1000, 16) == 16 and c(3, 1, 1000, 16) == 3 and c(99, 1, 1000, 16) == 16     # both ends clamped to the lists
    assert c(7, 4, 4, 16) == 4                           # max_nprobe == nprobe: the uniform call
    with pytest.raises(ValueError):
        c(1, 3, 2, 16)
    assert depth_ref.used_given([0, 1, 3, 9], 2, 4, 3).tolist() == [2, 2, 3, 3]


def test_restatement_on_hand_made_centroids(oracle):
    # small-integer centroids and queries: every d2 is an exact integer
    cents = np.array([[0, 0], [2, 1], [1, 3], [4, 4], [9, 9]], np.float32)
    lists = [np.array([0], np.uint32), np.array([1, 2], np.uint32), np.array([3], np.uint32), np.array([4, 5, 6], np.uint32),
             np.array([7], np.uint32)]
    oidx = oracle.index_from_parts(2, cents, lists)
    q = np.array([2.0, 2.0], np.float32)       # d2: c1 1, c2 2, c0 8, c3 8, c4 98
    assert depth_ref.probe_order(oidx, q, 5).tolist() == [1, 2, 0, 3, 4]
    assert depth_ref.probe_d2(oracle, oidx, q, 5).tolist() == [1, 2, 8, 8, 98]
    used = lambda ratio, p0=1, mx=5, qq=q: int(depth_ref.used_ratio(oracle, oidx, [qq], ratio, p0, mx)[0])
    assert used(1.0) == 1 and used(2.0) == 2 and used(7.9) == 2 and used(8.0) == 4 and used(97.0) == 4 and used(INF) == 5
    assert used(8.0, mx=3) == 3 and used(1.0, p0=3) == 3 and used(INF, mx=1000) == 5
    on = np.array([4.0, 4.0], np.float32)       # a query equal to a centroid: d2_0 == 0
    assert depth_ref.probe_d2(oracle, oidx, on, 2).tolist()[0] == 0
    assert used(1.0, qq=on) == 1 and used(1e30, qq=on) == 1 and used(INF, qq=on) == 1 and used(INF, p0=2, qq=on) == 2
    # cosine: the same rule over normalised centroids and queries
    n_oidx, nq = depth_ref.cosine_index_and_queries(oracle, oidx, lists, np.stack([q, on]))
    assert n_oidx.n_clusters == 5 and np.allclose((nq * nq).sum(1), 1.0, atol=1e-6)
    u = depth_ref.used_ratio(oracle, n_oidx, nq, INF, 1, 5)
    assert ((u == 5) | (u == 1)).all()


def test_symbols_exported_bound_and_in_sys_rs(lib):
    from pq_vector_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "pqv.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    raw = C.CDLL(_ffi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES
        assert getattr(lib, name).argtypes == _ffi.SIGNATURES[name][1]
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert re.search(r"pub fn %s\(" % name, sys_rs)
    # the descriptor: the header's fields in the header's order, the same layout in ctypes and in sys.rs
    m = re.search(r"typedef struct pqv_probe_depth \{(.*?)\} pqv_probe_depth;", hdr, re.S)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["kind", "max_nprobe", "d2_ratio", "depths"] == [n for n, _ in _ffi.ProbeDepth._fields_]
    assert C.sizeof(_ffi.ProbeDepth) == 24 and _ffi.ProbeDepth.depths.offset == 16 and _ffi.ProbeDepth.d2_ratio.offset == 8
    assert "pub struct PqvProbeDepth { pub kind: u32, pub max_nprobe: u32, pub d2_ratio: f32, pub depths: *const c_void }" in sys_rs
    assert (_ffi.PQV_DEPTH_GIVEN, _ffi.PQV_DEPTH_RATIO) == (0, 1)
    assert "#define PQV_DEPTH_GIVEN 0" in hdr and "#define PQV_DEPTH_RATIO 1" in hdr
    assert "pub fn topk_depth" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()


def test_c_abi_checks_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)         # never dereferenced: every check below comes before a handle is read
    nq = 2
    q = (C.c_float * (4 * nq))()
    rows, dist, used = (C.c_uint32 * (2 * nq))(), (C.c_float * (2 * nq))(), (C.c_uint32 * nq)()
    depths = (C.c_uint32 * nq)(1, 2)

    def desc(kind, max_nprobe, ratio=0.0, arr=None):
        return C.byref(_ffi.ProbeDepth(kind, max_nprobe, ratio, C.cast(arr, C.c_void_p) if arr is not None else None))

    def host(s, d, nprobe=1):
        return lib.pqv_topk_depth(s, d, q, nq, 4, 2, nprobe, 0, 1, rows, dist, None, None, used)

    def device(s, d, nprobe=1):
        return lib.pqv_topk_depth_device(s, d, None, nq, 2, nprobe, 0, 1, None, None, None, None, None, None, None)

    def err(rc, text):
        assert rc == inv and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())

    given, ratio = _ffi.PQV_DEPTH_GIVEN, _ffi.PQV_DEPTH_RATIO
    for call in (host, device):
        err(call(None, desc(ratio, 4, 2.0)), b"searcher must not be NULL")
        err(call(None, None), b"searcher must not be NULL")
        err(call(fake, None), b"depth must not be NULL")
        err(call(fake, desc(ratio, 2, 2.0), 3), b"max_nprobe must be >= nprobe")
        err(call(fake, desc(given, 0, 0.0, depths), 1), b"max_nprobe must be >= nprobe")
        err(call(fake, desc(7, 2, 2.0), 3), b"max_nprobe must be >= nprobe")           # ahead of the kind
        err(call(fake, desc(2, 4, 2.0, depths)), b"unknown depth kind 2")
        err(call(fake, desc(0xFFFFFFFF, 4, 2.0, depths)), b"unknown depth kind")
        err(call(fake, desc(given, 4, 2.0, None)), b"depths must not be NULL")
        for bad in (float("nan"), 0.999, 0.0, -1.0, -INF):
            err(call(fake, desc(ratio, 4, bad, depths)), b"d2_ratio must be >= 1 and not NaN")
        # the plain call's own checks follow: k and nprobe need no handle either
        err(lib.pqv_topk_depth(fake, desc(ratio, 4, 1.0), q, nq, 4, 0, 1, 0, 1, rows, dist, None, None, used), b"k must be > 0")
        err(lib.pqv_topk_depth_device(fake, desc(ratio, 4, INF), None, nq, 0, 1, 0, 1, None, None, None, None, None, None, None), b"k must be > 0")
        err(call(fake, desc(given, 4, 0.0, depths), 0), b"nprobe must be > 0")
    err(lib.pqv_topk_depth(fake, desc(ratio, 4, 1.0), q, nq, 4, 2, 1, 9, 1, rows, dist, None, None, used), b"unknown metric")


class _FakeCorpus:
    rows = 6


def test_python_wrapper_checks_before_device_use():
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters, s._corpus, s._columns = None, 4, 2, _FakeCorpus(), {}
    q = np.zeros((2, 4), np.float32)
    fake = pqv.RowKeys(8, s)
    try:
        with pytest.raises(pqv.PqvError, match="probe_depths and d2_ratio are mutually exclusive"):
            s.topk(q, 2, 1, max_nprobe=4, probe_depths=[1, 2], d2_ratio=2.0)
        with pytest.raises(pqv.PqvError, match="need max_nprobe"):
            s.topk(q, 2, 1, probe_depths=[1, 2])
        with pytest.raises(pqv.PqvError, match="need max_nprobe"):
            s.topk_device(8, 2, 2, 1, 8, 8, d2_ratio=2.0)
        with pytest.raises(pqv.PqvError, match="max_nprobe and max_candidates are mutually exclusive"):
            s.topk(q, 2, 1, max_candidates=5, max_nprobe=4, d2_ratio=2.0)
        with pytest.raises(pqv.PqvError, match="do not combine with mask= or keys=") as e:
            s.topk(q, 2, 1, max_nprobe=4, d2_ratio=2.0, keys=fake, query_keys=[1, 2])
        assert e.value.code == _ffi.PQV_ERR_UNSUPPORTED
        with pytest.raises(pqv.PqvError, match="do not combine with mask= or keys="):
            s.topk_device(8, 2, 2, 1, 8, 8, max_nprobe=4, probe_depths=8, keys=fake, query_keys=8)
        for bad in ([1], [1, 2, 3], [[1, 2]], [1.5, 2.0], [-1, 2], [1, 2 ** 32]):
            with pytest.raises(pqv.PqvError, match=r"probe_depths must be 2 integers"):
                s.topk(q, 2, 1, max_nprobe=4, probe_depths=bad)
    finally:
        fake._h = None
    d, alive = pqv.api._probe_depth(np.array([3, 0], np.int64), None, 4, 0, None, None, 2)
    assert (d.kind, d.max_nprobe, d.depths) == (_ffi.PQV_DEPTH_GIVEN, 4, alive.ctypes.data) and alive.dtype == np.uint32 and alive.tolist() == [3, 0]
    d, alive = pqv.api._probe_depth(None, INF, 9, 0, None, None, 2)
    assert (d.kind, d.max_nprobe, d.d2_ratio, d.depths, alive) == (_ffi.PQV_DEPTH_RATIO, 9, INF, None, None)
    d, _ = pqv.api._probe_depth(4096, None, 9, 0, None, None, 2, device=True)
    assert (d.kind, d.depths) == (_ffi.PQV_DEPTH_GIVEN, 4096)
    # the builder: d2_ratio needs max_nprobe and takes no filter; max_nprobe alone keeps its refusal
    with pytest.raises(pqv.PqvError, match="d2_ratio must be >= 1 and not NaN"):
        pqv.TopkBuilder(s, q[0]).d2_ratio(0.5)
    with pytest.raises(pqv.PqvError, match="d2_ratio must be >= 1 and not NaN"):
        pqv.TopkBuilder(s, q[0]).d2_ratio(float("nan"))
    with pytest.raises(pqv.PqvError, match="need max_nprobe"):
        pqv.TopkBuilder(s, q[0]).k(2).nprobe(1).d2_ratio(2.0).search()
    with pytest.raises(pqv.PqvError, match="does not combine with where") as e:
        pqv.TopkBuilder(s, q[0]).k(2).nprobe(1).d2_ratio(2.0).max_nprobe(4).where(np.ones(6, bool)).search()
    assert e.value.code == _ffi.PQV_ERR_UNSUPPORTED
    with pytest.raises(pqv.PqvError, match="pqv_topk_expand needs a row mask or row keys"):
        pqv.TopkBuilder(s, q[0]).k(2).nprobe(1).max_nprobe(4).search()
