"""Range search, host side: the ABI surface, argument validation before any device use, and the numpy range oracle
(tests/range_oracle.py) that the GPU tests compare against, pinned to the C oracle's distance chains."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from range_oracle import REF4, SEQ, l2_chain, range_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_range_symbols_exported_bound_and_in_sys_rs(lib):
    from pq_vector_amd import _ffi
    for name in ("pqv_range_search", "pqv_range_free"):
        assert name in _ffi.SIGNATURES
        assert getattr(lib, name).argtypes == _ffi.SIGNATURES[name][1]
        assert re.search(r"\b%s\s*\(" % name, open(os.path.join(ROOT, "include", "pqv.h")).read())
        assert re.search(r"pub fn %s\(" % name, open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read())
    assert len(_ffi.SIGNATURES["pqv_range_search"][1]) == 15
    assert "range_search" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert lib.pqv_abi_version() == 101


def test_range_c_abi_validates_before_device_use(lib):
    from pq_vector_amd import _ffi
    lims, rows, dist = _ffi.u64p(), _ffi.u32p(), _ffi.f32p()
    q = (C.c_float * 4)()
    rc = lib.pqv_range_search(None, q, 1, 4, 1.0, 1, 0, 0, 0, 1, C.byref(lims), C.byref(rows), C.byref(dist), None, None)
    assert rc == _ffi.PQV_ERR_INVALID and b"searcher must not be NULL" in lib.pqv_last_error()
    lib.pqv_range_free(None, None, None)        # NULL buffers are fine


def test_range_builder_validation():
    import pq_vector_amd as pqv
    assert pqv.RangeBuilder in (getattr(pqv, n) for n in pqv.__all__)
    q = np.zeros(4, np.float32)
    with pytest.raises(pqv.PqvError, match="radius must be set"):
        pqv.RangeBuilder("/nonexistent.parquet", q).nprobe(2).search()
    with pytest.raises(pqv.PqvError, match="nprobe must be set"):
        pqv.RangeBuilder("/nonexistent.parquet", q).radius(1.0).search()
    with pytest.raises(pqv.PqvError, match="nprobe must be > 0"):
        pqv.RangeBuilder("/nonexistent.parquet", q).radius(1.0).nprobe(0)
    with pytest.raises(pqv.PqvError, match="radius must not be NaN") as e:
        pqv.RangeBuilder("/nonexistent.parquet", q).radius(float("nan"))
    assert e.value.code == -1


def test_searcher_range_search_validation_before_device_use():
    import pq_vector_amd as pqv
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters = None, 4, 2
    with pytest.raises(pqv.PqvError, match="radius must not be NaN"):
        s.range_search(np.zeros((2, 4), np.float32), math.nan, 1)
    with pytest.raises(pqv.PqvError, match="Query dimension mismatch: expected 4, got 3"):
        s.range_search(np.zeros((2, 3), np.float32), 1.0, 1)
    with pytest.raises(pqv.PqvError, match="nprobe must be > 0"):
        s.range_search(np.zeros((2, 4), np.float32), 1.0, 0)
    s._h = None


@pytest.mark.parametrize("dim", [1, 3, 4, 30, 64, 130])
def test_numpy_chains_match_c_oracle_bits(oracle, dim):
    rng = np.random.default_rng(dim)
    x = (rng.standard_normal((3000 // max(1, dim // 32), dim)) * rng.choice([1e-3, 1.0, 1e3], size=(1, dim))).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    r4, sq = l2_chain(x, q, REF4), l2_chain(x, q, SEQ)
    for i in range(len(x)):
        assert r4[i].view(np.uint32) == oracle.l2_ref4(x[i], q).view(np.uint32)
        assert sq[i].view(np.uint32) == oracle.l2_seq(x[i], q).view(np.uint32)


def test_numpy_range_oracle_semantics(oracle):
    rng = np.random.default_rng(3)
    data = rng.integers(0, 3, size=(3000, 8)).astype(np.float32)
    oidx = oracle.build_index(data, n_clusters=6, workers=1, max_iters=4)
    q = data[17]
    cand = oidx.candidate_rows(q, 3)
    d2 = np.array([oracle.l2_ref4(data[r], q) for r in cand], np.float32)
    radius = float(np.sort(np.sqrt(d2))[len(d2) // 3])
    rows, dist, nw, nc = range_query(cand, data, q, radius)
    assert nc == len(cand) and nw == len(rows) == int((np.sqrt(d2) <= np.float32(radius)).sum())
    # (d2, position) order: equal distances keep candidate order
    pos = {int(r): i for i, r in enumerate(cand)}
    keys = [(float(d), pos[int(r)]) for r, d in zip(rows, dist)]
    assert keys == sorted(keys)
    assert (dist.view(np.uint32) == np.sqrt(d2[[pos[int(r)] for r in rows]]).view(np.uint32)).all()
    assert 17 in rows.tolist() and dist[0] == 0.0
    # caps: a prefix, n_within unchanged; candidates cut in a list's middle
    r2, d2b, nw2, _ = range_query(cand, data, q, radius, max_results=5)
    assert nw2 == nw and (r2 == rows[:5]).all()
    r3, _, nw3, nc3 = range_query(cand, data, q, math.inf, max_candidates=len(cand) // 2 + 1)
    assert nc3 == len(cand) and nw3 == len(cand) // 2 + 1 and set(r3.tolist()) == set(cand[:nw3].tolist())
    assert range_query(cand, data, q, -1.0)[2] == 0
    r2cut = float(np.sort(d2)[len(d2) // 3])
    r4, d4, nw4, _ = range_query(cand, data, q, r2cut, sqrt_out=False)
    assert nw4 == int((d2 <= np.float32(r2cut)).sum()) and (d4 <= np.float32(r2cut)).all()
