"""CPU tests of index append (pqv_index_assign / pqv_index_append): the ABI surface and NULL handling of the product library,
and the numpy model tests/append_ref.py that the GPU tests take their expectations from, checked against the reference blob."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import append_ref
import assign_exact
import build_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "pq-vector_amd", "libpqv_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pq-vector_amd", "csrc")])
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_symbols_are_bound_with_the_header_arity(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_sys
    from pq_vector_amd import _ffi
    hdr = {name: params for name, _, params in gen_rust_sys.parse_header()}
    for name in ("pqv_index_assign", "pqv_index_append"):
        assert name in _ffi.SIGNATURES and name in hdr
        assert len(_ffi.SIGNATURES[name][1]) == len(hdr[name]) == 5
        assert hasattr(C.CDLL(_ffi.LIB_PATH), name)
    assert lib.pqv_abi_version() == 101


def test_null_arguments_are_invalid_before_any_device_work(lib):
    """No corpus exists without a device, so the corpus is NULL throughout; index / out / cluster_out take turns."""
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi
    idx = pqv.Index.from_parts(2, np.zeros((1, 2), np.float32), [np.zeros(0, np.uint32)])
    null = _ffi.vp()
    buf = np.zeros(4, np.uint32)
    bufp = buf.ctypes.data_as(_ffi.u32p)
    nullp = C.cast(None, _ffi.u32p)

    def invalid(rc):
        assert rc == _ffi.PQV_ERR_INVALID
        assert lib.pqv_last_error().decode() != ""

    invalid(lib.pqv_index_assign(null, null, 0, 0, bufp))
    invalid(lib.pqv_index_assign(idx._h, null, 0, 0, bufp))
    invalid(lib.pqv_index_assign(idx._h, null, 0, 0, nullp))
    invalid(lib.pqv_index_assign(null, null, 0, 0, nullp))
    out = _ffi.vp(1)                       # must come back NULL
    invalid(lib.pqv_index_append(null, null, 0, 0, C.byref(out)))
    assert not out.value
    out = _ffi.vp(1)
    invalid(lib.pqv_index_append(idx._h, null, 0, 0, C.byref(out)))
    assert not out.value
    invalid(lib.pqv_index_append(idx._h, null, 0, 0, C.cast(None, C.POINTER(_ffi.vp))))


@pytest.fixture(scope="module")
def case(oracle):
    rng = np.random.default_rng(11)
    n0, m, dim, k = 3000, 1000, 30, 7
    X = rng.random((n0 + m, dim), dtype=np.float32)
    oidx = oracle.build_index(X[:n0], n_clusters=k, max_iters=5, workers=1)
    return X, n0, m, dim, k, oidx


def test_model_equals_the_reference_blob_over_the_longer_column(oracle, case):
    X, n0, m, dim, k, oidx = case
    Cn = oidx.centroids
    lists, assign = append_ref.append_lists(oidx.lists(), X, Cn, n0, m)
    assert len(assign) == m
    want = build_reference.reference_blob(dim, Cn, assign_exact.nearest(X, Cn)[0], k)[0]
    assert append_ref.blob(oracle, dim, Cn, lists) == want
    for l in lists:
        assert (np.diff(l.astype(np.int64)) > 0).all()
    assert sum(len(l) for l in lists) == n0 + m
    assert append_ref.row_bound(lists) == n0 + m
    assert append_ref.row_bound(oidx.lists()) == n0
    off, rows = append_ref.offsets_and_rows(lists)
    assert int(off[-1]) == len(rows) == n0 + m


def test_model_keeps_old_lists_that_are_not_the_nearest_assignment(case):
    X, n0, m, dim, k, oidx = case
    Cn = oidx.centroids
    wrong = [np.arange(c, n0, k, dtype=np.uint32) for c in range(k)]          # rows dealt round robin
    assert any(not np.array_equal(w, l) for w, l in zip(wrong, oidx.lists()))
    lists, assign = append_ref.append_lists(wrong, X, Cn, n0, m)
    for c in range(k):
        assert np.array_equal(lists[c][:len(wrong[c])], wrong[c])
        assert np.array_equal(lists[c][len(wrong[c]):], n0 + np.nonzero(assign == c)[0])


def test_model_row_bound_rule(case):
    X, n0, m, dim, k, oidx = case
    Cn = oidx.centroids
    with pytest.raises(ValueError, match="below the row bound"):
        append_ref.append_lists(oidx.lists(), X, Cn, n0 - 1, m)
    with pytest.raises(ValueError, match="past the corpus"):
        append_ref.append_lists(oidx.lists(), X, Cn, n0, m + 1)
    same, _ = append_ref.append_lists(oidx.lists(), X, Cn, n0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(same, oidx.lists()))
    gap, assign = append_ref.append_lists(oidx.lists(), X, Cn, n0 + 17, m - 17)
    got = np.sort(np.concatenate(gap))
    assert np.array_equal(got, np.concatenate([np.arange(n0), np.arange(n0 + 17, n0 + m)]))
    assert append_ref.row_bound([np.zeros(0, np.uint32)] * 3) == 0
