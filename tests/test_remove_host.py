"""CPU tests of index remove and compact (pqv_index_remove / _device / _rows, pqv_index_compact): the ABI surface and the
validation of the product library, its host path against the numpy model tests/remove_ref.py, and the model itself against the
reference blob of the surviving rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import append_ref
import assign_exact
import build_reference
import remove_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pqv_index_remove": 5, "pqv_index_remove_device": 6, "pqv_index_remove_rows": 5, "pqv_index_compact": 6}


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
    for name, arity in NAMES.items():
        assert name in _ffi.SIGNATURES and name in hdr
        assert len(_ffi.SIGNATURES[name][1]) == len(hdr[name]) == arity
        assert hasattr(C.CDLL(_ffi.LIB_PATH), name)
    assert lib.pqv_abi_version() == 101


def _invalid(lib, rc, needle=None):
    from pq_vector_amd import _ffi
    assert rc == _ffi.PQV_ERR_INVALID
    text = lib.pqv_last_error().decode()
    assert text != ""
    if needle:
        assert needle in text, text


def test_validation_comes_before_any_device_work(lib):
    """Every case is PQV_ERR_INVALID with its text whether or not a device exists; `out` comes back NULL."""
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi
    dim, Cn, lists = remove_ref.hand_made()
    idx = pqv.Index.from_parts(dim, Cn, lists)
    null, nullout = _ffi.vp(), C.cast(None, C.POINTER(_ffi.vp))
    flags = np.zeros(8, np.uint8)
    fp, nofp = flags.ctypes.data_as(_ffi.u8p), C.cast(None, _ffi.u8p)
    rows = np.zeros(4, np.uint32)
    rp, norp = rows.ctypes.data_as(_ffi.u32p), C.cast(None, _ffi.u32p)

    def out():
        return _ffi.vp(1)

    o = out(); _invalid(lib, lib.pqv_index_remove(null, 0, fp, 8, C.byref(o)), "index must not be NULL"); assert not o.value
    _invalid(lib, lib.pqv_index_remove(idx._h, 0, fp, 8, nullout), "out must not be NULL")
    o = out(); _invalid(lib, lib.pqv_index_remove(idx._h, 0, nofp, 8, C.byref(o)), "remove must not be NULL"); assert not o.value
    o = out(); _invalid(lib, lib.pqv_index_remove(idx._h, 0, fp, (1 << 32) + 1, C.byref(o)), "2^32"); assert not o.value

    o = out(); _invalid(lib, lib.pqv_index_remove_device(null, 0, _ffi.vp(64), 8, null, C.byref(o)), "index must not be NULL"); assert not o.value
    _invalid(lib, lib.pqv_index_remove_device(idx._h, 0, _ffi.vp(64), 8, null, nullout), "out must not be NULL")
    o = out(); _invalid(lib, lib.pqv_index_remove_device(idx._h, 0, null, 8, null, C.byref(o)), "remove must not be NULL"); assert not o.value
    o = out(); _invalid(lib, lib.pqv_index_remove_device(idx._h, 0, _ffi.vp(64), (1 << 32) + 1, null, C.byref(o)), "2^32"); assert not o.value

    o = out(); _invalid(lib, lib.pqv_index_remove_rows(null, 0, rp, 4, C.byref(o)), "index must not be NULL"); assert not o.value
    _invalid(lib, lib.pqv_index_remove_rows(idx._h, 0, rp, 4, nullout), "out must not be NULL")
    o = out(); _invalid(lib, lib.pqv_index_remove_rows(idx._h, 0, norp, 4, C.byref(o)), "rows must not be NULL"); assert not o.value

    # compact: no corpus exists without a device, so the corpus is NULL throughout
    co, io = out(), out()
    _invalid(lib, lib.pqv_index_compact(idx._h, null, 0, C.byref(co), C.byref(io), norp), "index/corpus must not be NULL")
    assert not co.value and not io.value
    co, io = out(), out()
    _invalid(lib, lib.pqv_index_compact(null, null, 0, C.byref(co), C.byref(io), norp), "index/corpus must not be NULL")
    assert not co.value and not io.value
    io = out()
    _invalid(lib, lib.pqv_index_compact(idx._h, null, 0, nullout, C.byref(io), norp), "corpus_out/index_out must not be NULL")
    assert not io.value
    co = out()
    _invalid(lib, lib.pqv_index_compact(idx._h, null, 0, C.byref(co), nullout, norp), "corpus_out/index_out must not be NULL")
    assert not co.value


def test_device_form_needs_a_device_only_after_validation(lib):
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi
    dim, Cn, lists = remove_ref.hand_made()
    idx = pqv.Index.from_parts(dim, Cn, lists)
    o = _ffi.vp(1)
    rc = lib.pqv_index_remove_device(idx._h, 0, _ffi.vp(), 0, _ffi.vp(), C.byref(o))           # n_flags 0: NULL flags are fine
    if pqv.device_count() == 0:
        assert rc == _ffi.PQV_ERR_NO_DEVICE and not o.value
        assert "no HIP device" in lib.pqv_last_error().decode()
    else:
        assert rc == _ffi.PQV_OK
        made = pqv.Index(o)
        assert made.to_bytes() == idx.to_bytes()
    # ... and an invalid argument is reported first either way
    _invalid(lib, lib.pqv_index_remove_device(idx._h, 0, _ffi.vp(), 5, _ffi.vp(), C.byref(o)), "remove must not be NULL")


def _check_index(oracle, index, dim, Cn, lists, bound):
    off, rows = append_ref.offsets_and_rows(lists)
    assert index.to_bytes() == remove_ref.blob(oracle, dim, Cn, lists)
    assert np.array_equal(index.list_offsets, off)
    assert np.array_equal(index.list_rows, rows)
    assert index.n_rows == len(rows)
    assert index.row_bound == bound


def test_host_path_equals_the_model(lib, oracle):
    """PQV_DEVICE_LISTS=0 and a missing device both take the host path; it is the one this test reaches where no device exists
    (where one exists the same expectations hold for the device path)."""
    import pq_vector_amd as pqv
    dim, Cn, lists = remove_ref.hand_made()
    idx = pqv.Index.from_parts(dim, Cn, lists)
    before = idx.to_bytes()
    bound = append_ref.row_bound(lists)
    rng = np.random.default_rng(3)
    for name, flags in remove_ref.patterns(lists, rng).items():
        want = remove_ref.remove(lists, flags)
        got = idx.remove(flags=flags)
        _check_index(oracle, got, dim, Cn, want, bound)
        messy = remove_ref.messy_rows(flags, bound)               # any order, duplicates, unindexed ids
        want_rows = remove_ref.remove_rows(lists, messy)
        assert all(np.array_equal(a, b) for a, b in zip(want_rows, want)), name
        _check_index(oracle, idx.remove(messy), dim, Cn, want, bound)
        assert idx.to_bytes() == before, name
    # bool flags, and exactly one way of naming the rows
    assert idx.remove(flags=np.ones(bound, bool)).n_rows == 0
    with pytest.raises(pqv.PqvError, match="exactly one"):
        idx.remove()
    with pytest.raises(pqv.PqvError, match="exactly one"):
        idx.remove([1], flags=np.zeros(3, np.uint8))
    with pytest.raises(pqv.PqvError, match="bool or uint8"):
        idx.remove(flags=np.zeros(3, np.int32))


def test_host_path_chain_keeps_the_row_bound(lib, oracle):
    import pq_vector_amd as pqv
    dim, Cn, lists = remove_ref.hand_made()
    idx = pqv.Index.from_parts(dim, Cn, lists)
    bound = append_ref.row_bound(lists)
    top = np.arange(bound - 300, bound, dtype=np.uint32)          # the largest ids leave: the bound must not follow them down
    once = idx.remove(top)
    want = remove_ref.remove_rows(lists, top)
    assert remove_ref.row_bound(want) < bound
    _check_index(oracle, once, dim, Cn, want, bound)
    twice = once.remove(flags=(np.arange(bound) % 3 == 0))
    _check_index(oracle, twice, dim, Cn, remove_ref.remove(want, np.arange(bound) % 3 == 0), bound)
    # removing nothing is a copy
    assert twice.remove(np.zeros(0, np.uint32)).to_bytes() == twice.to_bytes()


# ------------------------------------------------------------------------------------------------------------- model properties
@pytest.fixture(scope="module")
def case(oracle):
    rng = np.random.default_rng(12)
    n, dim, k = 3000, 30, 7
    X = rng.random((n, dim), dtype=np.float32)
    oidx = oracle.build_index(X, n_clusters=k, max_iters=5, workers=1)
    Cn = oidx.centroids
    assign = assign_exact.nearest(X, Cn)[0]
    lists = [np.nonzero(assign == c)[0].astype(np.uint32) for c in range(k)]
    flags = rng.random(n) < 0.3
    return X, dim, k, Cn, lists, flags


def test_model_remove_then_compact_is_indexing_the_survivors(oracle, case):
    X, dim, k, Cn, lists, flags = case
    removed = remove_ref.remove(lists, flags)
    X_new, lists_new, old_row = remove_ref.compact(removed, X)
    survivors = np.nonzero(~flags)[0]
    assert np.array_equal(old_row, survivors)
    assert np.array_equal(X_new.view(np.uint32), X[survivors].view(np.uint32))
    want = build_reference.reference_blob(dim, Cn, assign_exact.nearest(X[survivors], Cn)[0], k)[0]
    assert remove_ref.blob(oracle, dim, Cn, lists_new) == want


def test_model_row_bound_does_not_move_and_rank_is_monotone(case):
    X, dim, k, Cn, lists, flags = case
    bound = remove_ref.row_bound(lists)
    assert bound == len(X)
    f = flags.copy()
    f[-50:] = True                                   # the last rows leave
    removed = remove_ref.remove(lists, f)
    assert remove_ref.row_bound(removed) < bound     # the model's lists end lower; the CONTRACT's bound is the old one (carried)
    new_id = remove_ref.rank_map(removed, len(X))
    kept = np.nonzero(new_id >= 0)[0]
    assert np.array_equal(kept, np.nonzero(~f)[0])
    assert (np.diff(new_id[kept]) == 1).all() and new_id[kept[0]] == 0          # strictly monotone, dense from 0
    _, lists_new, old_row = remove_ref.compact(removed, X)
    for a, b in zip(removed, lists_new):
        assert len(a) == len(b)
        assert (np.diff(b.astype(np.int64)) > 0).all()                            # lists stay ascending
        assert np.array_equal(old_row[b.astype(np.int64)], a)
    assert remove_ref.row_bound(lists_new) == len(old_row) == sum(len(l) for l in lists_new)


def test_model_refuses_what_compact_refuses(case):
    X, dim, k, Cn, lists, flags = case
    twice = [l.copy() for l in lists]
    twice[1] = np.concatenate([twice[1], twice[0][:1]])
    with pytest.raises(ValueError, match="more than once"):
        remove_ref.compact(twice, X)
    with pytest.raises(ValueError, match="out of range"):
        remove_ref.compact(lists, X[:-1])
    # a flags array shorter than the ids leaves the rows beyond it alone; rows that are not indexed are ignored
    short = remove_ref.remove(lists, np.ones(10, np.uint8))
    assert sum(len(l) for l in short) == len(X) - 10
    assert all(np.array_equal(a, b) for a, b in zip(remove_ref.remove_rows(lists, [len(X) + 7]), lists))
