"""Distinct top-k, host side: the numpy restatement (tests/distinct_ref.py) on a hand-made example, a Python model of the kernels'
WaveDistinctTopk (csrc/kernels_distinct.hip) held to the definition, the ABI surface, and the argument validation that needs no
device (the checks that need a real searcher are in tests/test_gpu_distinct.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distinct_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pqv_topk_distinct", "pqv_topk_distinct_device")
KEY_EMPTY = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_restatement_on_a_hand_made_example():
    # 12 rows of dimension 1, the query at 0: d2 = value^2.  The candidate sequence is a permutation, so position != row.
    data = np.array([3, 1, 1, 2, 5, 1, 4, 2, 0.5, 6, 2, 7], np.float32).reshape(12, 1)
    col = np.array([10, 20, 30, 20, 10, 30, 40, 50, 60, 60, 40, 70], np.int64)
    cand = np.array([4, 5, 2, 1, 0, 3, 7, 6, 8, 9, 10, 11], np.uint32)
    q = np.zeros(1, np.float32)
    r, d2, g, nc, ncons = distinct_ref.distinct_topk(cand, col, None, None, data, q, 12)
    # rows 5 (pos 1), 2 (pos 2) and 1 (pos 3) tie at d2 = 1: inside group 30 the position decides (row 5), and between the groups
    # 30 and 20 it decides too (30 first); rows 3 / 7 / 10 tie at 4: group 20 is taken already, 50 (pos 6) precedes 40 (pos 10)
    assert r.tolist() == [8, 5, 1, 7, 10, 0, 11]
    assert g.tolist() == [60, 30, 20, 50, 40, 10, 70]
    assert d2.tolist() == [0.25, 1.0, 1.0, 4.0, 4.0, 9.0, 49.0]
    assert nc == 12 and ncons == 12
    assert distinct_ref.distinct_topk(cand, col, None, None, data, q, 3)[0].tolist() == [8, 5, 1]
    # NULL keys belong to no group; a mask removes rows before grouping; the cap cuts before both
    valid = np.ones(12, np.uint8); valid[8] = 0; valid[5] = 0
    r, _, g, _, ncons = distinct_ref.distinct_topk(cand, col, valid, None, data, q, 4)
    assert r.tolist() == [2, 1, 7, 10] and g.tolist() == [30, 20, 50, 40] and ncons == 10
    mask = np.ones(12, bool); mask[[2, 1]] = False
    r, _, g, _, ncons = distinct_ref.distinct_topk(cand, col, valid, mask, data, q, 3)
    assert r.tolist() == [3, 7, 10] and g.tolist() == [20, 50, 40] and ncons == 8
    r, _, g, nc, ncons = distinct_ref.distinct_topk(cand, col, None, None, data, q, 12, max_candidates=5)
    assert r.tolist() == [5, 1, 0] and g.tolist() == [30, 20, 10] and nc == 12 and ncons == 5
    # i32 columns are widened
    assert distinct_ref.distinct_topk(cand, col.astype(np.int32), None, None, data, q, 12)[2].dtype == np.int64
    assert distinct_ref.distinct_topk(cand[:0], col, None, None, data, q, 3)[0].size == 0


class WaveDistinctModel:
    """WaveDistinctTopk<S, GW>: element e in slot e // 64, lane e % 64; every step below is the kernel's, slot by slot."""

    def __init__(self, k):
        self.k = k
        self.S = 1 if k <= 64 else 4 if k <= 256 else 16
        self.key = [[KEY_EMPTY] * 64 for _ in range(self.S)]
        self.grp = [[0] * 64 for _ in range(self.S)]

    def kth(self):
        e = self.k - 1
        return self.key[e >> 6][e & 63]

    def insert(self, x, g):
        S, key, grp = self.S, self.key, self.grp
        e_old, old_key = -1, KEY_EMPTY
        for s in range(S):                                   # a ballot per slot: the one filled entry of g's group
            m = [l for l in range(64) if key[s][l] != KEY_EMPTY and grp[s][l] == g]
            if m:
                e_old, old_key = s * 64 + m[0], key[s][m[0]]
        if e_old >= 0 and old_key < x:
            return
        p = sum(1 for s in range(S) for l in range(64) if key[s][l] < x)
        hi = e_old if e_old >= 0 else S * 64 - 1
        for s in range(S - 1, -1, -1):
            if s * 64 > hi or s * 64 + 63 < p:
                continue
            up_k = [None] + key[s][:63]                      # shfl_up by one inside the slot ...
            up_g = [None] + grp[s][:63]
            if s > 0:                                        # ... lane 0 takes lane 63 of the slot below (not yet changed)
                up_k[0], up_g[0] = key[s - 1][63], grp[s - 1][63]
            for l in range(64):
                e = s * 64 + l
                if p < e <= hi:
                    key[s][l], grp[s][l] = up_k[l], up_g[l]
                elif e == p:
                    key[s][l], grp[s][l] = x, g
        assert all(v is not None for s in range(S) for v in key[s])

    def offer(self, tile):
        """one candidate per lane, the kernel's loop: the lowest admitted lane first, the rest re-tested against the new k-th"""
        mine = list(tile)
        m = [l for l, (x, _) in enumerate(mine) if x < self.kth()]
        while m:
            x, g = mine[m[0]]
            self.insert(x, g)
            thr = self.kth()
            m = [l for l in m[1:] if mine[l][0] < thr]

    def result(self):
        flat = [(self.key[s][l], self.grp[s][l]) for s in range(self.S) for l in range(64)]
        return [e for e in flat[:self.k] if e[0] != KEY_EMPTY], flat


def _definition(stream, k):
    best = {}
    for x, g in stream:
        if g not in best or x < best[g]:
            best[g] = x
    return sorted((x, g) for g, x in best.items())[:k]


@pytest.mark.parametrize("k", [1, 3, 64, 65, 200])
def test_wave_distinct_model_equals_the_definition(k):
    """400 random streams per k (2 000 in all), each offered in random, ascending and descending key order, in tiles of up to 64
    lanes: the first k entries are always the k smallest group representatives, the whole list stays sorted and distinct."""
    rng = np.random.default_rng(1000 + k)
    for it in range(400):
        n = int(rng.integers(1, 40 if it % 8 else 330))
        n_groups = int(rng.integers(1, max(2, 2 * n)))
        d = rng.integers(0, max(2, n // 2), n)              # few distance classes: ties inside and between groups
        pos = rng.permutation(4 * n)[:n]                    # unique positions
        grp = rng.integers(-n_groups, n_groups, n)
        stream = [((int(a) << 32) | int(b), int(c)) for a, b, c in zip(d, pos, grp)]
        exp = _definition(stream, k)
        for order in ("random", "ascending", "descending"):
            s = stream if order == "random" else sorted(stream, reverse=order == "descending")
            w = WaveDistinctModel(k)
            i = 0
            while i < len(s):
                t = int(rng.integers(1, 65))
                w.offer(s[i:i + t])
                i += t
            got, flat = w.result()
            assert got == exp, (k, it, order)
            keys = [x for x, _ in flat]
            assert keys == sorted(keys)
            filled = [g for x, g in flat if x != KEY_EMPTY]
            assert len(filled) == len(set(filled))


def test_slot_boundary_replace_shift():
    """a replace whose span crosses the slot boundary: elements (p, e_old] move up, nothing falls off the end"""
    w = WaveDistinctModel(130)
    for i in range(130):
        w.offer([(((i + 1) << 32) | i, i)])
    before = w.result()[0]
    w.offer([((0 << 32) | 999, 100)])                    # group 100 sat at element 100 (slot 1); its new key ranks first
    got = w.result()[0]
    assert got[0] == (999, 100) and len(got) == 130
    assert got[1:] == [e for e in before if e[1] != 100]
    w.offer([((50 << 32) | 5, 3)])                       # a worse member of a listed group: admitted by the k-th, then dropped
    assert w.result()[0] == got


def test_distinct_symbols_exported_bound_and_in_sys_rs(lib):
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
    # the masked twins plus keys and group_key; the device form has no tie flags
    assert len(_ffi.SIGNATURES["pqv_topk_distinct"][1]) == len(_ffi.SIGNATURES["pqv_topk_masked"][1]) + 2
    assert len(_ffi.SIGNATURES["pqv_topk_distinct_device"][1]) == len(_ffi.SIGNATURES["pqv_topk_masked_device"][1]) + 1
    for f, needle in (("bindings/rust/src/lib.rs", "pub fn topk_distinct("), ("bindings/rust/src/lib.rs", "pub struct DistinctSearchResult"),
                      ("pq-vector_amd/host/pqv.hpp", "void topk_distinct(")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    assert lib.pqv_abi_version() == 101


def test_distinct_c_abi_validates_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)         # never dereferenced: the NULL checks come first
    q = (C.c_float * 4)()
    rows, dist, grp = (C.c_uint32 * 2)(), (C.c_float * 2)(), (C.c_int64 * 2)()

    def host(s, keys, k=2):
        return lib.pqv_topk_distinct(s, keys, None, q, 1, 4, k, 1, 0, 0, 1, rows, dist, grp, None, None)

    def device(s, keys, k=2):
        return lib.pqv_topk_distinct_device(s, keys, None, None, 1, k, 1, 0, 0, 1, None, None, None, None, None, None)

    for call in (host, device):
        assert call(None, fake) == inv and b"searcher must not be NULL" in lib.pqv_last_error()
        assert call(fake, None) == inv and b"row keys must not be NULL" in lib.pqv_last_error()
        assert call(None, None) == inv and b"searcher must not be NULL" in lib.pqv_last_error()
        assert call(fake, fake, k=0) == inv and b"k must be > 0" in lib.pqv_last_error()


def test_k_must_be_positive_without_a_device():
    """ "k must be > 0" comes from validate_topk behind the handle checks; the Python layer and the builders refuse k = 0 themselves"""
    import pq_vector_amd as pqv
    assert pqv.DistinctSearchResult in (getattr(pqv, n) for n in pqv.__all__)
    with pytest.raises(pqv.PqvError, match="k must be > 0"):
        pqv.TopkBuilder("nowhere.parquet", [0.0]).distinct_on("doc").k(0)
    with pytest.raises(pqv.PqvError, match="needs a column name or a RowKeys"):
        pqv.TopkBuilder("nowhere.parquet", [0.0]).distinct_on(3)
    with pytest.raises(pqv.PqvError, match="needs a Searcher source"):
        pqv.TopkBuilder("nowhere.parquet", [0.0]).distinct_on(pqv.RowKeys(None, None))
    with pytest.raises(pqv.PqvError, match="needs a column name"):
        pqv.TableTopkBuilder(["a.parquet", "b.parquet"], [0.0]).distinct_on(pqv.RowKeys(None, None))
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters, s._columns = None, 4, 2, {}
    qq = np.zeros((2, 4), np.float32)
    closed = pqv.RowKeys(None, s)
    with pytest.raises(pqv.PqvError, match="row keys must not be NULL"):
        s.topk_distinct(qq, 2, 1, closed)
    with pytest.raises(pqv.PqvError, match="keys must be a RowKeys"):
        s.topk_distinct(qq, 2, 1, None)
    with pytest.raises(pqv.PqvError, match="row keys must not be NULL"):
        s.topk_distinct_device(8, 2, 2, 1, closed, 8, 8)
