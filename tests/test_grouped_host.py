"""Grouped top-k, host side: the numpy restatement (tests/grouped_ref.py) on a hand-made example, a Python model of the kernels'
WaveGroupedTopk (csrc/kernels_grouped.hip) held to the definition, the ABI surface, and the argument validation that needs no
device (the checks that need a real searcher are in tests/test_gpu_grouped.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distinct_ref
import grouped_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pqv_topk_grouped", "pqv_topk_grouped_device")
KEY_EMPTY = (1 << 64) - 1
SLOT_EMPTY = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_restatement_on_a_hand_made_example():
    # test_distinct_host's example: 12 rows of dimension 1, the query at 0: d2 = value^2; the candidate sequence is a permutation
    data = np.array([3, 1, 1, 2, 5, 1, 4, 2, 0.5, 6, 2, 7], np.float32).reshape(12, 1)
    col = np.array([10, 20, 30, 20, 10, 30, 40, 50, 60, 60, 40, 70], np.int64)
    cand = np.array([4, 5, 2, 1, 0, 3, 7, 6, 8, 9, 10, 11], np.uint32)
    q = np.zeros(1, np.float32)
    E = grouped_ref.EMPTY
    r, d2, g, c, nf, nc, ncons = grouped_ref.grouped_topk(cand, col, None, None, data, q, 4, 2)
    # S = rows 8 | 5 2 1 (d2 1, positions 1 2 3) | 3 7 10 (d2 4, positions 5 6 10) | 0 | 6 | 4 | 9 | 11.  Groups by first row: 60, 30, 20, 50.
    # Group 60's second row is row 9 at d2 = 36, behind eight rows of other groups; group 50 has one row.
    assert nf == 4 and g.tolist() == [60, 30, 20, 50] and c.tolist() == [2, 2, 2, 1]
    assert r.tolist() == [[8, 9], [5, 2], [1, 3], [7, E]]
    assert d2[:3].tolist() == [[0.25, 36.0], [1.0, 1.0], [1.0, 4.0]] and d2[3, 0] == 4.0 and np.isposinf(d2[3, 1])
    assert nc == 12 and ncons == 12
    # m = 1 is the distinct call; m larger than every group returns every row of the k groups
    r1 = grouped_ref.grouped_topk(cand, col, None, None, data, q, 12, 1)
    rd = distinct_ref.distinct_topk(cand, col, None, None, data, q, 12)
    assert r1[4] == len(rd[0]) and r1[0][:r1[4], 0].tolist() == rd[0].tolist() and r1[2][:r1[4]].tolist() == rd[2].tolist()
    r, _, g, c, nf, _, _ = grouped_ref.grouped_topk(cand, col, None, None, data, q, 9, 5)
    assert nf == 7 and c.tolist() == [2, 2, 2, 1, 2, 2, 1, 0, 0] and g[7:].tolist() == [0, 0] and (r[7:] == E).all()
    assert r[4].tolist() == [10, 6, E, E, E] and r[5].tolist() == [0, 4, E, E, E]
    # NULL keys belong to no group; a mask removes rows before grouping; the cap cuts before both
    valid = np.ones(12, np.uint8); valid[8] = 0; valid[5] = 0
    r, _, g, c, nf, _, ncons = grouped_ref.grouped_topk(cand, col, valid, None, data, q, 2, 3)
    assert g.tolist() == [30, 20] and r.tolist() == [[2, E, E], [1, 3, E]] and c.tolist() == [1, 2] and ncons == 10
    r, _, g, c, nf, nc, ncons = grouped_ref.grouped_topk(cand, col, None, None, data, q, 12, 2, max_candidates=5)
    assert nf == 3 and g[:3].tolist() == [30, 20, 10] and r[:3].tolist() == [[5, 2], [1, E], [0, 4]] and nc == 12 and ncons == 5
    assert grouped_ref.grouped_topk(cand[:0], col, None, None, data, q, 3, 2)[4] == 0


class WaveGroupedModel:
    """WaveGroupedTopk<S>: element e in slot register e // 64, lane e % 64, ascending by (slot, key); every step below is the
    kernel's, register by register."""

    def __init__(self, k, m):
        self.k, self.m = k, m
        km = k * m
        assert km <= 1024
        self.S = 1 if km <= 64 else 4 if km <= 256 else 16
        self.key = np.full((self.S, 64), KEY_EMPTY, np.uint64)       # one row per register, one column per lane
        self.slot = np.full((self.S, 64), SLOT_EMPTY, np.uint32)
        self.n = 0
        self.crossings = 0       # replaces whose span crossed a 64-entry register boundary

    def insert(self, x, sl):
        S, key, slot, m = self.S, self.key, self.slot, self.m
        x = np.uint64(x)
        lo = cnt = below = 0
        for s in range(S):                                   # three ballots per register
            same = slot[s] == sl
            lo += int((slot[s] < sl).sum())
            cnt += int(same.sum())
            below += int((same & (key[s] < x)).sum())
        p = lo + below
        if cnt < m:
            hi = self.n
            assert hi < S * 64
            self.n += 1
        else:
            if below == cnt:
                return
            hi = lo + cnt - 1
            if p // 64 != hi // 64:
                self.crossings += 1
        lanes = np.arange(64)
        for s in range(S - 1, -1, -1):
            if s * 64 > hi or s * 64 + 63 < p:
                continue
            up_k, up_s = np.roll(key[s], 1), np.roll(slot[s], 1)         # shfl_up by one inside the register (lane 0: itself) ...
            up_k[0], up_s[0] = key[s][0], slot[s][0]
            if s > 0:                                        # ... lane 0 takes lane 63 of the register below (not yet changed)
                up_k[0], up_s[0] = key[s - 1][63], slot[s - 1][63]
            e = s * 64 + lanes
            move, put = (e > p) & (e <= hi), e == p
            assert s > 0 or not move[0]                      # (lane 0 of register 0 never takes a shifted value)
            key[s] = np.where(put, x, np.where(move, up_k, key[s]))
            slot[s] = np.where(put, np.uint32(sl), np.where(move, up_s, slot[s]))

    def offer(self, tile):
        """one candidate per lane, lowest lane first"""
        for x, sl in tile:
            self.insert(x, sl)

    def flat(self):
        return list(zip(self.slot.reshape(-1).tolist(), self.key.reshape(-1).tolist()))

    def filled(self):
        f = self.flat()
        assert all(e == (SLOT_EMPTY, KEY_EMPTY) for e in f[self.n:])
        return f[:self.n]

    def result(self):
        """the fold's segmented write-out: {slot: keys ascending}"""
        out = {}
        for sl, x in self.filled():
            out.setdefault(sl, []).append(x)
        return out


def _definition(stream, k, m):
    """stream of (key, group value): groups ranked by their smallest key, the first k kept, m smallest keys each"""
    by = {}
    for x, g in stream:
        by.setdefault(g, []).append(x)
    ranked = sorted(by, key=lambda g: min(by[g]))[:k]
    return ranked, {i: sorted(by[g])[:m] for i, g in enumerate(ranked)}


@pytest.mark.parametrize("k,m", [(1, 2), (5, 3), (16, 4), (13, 5), (64, 4), (33, 8), (128, 8)])
def test_wave_grouped_model_equals_the_definition(k, m):
    """60 random streams per (k, m) (420 in all) with heavy d2 ties, each offered ascending, descending and shuffled, split over
    several waves' lists and folded through the same offer: every slot ends with its m smallest keys, the list stays sorted by
    (slot, key) and never holds more than m entries of a slot."""
    rng = np.random.default_rng(7000 + 100 * k + m)
    for it in range(60):
        n = int(rng.integers(1, 60 if it % 20 else 3 * k * m + 50))
        n_groups = int(rng.integers(1, max(2, n // 2 if it % 2 else 2 * k)))
        d = rng.integers(0, max(2, n // 8), n)               # few distance classes: ties inside and between groups
        pos = rng.permutation(4 * n)[:n]                     # unique positions
        grp = rng.integers(-n_groups, n_groups, n)
        stream = [((int(a) << 32) | int(b), int(c)) for a, b, c in zip(d, pos, grp)]
        ranked, exp = _definition(stream, k, m)
        slot_of = {g: i for i, g in enumerate(ranked)}       # pass 1 and the set kernel: group value -> slot
        members = [(x, slot_of[g]) for x, g in stream if g in slot_of]       # only members are offered
        for order in ("shuffled", "ascending", "descending"):
            s = members if order == "shuffled" else sorted(members, reverse=order == "descending")
            n_waves = int(rng.integers(1, 6))
            waves = [WaveGroupedModel(k, m) for _ in range(n_waves)]
            i = 0
            while i < len(s):
                t = int(rng.integers(1, 65))
                waves[int(rng.integers(0, n_waves))].offer(s[i:i + t])
                i += t
            fold = WaveGroupedModel(k, m)
            for w in waves:
                part = w.filled()                            # the written part of a partial list, 64 entries per step
                for e0 in range(0, len(part), 64):
                    fold.offer([(x, sl) for sl, x in part[e0:e0 + 64]])
            for w in waves + [fold]:
                f = w.filled()
                assert f == sorted(f) and len(f) <= k * m
                assert all(len(v) <= m for v in w.result().values())
            assert fold.result() == exp, (k, m, it, order)


def test_replace_across_a_register_boundary():
    """(k, m) = (33, 8): slot 7's segment is elements 56..63 and slot 8's 64..71.  A replace in slot 8 that ranks first moves
    inside register 1 only; with slot 7 one entry short, slot 8 straddles the boundary (63..70) and the replace shifts across it."""
    k, m = 33, 8
    w = WaveGroupedModel(k, m)
    for sl in range(k):
        for i in range(m if sl != 7 else m - 1):
            w.offer([(((10 + i) << 32) | (sl * 8 + i), sl)])
    assert w.n == k * m - 1 and w.flat()[63][0] == 8 and w.flat()[70][0] == 8
    before = w.result()
    w.offer([((1 << 32) | 999, 8)])                          # ranks first in slot 8: element 63; the largest, element 70, leaves
    assert w.crossings == 1
    got = w.result()
    assert got[8] == [(1 << 32) | 999] + before[8][:-1]
    assert {s: v for s, v in got.items() if s != 8} == {s: v for s, v in before.items() if s != 8}
    f = w.filled()
    assert f == sorted(f) and w.n == k * m - 1
    w.offer([((99 << 32) | 5, 8)])                           # not smaller than slot 8's largest: dropped
    assert w.result() == got
    w.offer([((99 << 32) | 6, 7)])                           # slot 7 has room: inserted at its end, everything behind moves up
    assert w.n == k * m and w.result()[7][-1] == (99 << 32) | 6 and w.result()[8] == got[8]


def test_grouped_symbols_exported_bound_and_in_sys_rs(lib):
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
    # the distinct twins plus group_size and group_rows
    assert len(_ffi.SIGNATURES["pqv_topk_grouped"][1]) == len(_ffi.SIGNATURES["pqv_topk_distinct"][1]) + 2
    assert len(_ffi.SIGNATURES["pqv_topk_grouped_device"][1]) == len(_ffi.SIGNATURES["pqv_topk_distinct_device"][1]) + 2
    for f, needle in (("bindings/rust/src/lib.rs", "pub fn topk_grouped("), ("bindings/rust/src/lib.rs", "pub struct GroupSearchResult"),
                      ("pq-vector_amd/host/pqv.hpp", "void topk_grouped(")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    assert "more than one row per group;" not in hdr         # no longer out of the distinct call's scope
    assert lib.pqv_abi_version() == 101


def test_grouped_c_abi_validates_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)         # never dereferenced: the NULL and zero checks come first
    q = (C.c_float * 4)()
    rows, dist, grp, cnt = (C.c_uint32 * 4)(), (C.c_float * 4)(), (C.c_int64 * 2)(), (C.c_uint32 * 2)()

    def host(s, keys, k=2, m=2):
        return lib.pqv_topk_grouped(s, keys, None, q, 1, 4, k, m, 1, 0, 0, 1, rows, dist, grp, cnt, None, None)

    def device(s, keys, k=2, m=2):
        return lib.pqv_topk_grouped_device(s, keys, None, None, 1, k, m, 1, 0, 0, 1, None, None, None, None, None, None, None)

    for call in (host, device):
        assert call(None, fake) == inv and b"searcher must not be NULL" in lib.pqv_last_error()
        assert call(fake, None) == inv and b"row keys must not be NULL" in lib.pqv_last_error()
        assert call(None, None) == inv and b"searcher must not be NULL" in lib.pqv_last_error()
        assert call(fake, fake, k=0) == inv and b"k must be > 0" in lib.pqv_last_error()
        assert call(fake, fake, m=0) == inv and b"group_size must be > 0" in lib.pqv_last_error()
        assert call(fake, fake, k=0, m=0) == inv and b"k must be > 0" in lib.pqv_last_error()


def test_python_layer_without_a_device():
    import pq_vector_amd as pqv
    assert pqv.GroupSearchResult in (getattr(pqv, n) for n in pqv.__all__)
    with pytest.raises(pqv.PqvError, match="group_size must be > 0"):
        pqv.TopkBuilder("nowhere.parquet", [0.0]).distinct_on("doc").group_size(0)
    # group_size() without distinct_on() is an error at search(), before any file or device is touched
    with pytest.raises(pqv.PqvError, match=r"group_size\(\) needs distinct_on\(\)"):
        pqv.TopkBuilder("nowhere.parquet", [0.0]).k(3).nprobe(1).group_size(2).search()
    with pytest.raises(pqv.PqvError, match=r"group_size\(\) needs distinct_on\(\)"):
        pqv.TableTopkBuilder(["a.parquet", "b.parquet"], [0.0]).k(3).nprobe(1).group_size(2).search()
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters, s._columns = None, 4, 2, {}
    qq = np.zeros((2, 4), np.float32)
    closed = pqv.RowKeys(None, s)
    with pytest.raises(pqv.PqvError, match="row keys must not be NULL"):
        s.topk_grouped(qq, 2, 2, 1, closed)
    with pytest.raises(pqv.PqvError, match="keys must be a RowKeys"):
        s.topk_grouped(qq, 2, 2, 1, None)
    with pytest.raises(pqv.PqvError, match="row keys must not be NULL"):
        s.topk_grouped_device(8, 2, 2, 2, 1, closed, 8, 8)
