"""The round-robin cap of table searchers, host side: pqv_round_robin_quota against the oracle's CandidateCursor
(access.rs:214-242) and a numpy restatement of its closed form, the PQV_TABLE_CAP_ROUND_ROBIN constant across the header,
ctypes and the Rust externs, and the table builders' max_candidates checks before any device use."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cursor_tallies(oracle, counts, m):
    """Per-file counts of what one next_batch(m) of a fresh cursor takes (the oracle's restatement of access.rs:214-242)."""
    lists = [np.arange(c, dtype=np.uint32) for c in counts]
    taken = np.zeros(len(counts), dtype=np.uint64)
    for f, row in oracle.candidate_cursor_take(lists, int(m)):
        assert row == taken[f]                   # each file's candidates in their own order
        taken[f] += 1
    return taken


def _closed_form(counts, m):
    """t_f = min(c_f, L) + [c_f > L and f among the first M - S(L) such files], L the largest level with S(L) <= M."""
    c = np.asarray(counts, dtype=object)
    total = sum(int(x) for x in c)
    if m == 0 or m >= total:
        return [int(x) for x in c]
    lo, hi = 0, max(int(x) for x in c)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if sum(min(int(x), mid) for x in c) <= m:
            lo = mid
        else:
            hi = mid
    rem = m - sum(min(int(x), lo) for x in c)
    out = []
    for x in c:
        t = min(int(x), lo)
        if int(x) > lo and rem:
            t += 1
            rem -= 1
        out.append(t)
    return out


def test_quota_equals_the_cursor_on_random_counts(oracle):
    import pq_vector_amd as pqv
    rng = np.random.default_rng(2048)
    n_cases = 0
    for it in range(1000):
        F = int(rng.integers(1, 20))
        counts = rng.integers(0, 60, F)
        if it % 7 == 0:
            counts[rng.random(F) < 0.4] = 0                   # zero-count files
        if it % 11 == 0:
            counts[:] = int(rng.integers(0, 30))              # all equal
        total = int(counts.sum())
        for m in {int(rng.integers(0, total + 8)), 1, max(F - 1, 1), F, max(total - 1, 0), total, total + 5}:
            got = pqv.round_robin_quota(counts, m)
            want = counts.astype(np.uint64) if m == 0 else _cursor_tallies(oracle, counts, m)
            assert got.tolist() == want.tolist(), (counts.tolist(), m)
            assert int(got.sum()) == (total if m == 0 else min(m, total))
            n_cases += 1
    assert n_cases > 3000


def test_quota_of_counts_beyond_32_bits_follows_the_closed_form():
    import pq_vector_amd as pqv
    rng = np.random.default_rng(7)
    for _ in range(200):
        F = int(rng.integers(1, 9))
        counts = rng.integers(0, 1 << 40, F, dtype=np.uint64)
        counts[rng.random(F) < 0.2] = 0
        total = int(sum(int(x) for x in counts))
        for m in (1, F, int(rng.integers(1, max(2, total))), max(total - 1, 1), total, total + 5, (1 << 63)):
            assert pqv.round_robin_quota(counts, m).tolist() == _closed_form(counts, m)
    # the one-file case is a prefix; no files is no work
    assert pqv.round_robin_quota([1 << 35], 12345).tolist() == [12345]
    assert pqv.round_robin_quota(np.zeros(0, np.uint64), 5).tolist() == []


def test_flag_constant_matches_across_header_ffi_and_rust():
    from pq_vector_amd import _ffi
    import pq_vector_amd as pqv
    hdr = open(os.path.join(ROOT, "include", "pqv.h")).read()
    m = re.search(r"#define\s+PQV_TABLE_CAP_ROUND_ROBIN\s+(0x[0-9a-fA-F]+)u", hdr)
    assert m and int(m.group(1), 16) == _ffi.PQV_TABLE_CAP_ROUND_ROBIN == pqv.PQV_TABLE_CAP_ROUND_ROBIN == 0x8
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    m = re.search(r"pub const PQV_TABLE_CAP_ROUND_ROBIN: u32 = (0x[0-9a-fA-F]+);", sys_rs)
    assert m and int(m.group(1), 16) == 0x8
    assert "pub fn pqv_round_robin_quota(counts: *const u64, n_files: u32, max_candidates: u64, quota: *mut u64) -> c_int;" in sys_rs
    assert '"pqv_round_robin_quota": (C.c_int, [u64p, C.c_uint32, C.c_uint64, u64p])' in open(_ffi.__file__).read()
    # the other creation flags keep their bits
    assert len({_ffi.PQV_LAYOUT_ROW_ORDER, _ffi.PQV_RELEASE_ROW_ORDER, _ffi.PQV_RELEASE_IF_COPIED, _ffi.PQV_TABLE_CAP_ROUND_ROBIN}) == 4


def test_quota_rejects_null_arguments():
    import ctypes as C
    from pq_vector_amd import _ffi
    lib = _ffi.lib()
    out = (C.c_uint64 * 2)()
    assert lib.pqv_round_robin_quota(None, 2, 5, out) == _ffi.PQV_ERR_INVALID
    assert lib.pqv_round_robin_quota(None, 0, 5, None) == _ffi.PQV_OK


@pytest.mark.parametrize("bad", [0, -1, 1 << 64, 2.5, "10", None, True])
def test_builders_reject_a_bad_max_candidates_before_device_use(bad, tmp_path):
    import pq_vector_amd as pqv
    missing = [str(tmp_path / "nowhere.parquet")]             # never opened: the check comes first
    q = np.zeros(4, np.float32)
    for builder in (pqv.TableTopkBuilder(missing, q).k(3).nprobe(2), pqv.TableRangeBuilder(missing, q).radius(1.0).nprobe(2)):
        with pytest.raises(pqv.PqvError, match="max_candidates") as e:
            builder.max_candidates(bad)
        assert e.value.code == pqv._ffi.PQV_ERR_INVALID


def test_builders_accept_a_cap_without_touching_a_device(tmp_path):
    import pq_vector_amd as pqv
    missing = [str(tmp_path / "nowhere.parquet")]
    q = np.zeros(4, np.float32)
    b = pqv.TableTopkBuilder(missing, q).k(3).nprobe(2).max_candidates(np.uint64(2048))
    assert b._max_candidates == 2048
    r = pqv.TableRangeBuilder(missing, q).radius(1.0).nprobe(2).max_candidates(1)
    assert r._max_candidates == 1
