"""numpy model of pqv_index_remove / pqv_index_compact (test infrastructure, like append_ref.py): none of it is code under test.

Remove rule: list c of the result = list c of the old index without the rows whose flag byte is non-zero, order kept; a row id
at or above len(flags) stays; a list that loses every row stays, empty.  The row bound (append_ref.row_bound of the OLD lists) is
carried over, not lowered.
Compact rule: M = the set of rows in the lists; the new id of row r is its rank in M; X_new = X[sorted M]; every list has the rank
applied element by element; old_row[j] = the old id of new row j."""
import numpy as np

import append_ref


def remove(lists, flags):
    """lists: k arrays of row ids; flags: bool / uint8 [n_flags], non-zero removes.  -> k uint32 arrays."""
    flags = np.asarray(flags).reshape(-1) != 0
    out = []
    for l in lists:
        l = np.asarray(l, np.uint32)
        inside = l.astype(np.int64) < len(flags)
        gone = np.zeros(len(l), bool)
        gone[inside] = flags[l[inside].astype(np.int64)]
        out.append(l[~gone])
    return out


def remove_rows(lists, rows):
    """rows: ids to remove, any order, duplicates allowed, ids that are not indexed ignored: the byte form over max id + 1 flags."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    rows = rows[rows < append_ref.row_bound(lists)]          # (flags at or above the bound touch no list: not materialised)
    flags = np.zeros(int(rows.max()) + 1 if rows.size else 0, np.uint8)
    flags[rows] = 1
    return remove(lists, flags)


def members(lists):
    """sorted unique row ids of the lists; raises ValueError where a row occurs more than once (pqv_index_compact refuses it)."""
    if not len(lists):
        return np.zeros(0, np.uint32)
    allr = np.concatenate([np.asarray(l, np.uint32) for l in lists]) if sum(len(l) for l in lists) else np.zeros(0, np.uint32)
    m = np.unique(allr)
    if len(m) != len(allr):
        raise ValueError("a row is indexed more than once")
    return m.astype(np.uint32)


def rank_map(lists, n):
    """new_id int64 [n]: rank of r among the members for a member r, -1 for every other row."""
    m = members(lists)
    new_id = np.full(n, -1, np.int64)
    new_id[m.astype(np.int64)] = np.arange(len(m))
    return new_id


def compact(lists, X):
    """-> (X_new, lists_new, old_row).  Raises ValueError for a repeated row or an id past X."""
    old_row = members(lists)
    if len(old_row) and int(old_row[-1]) >= len(X):
        raise ValueError("row id out of range")
    new_id = rank_map(lists, len(X))
    lists_new = [new_id[np.asarray(l, np.int64)].astype(np.uint32) for l in lists]
    return X[old_row.astype(np.int64)], lists_new, old_row


# the hand-made index of the tests: empty lists first, last and adjacent, a word boundary on either side, one list longer than a
# block's share of positions; ids that are not sorted across lists, and some row ids below the bound that no list holds
LENGTHS = [0, 0, 1, 63, 64, 65, 0, 4097, 0]
HAND_MADE_SPARE = 500


def hand_made(seed=5, dim=3):
    """-> (dim, centroids, lists): sum(LENGTHS) of the row ids [0, sum(LENGTHS) + HAND_MADE_SPARE) dealt at random."""
    rng = np.random.default_rng(seed)
    total = sum(LENGTHS)
    ids = rng.permutation(total + HAND_MADE_SPARE)[:total].astype(np.uint32)
    lists, at = [], 0
    for n in LENGTHS:
        lists.append(np.sort(ids[at:at + n]))
        at += n
    Cn = rng.random((len(LENGTHS), dim), dtype=np.float32)
    return dim, Cn, lists


def patterns(lists, rng):
    """name -> remove flags over row ids (uint8): the patterns every remove test runs, several of them defined by LIST POSITION."""
    off, rows = append_ref.offsets_and_rows(lists)
    bound = append_ref.row_bound(lists)
    npos = len(rows)

    def of(positions, n=bound):
        f = np.zeros(n, np.uint8)
        ids = rows[np.asarray(positions, np.int64)]
        f[ids[ids < n]] = 1
        return f
    out = {}
    out["none"] = np.zeros(bound, np.uint8)
    out["all"] = np.ones(bound, np.uint8)
    out["first_position"] = of([0])
    out["last_position"] = of([npos - 1])
    out["every_other_row"] = (np.arange(bound) % 2 == 0).astype(np.uint8)
    out["positions_60_199"] = of(np.arange(60, 200))              # whole words and both partial ends
    longest = int(np.argmax(np.diff(off.astype(np.int64))))
    out["one_whole_list"] = of(np.arange(int(off[longest]), int(off[longest + 1])))
    out["random_0.1"] = (rng.random(bound) < 0.1).astype(np.uint8)
    out["random_0.9"] = (rng.random(bound) < 0.9).astype(np.uint8)
    out["n_flags_0"] = np.zeros(0, np.uint8)
    f = np.zeros(bound - 100, np.uint8)                           # shorter than the bound, ones at its end: rows beyond stay
    f[-40:] = 1
    out["shorter_than_the_bound"] = f
    out["longer_than_the_bound"] = np.ones(bound + 1000, np.uint8)
    return out


PATTERN_NAMES = ["none", "all", "first_position", "last_position", "every_other_row", "positions_60_199", "one_whole_list",
                 "random_0.1", "random_0.9", "n_flags_0", "shorter_than_the_bound", "longer_than_the_bound"]


def messy_rows(flags, bound):
    """the rows form of a flags array: descending, with duplicates and ids that no list holds"""
    ids = np.nonzero(flags)[0].astype(np.uint32)
    return np.concatenate([ids[::-1], ids[:7], np.array([bound + 5, 0xFFFFFFFF], np.uint32)])


def row_bound(lists):
    return append_ref.row_bound(lists)


def blob(oracle, dim, C, lists):
    return append_ref.blob(oracle, dim, C, lists)
