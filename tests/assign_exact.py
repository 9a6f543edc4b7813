"""Exact nearest-centroid assignment, decided in float64 with a rigorous rounding bound (test infrastructure).

`nearest(X, C)` returns, for every row of X [n, d] f32, the index the reference's nearest_centroid returns
(src/ivf/index.rs:244-257): distances by the 4-grouped f32 chain squared_l2_distance (index.rs:461-480, the C oracle's
pqo_squared_l2_ref4), strict '<' from +inf, so the lowest index wins a tie and NaN never wins.  Evaluating that chain
for every (row, centroid) pair costs as much as the oracle itself; instead an f64 GEMM estimates every distance, and
the chain is evaluated only where the estimate cannot decide.

The bound.  Let S_ij = sum_e (x_e - c_e)^2 exactly, u = 2^-24, G = d // 4, r = d % 4.
  * The chain.  Each term passes through at most m = G + r + 6 roundings: the difference and the square (the
    difference's error enters squared: 3 factors (1 + delta)), 3 additions inside its group of four, G group
    accumulations, r tail additions.  Every term is non-negative, so |chain - S| <= gamma_m * S with
    gamma_m = m u / (1 - m u) (about 1.2e-5 at d = 768).  Additions and subtractions whose result is subnormal are
    exact; a square that underflows adds at most 2^-150 absolutely, so a = d * 2^-149 covers all of them.
    Every intermediate is at most S (1 + gamma_m), so no step overflows while S (1 + gamma_m) < 2^127.
  * The estimate.  e_ij = nx_i + f_ij, f_ij = nc_j - 2 x_i.c_j from one f64 GEMM (torch.addmm), nx / nc the f64
    squared norms.  Products of two f32 values are exact in f64 (48-bit significands, no underflow), so only the
    summations round: in any order, FMA or not, the error of a sum of t terms is at most gamma64_t times the sum of
    their magnitudes, and sum_e |x_e c_e| <= (nx + nc) / 2.  Norms, dot product, the +nc term, the +nx term and the
    f64 arithmetic of the thresholds below add up to |e_ij - S_ij| <= K (nx_i + nc_j), K = (4 d + 32) 2^-53.
    This is the term that keeps data far from the origin (where e is a difference of huge norms) safe.
  * Hence lo_ij = (1 - gamma_m) e_ij - K (nx_i + nc_j) - a <= chain_ij <= (1 + gamma_m)(e_ij + K (nx_i + nc_j)) + a.
Decision for row i: j* = argmin_j e_ij, Kmax_i = K (nx_i + max_j nc_j), R_i = (1 + gamma_m)(e_ij* + Kmax_i) + Kmax_i + 2a.
Every j with e_ij > R_i / (1 - gamma_m) has chain_ij >= lo_ij > R_i - Kmax_i - a >= chain_ij*, so it can neither be
nor tie the minimum.  If j* is the only index left, j* is the answer; otherwise the exact f32 chain
(range_oracle.l2_chain, REF4: its bits are pinned to the C oracle by tests/test_range_host.py) is evaluated on the
candidates that are left and the lowest index among the minima wins.  Rows or centroids with a non-finite value, and
rows whose bound reaches 2^127 (where a chain could overflow), take the exact path over all centroids.

`bound_scale` multiplies gamma_m, K and a; 0 turns the bound off (the negative control of tests/test_assign_exact_host.py).
"""
import numpy as np

from range_oracle import REF4, l2_chain

_PAIR_BATCH = 1 << 16
_OVERFLOW = 2.0 ** 127


def chain_gamma(dim):
    m = dim // 4 + dim % 4 + 6
    mu = m * 2.0 ** -24
    return mu / (1.0 - mu)


def _slab_rows(k):
    return max(1, (1 << 24) // max(k, 1))          # 16 M f64 (128 MiB) per distance slab


def _exact_pairs(X, C, rows, cols):
    """f32 chain values for the (row, centroid) pairs, in batches."""
    out = np.empty(len(rows), np.float32)
    for p0 in range(0, len(rows), _PAIR_BATCH):
        r, c = rows[p0:p0 + _PAIR_BATCH], cols[p0:p0 + _PAIR_BATCH]
        with np.errstate(over="ignore", invalid="ignore"):      # non-finite rows: inf / NaN, as in the reference
            out[p0:p0 + len(r)] = l2_chain(X[r], C[c], REF4)
    return out


def _resolve(X, C, rows, cols):
    """Reference semantics over each row's candidates: the lowest index among the smallest chain values below +inf
    (NaN and +inf never win), index 0 when none is.  rows ascending; cols ascending within a row."""
    d2 = _exact_pairs(X, C, rows, cols)
    d2[~(d2 < np.inf)] = np.inf
    order = np.lexsort((cols, d2, rows))
    r_sorted = rows[order]
    first = np.ones(len(order), bool)
    first[1:] = r_sorted[1:] != r_sorted[:-1]
    pick = order[first]
    ans = np.where(d2[pick] < np.inf, cols[pick], 0).astype(np.uint32)
    return rows[pick], ans


def nearest(X, C, bound_scale=1.0):
    """-> (assign [n] u32, stats {"rows", "exact_rows", "max_candidates"}).  X [n, d] f32 (any array numpy can slice:
    it is read one slab at a time), C [k, d] f32."""
    import torch
    C = np.ascontiguousarray(C, dtype=np.float32)
    n, d = X.shape
    k = C.shape[0]
    assert k >= 1 and C.shape[1] == d
    gam = chain_gamma(d) * bound_scale
    K = (4 * d + 32) * 2.0 ** -53 * bound_scale
    a = d * 2.0 ** -149 * bound_scale
    Cd = torch.from_numpy(C).double()
    col_ok = torch.isfinite(Cd).all(dim=1)
    Cd[~col_ok] = 0.0
    nc = (Cd * Cd).sum(dim=1)
    nc_max = float(nc[col_ok].max()) if bool(col_ok.any()) else 0.0
    CdT = Cd.t().contiguous()
    bad_cols = torch.nonzero(~col_ok).flatten()
    assign = np.empty(n, np.uint32)
    ex_rows, ex_cols = [], []
    exact_rows = max_cand = 0
    for s in range(0, n, _slab_rows(k)):
        xs = np.ascontiguousarray(X[s:s + _slab_rows(k)], dtype=np.float32)
        Xd = torch.from_numpy(xs).double()
        row_ok = torch.isfinite(Xd).all(dim=1)
        Xd[~row_ok] = 0.0
        nx = (Xd * Xd).sum(dim=1)
        f = torch.addmm(nc[None, :], Xd, CdT, alpha=-2.0)          # e - nx
        if len(bad_cols):
            f[:, bad_cols] = np.inf
        fmin, jstar = f.min(dim=1)
        e_min = nx + fmin
        kmax = K * (nx + nc_max)
        R = (1.0 + gam) * (e_min + kmax) + kmax + 2.0 * a
        thr = R / (1.0 - gam) - nx
        full = ~row_ok | ~(R < _OVERFLOW)                          # (NaN R included)
        mask = f <= thr[:, None]
        mask[full] = True
        count = mask.sum(dim=1)
        js = jstar.numpy().astype(np.uint32)
        assign[s:s + len(xs)] = js
        amb = torch.nonzero(count > 1).flatten()
        if len(amb):
            r_loc, c_idx = torch.nonzero(mask[amb], as_tuple=True)
            ex_rows.append(amb[r_loc].numpy().astype(np.int64) + s)
            ex_cols.append(c_idx.numpy().astype(np.int64))
            exact_rows += len(amb)
            max_cand = max(max_cand, int(count[amb].max()))
        if len(ex_rows) and sum(len(r) for r in ex_rows) >= _PAIR_BATCH:
            _flush(X, C, ex_rows, ex_cols, assign)
    _flush(X, C, ex_rows, ex_cols, assign)
    return assign, {"rows": n, "exact_rows": exact_rows, "max_candidates": max_cand}


def _flush(X, C, ex_rows, ex_cols, assign):
    if not ex_rows:
        return
    rows, ans = _resolve(X, C, np.concatenate(ex_rows), np.concatenate(ex_cols))
    assign[rows] = ans
    ex_rows.clear()
    ex_cols.clear()


def explain(X, C, row, got, want):
    """What a failing test reports about one row: both clusters, both chain values, the f64 margin e_got - e_want."""
    x = np.asarray(X[row], np.float32)
    cg, cw = np.asarray(C[got], np.float32), np.asarray(C[want], np.float32)
    chain = l2_chain(np.stack([cg, cw]), x, REF4)
    e = ((x.astype(np.float64)[None, :] - np.stack([cg, cw]).astype(np.float64)) ** 2).sum(axis=1)
    return {"row": int(row), "got": int(got), "want": int(want), "chain_got": float(chain[0]),
            "chain_want": float(chain[1]), "f64_margin": float(e[0] - e[1])}


def mismatches(X, C, got, want):
    """-> None when got == want, else a report: how many rows differ and explain() of the first one."""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero(got != want)[0]
    if len(bad) == 0:
        return None
    r = int(bad[0])
    return {"n_differ": int(len(bad)), "first": explain(X, C, r, int(got[r]), int(want[r]))}
