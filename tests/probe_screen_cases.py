"""The tied centroid tables of tests/test_gpu_probe_screen.py (test infrastructure: numpy only, nothing here calls the library).
tests/test_probe_screen_bound.py holds them to their premise on the CPU -- how many contenders the screened probe's bound leaves a
query -- so that the GPU test needs no `if`.

all_equal(kc): every centroid is one point P; rows and queries P + 0.05 N(0, 1).  Every centroid's bounds are the same two numbers,
so every centroid is a contender of every query: kc > PR_CAP = 2048 sends every query to the all-exact fallback.
split_2040(): 2040 copies of one point A and 264 distinct centroids at A + 3 + U(0, 1), shuffled; queries A + 0.05 N(0, 1) -- their
contenders are exactly the 2040 copies, eight below the cap: 64 rounds of 32 -- but query FAR, 0.01 beside one of the 264."""
import numpy as np

DIM = 8
NQ = 17
FAR = 5                     # the one query of split_2040 that lies beside a far centroid
PR_CAP = 2048               # kernels_probe_screen.hip
N_COPIES, N_FAR = 2040, 264
# what query FAR may keep at nprobe 1 and 7, whatever the score's rounding: a contender has lb <= T <= the upper bound of the
# nprobe-th nearest centroid, so with W the widest interval of the query (it depends on the norms alone) its distance is at most
# (the nprobe-th smallest distance) + 2 W; counted in tests/test_probe_screen_bound.py
FAR_MAX = {1: 48, 7: 128}
ALL_EQUAL_KC = (2304, 3328)          # bounds parked in LDS (2 kc <= 32 * 196 words: kc <= 3136), and made again per read


def refused_tables(kc=130, dim=36):
    """name -> (data, centroids): tables whose |c - mean|^2 the screen cannot hold (probe_screen_images leaves ps.ok false).
    `norm above 3e38`: centroids next to FLT_MAX in +- pairs (test_gpu_probe_screen.py's `huge`), one of them scaled to a finite
    |c|^2 = 3.3e38; `inf component`: uniform centroids, one component +inf (the mean, and so every centred norm, is not finite)."""
    rng = np.random.default_rng(kc * 1000 + dim)
    n = _rows(kc)
    big = np.sqrt(2.4e38 / dim)
    sgn = np.where(rng.random((kc // 2, dim)) < 0.85, 1.0, -1.0)
    half = (big * (0.9 + 0.2 * rng.random((kc // 2, 1))) * sgn).astype(np.float32)
    cent = np.concatenate([half, -half])
    cent[5] = (np.sqrt(3.3e38 / dim) * sgn[5]).astype(np.float32)
    data = (cent[rng.integers(0, kc, n)] * (1.0 + 1e-3 * rng.standard_normal((n, 1)))).astype(np.float32)
    out = {"norm above 3e38": (data, cent)}
    data = rng.random((n, dim), dtype=np.float32)
    cent = data[rng.choice(n, kc, replace=False)].copy()
    cent[7, 3] = np.inf
    out["inf component"] = (data, cent)
    return out


def _rows(kc):
    return max(3 * kc, 600)


def all_equal(kc):
    """-> (data [n, 8], centroids [kc, 8], queries [NQ, 8])"""
    rng = np.random.default_rng(kc)
    point = rng.random(DIM, dtype=np.float32)
    cent = np.repeat(point[None, :], kc, axis=0)
    data = (point + np.float32(0.05) * rng.standard_normal((_rows(kc), DIM))).astype(np.float32)
    queries = (point + np.float32(0.05) * rng.standard_normal((NQ, DIM))).astype(np.float32)
    return data, np.ascontiguousarray(cent), queries


def split_2040():
    """-> (data [n, 8], centroids [2304, 8], queries [NQ, 8])"""
    kc = N_COPIES + N_FAR
    rng = np.random.default_rng(2040)
    a = rng.random(DIM, dtype=np.float32)
    far = (a + np.float32(3) + rng.random((N_FAR, DIM), dtype=np.float32)).astype(np.float32)
    cent = np.concatenate([np.repeat(a[None, :], N_COPIES, axis=0), far])
    order = rng.permutation(kc)
    cent = np.ascontiguousarray(cent[order])
    n = _rows(kc)
    data = (a + np.float32(0.05) * rng.standard_normal((n, DIM))).astype(np.float32)
    there = rng.random(n) < 0.25                                 # a quarter of the rows lie around the far centroids
    data[there] = (far[rng.integers(0, N_FAR, int(there.sum()))] + np.float32(0.05) * rng.standard_normal((int(there.sum()), DIM))).astype(np.float32)
    queries = (a + np.float32(0.05) * rng.standard_normal((NQ, DIM))).astype(np.float32)
    queries[FAR] = far[10] + np.float32(0.01 / np.sqrt(DIM))     # 0.01 away
    return data, cent, queries
