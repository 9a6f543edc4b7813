"""numpy restatement of the normalisation behind PQV_COSINE (include/pqv.h), in float32:

  sq(v) = the PQV_L2SQ_REF4 chain of v against zero (range_oracle.l2_chain, pinned to the C oracle's pqo_squared_l2_ref4),
  r(v)  = 1.0f / sqrtf(sq(v)), 0 where sq(v) == 0 (numpy's float32 sqrt and division are correctly rounded),
  n(v)  = v * r(v), one float32 multiply per value.

A cosine call must return what the PQV_L2SQ_REF4 call (sqrt_out 0) returns on the normalised index, corpus and queries, every
distance halved: reference_setup() builds that searcher."""
import numpy as np

from range_oracle import REF4, l2_chain


def sq(rows):
    x = np.ascontiguousarray(rows, dtype=np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    return l2_chain(x, np.zeros(x.shape[1], dtype=np.float32), REF4)


def r(rows):
    s = sq(rows)
    with np.errstate(divide="ignore"):
        out = np.float32(1.0) / np.sqrt(s)
    out[s == 0] = np.float32(0.0)
    return out.astype(np.float32)


def normalise(rows):
    x = np.ascontiguousarray(rows, dtype=np.float32)
    x2 = x.reshape(1, -1) if x.ndim == 1 else x
    out = (x2 * r(x2)[:, None]).astype(np.float32)
    return out.reshape(x.shape)


def half(d2):
    """The cosine distance of a d2 of unit vectors: the float32 product 0.5f * d2."""
    return (np.float32(0.5) * np.asarray(d2, dtype=np.float32)).astype(np.float32)


def normalised_index(pqv, dim, centroids, lists):
    return pqv.Index.from_parts(dim, normalise(np.asarray(centroids, dtype=np.float32).reshape(-1, dim)), lists)
