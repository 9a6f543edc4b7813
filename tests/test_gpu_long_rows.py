"""The masked kernel family on rows that span more than one chunk of the exact-distance tile.

masked_stream_kernel (window sources WIN 0..6: row mask, keyed i32 / i64, per-query RANGE i32 / i64, per-query IN i32 / i64),
dot_stream_kernel's masked form, distinct_stream_kernel and grouped_stream_kernel each carry a copy of stream_kernel's chunk loop
`for (c0 = 0; c0 < G; c0 += CG)`.  Every other module of the family uses rows of one chunk; here every shape but dim 3 runs the
loop two or three times -- a full chunk followed by a full, a ragged or a one-group chunk, with and without a scalar tail, in the
aligned and unaligned, REF4 (CG 32 / 64) and SEQ (CG 16) instantiations, on padded and unpadded storage (tests/long_rows_cases.py:
SHAPES, chunk_plan; the fixture asserts the chunk count before anything runs and cross-checks the stored dimension against
describe()).  Every index has a list of 40 rows (a flush tile with nvalid < 64 on every chunk) and one of more than 512.

Every expectation is computed on the CPU: the numpy restatements under tests/ (mask_ref, key_filter_ref, distinct_ref,
grouped_ref, dot_ref, cosine_ref over range_oracle.l2_chain, pinned to the C oracle at these dimensions by
tests/test_long_rows_host.py) over the C oracle's candidate_rows.  Rows, distance bits, n_found, n_candidates, tie flags, group
keys and group counts must be equal; there is no tolerance.  The seeds make every query's distances pairwise distinct
(asserted per shape, here and on the host), so ties and heap history play no part.

Sensitivity, tried once on a scratch copy of kernels_mask.hip (nothing mutated is built or loaded by any test):
  M1  masked_stream_kernel computes goff without c0 (every chunk re-reads the first one): this module fails --
      test_masked_calls and test_keyed_calls on every shape of two or more chunks -- while tests/test_gpu_mask.py passes.
  M2  masked_stream_kernel sums CG * EPL values after every chunk instead of ng * EPL (stale values of the previous chunk):
      this module fails -- test_masked_calls and test_keyed_calls on every shape with a ragged last chunk."""
import re

import numpy as np
import pytest

import key_filter_ref
import long_rows_cases as L
from test_gpu_distinct import _device as distinct_device
from test_gpu_dot import _device as dot_device
from test_gpu_grouped import _device as grouped_device
from test_gpu_mask import Setup, _bits, _device as masked_device

pytestmark = pytest.mark.gpu

KS = (10, 100, 300)             # S = 1, 4, 16
KMS = ((5, 3), (33, 8))


class Live:
    """One shape on the device: test_gpu_mask.Setup with the re-cut lists, and the Case that holds its references."""

    def __init__(self, pqv, oracle, name):
        c = L.SHAPES[name]
        sdim, g, cg, chunks, tail, _ = L.plan_of(name)
        assert (g, cg, chunks, tail) == c["sees"], f"shape {name}: the dispatch or the padding rule changed"
        assert len(chunks) >= 2 or c["dim"] == 3, f"shape {name} no longer runs the chunk loop twice"
        self.pqv, self.name = pqv, name
        self.st = Setup(pqv, oracle, L.N, c["dim"], L.KC, seed=c["seed"], flags=pqv.PQV_LAYOUT_ROW_ORDER if c["row_order"] else 0,
                        lists=L.reshape_lists)
        self.s, self.q = self.st.s, self.st.queries
        self.case = L.Case(name, oracle, parts=(self.st.data, self.st.queries, self.st.centroids, self.st.lists))
        self.metric = {"l2": c["metric"], "cos": pqv.PQV_COSINE, "dot": pqv.PQV_DOT}[c["kind"]]
        m = re.search(r"rows stored zero-padded from (\d+) to (\d+) dims", self.s.describe(L.NQ, 10, 2, c["metric"]))
        assert ((int(m.group(1)), int(m.group(2))) if m else (c["dim"], c["dim"])) == (c["dim"], sdim), f"shape {name}: stored dimension"
        self.case.assert_lists()
        self.case.assert_distinct()
        self._masks, self._keys = {}, {}

    def mask(self, sel):
        if sel not in self._masks:
            self._masks[sel] = self.s.row_mask(self.case.masks[sel])
        return self._masks[sel]

    def keys(self, tag, values, valid):
        if tag not in self._keys:
            col = self.pqv.Column.upload(values, valid, device=0)
            self._keys[tag] = self.s.row_keys(col)
            col.close()
        return self._keys[tag]


def _fixture(name, shapes):
    @pytest.fixture(scope="module", params=shapes, name=name)
    def live(request, pqv, oracle):
        return Live(pqv, oracle, request.param)
    return live


l2_fixture = _fixture("l2", L.L2_SHAPES)
cos_fixture = _fixture("cos", L.COS_SHAPES)
dot_fixture = _fixture("dot", L.DOT_SHAPES)


def _same_topk(got, exp, what, flags=False):
    assert (np.asarray(got[2]) == exp[2]).all(), "n_found " + what
    assert (np.asarray(got[3]) == exp[3]).all(), "n_candidates " + what
    assert (got[0] == exp[0]).all(), "rows " + what
    assert (_bits(got[1]) == _bits(exp[1])).all(), "distance bits " + what
    if flags:
        assert (got[4] == exp[4]).all(), "tie flags " + what


def _same_range(got, exp, what):
    for name, g, e in zip(("lims", "rows", "distance bits", "n_within", "n_candidates"), got, exp):
        g, e = (_bits(g), _bits(e)) if name == "distance bits" else (np.asarray(g), np.asarray(e))
        assert g.shape == e.shape and (g == e).all(), f"{name} {what}"


def _masked_entry_points(live, allowed, call_kw, device, sqrt_default, what):
    """topk (sqrt_out = 0; once with the default where sqrt_default), the device form with and without tie flags where
    `device` is given, range_search with the default output and with sqrt_out = 0, each with and without max_results."""
    case, s, q = live.case, live.s, live.q
    for nprobe in L.NPROBES:
        for k in KS:
            w = f"{what} k={k} nprobe={nprobe}"
            exp = case.topk(allowed, k, nprobe)
            _same_topk(s.topk(q, k, nprobe, metric=live.metric, sqrt_out=False, **call_kw), exp, "topk " + w)
            if device is not None:
                for flags in (False, True):
                    _same_topk(device(s, q, k, nprobe, flags), exp, f"device flags={flags} " + w, flags)
        if sqrt_default:
            _same_topk(s.topk(q, 10, nprobe, metric=live.metric, **call_kw), case.topk(allowed, 10, nprobe, sqrt_out=True),
                       f"topk, default output {what} nprobe={nprobe}")
        for sqrt_out in (True, False):
            radius = case.radius(allowed, nprobe, sqrt_out)
            for max_results in (0, 7):
                got = s.range_search(q, radius, nprobe, max_results=max_results, metric=live.metric, sqrt_out=sqrt_out, **call_kw)
                exp = case.range(allowed, radius, nprobe, sqrt_out=sqrt_out, max_results=max_results)
                _same_range(got, exp, f"range sqrt_out={sqrt_out} max_results={max_results} {what} nprobe={nprobe}")
                assert got[3][0] > 0


@pytest.mark.parametrize("sel", ["1/64", "1/2"])
def test_masked_calls(l2, sel):
    """WIN 0: pqv_topk_masked, pqv_topk_masked_device with and without tie flags, pqv_range_search_masked."""
    m = l2.mask(sel)
    _masked_entry_points(l2, l2.case.masks[sel], dict(mask=m),
                         lambda s, q, k, nprobe, flags: masked_device(s, q, k, nprobe, flags, mask=m, metric=l2.metric),
                         sqrt_default=sel == "1/2", what=f"mask {sel}")


@pytest.mark.parametrize("width", [32, 64])
def test_keyed_calls(l2, width):
    """WIN 1..6: keyed (EQ), per-query RANGE and per-query IN on an i32 and an i64 column that carries NULLs, host top-k and range
    search; then each filter once under a shared row mask."""
    case = l2.case
    conv = (lambda v: np.asarray(v, dtype=np.int64)) if width == 32 else L.wide
    values = case.tenant if width == 32 else L.wide(case.tenant)
    valid = case.tenant_valid
    keys = l2.keys(f"tenant{width}", values, valid)
    qk = conv(L.QUERY_KEYS)
    lo, hi = conv(L.QUERY_RANGES[0]), conv(L.QUERY_RANGES[1])
    sets = [[int(v) for v in conv(s)] for s in L.QUERY_SETS]
    lims, vals = key_filter_ref.sets_to_csr(sets)
    filters = (("eq", dict(query_keys=qk), (key_filter_ref.EQ, qk, None)),
               ("range", dict(query_key_ranges=(lo, hi)), (key_filter_ref.RANGE, lo, hi)),
               ("in", dict(query_key_sets=sets), (key_filter_ref.IN, lims, vals)))
    for tag, kw, (kind, a, b) in filters:
        allowed = case.key_allowed(values, valid, kind, a, b)
        assert allowed[0].sum() > 128                                   # (query 0 fills whole tiles in the long list)
        _masked_entry_points(l2, allowed, dict(keys=keys, **kw), None, sqrt_default=False, what=f"{tag} i{width}")
    shared = case.masks["1/2"]
    m = l2.mask("1/2")
    for tag, kw, (kind, a, b) in filters:
        allowed = case.key_allowed(values, valid, kind, a, b, shared=shared)
        for k, nprobe in ((100, L.KC), (10, 2)):
            _same_topk(l2.s.topk(l2.q, k, nprobe, metric=l2.metric, sqrt_out=False, keys=keys, mask=m, **kw), case.topk(allowed, k, nprobe),
                       f"{tag} i{width} under a shared mask k={k} nprobe={nprobe}")
        radius = case.radius(allowed, L.KC)
        _same_range(l2.s.range_search(l2.q, radius, L.KC, metric=l2.metric, keys=keys, mask=m, **kw), case.range(allowed, radius, L.KC),
                    f"range {tag} i{width} under a shared mask")


@pytest.mark.parametrize("width", [32, 64])
def test_grouped_calls(l2, width):
    """pqv_topk_distinct and pqv_topk_grouped, host and device forms, about 16 rows per key: an i32 column with every row
    considered, and an i64 column with NULLs under a shared mask."""
    case, s, q = l2.case, l2.s, l2.q
    if width == 32:
        column, valid, shared, m = case.group, None, None, None
    else:
        column, valid, shared, m = L.wide(case.group), case.group_valid, case.masks["1/2"], l2.mask("1/2")
    keys = l2.keys(f"group{width}", column, valid)
    for nprobe in L.NPROBES:
        for k, gs in KMS:
            w = f"i{width} k={k} m={gs} nprobe={nprobe}"
            exp = case.distinct(column, valid, shared, k, nprobe)
            for form, got in (("host", s.topk_distinct(q, k, nprobe, keys, mask=m, metric=l2.metric, sqrt_out=False)),
                              ("device", distinct_device(s, q, k, nprobe, keys, mask=m, metric=l2.metric))):
                assert (got[3] == exp[3]).all(), f"distinct n_found {form} {w}"
                assert (got[0] == exp[0]).all(), f"distinct rows {form} {w}"
                assert (_bits(got[1]) == _bits(exp[1])).all(), f"distinct distance bits {form} {w}"
                assert (got[2] == exp[2]).all(), f"distinct group keys {form} {w}"
                assert (got[4] == exp[4]).all(), f"distinct n_candidates {form} {w}"
            exp = case.grouped(column, valid, shared, k, gs, nprobe)
            assert exp[3].max() > 1                                      # (groups of several rows are expected)
            for form, got in (("host", s.topk_grouped(q, k, gs, nprobe, keys, mask=m, metric=l2.metric, sqrt_out=False)),
                              ("device", grouped_device(s, q, k, gs, nprobe, keys, mask=m, metric=l2.metric))):
                assert (got[4] == exp[4]).all(), f"grouped n_found {form} {w}"
                assert (got[2] == exp[2]).all(), f"grouped group keys {form} {w}"
                assert (got[3] == exp[3]).all(), f"grouped group_rows {form} {w}"
                assert (got[0] == exp[0]).all(), f"grouped rows {form} {w}"
                assert (_bits(got[1]) == _bits(exp[1])).all(), f"grouped distance bits {form} {w}"
                assert (got[5] == exp[5]).all(), f"grouped n_candidates {form} {w}"


@pytest.mark.parametrize("sel", ["1/64", "1/2"])
def test_masked_cosine(cos, sel):
    """PQV_COSINE under a mask: the chain runs on the normalised rows, the range hit test on 0.5 d2 (the sqrt_out == 2 branch)."""
    m = cos.mask(sel)
    _masked_entry_points(cos, cos.case.masks[sel], dict(mask=m),
                         lambda s, q, k, nprobe, flags: masked_device(s, q, k, nprobe, flags, mask=m, metric=cos.metric),
                         sqrt_default=False, what=f"cosine mask {sel}")


@pytest.mark.parametrize("sel", ["1/64", "1/2", "none"])
def test_dot_calls(dot, sel):
    """PQV_DOT: dot_stream_kernel's masked form (WIN = 1) and, sel = none, the unmasked call through the same dot_tile."""
    if sel == "none":
        allowed, kw, m = None, {}, None
    else:
        m = dot.mask(sel)
        allowed, kw = dot.case.masks[sel], dict(mask=m)
    _masked_entry_points(dot, allowed, kw, lambda s, q, k, nprobe, flags: dot_device(s, q, k, nprobe, flags, mask=m),
                         sqrt_default=False, what=f"dot mask {sel}")
