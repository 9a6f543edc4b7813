"""How the GPU tests issue the call a spec of tests/mutated_cases.py names (test infrastructure shared by
tests/test_gpu_mutated_search.py and tests/test_gpu_probe_screen_modes.py): a searcher with the masks, columns and row keys of a
model (Handles), one call of the library as the dict mutated_cases.expect() gives for it (run), and the names the modes are
grouped by."""
import numpy as np

import distinct_filter_ref
from key_filter_ref import EQ, RANGE
from mutated_cases import is_depth

METRIC = {"l2": 0, "cos": 2, "dot": 4}
GROUPS = ["plain", "range", "metrics", "masks", "keys", "expand", "distinct", "depth"]


def group_of(sp):
    if sp["call"].startswith(("distinct", "grouped")):
        return "distinct"
    if is_depth(sp):          # (a depth spec carries maxp too)
        return "depth"
    if sp["maxp"]:
        return "expand"
    if sp["metric"] != "l2":
        return "metrics"
    if sp["filt"]:
        return "keys"
    if sp["mask"]:
        return "masks"
    return "range" if sp["call"] == "range" else "plain"


def heap_order(sp):
    """pqv_topk without a filter returns the reference's heap order, every other form orders by (d2, position): where distances tie
    the two differ by contract"""
    return sp["call"] == "topk" and not sp["mask"] and not sp["filt"] and sp["metric"] != "dot"


class Handles:
    """A searcher with its masks and row keys: the arrays of a model, cut to the rows the corpus has.  keep: an allow array every
    mask is combined with -- and which alone is the mask of a call that names none."""

    def __init__(self, pqv, model, searcher, n_rows=None, keep=None, masks=("dense", "sparse")):
        self.pqv, self.model, self.case, self.s = pqv, model, model.case, searcher
        n = model.n if n_rows is None else n_rows
        self.n = n
        self.mask_bytes = {name: (model.masks[name][:n] if keep is None else model.masks[name][:n] & keep[:n]) for name in masks}
        if keep is not None:
            self.mask_bytes[None] = keep[:n].copy()
        self.masks = {name: searcher.row_mask(a) for name, a in self.mask_bytes.items()}
        self.keys = {}
        for col, (values, valid) in model.cols.items():
            column = pqv.Column.upload(values[:n], None if valid is None else valid[:n].astype(np.uint8))
            if col == "ts":
                searcher.attach_column("ts", column, own=True)
                self.keys[col] = searcher.row_keys("ts")
            else:
                self.keys[col] = searcher.row_keys(column)
                column.close()

    def mask(self, name):
        return self.masks.get(name) if name is None or isinstance(name, str) else None

    def close(self):
        for h in list(self.masks.values()) + list(self.keys.values()) + [self.s]:
            h.close()


def _filter_kw(H, sp, nq):
    if not sp["filt"]:
        return None, {}
    col, kind, fs = H.case.filter_of(sp["filt"], nq)
    return H.keys[col], distinct_filter_ref.call_kw(kind, fs)


def _device_filter(torch, H, sp, nq, dev):
    """the device form's filter keywords: the query keys uploaded on the current stream -> (keys, keywords, what must stay alive)"""
    if not sp["filt"]:
        return None, {}, ()
    col, kind, fs = H.case.filter_of(sp["filt"], nq)
    _, a, b = distinct_filter_ref.descriptor(kind, fs)
    a_t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev, non_blocking=True)
    if kind == EQ:
        return H.keys[col], {"query_keys": a_t.data_ptr()}, (a_t,)
    b_t = torch.from_numpy(np.ascontiguousarray(b if len(b) else np.zeros(1, np.int64))).to(dev, non_blocking=True)
    return H.keys[col], {"query_key_ranges" if kind == RANGE else "query_key_sets": (a_t.data_ptr(), b_t.data_ptr())}, (a_t, b_t)


def run(H, sp, mask=None):
    """one call of the library -> the dict mutated_cases.expect() gives for it.  mask: the RowMask of a spec that carries its allow
    array instead of a mask's name"""
    Q = H.case.queries(sp)
    nq, k, call, s = len(Q), sp["k"], sp["call"], H.s
    metric, mask = METRIC[sp["metric"]], (H.mask(sp["mask"]) if mask is None else mask)
    if call.endswith("_device"):
        return _run_device(H, sp, Q, mask)
    keys, fkw = _filter_kw(H, sp, nq)
    if call == "topk" and is_depth(sp):
        # a uniform call at nprobe = P first, on the same searcher and stream: the scratch of the ranks a query does not walk then
        # holds valid-looking entries (tests/test_gpu_depth.py)
        s.topk(Q, k, sp["maxp"], metric=metric, sqrt_out=False)
        dkw = dict(probe_depths=sp["depths"]) if sp["depths"] is not None else dict(d2_ratio=sp["ratio"])
        out = s.topk(Q, k, sp["nprobe"], metric=metric, sqrt_out=sp["sqrt"], max_nprobe=sp["maxp"], **dkw)
        names = ["rows", "d", "nf", "nc", "used"]
    elif call == "topk":
        out = s.topk(Q, k, sp["nprobe"], max_candidates=sp["maxc"], metric=metric, sqrt_out=sp["sqrt"], mask=mask, keys=keys, max_nprobe=sp["maxp"], **fkw)
        names = ["rows", "d", "nf", "nc", "used"]
    elif call == "range":
        out = s.range_search(Q, sp["radius"], sp["nprobe"], max_candidates=sp["maxc"], max_results=sp["maxr"], metric=metric, mask=mask,
                             keys=keys, **fkw)
        names = ["lims", "rows", "d", "nw", "nc"]
    elif call == "distinct":
        out = s.topk_distinct(Q, k, sp["nprobe"], H.keys["doc"], mask=mask, max_candidates=sp["maxc"], metric=metric, sqrt_out=False,
                              filter_keys=keys, max_nprobe=sp["maxp"], **fkw)
        names = ["rows", "d", "grp", "nf", "nc", "used"]
    else:
        out = s.topk_grouped(Q, k, sp["m"], sp["nprobe"], H.keys["doc"], mask=mask, max_candidates=sp["maxc"], metric=metric, sqrt_out=False,
                             filter_keys=keys, max_nprobe=sp["maxp"], **fkw)
        names = ["rows", "d", "grp", "grows", "nf", "nc", "used"]
    return dict(zip(names, out))


def _run_device(H, sp, Q, mask):
    """the device forms on a stream of the caller's, the outputs pre-filled with garbage there"""
    import torch
    dev = torch.device("cuda", 0)
    nq, k, call, s = len(Q), sp["k"], sp["call"], H.s
    grouped = call == "grouped_device"
    shape = (nq, k, sp["m"]) if grouped else (nq, k)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        q_t = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev, non_blocking=True)
        keys, fkw, alive = _device_filter(torch, H, sp, nq, dev)
        r_t = torch.full(shape, 5, dtype=torch.int32, device=dev)
        d_t = torch.full(shape, -1.0, dtype=torch.float32, device=dev)
        g_t = torch.full((nq, k), 77, dtype=torch.int64, device=dev)
        c_t = torch.full((nq, k), 99, dtype=torch.int32, device=dev)
        nf_t = torch.full((nq,), 9, dtype=torch.int32, device=dev)
        nc_t = torch.full((nq,), 9, dtype=torch.int64, device=dev)
        u_t = torch.full((nq,), 7777, dtype=torch.int32, device=dev)
        kw = dict(mask=mask, max_candidates=sp["maxc"], metric=METRIC[sp["metric"]], sqrt_out=False, stream=side.cuda_stream, **fkw)
        if sp["maxp"]:
            kw.update(max_nprobe=sp["maxp"], d_nprobe_used=u_t.data_ptr())
        if is_depth(sp):
            # (the uniform call at nprobe = P first, as in run(); its outputs go to buffers of their own)
            p_r, p_d = torch.empty_like(r_t), torch.empty_like(d_t)
            s.topk_device(q_t.data_ptr(), nq, k, sp["maxp"], p_r.data_ptr(), p_d.data_ptr(), metric=METRIC[sp["metric"]], sqrt_out=False,
                          stream=side.cuda_stream)
            if sp["depths"] is not None:          # the depths uploaded on the side stream, alive until the synchronise
                dep_t = torch.from_numpy(np.ascontiguousarray(sp["depths"], dtype=np.uint32).view(np.int32).copy()).to(dev, non_blocking=True)
                alive = alive + (dep_t, p_r, p_d)
                kw["probe_depths"] = dep_t.data_ptr()
            else:
                alive = alive + (p_r, p_d)
                kw["d2_ratio"] = sp["ratio"]
        if call == "topk_device":
            s.topk_device(q_t.data_ptr(), nq, k, sp["nprobe"], r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), keys=keys, **kw)
        elif grouped:
            s.topk_grouped_device(q_t.data_ptr(), nq, k, sp["m"], sp["nprobe"], H.keys["doc"], r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(),
                                  c_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), filter_keys=keys, **kw)
        else:
            s.topk_distinct_device(q_t.data_ptr(), nq, k, sp["nprobe"], H.keys["doc"], r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(),
                                   nf_t.data_ptr(), nc_t.data_ptr(), filter_keys=keys, **kw)
    side.synchronize()
    del alive
    out = {"rows": r_t.cpu().numpy().view(np.uint32), "d": d_t.cpu().numpy(), "nf": nf_t.cpu().numpy().astype(np.uint32),
           "nc": nc_t.cpu().numpy().astype(np.uint64)}
    if call != "topk_device":
        out["grp"] = g_t.cpu().numpy()
    if grouped:
        out["grows"] = c_t.cpu().numpy().view(np.uint32)
    if sp["maxp"]:
        out["used"] = u_t.cpu().numpy().astype(np.uint32)
    return out
