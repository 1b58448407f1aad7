#!/usr/bin/env python3
"""Device set operations over dense result columns (hdk_hip_concat_columns, hdk_hip_setop_columns,
DeviceColumns.union / intersect / except_) on one MI355X.  Rows are (a, 3 a + 1): two int64 columns, equal rows = equal a.

    isect90     INTERSECT, left 100 M rows, right 10 M distinct rows, 90 % of the left rows present on the right
    isect1      the same with 1 %
    exceptall   EXCEPT ALL, right 10 M rows in runs of about 10 equal rows, 10 % of the left rows present on the right
    union_half  UNION of two results of 100 M distinct rows each that share half their rows
    small       INTERSECT of 10 000 x 1 000 rows, wall clock, against the host

Per large case: hdk_hip_concat_columns alone and hdk_hip_setop_columns alone over the already sorted tagged block (HIP
events, median of --reps calls after warm-up, workspace and output preallocated), its count-only call, the method end to end
(DeviceColumns, wall clock: concat + sort + set operation + its allocations and the one wait), and three comparisons:
(a) the modelled bytes at the copy rate hdk_hip_mgr_measure_hbm reports in the same process -- the model: summary 8 n k,
keep 8 n (k + 1) + n / 8, compact n / 8 + 16 m o for n rows, k keys, o outs, m kept rows; concat 16 bytes per row and column
plus 8 per row for the side column --, (b) the same rows from existing stages (UNION: union(all) + group_by(ID ...);
INTERSECT / EXCEPT: join(semi / anti) on column 0 + group_by, which is the same only because equal a means equal rows and
only for the forms without ALL), (c) to_host() of both inputs + numpy.  Every output word is first compared with numpy
(counts per value by np.bincount: no host sort).

    python scripts/bench_setop_columns.py [--only isect90,isect1,exceptall,union_half,small] [--rows N] [--right-rows N] [--reps 5] [--out f.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = {"union": 0, "intersect": 1, "intersect_all": 2, "except": 3, "except_all": 4}


def events_ms(mgr, stream, call, reps):
    import torch
    ms = []
    for i in range(2 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        mgr.synchronizeStream(0)
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def wall_ms(fn, reps, warm=1):
    ms = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if hasattr(r, "free"):
            r.free()
        if i >= warm:
            ms.append(dt)
    return statistics.median(ms), ms


def expected(la, ra, op):
    """column a of the result, ascending: from the counts per value"""
    top = int(max(la.max(initial=0), ra.max(initial=0))) + 1
    cl, cr = np.bincount(la, minlength=top), np.bincount(ra, minlength=top)
    if op == "union":
        return np.flatnonzero((cl + cr) > 0)
    if op == "intersect":
        return np.flatnonzero((cl > 0) & (cr > 0))
    if op == "intersect_all":
        return np.repeat(np.arange(top), np.minimum(cl, cr))
    if op == "except":
        return np.flatnonzero((cl > 0) & (cr == 0))
    return np.repeat(np.arange(top), np.maximum(cl - cr, 0))


def host_way(mgr, L, R, op):
    """(c): both inputs to the host, then numpy"""
    la, ra = L.to_host()[0], R.to_host()[0]
    if op == "union":
        a = np.union1d(la, ra)
    elif op == "intersect":
        a = np.intersect1d(la, ra)
    elif op == "except":
        a = np.setdiff1d(la, ra)
    else:
        a = expected(la, ra, op)  # (numpy has no multiset difference: the counts)
    return a, 3 * a + 1


def columns_of(mgr, a):
    from hdk_amd.executor import DeviceColumns
    from hdk_amd.ir import Type
    from hdk_amd.plan import ColumnDesc
    n = len(a)
    block = mgr.to_device(np.concatenate([a, 3 * a + 1]), 0)
    ty = Type("int", 8, False)
    return DeviceColumns(None, mgr, 0, block, n, n, schema=[ColumnDesc("a", False, False, 0, ty, 0, "proj"),
                                                            ColumnDesc("b", False, False, 0, ty, 1, "proj")])


def stages(mgr, L, R, op, reps, copy_gbps):
    """the two calls alone, over preallocated memory, on the launch stream"""
    import torch
    from hdk_amd import _abi as A
    from hdk_amd._lib import check, lib
    lib_ = lib()
    nl, nr = L.num_rows, R.num_rows
    n = nl + nr
    pairs = (A.SetopCol * 2)(A.SetopCol(0, 0, 0, 0, (C.c_uint8 * 6)(), 0, 0, 0), A.SetopCol(1, 1, 0, 0, (C.c_uint8 * 6)(), 0, 0, 0))
    d_cat, d_srt = mgr.alloc(3 * n * 8, 0), mgr.alloc(3 * n * 8, 0)
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))

    def concat():
        check(lib_.hdk_hip_concat_columns(R.block.ptr, R.capacity, 2, nr, L.block.ptr, L.capacity, 2, nl, pairs, 2, 2,
                                          A.CONCAT_TAG_FIRST, d_cat.ptr, n, 0, None))

    cat_ms, cat_all = events_ms(mgr, stream, concat, reps)
    order = (A.OrderEntry * 2)(A.OrderEntry(0, 0, 0, 0, 0, 0), A.OrderEntry(1, 0, 0, 0, 0, 0))

    def sort():
        check(lib_.hdk_hip_sort_columns(d_cat.ptr, n, 3, n, order, 2, 0, 0, 0, d_srt.ptr, n, None, None, 0, 0, None))
        mgr.synchronizeStream(0)

    sort_ms, sort_all = wall_ms(sort, 2)
    d_cat.free()
    ws_bytes = lib_.hdk_hip_setop_columns_workspace_bytes(n)
    d_ws, d_rows = mgr.alloc(ws_bytes, 0), mgr.alloc(8, 0)
    idx = (C.c_int32 * 2)(0, 1)

    def setop(out_ptr, cap):
        check(lib_.hdk_hip_setop_columns(d_srt.ptr, n, 3, n, idx, 2, 2, OPS[op], idx, 2, out_ptr, cap, d_rows.ptr, d_ws.ptr, ws_bytes,
                                         0, None))

    setop(None, 0)
    mgr.synchronizeStream(0)
    kept = int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0])
    d_out = mgr.alloc(max(2 * kept * 8, 8), 0)
    full_ms, full_all = events_ms(mgr, stream, lambda: setop(d_out.ptr, kept), reps)
    count_ms, count_all = events_ms(mgr, stream, lambda: setop(None, 0), reps)
    got = mgr.to_host(d_out.ptr, 2 * kept * 8, 0, np.int64).reshape(2, kept) if kept else np.empty((2, 0), dtype=np.int64)
    for b in (d_srt, d_ws, d_rows, d_out):
        b.free()
    k, o = 2, 2
    model = 8 * n * k + 8 * n * (k + 1) + n // 8 + n // 8 + 16 * kept * o
    cat_model = 16 * n * 2 + 8 * n
    return {"rows_in_block": n, "kept_rows": kept, "workspace_bytes": ws_bytes,
            "concat_ms_median": cat_ms, "concat_ms_all": cat_all, "concat_modelled_bytes": cat_model,
            "concat_GBps": cat_model / (cat_ms * 1e-3) / 1e9, "concat_fraction_of_copy_rate": cat_model / (cat_ms * 1e-3) / 1e9 / copy_gbps,
            "sort_wall_ms_median": sort_ms, "sort_wall_ms_all": sort_all,
            "setop_ms_median": full_ms, "setop_ms_all": full_all, "setop_count_only_ms_median": count_ms,
            "setop_count_only_ms_all": count_all, "setop_compact_ms_by_difference": full_ms - count_ms,
            "setop_modelled_bytes": model, "setop_GBps": model / (full_ms * 1e-3) / 1e9,
            "setop_ms_at_copy_rate": model / (copy_gbps * 1e9) * 1e3,
            "setop_fraction_of_copy_rate": model / (full_ms * 1e-3) / 1e9 / copy_gbps}, got


def composed(L, R, op):
    """(b): the same rows from the stages that existed before"""
    ids = [("id", 0, None), ("id", 1, None)]
    if op == "union":
        first = L.union(R, all=True)
    else:
        first = L.join(R, [0], how="semi" if op == "intersect" else "anti")
    try:
        return first.group_by([0, 1], ids)
    finally:
        first.free()


def large_case(mgr, label, n, rn, reps, copy_gbps):
    rng = np.random.default_rng(15)
    if label == "union_half":
        op, what = "union", "UNION of two results of %d distinct rows each that share half their rows" % n
        la = rng.permutation(n).astype(np.int64)
        ra = rng.permutation(n).astype(np.int64) + n // 2
    else:
        if label == "exceptall":
            op, hit = "except_all", 0.1
            lens = rng.integers(1, 20, rn // 8 + 20)
            ra = (np.repeat(np.arange(len(lens), dtype=np.int64), lens)[:rn]) * 2
            what = "EXCEPT ALL, right rows in runs of about 10 equal rows, 10 % of the left rows present on the right"
        else:
            op, hit = "intersect", (0.9 if label == "isect90" else 0.01)
            ra = np.arange(rn, dtype=np.int64) * 2
            what = "INTERSECT, right rows distinct, %g %% of the left rows present on the right" % (hit * 100)
        distinct = np.unique(ra)
        la = distinct[rng.integers(0, len(distinct), n)]
        miss = rng.random(n) >= hit
        la[miss] = rng.integers(0, int(distinct[-1]) // 2, int(miss.sum())) * 2 + 1
        ra = ra[rng.permutation(rn)]
        del miss, distinct
    L, R = columns_of(mgr, la), columns_of(mgr, ra)
    out = {"what": what + "; two int64 columns, both compared, both written", "op": op, "left_rows": len(la), "right_rows": len(ra)}
    want = expected(la, ra, op)
    st, got = stages(mgr, L, R, op, reps, copy_gbps)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], 3 * want + 1), "hdk_hip_setop_columns disagrees with numpy"
    out.update(st)
    method = {"union": L.union, "intersect": L.intersect, "except_all": lambda r: L.except_(r, all=True)}[op]
    res = method(R)
    h = res.to_host()
    assert np.array_equal(h[0], want) and np.array_equal(h[1], 3 * want + 1), "the method disagrees with numpy"
    res.free()
    del h, got
    out["method_wall_ms_median"], out["method_wall_ms_all"] = wall_ms(lambda: method(R), 3)
    if op != "except_all":
        res = composed(L, R, op)
        assert np.array_equal(res.to_host()[0], want), "the composed stages disagree with numpy"
        res.free()
        out["composed_stages_wall_ms_median"], out["composed_stages_wall_ms_all"] = wall_ms(lambda: composed(L, R, op), 3)
        out["composed_over_method"] = out["composed_stages_wall_ms_median"] / out["method_wall_ms_median"]
    else:
        out["composed_stages"] = "not expressible: join(anti) + group_by has no multiset form"
    t0 = time.perf_counter()
    ha = host_way(mgr, L, R, op)[0]
    out["host_to_host_and_numpy_ms"] = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(ha, want)
    out["host_over_method"] = out["host_to_host_and_numpy_ms"] / out["method_wall_ms_median"]
    L.free()
    R.free()
    print(json.dumps({label: out}), flush=True)
    return {label: out}


def small_case(mgr, reps):
    rng = np.random.default_rng(16)
    ra = np.arange(1_000, dtype=np.int64) * 2
    la = rng.integers(0, 2_000, 10_000).astype(np.int64)
    L, R = columns_of(mgr, la), columns_of(mgr, ra)
    want = expected(la, ra, "intersect")

    def device_way():
        res = L.intersect(R)
        h = res.to_host()
        res.free()
        return h

    assert np.array_equal(device_way()[0], want) and np.array_equal(host_way(mgr, L, R, "intersect")[0], want)
    dev_ms, dev_all = wall_ms(device_way, reps, 3)
    host_ms, host_all = wall_ms(lambda: host_way(mgr, L, R, "intersect"), reps, 3)
    L.free()
    R.free()
    out = {"what": "INTERSECT of 10 000 x 1 000 rows, wall clock: DeviceColumns.intersect + to_host of the result against to_host of "
                   "both inputs + numpy", "device_ms_median": dev_ms, "device_ms_all": dev_all, "host_ms_median": host_ms,
           "host_ms_all": host_all, "host_over_device": host_ms / dev_ms, "winner": "host" if host_ms < dev_ms else "device"}
    print(json.dumps({"small": out}), flush=True)
    return {"small": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="isect90,isect1,exceptall,union_half,small")
    ap.add_argument("--rows", type=int, default=100_000_000, help="left rows of the large cases")
    ap.add_argument("--right-rows", type=int, default=10_000_000, help="right rows of the cases against a smaller result")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from hdk_amd._lib import check, lib
    from hdk_amd.hip_mgr import HipMgr
    mgr = HipMgr()
    only = args.only.split(",")
    reps = max(args.reps, 3)
    copy_gbps, read_gbps = C.c_double(0), C.c_double(0)
    check(lib().hdk_hip_mgr_measure_hbm(0, 4 << 30, 3, C.byref(copy_gbps), C.byref(read_gbps)))
    result = {"what": "hdk_hip_setop_columns / hdk_hip_concat_columns on one MI355X; HIP-event medians of %d calls after warm-up" % reps,
              "left_rows": args.rows, "right_rows": args.right_rows, "hbm_copy_GBps": copy_gbps.value,
              "hbm_read_GBps": read_gbps.value, "cases": {}}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    for label in ("isect90", "isect1", "exceptall", "union_half"):
        if label in only:
            result["cases"].update(large_case(mgr, label, args.rows, args.right_rows, reps, copy_gbps.value))
            save()
    if "small" in only:
        result["cases"].update(small_case(mgr, reps))
    save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
