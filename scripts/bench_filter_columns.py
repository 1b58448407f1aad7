#!/usr/bin/env python3
"""Device HAVING over dense result columns (hdk_hip_filter_columns) on one MI355X:

    a   C5's result (workloads.py: about 100 M rows, key + aggregate): HAVING <aggregate> > c, with c the quantile of the
        aggregate that lets about 1 % and about 50 % of the rows pass
    b   the same predicates followed by ORDER BY <aggregate> DESC LIMIT 10 (DeviceColumns.filter, then .sort)
    c   BH004's 10 000 rows with a two-leaf AND

For each: the time of the call on the launch stream (HIP events, median after warm-up; workspace and output preallocated,
the call itself never waits) and of the count-only call (out_cols = NULL: count + scan), the modelled bytes (count pass 8n per distinct leaf column + n/8; compact
pass n/8 + 8 bytes per column and passing row, read and written), the achieved GB/s next to the copy rate
hdk_hip_mgr_measure_hbm reports in the same process, and the host alternative of the same run:
fetch_columns().to_host() plus a numpy mask.

    python scripts/bench_filter_columns.py [--only a,b,c] [--c5-rows N] [--rows N] [--reps 7] [--out file.json]
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


def modelled_bytes(n, distinct_leaf_cols, num_cols, passing):
    return 8 * n * distinct_leaf_cols + n // 8 + n // 8 + 16 * num_cols * passing


def time_filter(mgr, cols, having, reps):
    """median ms of hdk_hip_filter_columns on `cols` (a DeviceColumns) with its workspace and output preallocated
    -> (median, all, passing rows, workspace bytes, median of the count-only call: count + scan without the compact pass)"""
    import torch
    from hdk_amd import _abi as A
    from hdk_amd._lib import check, lib
    L = lib()
    cp = cols.compiled
    nt, n = int(cp.plan.num_targets), cols.num_rows
    leaves = (A.HavingLeaf * len(having.leaves))()
    for i, lf in enumerate(having.leaves):
        leaves[i] = A.HavingLeaf(lf.lhs_col, lf.rhs_col, lf.cmp, int(lf.rhs_is_col), int(lf.cmp_fp), int(lf.lhs_is_fp),
                                 int(lf.lhs_nullable), int(lf.rhs_is_fp), int(lf.rhs_nullable), 0, A.to_i64(lf.lhs_null_bits),
                                 A.to_i64(lf.rhs_null_bits), A.to_i64(lf.rhs_lit))
    ops = (C.c_uint8 * max(len(having.prog), 1))(*having.prog)
    ws_bytes = L.hdk_hip_filter_columns_workspace_bytes(n)
    d_ws = mgr.alloc(ws_bytes, 0)
    d_rows = mgr.alloc(8, 0)

    def call(out_ptr, cap):
        check(L.hdk_hip_filter_columns(cols.block.ptr, cols.capacity, nt, n, leaves, len(having.leaves), ops, len(having.prog),
                                       out_ptr, cap, d_rows.ptr, None, d_ws.ptr, ws_bytes, 0, None))

    call(None, 0)
    mgr.synchronizeStream(0)
    passing = int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0])
    d_out = mgr.alloc(max(nt * passing * 8, 8), 0)
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))
    ms, count_ms = [], []
    for out_ptr, cap, into in ((d_out.ptr, passing, ms), (None, 0, count_ms)):
        for i in range(2 + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call(out_ptr, cap)
            e1.record(stream)
            mgr.synchronizeStream(0)
            if i >= 2:
                into.append(e0.elapsed_time(e1))
    for b in (d_ws, d_rows, d_out):
        b.free()
    return statistics.median(ms), ms, passing, ws_bytes, statistics.median(count_ms)


def wall(fn, reps):
    out = []
    for i in range(1 + reps):
        t0 = time.perf_counter()
        fn()
        if i >= 1:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def _columns_of(name, rows, mgr):
    from workloads import Workload
    w = Workload(name, rows, 0, mgr)
    step = w.ex.prepare(w.compiled, w.frag_ids)
    step.enqueue()
    cols = step.fetch_columns()
    step.free()
    return w, cols


def case_a_b(mgr, rows, reps, copy_gbps, only):
    from hdk_amd.ir import Cmp, Lit, OrderEntry, TargetRef
    from hdk_amd.plan import resolve_having
    w, cols = _columns_of("c5", rows, mgr)
    n, nt = cols.num_rows, int(cols.compiled.plan.num_targets)
    host = cols.to_host()
    agg = host[1]
    res = {}
    for label, q in (("1pct", 0.99), ("50pct", 0.5)):
        c = int(np.quantile(agg, q))
        conds = [Cmp(TargetRef(1), ">", Lit(c))]
        hv = resolve_having(cols.compiled, conds)
        if "a" in only:
            k_ms, k_all, passing, ws, cnt_ms = time_filter(mgr, cols, hv, reps)

            def device_way():
                kept = cols.filter(hv)
                got = kept.to_host()
                kept.free()
                return got

            def host_way():
                h = cols.to_host()
                m = h[1] > c
                return [x[m] for x in h]

            dev_ms, dev_all = wall(device_way, 3)
            host_ms, host_all = wall(host_way, 3)
            a, b = device_way(), host_way()
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the two ways disagree"
            model = modelled_bytes(n, 1, nt, passing)
            gbps = model / (k_ms * 1e-3) / 1e9
            res["a_" + label] = {"what": "HAVING target 1 > %d on C5's result" % c, "rows": n, "num_targets": nt, "passing": passing,
                                 "selectivity": passing / n, "call_ms_median": k_ms, "call_ms_all": k_all,
                                 "count_only_call_ms_median": cnt_ms, "modelled_bytes": model, "achieved_GBps": gbps,
                                 "fraction_of_copy_rate": gbps / copy_gbps, "workspace_bytes": ws,
                                 "filter_and_to_host_ms_median": dev_ms, "filter_and_to_host_ms_all": dev_all,
                                 "host_to_host_and_mask_ms_median": host_ms, "host_to_host_and_mask_ms_all": host_all,
                                 "host_over_device": host_ms / dev_ms}
            print(json.dumps({"a_" + label: res["a_" + label]}), flush=True)
        if "b" in only:
            def device_way():
                kept = cols.filter(hv)
                top = kept.sort([OrderEntry(1, desc=True)], limit=10)
                kept.free()
                got = top.to_host()
                top.free()
                return got

            def host_way():
                h = cols.to_host()
                m = np.flatnonzero(h[1] > c)
                part = m[np.argpartition(-h[1][m], 10)[:10]]
                part = part[np.lexsort((part, -h[1][part]))]
                return [x[part] for x in h]

            dev_ms, dev_all = wall(device_way, 3)
            host_ms, host_all = wall(host_way, 3)
            a, b = device_way(), host_way()
            assert np.array_equal(a[1], b[1]), "the two ways disagree on the ten values"
            res["b_" + label] = {"what": "HAVING target 1 > %d ORDER BY target 1 DESC LIMIT 10 on C5's result" % c, "rows": n,
                                 "filter_sort_and_to_host_ms_median": dev_ms, "filter_sort_and_to_host_ms_all": dev_all,
                                 "host_to_host_mask_argpartition_ms_median": host_ms, "host_to_host_mask_argpartition_ms_all": host_all,
                                 "host_over_device": host_ms / dev_ms}
            print(json.dumps({"b_" + label: res["b_" + label]}), flush=True)
    cols.free()
    w.ex.cache.clear()
    return res


def case_c(mgr, rows, reps, copy_gbps):
    from hdk_amd.ir import And, Cmp, Lit, TargetRef
    from hdk_amd.plan import resolve_having
    w, cols = _columns_of("bh4", rows, mgr)
    n, nt = cols.num_rows, int(cols.compiled.plan.num_targets)
    host = cols.to_host()
    lo, hi = (x.item() for x in (np.quantile(host[nt - 1], 0.25), np.quantile(host[0], 0.75)))
    lo, hi = (float(lo) if host[nt - 1].dtype == np.float64 else int(lo)), (float(hi) if host[0].dtype == np.float64 else int(hi))
    hv = resolve_having(cols.compiled, [And(Cmp(TargetRef(nt - 1), ">", Lit(lo)), Cmp(TargetRef(0), "<", Lit(hi)))])
    k_ms, k_all, passing, ws, cnt_ms = time_filter(mgr, cols, hv, reps)

    def device_way():
        kept = cols.filter(hv)
        got = kept.to_host()
        kept.free()
        return got

    def host_way():
        h = cols.to_host()
        m = (h[nt - 1] > lo) & (h[0] < hi)
        return [x[m] for x in h]

    dev_ms, dev_all = wall(device_way, reps)
    host_ms, host_all = wall(host_way, reps)
    a, b = device_way(), host_way()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the two ways disagree"
    model = modelled_bytes(n, 2, nt, passing)
    gbps = model / (k_ms * 1e-3) / 1e9
    out = {"what": "HAVING last target > %r AND target 0 < %r on BH004's result" % (lo, hi), "rows": n, "num_targets": nt,
           "passing": passing, "call_ms_median": k_ms, "call_ms_all": k_all, "count_only_call_ms_median": cnt_ms, "modelled_bytes": model,
           "achieved_GBps": gbps,
           "fraction_of_copy_rate": gbps / copy_gbps, "workspace_bytes": ws, "filter_and_to_host_ms_median": dev_ms,
           "filter_and_to_host_ms_all": dev_all, "host_to_host_and_mask_ms_median": host_ms, "host_to_host_and_mask_ms_all": host_all,
           "host_over_device": host_ms / dev_ms}
    print(json.dumps({"c": out}), flush=True)
    cols.free()
    w.ex.cache.clear()
    return {"c": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--c5-rows", type=int, default=1_000_000_000)
    ap.add_argument("--rows", type=int, default=256_000_000, help="rows of the bh4 input")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from hdk_amd._lib import check, lib
    from hdk_amd.hip_mgr import HipMgr
    mgr = HipMgr()
    only = args.only.split(",")
    reps = max(args.reps, 7)
    copy_gbps, read_gbps = C.c_double(0), C.c_double(0)
    check(lib().hdk_hip_mgr_measure_hbm(0, 4 << 30, 3, C.byref(copy_gbps), C.byref(read_gbps)))
    result = {"what": "hdk_hip_filter_columns on one MI355X; HIP-event medians of %d repetitions after warm-up" % reps,
              "c5_rows": args.c5_rows, "bh4_rows": args.rows, "hbm_copy_GBps": copy_gbps.value, "hbm_read_GBps": read_gbps.value,
              "cases": {}}
    if "a" in only or "b" in only:
        result["cases"].update(case_a_b(mgr, args.c5_rows, reps, copy_gbps.value, only))
    if "c" in only:
        result["cases"].update(case_c(mgr, args.rows, reps, copy_gbps.value))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
