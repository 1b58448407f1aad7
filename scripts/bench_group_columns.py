#!/usr/bin/env python3
"""Device GROUP BY over dense result columns (hdk_hip_group_columns) on one MI355X:

    a   C5-shaped input (key + aggregate, 100 M rows x 2 columns), already sorted by the key, runs of about 10 rows:
        outs = ID(key), SUM(value), COUNT(*)
    b   the same rows as one run
    c   the same rows, all keys distinct
    d   COUNT(DISTINCT x) GROUP BY key end to end (Executor.execute(result="columns"): the inner GROUP BY key, x, the sort
        of its dense columns by the key, the regroup, to_host) against the host path: the inner result's to_host() plus a
        numpy group-by of it

For a-c: the time of the call on the launch stream (HIP events, median after warm-up; workspace and output preallocated,
the call itself never waits) and of the count-only call, the modelled bytes (the count pass reads the
key columns, the reduce pass the key and the aggregated columns, and 8 bytes per out and run are written), the achieved
GB/s next to the copy rate hdk_hip_mgr_measure_hbm reports in the same process, and the host alternative: to_host() of
the two columns plus numpy's reduceat.

    python scripts/bench_group_columns.py [--only a,b,c,d] [--rows N] [--d-rows N] [--reps 7] [--out file.json]
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


def modelled_bytes(n, key_cols, agg_cols, outs, runs):
    return 8 * n * key_cols + 8 * n * (key_cols + agg_cols) + 8 * outs * runs


def time_group(mgr, d_in, n, reps):
    """median ms of hdk_hip_group_columns over the two columns at d_in -> (median, all, runs, workspace bytes, count-only median)"""
    import torch
    from hdk_amd import _abi as A
    from hdk_amd._lib import check, lib
    L = lib()
    keys = (C.c_int32 * 1)(0)
    outs = (A.GroupOut * 3)(A.GroupOut(0, A.AGG_ID, 0, 0, 0, 0), A.GroupOut(1, A.AGG_SUM, 0, 1, 0, A.to_i64(A.NULL_BIGINT)),
                            A.GroupOut(-1, A.AGG_COUNT, 0, 0, 0, 0))
    ws_bytes = L.hdk_hip_group_columns_workspace_bytes(n, 3)
    d_ws = mgr.alloc(ws_bytes, 0)
    d_rows = mgr.alloc(8, 0)

    def call(out_ptr, cap):
        check(L.hdk_hip_group_columns(d_in.ptr, n, 2, n, keys, 1, outs, 3, out_ptr, cap, d_rows.ptr, d_ws.ptr, ws_bytes, 0, None))

    call(None, 0)
    mgr.synchronizeStream(0)
    runs = int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0])
    d_out = mgr.alloc(3 * runs * 8, 0)
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))
    ms, count_ms = [], []
    for out_ptr, cap, into in ((d_out.ptr, runs, ms), (None, 0, count_ms)):
        for i in range(2 + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call(out_ptr, cap)
            e1.record(stream)
            mgr.synchronizeStream(0)
            if i >= 2:
                into.append(e0.elapsed_time(e1))
    got = mgr.to_host(d_out.ptr, 3 * runs * 8, 0, np.int64).reshape(3, runs)
    for b in (d_ws, d_rows, d_out):
        b.free()
    return statistics.median(ms), ms, runs, ws_bytes, statistics.median(count_ms), got


def wall(fn, reps):
    out = []
    for i in range(1 + reps):
        t0 = time.perf_counter()
        fn()
        if i >= 1:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def case_abc(mgr, label, n, reps, copy_gbps):
    rng = np.random.default_rng(10)
    if label == "a":
        lens = rng.integers(1, 20, n // 10 + 20)
        key = np.repeat(np.arange(len(lens), dtype=np.int64), lens)[:n]
        what = "runs of about 10 rows"
    elif label == "b":
        key = np.zeros(n, dtype=np.int64)
        what = "one run"
    else:
        key = np.arange(n, dtype=np.int64)
        what = "all rows distinct"
    val = rng.integers(-2**31, 2**31, n).astype(np.int64)
    host = np.concatenate([key, val])
    d_in = mgr.to_device(host, 0)
    k_ms, k_all, runs, ws, cnt_ms, got = time_group(mgr, d_in, n, reps)

    def host_way():
        h = mgr.to_host(d_in.ptr, 2 * n * 8, 0, np.int64)
        k, v = h[:n], h[n:]
        starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
        return k[starts], np.add.reduceat(v, starts), np.diff(np.append(starts, n))

    host_ms, host_all = wall(host_way, 2)
    want = host_way()
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), "the two ways disagree"
    d_in.free()
    model = modelled_bytes(n, 1, 1, 3, runs)
    gbps = model / (k_ms * 1e-3) / 1e9
    out = {"what": "GROUP BY column 0: ID, SUM(column 1), COUNT(*); " + what, "rows": n, "runs": runs, "call_ms_median": k_ms,
           "call_ms_all": k_all, "count_only_call_ms_median": cnt_ms, "modelled_bytes": model, "achieved_GBps": gbps,
           "fraction_of_copy_rate": gbps / copy_gbps, "workspace_bytes": ws, "host_to_host_and_reduceat_ms_median": host_ms,
           "host_to_host_and_reduceat_ms_all": host_all, "host_over_call": host_ms / k_ms}
    print(json.dumps({label: out}), flush=True)
    return {label: out}


def case_d(mgr, rows):
    from hdk_amd.executor import Executor
    from hdk_amd.ir import Agg, ColRef, KeyRef, QueryUnit
    from hdk_amd.plan import split_count_distinct
    from hdk_amd.storage import ArrowStorage
    rng = np.random.default_rng(11)
    domain = max(rows // 10, 1)
    st = ArrowStorage()
    st.import_numpy("t", {"key": rng.integers(0, domain, rows).astype(np.int64), "x": rng.integers(0, 8, rows).astype(np.int64)},
                    fragment_size=max(rows // 16, 1))
    ex = Executor(st, 0, mgr)
    q = QueryUnit("t", groupby=[ColRef("key")], targets=[KeyRef(0, "key"), Agg("count_distinct", ColRef("x"), "dx")])
    inner, _ = split_count_distinct(q)

    def device_way():
        cols = ex.execute(q, result="columns")
        got = cols.to_host()
        cols.free()
        return got

    def host_way():
        cols = ex.execute(inner, result="columns")
        k, x = cols.to_host()
        cols.free()
        order = np.argsort(k, kind="stable")
        k = k[order]
        starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
        return [k[starts], np.diff(np.append(starts, len(k)))]  # (x is never NULL here: every inner group counts)

    def inner_only():
        ex.execute(inner, result="columns").free()

    a, b = device_way(), host_way()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the two ways disagree"
    dev_ms, dev_all = wall(device_way, 3)
    host_ms, host_all = wall(host_way, 3)
    inner_ms, inner_all = wall(inner_only, 3)
    out = {"what": "SELECT key, COUNT(DISTINCT x) GROUP BY key; int64 key uniform in rows / 10 values, x in 0..7", "rows": rows,
           "groups": int(len(a[0])), "execute_and_to_host_ms_median": dev_ms, "execute_and_to_host_ms_all": dev_all,
           "inner_group_by_to_columns_ms_median": inner_ms, "inner_group_by_to_columns_ms_all": inner_all,
           "inner_to_host_and_numpy_group_by_ms_median": host_ms, "inner_to_host_and_numpy_group_by_ms_all": host_all,
           "host_over_device": host_ms / dev_ms}
    print(json.dumps({"d": out}), flush=True)
    ex.cache.clear()
    return {"d": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--rows", type=int, default=100_000_000, help="rows of cases a, b and c")
    ap.add_argument("--d-rows", type=int, default=100_000_000, help="rows of case d's table")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from hdk_amd._lib import check, lib
    from hdk_amd.hip_mgr import HipMgr
    mgr = HipMgr()
    only = args.only.split(",")
    reps = max(args.reps, 3)
    copy_gbps, read_gbps = C.c_double(0), C.c_double(0)
    check(lib().hdk_hip_mgr_measure_hbm(0, 4 << 30, 3, C.byref(copy_gbps), C.byref(read_gbps)))
    result = {"what": "hdk_hip_group_columns on one MI355X; HIP-event medians of %d repetitions after warm-up" % reps,
              "rows": args.rows, "d_rows": args.d_rows, "hbm_copy_GBps": copy_gbps.value, "hbm_read_GBps": read_gbps.value, "cases": {}}
    for label in ("a", "b", "c"):
        if label in only:
            result["cases"].update(case_abc(mgr, label, args.rows, reps, copy_gbps.value))
    if "d" in only:
        result["cases"].update(case_d(mgr, args.d_rows))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
