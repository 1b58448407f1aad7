#!/usr/bin/env python3
"""Device ORDER BY / LIMIT over dense result columns (hdk_hip_sort_columns) on one MI355X:

    a   C5's result (workloads.py: about 100 M rows, key + aggregate): ORDER BY <aggregate> DESC LIMIT 10 -- the top-N
        selection path -- including to_host() of its ten rows, next to the way without this entry point:
        fetch_columns().to_host() of the whole result, then numpy argpartition + sort of the ten
    b   the same result sorted fully by its key
    c   BH004's 10 000 rows with two order entries

For each: the time of the whole call on the launch stream (HIP events, median after warm-up; the call synchronises the
stream once per order entry, which is inside the span), the modelled bytes (key build 8n + 12n, per live
digit 8n + 12n + 12n, gather 4 + 16 per column and output row, selection 8n per prefix pass, 16n to compact), the achieved
GB/s next to the copy rate hdk_hip_mgr_measure_hbm reports in the same process, and the host alternative.

    python scripts/bench_sort_columns.py [--only a,b,c] [--c5-rows N] [--rows N] [--reps 7] [--out file.json]
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


def live_digits(words, desc):
    """Digits on which the sort keys of a non-nullable int64 column differ (the census of hdk_sort_build_keys)."""
    u = words.view(np.uint64) ^ np.uint64(1 << 63)
    if desc:
        u = ~u
    varying = int(np.bitwise_or.reduce(u)) & int(np.bitwise_or.reduce(~u))
    return [d for d in range(8) if (varying >> (8 * d)) & 255]


def time_sort(mgr, cols, entries, limit, reps, flags=0):
    """median ms of hdk_hip_sort_columns on `cols` (a DeviceColumns) with its workspace and output preallocated"""
    import torch
    from hdk_amd import _abi as A
    from hdk_amd import result_set
    from hdk_amd._lib import check, lib
    L = lib()
    cp = cols.compiled
    nt, n = int(cp.plan.num_targets), cols.num_rows
    out_rows = min(limit, n) if limit else n
    arr = (A.OrderEntry * len(entries))()
    for i, (t, desc) in enumerate(entries):
        is_fp, nullable, null_bits = result_set.dense_column_null(cp, t)
        arr[i] = A.OrderEntry(t, int(desc), 0, int(is_fp), int(nullable), A.to_i64(null_bits))
    ws_bytes = L.hdk_hip_sort_columns_workspace_bytes(n, len(entries))
    d_ws = mgr.alloc(ws_bytes, 0)
    d_out = mgr.alloc(nt * out_rows * 8, 0)
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))
    ms = []
    for i in range(2 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        check(L.hdk_hip_sort_columns(cols.block.ptr, cols.capacity, nt, n, arr, len(entries), 0, limit, flags, d_out.ptr, out_rows,
                                     None, d_ws.ptr, ws_bytes, 0, None))
        e1.record(stream)
        mgr.synchronizeStream(0)
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    d_ws.free()
    d_out.free()
    return statistics.median(ms), ms, ws_bytes


def wall(fn, reps):
    out = []
    for i in range(1 + reps):
        t0 = time.perf_counter()
        fn()
        if i >= 1:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def case_a_b(mgr, rows, reps, copy_gbps, only):
    from hdk_amd.ir import OrderEntry
    from workloads import Workload
    w = Workload("c5", rows, 0, mgr)
    step = w.ex.prepare(w.compiled, w.frag_ids)
    step.enqueue()
    cols = step.fetch_columns()
    step.free()
    n, nt = cols.num_rows, int(cols.compiled.plan.num_targets)
    host = cols.to_host()
    res = {}
    if "a" in only:
        k_ms, k_all, ws = time_sort(mgr, cols, [(1, True)], 10, reps)
        full_ms, _, _ = time_sort(mgr, cols, [(1, True)], 10, reps, flags=1)
        live = live_digits(host[1], True)

        def device_way():
            top = cols.sort([OrderEntry(1, desc=True)], limit=10)
            got = top.to_host()
            top.free()
            return got

        def host_way():
            h = cols.to_host()
            part = np.argpartition(-h[1], 10)[:10]
            part = part[np.lexsort((part, -h[1][part]))]
            return [c[part] for c in h]

        dev_ms, dev_all = wall(device_way, reps)
        host_ms, host_all = wall(host_way, reps)
        a, b = device_way(), host_way()
        assert np.array_equal(a[1], b[1]), "the two ways disagree on the ten values"
        model = 20 * n + 8 * n * len(live) + 16 * n  # key build, prefix passes, count + compact (the candidates' sort is noise)
        res["a"] = {"what": "ORDER BY target 1 DESC LIMIT 10 on C5's result: selection path", "rows": n, "num_targets": nt,
                    "live_digits_of_the_first_entry": live, "call_ms_median": k_ms, "call_ms_all": k_all,
                    "call_ms_median_no_select": full_ms, "modelled_bytes": model,
                    "achieved_GBps": model / (k_ms * 1e-3) / 1e9, "fraction_of_copy_rate": model / (k_ms * 1e-3) / 1e9 / copy_gbps,
                    "workspace_bytes": ws, "sort_and_to_host_ms_median": dev_ms, "sort_and_to_host_ms_all": dev_all,
                    "host_to_host_argpartition_ms_median": host_ms, "host_to_host_argpartition_ms_all": host_all,
                    "host_over_device": host_ms / dev_ms}
        print(json.dumps({"a": res["a"]}), flush=True)
    if "b" in only:
        k_ms, k_all, ws = time_sort(mgr, cols, [(0, False)], 0, reps)
        live = live_digits(host[0], False)
        model = 20 * n + 32 * n * len(live) + (4 + 16 * nt) * n
        t0 = time.perf_counter()
        order = np.argsort(host[0], kind="stable")
        _ = [c[order] for c in host]
        host_sort_ms = (time.perf_counter() - t0) * 1e3
        copy_ms, _ = wall(cols.to_host, 3)
        res["b"] = {"what": "ORDER BY target 0 (the key) on C5's result: full sort", "rows": n, "num_targets": nt, "live_digits": live,
                    "call_ms_median": k_ms, "call_ms_all": k_all, "modelled_bytes": model,
                    "achieved_GBps": model / (k_ms * 1e-3) / 1e9, "fraction_of_copy_rate": model / (k_ms * 1e-3) / 1e9 / copy_gbps,
                    "workspace_bytes": ws, "host_to_host_ms_median": copy_ms, "host_numpy_stable_argsort_and_take_ms_once": host_sort_ms}
        print(json.dumps({"b": res["b"]}), flush=True)
    cols.free()
    w.ex.cache.clear()
    return res


def case_c(mgr, rows, reps, copy_gbps):
    from hdk_amd.ir import OrderEntry
    from workloads import Workload
    w = Workload("bh4", rows, 0, mgr)
    step = w.ex.prepare(w.compiled, w.frag_ids)
    step.enqueue()
    cols = step.fetch_columns()
    step.free()
    n, nt = cols.num_rows, int(cols.compiled.plan.num_targets)
    entries = [(nt - 1, True), (0, False)]
    k_ms, k_all, ws = time_sort(mgr, cols, entries, 0, reps)

    def device_way():
        s = cols.sort([OrderEntry(t, desc=d) for t, d in entries])
        got = s.to_host()
        s.free()
        return got

    def host_way():
        h = cols.to_host()
        keys = [c.view(np.int64) for c in h]
        order = np.lexsort((keys[0], -h[nt - 1]))
        return [c[order] for c in h]

    dev_ms, dev_all = wall(device_way, reps)
    host_ms, host_all = wall(host_way, reps)
    out = {"what": "ORDER BY last target DESC, target 0 on BH004's result: two order entries", "rows": n, "num_targets": nt,
           "call_ms_median": k_ms, "call_ms_all": k_all, "workspace_bytes": ws,
           "modelled_bytes_at_8_live_digits_an_entry": 2 * (20 * n + 32 * n * 8) + (4 + 16 * nt) * n,
           "sort_and_to_host_ms_median": dev_ms, "sort_and_to_host_ms_all": dev_all,
           "host_to_host_lexsort_ms_median": host_ms, "host_to_host_lexsort_ms_all": host_all, "host_over_device": host_ms / dev_ms}
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
    result = {"what": "hdk_hip_sort_columns on one MI355X; HIP-event medians of %d repetitions after warm-up" % reps,
              "hbm_copy_GBps": copy_gbps.value, "hbm_read_GBps": read_gbps.value, "cases": {}}
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
