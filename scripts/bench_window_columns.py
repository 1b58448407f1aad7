#!/usr/bin/env python3
"""Device window functions over dense result columns (hdk_hip_window_columns) on one MI355X.

C5-shaped input (key + value, 100 M rows x 2 columns), already sorted by the key, in three shapes:

    a   partitions of about 10 rows
    b   one partition
    c   every row a partition of its own

each with three output sets, PARTITION BY column 0:

    1   ROW_NUMBER, RANK (ORDER BY column 1)
    2   a running SUM(column 1) (the ROWS frame)
    3   SUM(column 1) over the whole partition (the PARTITION frame) plus LAG(column 1, 1)

Per case: the time of the call on the launch stream (HIP events, median after warm-up; workspace and output preallocated,
the call itself never waits), the modelled bytes, the achieved GB/s next to the copy rate
hdk_hip_mgr_measure_hbm reports in the same process, and the host alternative: to_host() of the two columns plus a numpy
evaluation of the same window columns (which is also the check of the device's answer).

    python scripts/bench_window_columns.py [--only a,b,c] [--sets 1,2,3] [--rows N] [--reps 7] [--out file.json]
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


def modelled_bytes(n, key_cols, agg_cols, gathered_cols, outs, broadcast_outs, partitions, peer_groups):
    """count: the key columns; directory: the key columns read, 4 bytes per peer group and 8 per partition written; rows:
    the key, aggregated and gathered columns and the directory read, 8 bytes per row and out written; broadcast (when an
    aggregate has a RANGE or PARTITION frame): the key columns and the directory again, 8 bytes per row and such out read
    and written"""
    directory = 4 * (peer_groups + 2 * partitions)
    total = 8 * n * key_cols + (8 * n * key_cols + directory) + (8 * n * (key_cols + agg_cols + gathered_cols) + directory + 8 * n * outs)
    if broadcast_outs:
        total += 8 * n * key_cols + directory + 16 * n * broadcast_outs
    return total


def out_sets():
    from hdk_amd import _abi as A
    null = A.to_i64(A.NULL_BIGINT)
    return {
        "1": dict(what="ROW_NUMBER, RANK", order=[1], agg=0, gathered=0, bcast=0,
                  outs=[A.WindowOut(-1, A.WIN_ROW_NUMBER, 0, 0, 0, 0, 0), A.WindowOut(-1, A.WIN_RANK, 0, 0, 0, 0, 0)]),
        "2": dict(what="running SUM (ROWS)", order=[], agg=1, gathered=0, bcast=0,
                  outs=[A.WindowOut(1, A.WIN_SUM, A.FRAME_ROWS, 0, 1, null, 0)]),
        "3": dict(what="SUM (PARTITION), LAG(1)", order=[], agg=1, gathered=1, bcast=1,
                  outs=[A.WindowOut(1, A.WIN_SUM, A.FRAME_PARTITION, 0, 1, null, 0), A.WindowOut(1, A.WIN_LAG, 0, 0, 1, null, 1)]),
    }


def numpy_windows(which, k, v):
    """the same window columns on the host (v holds no NULL word; an int64 sum wraps)"""
    n = len(k)
    head = np.concatenate([[True], k[1:] != k[:-1]])
    starts = np.flatnonzero(head)
    start = starts[np.cumsum(head) - 1]
    r = np.arange(n, dtype=np.int64)
    if which == "1":
        phead = head | np.concatenate([[True], v[1:] != v[:-1]])
        pstarts = np.flatnonzero(phead)
        return [r - start + 1, pstarts[np.cumsum(phead) - 1] - start + 1], len(starts), len(pstarts)
    ps = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(v.view(np.uint64))])
    if which == "2":
        return [(ps[1:] - ps[start]).view(np.int64)], len(starts), len(starts)
    ends = np.append(starts[1:], n)
    total = (ps[ends] - ps[starts]).view(np.int64)
    lag = np.concatenate([[np.int64(-2**63)], v[:-1]])
    lag[head] = -2**63
    return [np.repeat(total, ends - starts), lag], len(starts), len(starts)


def time_window(mgr, d_in, n, spec, reps):
    import torch
    from hdk_amd import _abi as A
    from hdk_amd._lib import check, lib
    L = lib()
    no = len(spec["outs"])
    outs = (A.WindowOut * no)(*spec["outs"])
    part = (C.c_int32 * 1)(0)
    order = (C.c_int32 * 1)(*(spec["order"] or [0]))
    ws_bytes = L.hdk_hip_window_columns_workspace_bytes(n, no)
    d_ws = mgr.alloc(ws_bytes, 0)
    d_out = mgr.alloc(no * n * 8, 0)
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))
    ms = []
    for i in range(2 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        check(L.hdk_hip_window_columns(d_in.ptr, n, 2, n, part, 1, order, len(spec["order"]), outs, no, d_out.ptr, n, d_ws.ptr,
                                       ws_bytes, 0, None))
        e1.record(stream)
        mgr.synchronizeStream(0)
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    got = mgr.to_host(d_out.ptr, no * n * 8, 0, np.int64).reshape(no, n)
    d_ws.free()
    d_out.free()
    return statistics.median(ms), ms, ws_bytes, got


def case(mgr, label, n, sets, reps, copy_gbps):
    rng = np.random.default_rng(10)
    if label == "a":
        lens = rng.integers(1, 20, n // 10 + 20)
        key = np.repeat(np.arange(len(lens), dtype=np.int64), lens)[:n]
        what = "partitions of about 10 rows"
    elif label == "b":
        key = np.zeros(n, dtype=np.int64)
        what = "one partition"
    else:
        key = np.arange(n, dtype=np.int64)
        what = "every row a partition"
    val = rng.integers(-2**31, 2**31, n).astype(np.int64)
    d_in = mgr.to_device(np.concatenate([key, val]), 0)
    res = {}
    for which, spec in out_sets().items():
        if which not in sets:
            continue
        k_ms, k_all, ws, got = time_window(mgr, d_in, n, spec, reps)
        t0 = time.perf_counter()
        h = mgr.to_host(d_in.ptr, 2 * n * 8, 0, np.int64)
        want, partitions, peer_groups = numpy_windows(which, h[:n], h[n:])
        host_ms = (time.perf_counter() - t0) * 1e3
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "the two ways disagree"
        model = modelled_bytes(n, 1 + len(spec["order"]), spec["agg"], spec["gathered"], len(spec["outs"]), spec["bcast"], partitions,
                               peer_groups)
        gbps = model / (k_ms * 1e-3) / 1e9
        out = {"what": f"PARTITION BY column 0: {spec['what']}; {what}", "rows": n, "partitions": partitions, "call_ms_median": k_ms,
               "call_ms_all": k_all, "modelled_bytes": model, "achieved_GBps": gbps, "fraction_of_copy_rate": gbps / copy_gbps,
               "workspace_bytes": ws, "host_to_host_and_numpy_ms": host_ms, "host_over_call": host_ms / k_ms}
        print(json.dumps({label + which: out}), flush=True)
        res[label + which] = out
    d_in.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--sets", default="1,2,3")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from hdk_amd._lib import check, lib
    from hdk_amd.hip_mgr import HipMgr
    mgr = HipMgr()
    reps = max(args.reps, 3)
    copy_gbps, read_gbps = C.c_double(0), C.c_double(0)
    check(lib().hdk_hip_mgr_measure_hbm(0, 4 << 30, 3, C.byref(copy_gbps), C.byref(read_gbps)))
    result = {"what": "hdk_hip_window_columns on one MI355X; HIP-event medians of %d repetitions after warm-up" % reps,
              "rows": args.rows, "hbm_copy_GBps": copy_gbps.value, "hbm_read_GBps": read_gbps.value, "cases": {}}
    for label in ("a", "b", "c"):
        if label in args.only.split(","):
            result["cases"].update(case(mgr, label, args.rows, args.sets.split(","), reps, copy_gbps.value))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
