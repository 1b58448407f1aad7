#!/usr/bin/env python3
"""Device projection over dense result columns (hdk_hip_project_columns) on one MI355X.

C5-shaped input (100 M rows x 2 int64 columns: s, a sum, and n, a count >= 1) and a 10 000-row input, four select lists:

    1   s / n
    2   cast(s as double) / n
    3   CASE WHEN n = 0 THEN NULL ELSE cast(s as double) / n END * 100.0
    4   eight outs of mixed ops: s + n, s - n, s * n (all checked at 8 bytes), s / n, s % n, cast(s as double) * 0.5,
        CASE WHEN s > 0 THEN s ELSE 0 - s END, n (a pass-through)

Per case: every out word compared with numpy first; then the time of the call on the launch stream (HIP events, median
after warm-up; the output preallocated, the call itself never waits), the modelled bytes 8 * rows * (distinct inputs +
outs), the achieved GB/s next to the copy rate hdk_hip_mgr_measure_hbm reports in the same process, and
the host alternative: to_host() of the two columns plus the same numpy evaluation.  End to end: ORDER BY the ratio of
case 2 DESC LIMIT 10 as DeviceColumns.project + sort + to_host against to_host + numpy.

    python scripts/bench_project_columns.py [--rows N] [--small N] [--reps 7] [--out file.json]
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

NULL_D = 0x0010000000000000


def dbits(x):
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def select_lists():
    """-> {case: (what, ops as (code, check_width, flags, col, imm), outs as (first, count, is_fp))}"""
    from hdk_amd import _abi as A
    s, n = (A.P_PUSH_COL, 0, 0, 0, 0), (A.P_PUSH_COL, 0, 0, 1, 0)
    i2f = (A.P_CAST_I2F, 0, 0, 0, 0)
    lit = lambda v: (A.P_PUSH_INT, 0, 0, 0, v)  # noqa: E731
    flit = lambda v: (A.P_PUSH_FP, 0, 0, 0, dbits(v))  # noqa: E731
    fratio = [s, i2f, n, i2f, (A.P_DIV_F, 0, 0, 0, 0)]
    guarded = [n, lit(0), (A.P_CMP_I, 0, A.CMP_EQ, 0, 0), (A.P_PUSH_NULL_FP, 0, 0, 0, 0)] + fratio + [
        (A.P_SELECT, 0, 0, 0, 0), flit(100.0), (A.P_MUL_F, 0, 0, 0, 0)]
    mixed, outs = [], []
    for prog, fp in (([s, n, (A.P_ADD_I, 8, 0, 0, 0)], 0), ([s, n, (A.P_SUB_I, 8, 0, 0, 0)], 0), ([s, n, (A.P_MUL_I, 8, 0, 0, 0)], 0),
                     ([s, n, (A.P_DIV_I, 0, 0, 0, 0)], 0), ([s, n, (A.P_MOD_I, 0, 0, 0, 0)], 0),
                     ([s, i2f, flit(0.5), (A.P_MUL_F, 0, 0, 0, 0)], 1),
                     ([s, lit(0), (A.P_CMP_I, 0, A.CMP_GT, 0, 0), s, lit(0), s, (A.P_SUB_I, 8, 0, 0, 0), (A.P_SELECT, 0, 0, 0, 0)], 0),
                     ([n], 0)):
        outs.append((len(mixed), len(prog), fp))
        mixed += prog
    return {"1": ("s / n", [s, n, (A.P_DIV_I, 0, 0, 0, 0)], [(0, 3, 0)]),
            "2": ("cast(s as double) / n", fratio, [(0, 5, 1)]),
            "3": ("CASE WHEN n = 0 THEN NULL ELSE cast(s as double) / n END * 100.0", guarded, [(0, len(guarded), 1)]),
            "4": ("eight outs of mixed ops", mixed, outs)}


def trunc_div(s, n):
    """C division of int64 by a positive int64"""
    q = np.abs(s) // n
    return np.where(s < 0, -q, q)


def numpy_outs(which, s, n):
    with np.errstate(all="ignore"):
        if which == "1":
            return [trunc_div(s, n)]
        ratio = s.astype(np.float64) / n.astype(np.float64)
        if which == "2":
            return [ratio.view(np.int64)]
        if which == "3":
            return [np.where(n == 0, np.int64(NULL_D), (ratio * 100.0).view(np.int64))]
        q = trunc_div(s, n)
        return [s + n, s - n, s * n, q, s - q * n, (s.astype(np.float64) * 0.5).view(np.int64), np.where(s > 0, s, -s), n]


def time_project(mgr, d_in, n, ops, outs, reps):
    import torch
    from hdk_amd import _abi as A
    from hdk_amd._lib import check, lib
    L = lib()
    no = len(outs)
    c_ops = (A.ProjectOp * len(ops))(*[A.ProjectOp(c, w, f, 0, col, A.to_i64(imm)) for c, w, f, col, imm in ops])
    c_outs = (A.ProjectOut * no)(*[A.ProjectOut(first, count, fp, 1, (C.c_uint8 * 6)(), A.to_i64(NULL_D if fp else -2**63))
                                   for first, count, fp in outs])
    d_out = mgr.alloc(no * n * 8, 0)
    d_err = mgr.alloc(4, 0)
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))
    ms = []
    for i in range(2 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        check(L.hdk_hip_project_columns(d_in.ptr, n, 2, n, c_ops, len(ops), c_outs, no, d_out.ptr, n, d_err.ptr, 0, None))
        e1.record(stream)
        mgr.synchronizeStream(0)
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    got = mgr.to_host(d_out.ptr, no * n * 8, 0, np.int64).reshape(no, n)
    err = int(mgr.to_host(d_err.ptr, 4, 0, np.int32)[0])
    d_out.free()
    d_err.free()
    return statistics.median(ms), ms, got, err


def end_to_end(mgr, d_in, n, reps):
    """ORDER BY cast(s as double) / n DESC LIMIT 10: device project + sort + to_host of ten rows against to_host + numpy"""
    from hdk_amd.executor import DeviceColumns
    from hdk_amd.ir import FP64, Cast, OrderEntry, Proj, TargetRef, Type
    from hdk_amd.plan import ColumnDesc
    schema = [ColumnDesc("s", False, False, 0, Type("int", 8, False), 0), ColumnDesc("n", False, False, 0, Type("int", 8, False), 1)]
    cols = DeviceColumns(None, mgr, 0, d_in, n, n, 0, schema)
    select = [Proj(TargetRef("s"), "s"), Proj(TargetRef("n"), "n"), Proj(Cast(TargetRef("s"), FP64) / TargetRef("n"), "ratio")]
    dev_ms, host_ms, top = [], [], None
    for i in range(1 + reps):
        t0 = time.perf_counter()
        proj = cols.project(select)
        try:
            best = proj.sort([OrderEntry("ratio", desc=True)], limit=10)
        finally:
            proj.free()
        top = best.to_host()
        best.free()
        if i:
            dev_ms.append((time.perf_counter() - t0) * 1e3)
    for i in range(3):
        t0 = time.perf_counter()
        h = mgr.to_host(d_in.ptr, 2 * n * 8, 0, np.int64)
        ratio = h[:n].astype(np.float64) / h[n:].astype(np.float64)
        idx = np.argpartition(-ratio, 10)[:10]
        idx = idx[np.argsort(-ratio[idx], kind="stable")]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(np.sort(top[2])[::-1], ratio[idx]), "the two ways disagree"
    return {"what": "ORDER BY cast(s as double) / n DESC LIMIT 10 over s, n, ratio", "rows": n,
            "device_project_sort_to_host_ms_median": statistics.median(dev_ms), "device_ms_all": dev_ms,
            "host_to_host_numpy_argpartition_ms_median": statistics.median(host_ms), "host_ms_all": host_ms,
            "host_over_device": statistics.median(host_ms) / statistics.median(dev_ms)}


def run_size(mgr, label, n, reps, copy_gbps):
    rng = np.random.default_rng(12)
    s = rng.integers(-2**31, 2**31, n).astype(np.int64)
    cnt = rng.integers(1, 100, n).astype(np.int64)
    d_in = mgr.to_device(np.concatenate([s, cnt]), 0)
    res = {}
    for which, (what, ops, outs) in select_lists().items():
        k_ms, k_all, got, err = time_project(mgr, d_in, n, ops, outs, reps)
        t0 = time.perf_counter()
        h = mgr.to_host(d_in.ptr, 2 * n * 8, 0, np.int64)
        want = numpy_outs(which, h[:n], h[n:])
        host_ms = (time.perf_counter() - t0) * 1e3
        assert err == 0 and all(np.array_equal(a, b) for a, b in zip(got, want)), "the two ways disagree"
        model = 8 * n * (2 + len(outs))
        gbps = model / (k_ms * 1e-3) / 1e9
        out = {"what": what, "rows": n, "outs": len(outs), "ops": len(ops), "call_ms_median": k_ms, "call_ms_all": k_all,
               "modelled_bytes": model, "achieved_GBps": gbps, "fraction_of_copy_rate": gbps / copy_gbps,
               "host_to_host_and_numpy_ms": host_ms, "host_over_call": host_ms / k_ms}
        print(json.dumps({label + which: out}), flush=True)
        res[label + which] = out
    res[label + "_order_by_limit"] = end_to_end(mgr, d_in, n, reps)
    print(json.dumps({label + "_order_by_limit": res[label + "_order_by_limit"]}), flush=True)
    d_in.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--small", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from hdk_amd._lib import check, lib
    from hdk_amd.hip_mgr import HipMgr
    mgr = HipMgr()
    reps = max(args.reps, 3)
    copy_gbps, read_gbps = C.c_double(0), C.c_double(0)
    check(lib().hdk_hip_mgr_measure_hbm(0, 4 << 30, 3, C.byref(copy_gbps), C.byref(read_gbps)))
    result = {"what": "hdk_hip_project_columns on one MI355X; HIP-event medians of %d repetitions after warm-up" % reps,
              "hbm_copy_GBps": copy_gbps.value, "hbm_read_GBps": read_gbps.value, "cases": {}}
    result["cases"].update(run_size(mgr, "large", args.rows, reps, copy_gbps.value))
    result["cases"].update(run_size(mgr, "small", args.small, reps, copy_gbps.value))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
