#!/usr/bin/env python3
"""Device-side columnar results for projections (hdk_hip_columnarize_rows) on one MI355X:

    proj50 / proj1   DESIGN 3.6's filter/project: 256 M rows, 2 targets + positions, 50 % / 1 % of the rows pass; the
                     step's own buffer, row-wise and columnar
    wide             row-wise buffers of 3 .. 9 words per row (8 targets at 64 M rows, the others at 32 M), made on the
                     device, through BOTH row-wise kernels (HDK_HIP_ROWS_VARIANT=walk / lds)
    narrow           a columnar buffer with 1-, 2- and 4-byte columns (64 M rows)
    small            10 000 passing rows: the call alone, and to host arrays through fetch_columns() against fetch()
    topn             WHERE p ORDER BY v DESC LIMIT 10 over 128 M passing rows on the device against fetch() + numpy

For each call: the kernel time (HIP events on the launch stream, median of --reps calls after two warm-up calls, the output
preallocated), the modelled bytes (the consumed rows read once plus 8 x rows x outs written), and the achieved GB/s next to
the copy rate hdk_hip_mgr_measure_hbm reports in the same process.

    python scripts/bench_row_columns.py [--only proj50,proj1,wide,narrow,small,topn] [--rows N] [--reps 5] [--out file.json]
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


def scan_executor(mgr, rows):
    """t(a, b): a uniform in [0, 1000), b uniform int64, generated on the device"""
    import torch
    from hdk_amd.executor import Executor
    from hdk_amd.ir import Type
    from hdk_amd.storage import ArrowStorage, ChunkStats, Column, Table
    from workloads import SEED, TensorChunk, fragment_rows
    dev = torch.device("cuda", 0)
    st = ArrowStorage()
    ex = Executor(st, 0, mgr)
    frag_rows = fragment_rows(rows)
    i64 = Type("int", 8, False)
    cols = []
    for salt, (name, lo, hi) in enumerate((("a", 0, 1000), ("b", -2**40, 2**40))):
        cols.append(Column(name, i64, [None] * len(frag_rows), [ChunkStats(lo, hi - 1, False)] * len(frag_rows)))
        for f, n in enumerate(frag_rows):
            g = torch.Generator(device=dev)
            g.manual_seed(SEED + 1000 * salt + f)
            ex.cache.put(("t", name, f), TensorChunk(torch.randint(lo, hi, (n,), dtype=torch.int64, device=dev, generator=g)))
    st.add_table(Table("t", cols, frag_rows))
    torch.cuda.synchronize(dev)
    return ex


def projection(bound, columnar, **kw):
    from hdk_amd.ir import Cmp, ColRef, Lit, Proj, QueryUnit
    return QueryUnit("t", quals=[Cmp(ColRef("a"), "<", Lit(bound))], output_columnar=columnar,
                     targets=[Proj(ColRef("a"), "a"), Proj(ColRef("b"), "b")], **kw)


def time_call(mgr, call, reps):
    """median and all times (ms) of `call()` between two HIP events on the manager's stream, after two warm-up calls"""
    import torch
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))
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


def measure_buffer(mgr, plan, buf_ptr, entry_count, d_total, rows, row_bytes_read, reps, copy_gbps, positions=True):
    """hdk_hip_columnarize_rows over the buffer at buf_ptr into a preallocated block of `rows` rows"""
    from hdk_amd._lib import check, lib
    L = lib()
    nt = int(plan.num_targets)
    outs = nt + (1 if positions else 0)
    d_out = mgr.alloc(max(outs * rows * 8, 8), 0)
    d_rows = mgr.alloc(8, 0)

    def call():
        check(L.hdk_hip_columnarize_rows(C.byref(plan), buf_ptr, entry_count, d_total, d_out.ptr, rows,
                                         d_out.ptr + nt * rows * 8 if positions else None, d_rows.ptr, 0, None))

    k_ms, all_ms = time_call(mgr, call, reps)
    assert int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0]) == rows
    d_out.free()
    d_rows.free()
    model = rows * row_bytes_read + 8 * rows * outs
    gbps = model / (k_ms * 1e-3) / 1e9 if rows else 0.0
    return {"entry_count": entry_count, "rows": rows, "outs": outs, "bytes_read_per_row": row_bytes_read, "modelled_bytes": model,
            "kernel_ms_median": k_ms, "kernel_ms_all": all_ms, "achieved_GBps": gbps, "fraction_of_copy_rate": gbps / copy_gbps}


def bench_projection(mgr, ex, bound, reps, copy_gbps):
    res = {}
    for columnar in (False, True):
        step = ex.prepare(projection(bound, columnar))
        step.enqueue()
        mgr.synchronizeStream(0)
        total = int(mgr.to_host(step.d_total_matched.ptr, 4, 0, np.int32)[0])
        p = step.cp.plan
        read = 8 + sum(step.cp.slot_widths) if columnar else int(p.row_size_quad) * 8
        r = measure_buffer(mgr, p, step.out_ptr, int(step.cp.entry_count), step.d_total_matched.ptr, total, read, reps, copy_gbps)
        r["kernels"] = step.kernel_names()
        res["columnar" if columnar else "row-wise"] = r
        step.free()
    return res


def synthetic_plan(ntargets, entry_count, widths=None):
    """a projection plan of `ntargets` int64 targets (row-wise), or of integer columns of `widths` bytes (columnar)"""
    from hdk_amd.ir import ColRef, Proj, QueryUnit
    from hdk_amd.plan import compile_query
    from hdk_amd.storage import ArrowStorage
    st = ArrowStorage()
    dts = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
    ws = widths or [8] * ntargets
    st.import_numpy("s", {f"c{i}": np.zeros(4, dtype=dts[w]) for i, w in enumerate(ws)})
    return compile_query(st, QueryUnit("s", targets=[Proj(ColRef(f"c{i}"), f"c{i}") for i in range(len(ws))], scan_limit=entry_count,
                                       output_columnar=bool(widths)))


def bench_synthetic(mgr, cp, reps, copy_gbps, variant=None):
    from hdk_amd._lib import sync_switches
    if variant:
        os.environ["HDK_HIP_ROWS_VARIANT"] = variant
    sync_switches()
    try:
        n = int(cp.plan.entry_count)
        d_buf = mgr.alloc(cp.buffer_bytes, 0)
        mgr.setDeviceMem(d_buf.ptr, 0x3C, cp.buffer_bytes, 0)
        d_total = mgr.to_device(np.array([n, 0], dtype=np.int32), 0)
        read = 8 + sum(cp.slot_widths) if cp.plan.output_columnar else int(cp.plan.row_size_quad) * 8
        r = measure_buffer(mgr, cp.plan, d_buf.ptr, n, d_total.ptr, n, read, reps, copy_gbps)
        d_buf.free()
        d_total.free()
        return r
    finally:
        os.environ.pop("HDK_HIP_ROWS_VARIANT", None)
        sync_switches()


def bench_small(mgr, ex, rows_in, reps, copy_gbps):
    """about 10 000 passing rows of the scan: the call alone, then host arrays through both paths"""
    bound = max(1, round(10_000 * 1000 / rows_in))
    step = ex.prepare(projection(bound, False))
    step.enqueue()
    mgr.synchronizeStream(0)
    total = int(mgr.to_host(step.d_total_matched.ptr, 4, 0, np.int32)[0])
    r = measure_buffer(mgr, step.cp.plan, step.out_ptr, int(step.cp.entry_count), step.d_total_matched.ptr, total, 24, reps, copy_gbps)
    new_s, old_s = [], []
    for i in range(1 + reps):
        t0 = time.perf_counter()
        cols = step.fetch_columns(stream_synced=True, positions=True)
        host = cols.to_host()
        t1 = time.perf_counter()
        cols.free()
        res = step.fetch(stream_synced=True)
        from hdk_amd import result_set as rs
        pos, arrs = rs.projection_arrays(step.cp, res.buffer, res.total_matched)
        t2 = time.perf_counter()
        assert all(np.array_equal(a.view(np.int64), b) for a, b in zip(host, arrs + [pos]))
        if i >= 1:
            new_s.append(t1 - t0)
            old_s.append(t2 - t1)
    step.free()
    r["to_host_via_fetch_columns_ms_median"] = statistics.median(new_s) * 1e3
    r["to_host_via_fetch_ms_median"] = statistics.median(old_s) * 1e3
    r["note"] = "fetch() copies the whole %d-entry buffer; a caller that knows the count would copy less" % int(step.cp.entry_count)
    return r


def bench_topn(mgr, ex, reps):
    """WHERE a < 500 ORDER BY b DESC LIMIT 10: on the device against fetch() + numpy"""
    from hdk_amd import result_set as rs
    from hdk_amd.ir import OrderEntry
    dev_s, host_s = [], []
    for i in range(1 + reps):
        t0 = time.perf_counter()
        out = ex.execute(projection(500, False, order_by=[OrderEntry("b", desc=True)], limit=10), result="columns")
        got = out.to_host()
        t1 = time.perf_counter()
        passing = out.compiled.entry_count
        out.free()
        res = ex.execute(projection(500, False))
        _, (a, b) = rs.projection_arrays(res.compiled, res.buffer, res.total_matched)
        top = np.argpartition(b, len(b) - 10)[-10:]
        top = top[np.argsort(-b[top], kind="stable")]
        t2 = time.perf_counter()
        assert np.array_equal(got[1], b[top]) and np.array_equal(got[0], a[top])
        rows = len(b)
        del res, a, b
        if i >= 1:
            dev_s.append(t1 - t0)
            host_s.append(t2 - t1)
    return {"passing_rows": rows, "entry_count": int(passing), "device_ms_median": statistics.median(dev_s) * 1e3,
            "fetch_and_numpy_ms_median": statistics.median(host_s) * 1e3, "device_ms_all": [x * 1e3 for x in dev_s],
            "fetch_and_numpy_ms_all": [x * 1e3 for x in host_s],
            "note": "both sides include the scan; the device side runs scan, columnarize, top-N select and copies 10 rows"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="proj50,proj1,wide,narrow,small,topn")
    ap.add_argument("--rows", type=int, default=256_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from hdk_amd._lib import check, lib
    from hdk_amd.hip_mgr import HipMgr
    mgr = HipMgr()
    copy_gbps, read_gbps = C.c_double(0), C.c_double(0)
    check(lib().hdk_hip_mgr_measure_hbm(0, 4 << 30, 3, C.byref(copy_gbps), C.byref(read_gbps)))
    reps = max(args.reps, 5)
    result = {"what": "hdk_hip_columnarize_rows on one MI355X; HIP-event medians of %d calls after warm-up, output preallocated" % reps,
              "hbm_copy_GBps": copy_gbps.value, "hbm_read_GBps": read_gbps.value, "rows": args.rows, "cases": {}}
    only = args.only.split(",")
    ex = scan_executor(mgr, args.rows) if set(only) & {"proj50", "proj1", "topn"} else None

    def emit(name, r):
        result["cases"][name] = r
        print(json.dumps({name: r}), flush=True)

    for name in only:
        if name in ("proj50", "proj1"):
            emit(name, bench_projection(mgr, ex, 500 if name == "proj50" else 10, reps, copy_gbps.value))
        elif name == "wide":
            r = {}
            for words in range(3, 10):
                cp = synthetic_plan(words - 1, args.rows // (4 if words == 9 else 8))
                r["%d_words" % words] = {v: bench_synthetic(mgr, cp, reps, copy_gbps.value, v) for v in ("walk", "lds")}
                r["%d_words" % words]["default"] = bench_synthetic(mgr, cp, reps, copy_gbps.value)
            cp = synthetic_plan(1, args.rows // 4)
            r["2_words"] = {"row16": bench_synthetic(mgr, cp, reps, copy_gbps.value)}
            emit(name, r)
        elif name == "narrow":
            emit(name, bench_synthetic(mgr, synthetic_plan(0, args.rows // 4 + 1, widths=[1, 2, 4]), reps, copy_gbps.value))
        elif name == "small":
            small_rows = 10_000_000  # a table of its own: one row in a thousand passes
            emit(name, bench_small(mgr, scan_executor(mgr, small_rows), small_rows, reps, copy_gbps.value))
        elif name == "topn":
            emit(name, bench_topn(mgr, ex, min(reps, 3)))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
