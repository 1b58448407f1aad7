#!/usr/bin/env python3
"""Device-side columnar results (hdk_hip_columnarize_result) on three result tables of one MI355X:

    c5    C5's own output (workloads.py): 200 M entries row-wise, about half of them groups
    c2m   a 25.6 M-entry perfect-hash table (256 M rows by a key of 25.6 M values; scripts/bench_configs.py: c2m)
    bh4   BH004's 10 000-group table, the small-result case

For each: the kernel time of the three launches (HIP events on the launch stream, median), the modelled bytes (row-wise:
the table twice plus the output; columnar: the probed column plus the table plus the output), the achieved GB/s next to
the copy rate hdk_hip_mgr_measure_hbm reports in the same process, and the wall time to host numpy arrays through
fetch_columns().to_host() next to fetch() on the same buffer.

    python scripts/bench_result_columns.py [--only c5,c2m,bh4] [--c5-rows N] [--reps 7] [--out file.json]
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


def c2m_step(mgr, rows):
    """GROUP BY hk, SUM(val) with hk uniform in [0, rows / 10): perfect hash, rows / 10 entries, generated on the device."""
    import torch
    from hdk_amd.executor import Executor
    from hdk_amd.ir import Agg, ColRef, KeyRef, QueryUnit, Type
    from hdk_amd.storage import ArrowStorage, ChunkStats, Column, Table
    from workloads import SEED, TensorChunk, fragment_rows
    dev = torch.device("cuda", 0)
    st = ArrowStorage()
    ex = Executor(st, 0, mgr)
    frag_rows = fragment_rows(rows)
    domain = max(rows // 10, 1000)
    i64 = Type("int", 8, True)
    cols = []
    for salt, (name, lo, hi) in enumerate((("hk", 0, domain), ("val", -2**31, 2**31))):
        cols.append(Column(name, i64, [None] * len(frag_rows), [ChunkStats(lo, hi - 1, False)] * len(frag_rows)))
        for f, n in enumerate(frag_rows):
            g = torch.Generator(device=dev)
            g.manual_seed(SEED + 1000 * salt + f)
            ex.cache.put(("t", name, f), TensorChunk(torch.randint(lo, hi, (n,), dtype=torch.int64, device=dev, generator=g)))
    st.add_table(Table("t", cols, frag_rows))
    torch.cuda.synchronize(dev)
    q = QueryUnit("t", groupby=[ColRef("hk")], targets=[KeyRef(0, "hk"), Agg("sum", ColRef("val"), "s")])
    return ex.prepare(q), None


def workload_step(mgr, name, rows):
    from workloads import Workload
    w = Workload(name, rows, 0, mgr)
    return w.ex.prepare(w.compiled, w.frag_ids), w


def measure(mgr, step, reps, copy_gbps):
    import torch
    from hdk_amd import _abi as A
    from hdk_amd._lib import check, lib
    L = lib()
    cp, p = step.cp, step.cp.plan
    n, nt = int(cp.entry_count), int(p.num_targets)
    step.enqueue()
    mgr.synchronizeStream(0)
    iv = np.ascontiguousarray(cp.init_vals, dtype=np.int64)
    d_rows = mgr.alloc(8, 0)
    ws_bytes = L.hdk_hip_result_columns_workspace_bytes(n)
    d_ws = mgr.alloc(ws_bytes, 0)

    def call(out_ptr, cap):
        check(L.hdk_hip_columnarize_result(C.byref(p), step.out_ptr, n, iv.ctypes.data, out_ptr, cap, d_rows.ptr, d_ws.ptr,
                                           ws_bytes, 0, None))

    call(None, 0)
    mgr.synchronizeStream(0)
    rows = int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0])
    d_out = mgr.alloc(max(nt * rows * 8, 8), 0)
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))
    kernel_ms, count_ms = [], []
    for i in range(2 + reps):  # two warm-up calls
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record(stream)
        call(None, 0)
        e1.record(stream)
        call(d_out.ptr, rows)
        e2.record(stream)
        mgr.synchronizeStream(0)
        if i >= 2:
            count_ms.append(e0.elapsed_time(e1))
            kernel_ms.append(e1.elapsed_time(e2))
    table_bytes = int(step.buffer_bytes)
    out_bytes = nt * rows * 8
    if p.output_columnar:
        probed = n * (cp.slot_widths[p.idx_target_as_key] if p.keyless else 8)
        model = probed + table_bytes + out_bytes
    else:
        model = 2 * table_bytes + out_bytes
    k_ms = statistics.median(kernel_ms)
    # end to end: host numpy arrays through the new path, and the host copy of the whole buffer through fetch()
    new_s, old_s = [], []
    for i in range(1 + reps):
        t0 = time.perf_counter()
        cols = step.fetch_columns(stream_synced=True)
        host = cols.to_host()
        t1 = time.perf_counter()
        cols.free()
        res = step.fetch(stream_synced=True)
        t2 = time.perf_counter()
        if i >= 1:
            new_s.append(t1 - t0)
            old_s.append(t2 - t1)
        assert len(host) == nt and len(host[0]) == rows and res.buffer.nbytes == table_bytes
        del host, res, cols
    for d in (d_rows, d_ws, d_out):
        d.free()
    gbps = model / (k_ms * 1e-3) / 1e9
    return {
        "entry_count": n, "rows": rows, "num_targets": nt, "layout": "columnar" if p.output_columnar else "row-wise",
        "row_bytes": int(p.row_size_quad) * 8, "table_bytes": table_bytes, "output_bytes": out_bytes,
        "modelled_bytes": model, "kernel_ms_median": k_ms, "kernel_ms_all": kernel_ms,
        "count_only_ms_median": statistics.median(count_ms),
        "achieved_GBps": gbps, "fraction_of_copy_rate": gbps / copy_gbps,
        "to_host_via_fetch_columns_ms_median": statistics.median(new_s) * 1e3,
        "to_host_via_fetch_ms_median": statistics.median(old_s) * 1e3,
        "to_host_via_fetch_columns_ms_all": [x * 1e3 for x in new_s], "to_host_via_fetch_ms_all": [x * 1e3 for x in old_s],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="c5,c2m,bh4")
    ap.add_argument("--c5-rows", type=int, default=1_000_000_000)
    ap.add_argument("--rows", type=int, default=256_000_000, help="rows of the c2m and bh4 inputs")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from hdk_amd._lib import check, lib
    from hdk_amd.hip_mgr import HipMgr
    mgr = HipMgr()
    copy_gbps, read_gbps = C.c_double(0), C.c_double(0)
    check(lib().hdk_hip_mgr_measure_hbm(0, 4 << 30, 3, C.byref(copy_gbps), C.byref(read_gbps)))
    result = {"what": "hdk_hip_columnarize_result: count + scan + compact on one MI355X; medians of %d repetitions after warm-up" % args.reps,
              "hbm_copy_GBps": copy_gbps.value, "hbm_read_GBps": read_gbps.value, "tables": {}}
    for name in args.only.split(","):
        if name == "c5":
            step, keep = workload_step(mgr, "c5", args.c5_rows)
            note = "C5's own output (workloads.py), %d input rows" % args.c5_rows
        elif name == "c2m":
            step, keep = c2m_step(mgr, args.rows)
            note = "GROUP BY hk, SUM(val): %d rows, hk uniform in [0, rows / 10)" % args.rows
        else:
            step, keep = workload_step(mgr, name, args.rows)
            note = "workloads.py %s, %d input rows" % (name, args.rows)
        r = measure(mgr, step, max(args.reps, 5), copy_gbps.value)
        r["input"] = note
        r["kernels"] = step.kernel_names()
        result["tables"][name] = r
        print(json.dumps({name: r}), flush=True)
        step.free()
        step.ex.cache.clear()
        del step, keep
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
