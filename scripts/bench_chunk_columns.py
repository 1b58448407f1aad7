#!/usr/bin/env python3
"""Scanning a device result (hdk_hip_chunk_columns, Executor.register_columns) on one MI355X.  The result is (k, v): two
int64 columns, k in [0, 1024) with NULLs as a 4-byte slot writes them (INT32_MIN sign-extended), v small integers.

    call     hdk_hip_chunk_columns alone over preallocated output, statistics and workspace: HIP events, median of --reps
             calls after warm-up, against the copy rate hdk_hip_mgr_measure_hbm reports in the same process.  The model:
             8 bytes read and 8 written per word; the partials (32 bytes per column and 4 096 rows) are left out
    chained  SELECT k, SUM(v), COUNT(*) FROM <result> GROUP BY k end to end, wall clock: register_columns + execute +
             drop_registered, against the way there was before: to_host() + import_numpy + execute (the upload happens
             inside execute) + the cache dropped again
    small    the same chained comparison over 10 000 rows, where the host is expected to win

Every figure is a median; the single values are kept next to it.  The statistics and the outer result are first compared
with numpy.

    python scripts/bench_chunk_columns.py [--only call,chained,small] [--rows N] [--reps 5] [--out f.json]
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

NULL_I32, NULL_I64 = -2**31, -2**63
KEYS = 1024


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
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            ms.append(dt)
    return statistics.median(ms), ms


def make_columns(mgr, n, seed=16):
    from hdk_amd.executor import DeviceColumns
    from hdk_amd.ir import Type
    from hdk_amd.plan import ColumnDesc
    rng = np.random.default_rng(seed)
    k = rng.integers(0, KEYS, n).astype(np.int64)
    k[::97] = NULL_I32
    v = rng.integers(-100, 100, n).astype(np.int64)
    block = mgr.to_device(np.concatenate([k, v]), 0)
    schema = [ColumnDesc("k", False, True, NULL_I32, Type("int", 4, True), 0, "key"),
              ColumnDesc("v", False, False, 0, Type("int", 8, False), 1, "agg", "sum")]
    return DeviceColumns(None, mgr, 0, block, n, n, schema=schema), k, v


def outer_unit(table):
    from hdk_amd.ir import Agg, ColRef, KeyRef, QueryUnit
    return QueryUnit(table, groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s"), Agg("count", None, "n")],
                     bigint_count=True)


def expected_groups(k, v):
    valid = k != NULL_I32
    s = np.bincount(k[valid], weights=v[valid].astype(np.float64), minlength=KEYS)
    c = np.bincount(k[valid], minlength=KEYS)
    rows = {int(i): (int(s[i]), int(c[i])) for i in np.flatnonzero(c)}
    if (~valid).any():
        rows[None] = (int(v[~valid].sum()), int((~valid).sum()))
    return rows


def groups_of(res):
    cols = res.to_columns()
    return {k: (s, n) for k, s, n in zip(cols["k"], cols["s"], cols["n"])}


def call_case(mgr, n, reps, copy_gbps):
    import torch
    from hdk_amd import _abi as A
    from hdk_amd._lib import check, lib
    from hdk_amd.storage import DEFAULT_FRAGMENT_SIZE
    L = lib()
    cols, k, v = make_columns(mgr, n)
    frag = DEFAULT_FRAGMENT_SIZE
    nf = max(1, -(-n // frag))
    ocap = (n + 31) // 32 * 32
    sel = (A.ChunkCol * 2)(A.ChunkCol(0, 0, 1, (C.c_uint8 * 2)(), NULL_I32, NULL_I64), A.ChunkCol(1, 0, 0, (C.c_uint8 * 2)(), 0, NULL_I64))
    need = L.hdk_hip_chunk_columns_workspace_bytes(n, frag, 2)
    out, d_stats, ws = mgr.alloc(2 * ocap * 8, 0), mgr.alloc(2 * nf * 32, 0), mgr.alloc(max(need, 8), 0)
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))

    def call():
        check(L.hdk_hip_chunk_columns(cols.block.ptr, n, 2, n, sel, 2, frag, out.ptr, ocap, d_stats.ptr, ws.ptr, need, 0, None))

    call()
    mgr.synchronizeStream(0)
    st = mgr.to_host(d_stats.ptr, 2 * nf * 32, 0, np.int64).reshape(2, nf, 4)
    for f in range(nf):
        kk, vv = k[f * frag:(f + 1) * frag], v[f * frag:(f + 1) * frag]
        ok = kk != NULL_I32
        assert st[0, f].tolist() == [int(kk[ok].min()), int(kk[ok].max()), int((~ok).sum()), int(ok.sum())], (f, st[0, f])
        assert st[1, f].tolist() == [int(vv.min()), int(vv.max()), 0, len(vv)], (f, st[1, f])
    got = mgr.to_host(out.ptr, n * 8, 0, np.int64)
    assert np.array_equal(got, np.where(k == NULL_I32, NULL_I64, k))
    ms, all_ms = events_ms(mgr, stream, call, reps)
    for b in (out, d_stats, ws):
        b.free()
    cols.free()
    model_bytes = 2 * n * 16
    res = {"what": "hdk_hip_chunk_columns alone, %d rows x 2 columns in fragments of %d rows" % (n, frag), "ms_median": ms,
           "ms_all": all_ms, "model_bytes": model_bytes, "model_GBps": model_bytes / ms / 1e6, "workspace_bytes": need,
           "fraction_of_copy_rate": model_bytes / ms / 1e6 / copy_gbps}
    print(json.dumps({"call": res}), flush=True)
    return {"call": res}


def chained_case(mgr, n, reps, label):
    from hdk_amd.executor import Executor
    from hdk_amd.storage import ArrowStorage
    cols, k, v = make_columns(mgr, n)
    want = expected_groups(k, v)
    ex = Executor(ArrowStorage(), 0, mgr)

    def device_way():
        ex.register_columns("r", cols)
        try:
            return ex.execute(outer_unit("r"))
        finally:
            ex.drop_registered("r")

    def host_way():
        h = cols.to_host()
        host = [np.where(h[0] == NULL_I32, NULL_I64, h[0]), h[1]]  # the sentinel rewrite, on the host
        ex.storage.import_numpy("h", {"k": host[0], "v": host[1]})
        try:
            return ex.execute(outer_unit("h"))
        finally:
            ex.storage.drop_table("h")
            ex.cache.clear()

    assert groups_of(device_way()) == want and groups_of(host_way()) == want
    dev_ms, dev_all = wall_ms(device_way, reps, 1 if n > 10**6 else 3)
    host_ms, host_all = wall_ms(host_way, reps, 1 if n > 10**6 else 3)
    cols.free()
    res = {"what": "SELECT k, SUM(v), COUNT(*) FROM <result of %d rows x 2> GROUP BY k, wall clock: register_columns + execute + "
                   "drop_registered against to_host + import_numpy + execute (with its upload)" % n,
           "device_ms_median": dev_ms, "device_ms_all": dev_all, "host_ms_median": host_ms, "host_ms_all": host_all,
           "host_over_device": host_ms / dev_ms, "winner": "host" if host_ms < dev_ms else "device"}
    print(json.dumps({label: res}), flush=True)
    return {label: res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="call,chained,small")
    ap.add_argument("--rows", type=int, default=100_000_000)
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
    result = {"what": "hdk_hip_chunk_columns / Executor.register_columns on one MI355X; medians of %d calls after warm-up" % reps,
              "rows": args.rows, "hbm_copy_GBps": copy_gbps.value, "hbm_read_GBps": read_gbps.value, "cases": {}}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    if "call" in only:
        result["cases"].update(call_case(mgr, args.rows, reps, copy_gbps.value))
        save()
    if "chained" in only:
        result["cases"].update(chained_case(mgr, args.rows, reps, "chained"))
        save()
    if "small" in only:
        result["cases"].update(chained_case(mgr, 10_000, reps, "small"))
    save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
