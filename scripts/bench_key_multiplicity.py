#!/usr/bin/env python3
"""The key multiplicity of a join key (hdk_hip_key_multiplicity) and a join against a device result on one MI355X.

Single-key cases, the call alone over a preallocated record and workspace: HIP events, median of --reps calls after
warm-up, each against the copy rate hdk_hip_mgr_measure_hbm reports in the same process and against the way there was
before, to_host() + np.unique(return_counts=True) on the same column (wall clock).  The model: 8 bytes read per row, and per
slot of the histogram 4 bytes zeroed and 4 read; the atomic adds are left out (they stay in the L2 when the table fits).
    a  --rows rows, a dense unique key in random order
    b  the same keys sorted
    c  --rows rows of ONE key: the wave-uniform add; what the numbers decide is whether c stays within a small factor of a
    d  --big-rows rows over a range of as many slots
Composite key (the sorted route; wall clock, the call synchronises where its sort does):
    e  --rows rows over a 2-column key
End to end, wall clock:
    f  a --fact-rows fact table JOIN a --rows device result (a GROUP BY of a registered table), SUM(val + s); the result
       registered and joined where it lies against the same result through to_host() + import_numpy

Every figure is a median; the single values are kept next to it.  Each answer is first compared with numpy.

    python scripts/bench_key_multiplicity.py [--only a,b,c,d,e,f] [--rows N] [--reps 5] [--out f.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_chunk_columns import events_ms, wall_ms  # noqa: E402  (the timing helpers of the sibling script)

NULL_I64 = -2**63


def call_case(mgr, label, what, cols, keys_desc, entry_count, reps, copy_gbps, want, sync_route=False):
    """cols: the int64 columns of the block; keys_desc: (col, min, max) per key"""
    import torch
    from hdk_amd import _abi as A
    from hdk_amd._lib import check, lib
    L = lib()
    n = len(cols[0])
    block = mgr.to_device(np.concatenate(cols), 0)
    keys = (A.MultiplicityKey * len(keys_desc))()
    for i, (c, mn, mx) in enumerate(keys_desc):
        keys[i] = A.MultiplicityKey(c, 1, (C.c_uint8 * 3)(), NULL_I64, mn, mx, mx + 1)
    need = L.hdk_hip_key_multiplicity_workspace_bytes(n, keys, len(keys_desc), entry_count)
    rec, ws = mgr.alloc(32, 0), mgr.alloc(max(need, 8), 0)
    stream = torch.cuda.ExternalStream(mgr.getStream(0), device=torch.device("cuda", 0))

    def call():
        check(L.hdk_hip_key_multiplicity(block.ptr, n, len(cols), n, keys, len(keys_desc), entry_count, 1, 0, rec.ptr, ws.ptr, need,
                                         0, None))

    call()
    mgr.synchronizeStream(0)
    got = tuple(int(x) for x in mgr.to_host(rec.ptr, 32, 0, np.uint64))
    assert got == want, (label, got, want)

    def synced():
        call()
        mgr.synchronizeStream(0)

    ms, all_ms = wall_ms(synced, reps, 2) if sync_route else events_ms(mgr, stream, call, reps)

    def host_way():
        h = mgr.to_host(block.ptr, len(cols) * n * 8, 0, np.int64).reshape(len(cols), n)
        if len(keys_desc) == 1:
            return int(np.unique(h[keys_desc[0][0]], return_counts=True)[1].max())
        return int(np.unique(np.stack([h[c] for c, _, _ in keys_desc], axis=1), axis=0, return_counts=True)[1].max())

    assert host_way() == want[0]
    host_ms, host_all = wall_ms(host_way, 1 if len(keys_desc) > 1 else 3, 0)  # (np.unique over rows takes a minute)
    for b in (block, rec, ws):
        b.free()
    res = {"what": what, "rows": n, "entry_count": entry_count, "record": got, "ms_median": ms, "ms_all": all_ms,
           "timed_with": "wall clock, stream synchronised" if sync_route else "HIP events", "workspace_bytes": need,
           "host_ms_median": host_ms, "host_ms_all": host_all, "host_over_device": host_ms / ms}
    if not sync_route:
        model = 8 * n + 8 * entry_count
        res.update({"model_bytes": model, "model_GBps": model / ms / 1e6, "fraction_of_copy_rate": model / ms / 1e6 / copy_gbps,
                    "rows_per_us": n / ms / 1e3})
    print(json.dumps({label: res}), flush=True)
    return {label: res}


def join_case(mgr, fact_rows, n, reps):
    """f: fact JOIN (SELECT k, SUM(v) s FROM t GROUP BY k) d ON fact.k = d.k, SUM(val + s)"""
    from hdk_amd.executor import Executor
    from hdk_amd.ir import Agg, BinOp, ColRef, JoinSpec, KeyRef, QueryUnit
    from hdk_amd.storage import ArrowStorage
    rng = np.random.default_rng(17)
    st = ArrowStorage()
    st.import_numpy("fact", {"k": rng.integers(0, n, fact_rows).astype(np.int64), "val": rng.integers(0, 100, fact_rows).astype(np.int64)})
    tk = rng.permutation(n).astype(np.int64)
    tv = rng.integers(-100, 100, n).astype(np.int64)
    st.import_numpy("t", {"k": tk, "v": tv})
    ex = Executor(st, 0, mgr)
    # the registered table the inner unit aggregates, and the aggregate as dense columns
    tcols = ex.execute(QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "v")]), result="columns")
    ex.register_columns("treg", tcols)
    tcols.free()
    agg = ex.execute(QueryUnit("treg", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s")]), result="columns")
    assert agg.num_rows == n

    def unit(table):
        return QueryUnit("fact", joins=[JoinSpec(table, ColRef("k"), "k")],
                         targets=[Agg("sum", BinOp("+", ColRef("val"), ColRef("s", table)), "x"), Agg("count", None, "n")])

    def device_way():
        ex.register_columns("d", agg, joinable=True)
        try:
            return ex.execute(unit("d")).to_columns()
        finally:
            ex.drop_registered("d")

    def host_way():
        h = agg.to_host()
        ex.storage.import_numpy("h", {"k": h[0], "s": h[1]})
        try:
            return ex.execute(unit("h")).to_columns()
        finally:
            for cache in (ex._join_cache, ex._fused_cache):
                for key in [k for k in cache if k[0] == "h"]:
                    cache.pop(key).free()
            ex.storage.drop_table("h")
            for key in [k for k in ex.cache._chunks if k[0] == "h"]:
                ex.cache._chunks.pop(key).free()

    fk = st.get("fact").columns["k"].fragments
    s_of = np.zeros(n, dtype=np.int64)
    s_of[tk] = tv
    want_x = sum(int(s_of[f].sum()) for f in fk) + sum(int(f.sum()) for f in st.get("fact").columns["val"].fragments)
    a, b = device_way(), host_way()
    assert a["x"][0] == b["x"][0] == want_x and a["n"][0] == b["n"][0] == fact_rows, (a, b, want_x)
    dev_ms, dev_all = wall_ms(device_way, reps, 1)
    host_ms, host_all = wall_ms(host_way, reps, 1)
    agg.free()
    ex.drop_registered("treg")
    res = {"what": "SELECT SUM(val + s) FROM fact (%d rows) JOIN <GROUP BY result of %d rows> d ON fact.k = d.k, wall clock: "
                   "register_columns + execute (key multiplicity, build, probe) + drop_registered against to_host + import_numpy + "
                   "execute (upload, build, probe)" % (fact_rows, n),
           "device_ms_median": dev_ms, "device_ms_all": dev_all, "host_ms_median": host_ms, "host_ms_all": host_all,
           "host_over_device": host_ms / dev_ms}
    print(json.dumps({"f": res}), flush=True)
    return {"f": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b,c,d,e,f")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--big-rows", type=int, default=100_000_000)
    ap.add_argument("--fact-rows", type=int, default=256_000_000)
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
    result = {"what": "hdk_hip_key_multiplicity / a join against a registered result on one MI355X; medians of %d calls after warm-up"
                      % reps, "hbm_copy_GBps": copy_gbps.value, "hbm_read_GBps": read_gbps.value, "cases": {}}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    n = args.rows
    rng = np.random.default_rng(17)
    t0 = time.perf_counter()
    if "a" in only:
        k = rng.permutation(n).astype(np.int64)
        result["cases"].update(call_case(mgr, "a", "a dense unique key in random order", [k], [(0, 0, n - 1)], n, reps, copy_gbps.value,
                                         (1, n, n, 0)))
        save()
    if "b" in only:
        k = np.arange(n, dtype=np.int64)
        result["cases"].update(call_case(mgr, "b", "the same keys sorted", [k], [(0, 0, n - 1)], n, reps, copy_gbps.value, (1, n, n, 0)))
        save()
    if "c" in only:
        k = np.full(n, 7, dtype=np.int64)
        result["cases"].update(call_case(mgr, "c", "one key in every row, a table of 1 024 slots", [k], [(0, 0, 1023)], 1024, reps,
                                         copy_gbps.value, (n, 1, n, 0)))
        save()
    if "d" in only:
        m = args.big_rows
        k = rng.integers(0, m, m).astype(np.int64)
        cnt = np.bincount(k, minlength=m)
        want = (int(cnt.max()), int(np.count_nonzero(cnt)), m, 0)
        del cnt
        result["cases"].update(call_case(mgr, "d", "random keys over a range of as many slots as rows", [k], [(0, 0, m - 1)], m, reps,
                                         copy_gbps.value, want))
        save()
    if "e" in only:
        a, b = rng.integers(0, 3000, n).astype(np.int64), rng.integers(0, 3000, n).astype(np.int64)
        cnt = np.unique(a * 3000 + b, return_counts=True)[1]
        result["cases"].update(call_case(mgr, "e", "a 2-column key, 9 M possible pairs, random order (the sorted route)", [a, b],
                                         [(0, 0, 2999), (1, 0, 2999)], 0, reps, copy_gbps.value, (int(cnt.max()), len(cnt), n, 0),
                                         sync_route=True))
        save()
    if "f" in only:
        result["cases"].update(join_case(mgr, args.fact_rows, n, 3))
    result["seconds"] = time.perf_counter() - t0
    save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
