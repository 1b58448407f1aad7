"""The routing corpus: a deterministic list of plans crossed with row counts, launch flags and routing switches, and what
`hdk_hip_describe_launch` answers for each combination on the assumed MI355X.

tests/golden/routing_corpus.json holds the answers as they were recorded (PYTHONPATH=. python tests/routing_corpus.py writes it);
tests/test_routing_corpus.py asserts that the library still gives every one of them.  tests/golden/routing_workspaces.json
holds `hdk_hip_workspace_size` on device 0 for the same plans at one billion rows (the same command with --workspaces,
on a machine with the device): for an LDS-strategy plan that is plan region + grid x slab words x 8, so it
exposes the grid.
"""
import ctypes as C
import dataclasses
import json
import os

import numpy as np

from hdk_amd import _abi as A
from hdk_amd._lib import lib, sync_switches
from hdk_amd.ir import And, Agg, Cast, Cmp, ColRef, ExtractYear, FP64, INT32, JoinSpec, KeyRef, Lit, Not, Or, QueryUnit, Type
from hdk_amd.plan import compile_query
from hdk_amd.storage import ArrowStorage, ChunkStats, Column, Table

import fuzz_queries as FQ
import join_variants_cases
import joins_cases
import projection_cases as PC
import syn_queries as SQ
import test_kernel_routing_cpu as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "routing_corpus.json")
GOLDEN_WORKSPACES = os.path.join(os.path.dirname(GOLDEN), "routing_workspaces.json")

ROWS = (100_000, 1_000_000, 1_000_000_000)
FLAGS = {"generic": A.LAUNCH_FORCE_GENERIC, "scalar": A.LAUNCH_FORCE_SCALAR, "global": A.LAUNCH_FORCE_GLOBAL_ATOMICS,
         "partitioned": A.LAUNCH_FORCE_PARTITIONED, "no_cluster": A.LAUNCH_NO_CLUSTER_PROBES, "cluster": A.LAUNCH_CLUSTER_PROBES}
# The switches of csrc/switches.h that a matcher reads and that can change the route.  The valued ones that a matcher reads
# (BHM_PART_MIN_BINS, BHM_PART_REPLICAS, PART_G_LOG2, PERFECT_SLICE_LOG2) size a route's passes and do not choose it: not here.
SWITCHES = ("BH_PARTITIONS_ALWAYS", "BHM_PART_TUPLES", "BHM_WIDE_TUPLES", "FAST_NO_XMODE", "NO_BATCHED_MATCHING_SETS", "NO_BH_DENSE",
            "NO_BH_DENSE_PARTITIONS", "NO_BH_DIRECT", "NO_BH_LDS", "NO_BH_MOD_KEYS", "NO_BH_PACKED", "NO_BH_PARTITIONS", "NO_BH_PLAIN",
            "NO_BHM", "NO_BHM_PARTITIONS", "NO_COLS_KERNEL", "NO_PERFECT_PARTITIONS", "NO_SLICED2", "PART_AOS", "PART_GENERAL", "PART_WIDE",
            "PERFECT_PARTITIONS_ALWAYS", "PROJECT_NO_FAST_JOIN", "PROJECT_ONE_PASS", "S2_NO_PACKED_PAIR", "S2_NO_Y", "SLICED2_ALWAYS",
            "SLICE_FINE_KEYS", "SLICE_GENERAL", "SLICE_TWO_LEVELS", "SLICE_WIDE")
VARIANTS = ("none",) + tuple(FLAGS) + SWITCHES
FUZZ_DRAWS = 40  # (thinned: the golden table stays below the largest file of tests/golden)


def _stats_table(st, name, specs, n=1000):
    """A table that holds statistics only (bench.py's tables live on the device: routing reads their bounds, not their rows)."""
    cols = [Column(c, t, [None], [ChunkStats(lo, hi, False)]) for c, (t, lo, hi) in specs.items()]
    st.add_table(Table(name, cols, [n]))


def _bench_plans():
    """workloads.py's configurations over statistics-only tables."""
    I64, I32 = Type("int", 8, True), Type("int", 4, True)
    out = []
    for name, domain in (("c2", 64), ("c5", 100_000_000)):
        st = ArrowStorage()
        _stats_table(st, "t", {"key": (I64, 0, domain - 1), "val": (I64, -2**31, 2**31 - 1)})
        out.append((name, compile_query(st, QueryUnit("t", groupby=[ColRef("key")], targets=[KeyRef(0, "key"), Agg("sum", ColRef("val"), "s")]))))
    for i, g in enumerate((10, 100, 1000, 10_000, 100_000)):
        st = ArrowStorage()
        _stats_table(st, "syn", {"x": (I32, 1, g), "y10": (I32, 1, 10)})
        y = ColRef("y10")
        out.append((f"bh{i + 1}", compile_query(st, QueryUnit("syn", groupby=[Cast(ColRef("x"), FP64)], targets=[KeyRef(0, "key0")] + [
            Agg(k, y, k) for k in ("count", "sum", "max", "min", "avg")]))))
    import workloads as W
    for name, make in W.SYN_SUITE.items():
        st = ArrowStorage()
        ctype = I64 if name in W.SYN_WIDE else I32
        _stats_table(st, "syn", {c: (ctype, 1, SQ.SYN_COLUMNS[c]) for c in sorted(W._query_columns(make(SQ)))})
        out.append((name, compile_query(st, make(SQ))))
    st = ArrowStorage()
    _stats_table(st, "trips", {"cab_type": (Type("dict", 4), 0, 1), "passenger_count": (Type("int", 2), 0, 6),
                               "pickup_datetime": (Type("timestamp", 8, unit="s"), 1230768000, 1451606399),
                               "trip_distance": (Type("decimal", 8, scale=2), 0, 4999), "total_amount": (Type("decimal", 8, scale=2), 0, 19999)})
    st.get("trips").columns["cab_type"].dictionary = ["green", "yellow"]
    pc, ts = ColRef("passenger_count"), ColRef("pickup_datetime")
    for name, q in (("q1", QueryUnit("trips", groupby=[ColRef("cab_type")], targets=[KeyRef(0, "c"), Agg("count", None, "n")])),
                    ("q2", QueryUnit("trips", groupby=[pc], targets=[KeyRef(0, "p"), Agg("avg", ColRef("total_amount"), "a")])),
                    ("q3", QueryUnit("trips", groupby=[pc, ExtractYear(ts)], targets=[KeyRef(0, "p"), KeyRef(1, "y"), Agg("count", None, "n")])),
                    ("q4", QueryUnit("trips", groupby=[pc, ExtractYear(ts), Cast(ColRef("trip_distance"), INT32)],
                                     targets=[KeyRef(0, "p"), KeyRef(1, "y"), KeyRef(2, "d"), Agg("count", None, "n")]))):
        out.append((name, compile_query(st, q)))
    return out


def _routing_test_plans():
    """Every query of tests/test_kernel_routing_cpu.py, written out again: that file builds its queries inside its tests.  A query
    added there is added here (and to `_star_plans`) with a re-recorded row; nothing checks that for you."""
    rng = np.random.default_rng(3)
    n = 30_000
    st = ArrowStorage()
    y = rng.integers(1, 11, n).astype(np.int32)
    y[rng.random(n) < 0.02] = A.NULL_INT
    grid = lambda hi: (np.arange(n) % hi + 1).astype(np.int32)  # noqa: E731  (every value present: the statistics of the big tables)
    st.import_numpy("syn", {"x10": grid(10), "x1k": grid(1000), "x100k": (np.arange(n) * 3 % 100_000 + 1).astype(np.int32), "x4k": grid(4000),
                            "y10": y, "sparse": (rng.integers(0, 90_000, n) * 7919).astype(np.int32), "d": rng.normal(size=n)}, fragment_size=n // 3 + 1)
    st.import_numpy("t", {"key": rng.integers(0, 64, n, dtype=np.int64), "val": rng.integers(-2**31, 2**31, n, dtype=np.int64),
                          "c": rng.integers(-50, 50, n).astype(np.int32), "k2": rng.integers(0, 7, n).astype(np.int16),
                          "wide": rng.integers(0, 2**40, n, dtype=np.int64)}, fragment_size=n // 3 + 1)
    K, V, C_, Y = ColRef("key"), ColRef("val"), ColRef("c"), ColRef("y10")
    sumv = [KeyRef(0), Agg("sum", V)]
    a, b, c = Cmp(C_, "<", Lit(10)), Cmp(V, ">", Lit(0)), Cmp(K, "<>", Lit(7))
    ya, yb, yc = Cmp(Y, "<=", Lit(7)), Cmp(ColRef("x10"), ">", Lit(2)), Cmp(ColRef("x1k"), "<>", Lit(5))
    qs = [
        QueryUnit("t", groupby=[K], targets=sumv), QueryUnit("t", targets=[Agg("sum", V)]),
        QueryUnit("t", quals=[Cmp(C_, "<", Lit(0))], groupby=[K], targets=sumv),
        QueryUnit("t", quals=[Or(Cmp(V, "<", Lit(0)), Cmp(K, "=", Lit(3)))], groupby=[K], targets=sumv),
        QueryUnit("t", quals=[Or(Cmp(C_, "<", Lit(0)), Cmp(V, ">", Lit(5)))], groupby=[K], targets=sumv),
        QueryUnit("t", groupby=[K, ColRef("k2")], targets=[KeyRef(0), KeyRef(1), Agg("count", None)]),
        QueryUnit("t", quals=[Or(Cmp(C_, "<", Lit(0)), Cmp(V, ">", Lit(5)))], groupby=[K, ColRef("k2")], targets=[KeyRef(0), KeyRef(1), Agg("count", None)]),
        QueryUnit("t", groupby=[K, ColRef("k2")], targets=[KeyRef(0), KeyRef(1), Agg("sum", V), Agg("max", C_)]),
        QueryUnit("t", quals=[Or(And(a, b), Or(And(a, c), And(b, c)))], groupby=[K], targets=sumv),
        QueryUnit("t", quals=[Or(Or(And(a, b), And(a, c)), And(b, c))], groupby=[K], targets=sumv),
        R._bh("x10", quals=[Or(And(ya, yb), Or(And(ya, yc), And(yb, yc)))]), R._bh("x10", quals=[Or(Or(And(ya, yb), And(ya, yc)), And(yb, yc))]),
        R._bh("x10"), R._bh("x1k"), R._bh("x4k"), R._bh("x100k"), R._bh("x10", quals=[ya]),
        QueryUnit("syn", groupby=[Cast(ColRef("x10"), FP64)], targets=[KeyRef(0), Agg("sum", ColRef("d"))]),
        QueryUnit("syn", groupby=[ColRef("x1k") % 37], targets=[KeyRef(0), Agg("sum", Y)]),
        QueryUnit("syn", groupby=[ColRef("x1k") % 37], targets=[KeyRef(0), Agg("sum", ColRef("d"))]),
        QueryUnit("syn", groupby=[ColRef("sparse")], force_baseline=True, baseline_entry_count=180_001, targets=[KeyRef(0), Agg("sum", Y), Agg("count", None)]),
        QueryUnit("t", groupby=[ColRef("wide")], force_baseline=True, baseline_entry_count=200_000_000, targets=sumv),
        QueryUnit("t", groupby=[ColRef("wide")], force_baseline=True, baseline_entry_count=200_000, targets=[KeyRef(0), Agg("min", ColRef("c")), Agg("avg", V)]),
    ]
    out = [(f"r{i}", compile_query(st, q)) for i, q in enumerate(qs)]
    # BH004's 10 000 groups, and the same key as a perfect hash
    st10k = ArrowStorage()
    st10k.import_numpy("syn", {"x10k": (np.arange(20_000) % 10_000 + 1).astype(np.int32), "y10": (np.arange(20_000) % 10 + 1).astype(np.int32)})
    out.append(("r10k", compile_query(st10k, R._bh("x10k"))))
    out.append(("r10kp", compile_query(st10k, QueryUnit("syn", groupby=[ColRef("x10k")], targets=[KeyRef(0, "k")] + [
        Agg(k, ColRef("y10")) for k in ("count", "sum", "max", "min", "avg")]))))
    return out


def _star_plans():
    """the star-schema shapes against a 10 M-key dimension (statistics only), as the executor fuses them"""
    I64, I32 = Type("int", 8, True), Type("int", 4, True)
    nd = 10_000_000
    st = ArrowStorage()
    _stats_table(st, "dim", {"key": (I64, 0, nd - 1), "dval": (I64, 0, 10**6 - 1), "attr": (I64, 0, 63), "dbig": (I64, 0, 2**40)}, nd)
    st.get("dim").__dict__["_unique_keys_cache"] = {("key", False, 1): 1}
    _stats_table(st, "fact", {"fk": (I64, 0, nd - 1), "val": (I64, -2**31, 2**31 - 1), "g": (I64, 0, 63), "g32": (I32, 0, 63)})
    j = [JoinSpec("dim", ColRef("fk"), "key")]
    V, D, At = ColRef("val"), ColRef("dval", "dim"), ColRef("attr", "dim")
    lt = [Cmp(D, "<", Lit(500_000))]
    qs = {"c3": QueryUnit("fact", joins=j, targets=[Agg("sum", V + D)]),
          "c3g": QueryUnit("fact", joins=j, groupby=[D / 15625], targets=[KeyRef(0), Agg("sum", V)]),
          "c3m": QueryUnit("fact", joins=j, targets=[Agg("sum", V), Agg("count", None), Agg("max", D)]),
          "c3gm": QueryUnit("fact", joins=j, groupby=[D % 64], targets=[KeyRef(0), Agg("sum", V)]),
          "c3f": QueryUnit("fact", joins=j, quals=lt, groupby=[At], targets=[KeyRef(0), Agg("sum", V), Agg("count", None)]),
          "c3x": QueryUnit("fact", joins=j, quals=lt, groupby=[ColRef("g32")], targets=[KeyRef(0), Agg("sum", V)]),
          "c3x2": QueryUnit("fact", joins=j, quals=lt, targets=[Agg("sum", V), Agg("sum", ColRef("g")), Agg("count", None)]),
          "c3d": QueryUnit("fact", joins=j, targets=[Agg("sum", D), Agg("min", V)]),
          "c3w": QueryUnit("fact", joins=j, targets=[Agg("sum", V + ColRef("dbig", "dim"))])}  # (a payload beyond 32 bits: no slices)
    return [(name, R._fused(compile_query(st, q))) for name, q in qs.items()]


def _case_plans():
    out = []
    for tag, make in (("j", joins_cases.make_case), ("jv", join_variants_cases.make_variants)):
        st, _sql, cases, proj_cases = make()
        for case in list(cases) + list(proj_cases):
            cp = compile_query(st, case[1])
            out.append((f"{tag}_{case[0]}", cp))
            if cp.plan.num_joins == 1 and cp.plan.joins[0].kind == A.JOIN_ONE_TO_ONE:
                out.append((f"{tag}_{case[0]}_fused", R._fused(cp)))
    case = PC.Case("L3")
    for f in PC.FILTERS:
        out.append((f"p_{f}", compile_query(case.st, PC.query(f, f != "none"))))
    for f in PC.JOIN_FILTERS:
        out.append((f"pj_{f}", compile_query(case.st, PC.query(f, False, join=True))))
    rng = np.random.default_rng(6)
    cols = ("x10", "y10", "z10", "x100", "y100", "z100", "x1k", "x10k", "x100k")
    narrow = SQ.syn_table(rng, 60_000, cols)
    for tag, table in (("s4", narrow), ("s8", {k: v.astype(np.int64) for k, v in narrow.items()})):
        st = ArrowStorage()
        st.import_numpy("syn", table, fragment_size=20_000)
        qs = {"nga1": SQ.nga(1), "nga5": SQ.nga(5), "msbs1": SQ.msbs(1), "msbs1d": SQ.msbs(1, key_type=FP64), "msbs2": SQ.msbs(2),
              "msbs3": SQ.msbs(3, key_type=FP64), "msphs1": SQ.msphs(1), "msphs2": SQ.msphs(2), "msphs3": SQ.msphs(3), "phm1": SQ.phm(1),
              "phm3": SQ.phm(3), "phm5": SQ.phm(5), "msphs1f": SQ.filtered(SQ.msphs(1), "x10", "<", 8),
              "msphs2o": dataclasses.replace(SQ.msphs(2), quals=[Or(Cmp(ColRef("x10"), "<", Lit(4)), Not(Cmp(ColRef("x100"), ">", Lit(50))))]),
              "ngaf": QueryUnit("syn", quals=[Cmp(ColRef("x10"), ">", Lit(3))], targets=[Agg("sum", ColRef("x100")), Agg("sum", ColRef("y100"))])}
        out += [(f"{tag}_{k}", compile_query(st, q)) for k, q in qs.items()]
    return out


def _fuzz_plans():
    from hdk_amd.plan import QueryMustRunOnCpu
    rng = np.random.default_rng(20261019)
    st = FQ.make_tables(rng, 4000, 300)
    stw = FQ.make_tables_wide(rng, 4000, 300)
    out = []
    for i in range(FUZZ_DRAWS):
        wide, proj = i % 4 == 3, i % 5 == 4
        q = FQ.random_query_wide(rng, projection=proj, not_null=False) if wide else FQ.random_query(rng, projection=proj)
        try:
            out.append((f"f{i}", compile_query(stw if wide else st, q)))
        except QueryMustRunOnCpu:
            pass
    return out


def corpus():
    """[(id, compiled plan)], the same list on every call"""
    return _routing_test_plans() + _star_plans() + _bench_plans() + _case_plans() + _fuzz_plans()


def describe(cp, total_rows, flags=0, device=R.ASSUMED_MI355X):
    ko = A.KernelOptions(0, 0, 0, flags, total_rows, 0, 0)
    out = C.create_string_buffer(256)
    st = lib().hdk_hip_describe_launch(C.byref(cp.plan), C.byref(ko), device, out, 256)
    return out.value.decode() if st == 0 else f"error {st}"


def describe_all(plans):
    """{id: [{variant: names} per row count]}"""
    out = {pid: [{} for _ in ROWS] for pid, _ in plans}
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("HDK_HIP_") and k != "HDK_HIP_LIB"}
    try:
        for v in VARIANTS:
            if v in SWITCHES:
                os.environ["HDK_HIP_" + v] = "1"
            sync_switches()
            for pid, cp in plans:
                for ri, rows in enumerate(ROWS):
                    out[pid][ri][v] = describe(cp, rows, FLAGS.get(v, 0))
            os.environ.pop("HDK_HIP_" + v, None)
    finally:
        os.environ.update(saved)
        sync_switches()
    return out


def pack(table):
    """the table with every string written once and a variant's answer only where it differs from the plain launch's"""
    names = sorted({s for rows in table.values() for r in rows for s in r.values()})
    idx = {s: i for i, s in enumerate(names)}
    packed = {pid: [[idx[r["none"]], {str(VARIANTS.index(v)): idx[s] for v, s in r.items() if s != r["none"]}] for r in rows]
              for pid, rows in table.items()}
    return {"variants": list(VARIANTS), "rows": list(ROWS), "names": names, "plans": packed}


def unpack(g):
    return {pid: [{v: g["names"][diff.get(str(vi), base)] for vi, v in enumerate(g["variants"])} for base, diff in rows]
            for pid, rows in g["plans"].items()}


def workspace_sizes(plans, device=0):
    sync_switches()
    out = {}
    for pid, cp in plans:
        ko = A.KernelOptions(0, 0, 0, 0, ROWS[-1], 0, 0)
        b = C.c_size_t(0)
        st = lib().hdk_hip_workspace_size(C.byref(cp.plan), C.byref(ko), device, C.byref(b))
        out[pid] = int(b.value) if st == 0 else -st
    return out


if __name__ == "__main__":
    import sys
    if "--workspaces" in sys.argv:
        sync_switches()
        text = json.dumps(workspace_sizes(corpus()), separators=(",", ":"))
        path = GOLDEN_WORKSPACES
    else:
        text = json.dumps(pack(describe_all(corpus())), separators=(",", ":"))
        path = GOLDEN
    path = sys.argv[sys.argv.index("-o") + 1] if "-o" in sys.argv else path
    with open(path, "w") as f:
        f.write(text + "\n")
    print(path, len(text), "bytes")
