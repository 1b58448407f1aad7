"""GROUP BY over dense result columns through the query path: DeviceColumns.group_by as a roll-up of a finer GROUP BY,
ir.Agg("count_distinct") through Executor.execute(result="columns"), SELECT DISTINCT, and the schema a regrouped result
carries through sort(), filter(), to_columns() and to_arrow().  References: this library's own direct GROUP BY (held to
the oracle by the existing tests), numpy on the table, and SQLite."""
import dataclasses
import sqlite3

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd.ir import Agg, Cmp, ColRef, KeyRef, Lit, OrderEntry, Proj, QueryMustRunOnCpu, QueryUnit, TargetRef
from hdk_amd.plan import compile_query, describe_columns
from hdk_amd.storage import ArrowStorage

pytestmark = pytest.mark.gpu

N = 50_000
NULL = A.NULL_BIGINT


def _columns():
    rng = np.random.default_rng(2031)
    k = rng.integers(0, 300, N).astype(np.int64)
    g = rng.integers(0, 4, N).astype(np.int64)
    x = rng.integers(0, 40, N).astype(np.int64)
    x[rng.random(N) < 0.1] = NULL
    x[k == 7] = NULL  # a group whose distinct arguments are all NULL
    v = rng.integers(-1000, 1000, N).astype(np.int64)
    w = rng.integers(-50, 50, N).astype(np.int64)
    w[rng.random(N) < 0.6] = NULL
    w[k == 11] = NULL
    f = rng.integers(1, 1000, N) / 4.0
    return {"k": k, "g": g, "x": x, "v": v, "w": w, "f": f}


@pytest.fixture(scope="module")
def table():
    return _columns()


@pytest.fixture(scope="module")
def storage(table):
    st = ArrowStorage()
    st.import_numpy("t", table, fragment_size=20_000)
    return st


@pytest.fixture(scope="module")
def db(table):
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE t (k INTEGER, g INTEGER, x INTEGER, v INTEGER, w INTEGER, f REAL)")
    cols = [table[c].tolist() for c in ("k", "g", "x", "v", "w")] + [table["f"].tolist()]
    rows = [tuple(None if (i < 5 and c == NULL) else c for i, c in enumerate(r)) for r in zip(*cols)]
    con.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?, ?)", rows)
    return con


def _sorted_rows(columns, by):
    names = list(columns)
    rows = list(zip(*[columns[c] for c in names]))
    key = [names.index(b) for b in by]
    return names, sorted(rows, key=lambda r: tuple((r[i] is None, r[i]) for i in key))


def _assert_rows_equal(got, want, approx=()):
    assert got[0] == want[0]
    assert len(got[1]) == len(want[1])
    for a, b in zip(got[1], want[1]):
        for name, x, y in zip(got[0], a, b):
            if name in approx and x is not None and y is not None:
                assert abs(x - y) <= 1e-6 * abs(y), (name, a, b)
            else:
                assert x == y, (name, a, b)


# (two keys and six aggregates: the fine plan uses all of the library's 8 targets)
_AGGS = [Agg("count", None, "n"), Agg("sum", ColRef("v"), "s"), Agg("min", ColRef("w"), "mn"), Agg("max", ColRef("w"), "mx"),
         Agg("count", ColRef("w"), "cw"), Agg("sum", ColRef("f"), "sf")]
_ROLLUP = [("id", "k", None), ("sum", "n", "n"), ("sum", "s", "s"), ("min", "mn", "mn"), ("max", "mx", "mx"), ("sum", "cw", "cw"),
           ("sum", "sf", "sf")]


@pytest.mark.parametrize("baseline", [False, True])
def test_roll_up_equals_the_direct_group_by(gpu_executor_factory, storage, table, baseline):
    ex = gpu_executor_factory(storage)
    fine = QueryUnit("t", groupby=[ColRef("k"), ColRef("x")], targets=[KeyRef(0, "k"), KeyRef(1, "x")] + _AGGS,
                     force_baseline=baseline)
    direct = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k")] + _AGGS)
    kind = compile_query(storage, fine).plan.query_kind
    assert kind == (A.Q_BASELINE_HASH if baseline else A.Q_PERFECT_HASH)
    cols = ex.execute(fine, result="columns")
    want = ex.execute(direct, result="columns")
    try:
        assert cols.columns() == describe_columns(cols.compiled) and cols.num_rows > 5 * want.num_rows
        rolled = cols.group_by(["k"], _ROLLUP)
        try:
            assert rolled.num_rows == want.num_rows == 300 and rolled.schema is not None
            got = rolled.to_columns()
            assert got["k"] == sorted(got["k"])  # the regroup sorts by its keys
            _assert_rows_equal(_sorted_rows(got, ["k"]), _sorted_rows(want.to_columns(), ["k"]), approx=("sf",))
            # numpy on the table
            k = table["k"]
            assert got["n"] == np.bincount(k, minlength=300).tolist()
            assert got["s"] == np.bincount(k, weights=table["v"], minlength=300).astype(np.int64).tolist()
            assert got["mn"][11] is None and got["mx"][11] is None and got["cw"][11] == 0  # no value in the group
            valid = table["w"] != NULL
            assert got["cw"] == np.bincount(k[valid], minlength=300).tolist()
            assert got["mx"][3] == int(table["w"][valid & (k == 3)].max())
        finally:
            rolled.free()
        assert cols.block is not None and cols.block.ptr  # the source stays valid
    finally:
        cols.free()
        want.free()


def _count_distinct_sql(db, keys, where=""):
    names = ", ".join(keys)
    sql = (f"SELECT {names}, COUNT(DISTINCT x), COUNT(*), SUM(v), MIN(w), MAX(w), COUNT(w) FROM t {where} GROUP BY {names} "
           f"ORDER BY {names}")
    return [tuple(r) for r in db.execute(sql)]


@pytest.mark.parametrize("keys", [["k"], ["k", "g"]])
@pytest.mark.parametrize("filtered", [False, True])
def test_count_distinct_against_sqlite_and_numpy(gpu_executor_factory, storage, table, db, keys, filtered):
    ex = gpu_executor_factory(storage)
    q = QueryUnit("t", quals=[Cmp(ColRef("v"), ">", Lit(0))] if filtered else [], groupby=[ColRef(c) for c in keys],
                  targets=[KeyRef(i, c) for i, c in enumerate(keys)] +
                  [Agg("count_distinct", ColRef("x"), "dx"), Agg("count", None, "n"), Agg("sum", ColRef("v"), "s"),
                   Agg("min", ColRef("w"), "mn"), Agg("max", ColRef("w"), "mx"), Agg("count", ColRef("w"), "cw")])
    got = ex.execute(q, result="columns")
    try:
        cols = got.to_columns()
        assert list(cols) == keys + ["dx", "n", "s", "mn", "mx", "cw"]
        rows = list(zip(*cols.values()))
        assert rows == _count_distinct_sql(db, keys, "WHERE v > 0" if filtered else "")  # (the regroup sorts by the keys)
        if keys == ["k"]:
            assert cols["dx"][7] == 0  # every argument of the group is NULL
            keep = (table["v"] > 0) if filtered else np.ones(N, dtype=bool)
            for kk in (0, 7, 150, 299):
                xs = table["x"][keep & (table["k"] == kk)]
                assert cols["dx"][kk] == len(set(xs[xs != NULL].tolist()))
    finally:
        got.free()


def test_count_distinct_then_having_order_and_limit(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    q = QueryUnit("t", groupby=[ColRef("k")],
                  targets=[Agg("count_distinct", ColRef("x"), "dx"), KeyRef(0, "k"), Agg("count_distinct", ColRef("x"), "again")],
                  having=[Cmp(TargetRef("dx"), ">=", Lit(39))], order_by=[OrderEntry("dx", desc=True), OrderEntry("k")], limit=7, offset=1)
    got = ex.execute(q, result="columns")
    try:
        want = db.execute("SELECT COUNT(DISTINCT x), k, COUNT(DISTINCT x) FROM t GROUP BY k HAVING COUNT(DISTINCT x) >= 39 "
                          "ORDER BY 1 DESC, k LIMIT 7 OFFSET 1").fetchall()
        cols = got.to_columns()
        assert list(cols) == ["dx", "k", "again"] and len(want) == 7
        assert list(zip(*cols.values())) == [tuple(r) for r in want]
    finally:
        got.free()
    with pytest.raises(ValueError, match="columns"):
        ex.execute(dataclasses.replace(q, having=[], order_by=[], limit=None, offset=0))
    with pytest.raises(QueryMustRunOnCpu):
        ex.execute(dataclasses.replace(q, targets=q.targets + [Agg("avg", ColRef("v"))]), result="columns")


def test_select_distinct(gpu_executor_factory, storage, table):
    ex = gpu_executor_factory(storage)
    cols = ex.execute(QueryUnit("t", groupby=[ColRef("g"), ColRef("x")], targets=[KeyRef(0, "g"), KeyRef(1, "x"), Agg("count")]),
                      result="columns")
    try:
        d = cols.group_by([1], [("id", "x", None)])
        try:
            assert d.to_columns() == {"x": sorted(set(table["x"][table["x"] != NULL].tolist())) + [None]}  # NULLs last
        finally:
            d.free()
        ordered = cols.sort([OrderEntry("g")])
        try:
            pre = ordered.group_by(["g"], [("id", 0, "g"), ("count", None, "groups")], presorted=True)
            try:
                assert pre.to_columns() == {"g": [0, 1, 2, 3], "groups": [41, 41, 41, 41]}
            finally:
                pre.free()
        finally:
            ordered.free()
    finally:
        cols.free()


def test_a_regrouped_result_carries_its_schema(gpu_executor_factory, table):
    import pyarrow as pa
    n = 6_000
    st = ArrowStorage()
    st.import_arrow(pa.table({"s": pa.array([("a", "b", "c")[i % 3] for i in range(n)]).dictionary_encode(),
                              "k": pa.array(table["k"][:n]), "v": pa.array(table["v"][:n]), "f": pa.array(table["f"][:n])}), "t")
    ex = gpu_executor_factory(st)
    q = QueryUnit("t", groupby=[ColRef("s"), ColRef("k")],
                  targets=[KeyRef(0, "s"), KeyRef(1, "k"), Agg("count", None, "n"), Agg("sum", ColRef("f"), "sf"),
                           Agg("max", ColRef("v"), "mx")])
    cols = ex.execute(q, result="columns")
    try:
        # a plan-made result's schema is the plan's description, and it reads as the buffer does
        assert cols.columns() == describe_columns(cols.compiled) and cols.num_cols == 5
        plain = ex.execute(q)
        assert sorted(zip(*cols.to_columns().values())) == sorted(zip(*plain.to_columns().values()))
        assert cols.to_arrow().schema == plain.to_arrow().schema
        # ... whether or not a stage ran first: a pass-through select keeps every type, the 4-byte COUNT's included
        picked = ex.execute(dataclasses.replace(q, select=[Proj(TargetRef(c), c) for c in ("s", "k", "n", "sf", "mx")]),
                            result="columns")
        try:
            assert picked.to_arrow().schema == cols.to_arrow().schema
            assert str(picked.to_arrow().schema.field("n").type) == "int32"
        finally:
            picked.free()
        by_s = cols.group_by(["s"], [("id", "s", None), ("sum", "n", "rows"), ("max", "mx", None), ("sum", "sf", "total"),
                                     ("count", None, "keys"), ("max", "s", "last")])
        try:
            assert [d.name for d in by_s.columns()] == ["s", "rows", "max_2", "total", "keys", "last"]
            got = by_s.to_columns()
            assert sorted(got["s"]) == ["a", "b", "c"] and got["last"] == got["s"] and sum(got["rows"]) == n
            for s, rows, mx, total in zip(got["s"], got["rows"], got["max_2"], got["total"]):
                sel = np.arange(n) % 3 == "abc".index(s)
                assert rows == int(sel.sum()) and mx == int(table["v"][:n][sel].max())
                assert abs(total - float(table["f"][:n][sel].sum())) <= 1e-6 * total
            at = by_s.to_arrow()
            assert at.column_names == list(got) and at.num_rows == 3
            assert [str(t) for t in at.schema.types] == ["string", "int64", "int64", "double", "int64", "string"]
            assert at.column("rows").to_pylist() == got["rows"]
            # sort() and filter() read the schema the result carries
            top = by_s.sort([OrderEntry("rows", desc=True), OrderEntry("max_2")], limit=2)
            kept = by_s.filter([Cmp(TargetRef("rows"), ">=", Lit(n // 3)), Cmp(TargetRef("total"), ">", Lit(0.5))])
            try:
                assert top.schema == by_s.schema and top.num_rows == 2
                assert top.to_columns()["rows"] == sorted(got["rows"], reverse=True)[:2]
                assert kept.num_rows == 3 and kept.to_columns() == got
                with pytest.raises(QueryMustRunOnCpu):
                    by_s.sort([OrderEntry("s")])
                again = kept.group_by(["keys"], [("count", None, "n"), ("sum", "rows", None)], presorted=False)
                try:
                    assert sum(again.to_columns()["sum_1"]) == n
                finally:
                    again.free()
            finally:
                top.free()
                kept.free()
            with pytest.raises(ValueError):
                by_s.group_by(["s"], [("sum", "last", None)])
        finally:
            by_s.free()
    finally:
        cols.free()


def test_every_intermediate_block_is_freed(gpu_executor_factory, storage):
    ex = gpu_executor_factory(storage)
    q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("count_distinct", ColRef("x"), "dx"), Agg("count", None, "n")],
                  having=[Cmp(TargetRef("dx"), ">", Lit(30))], order_by=[OrderEntry("dx")], limit=50)
    ex.execute(q, result="columns").free()  # (the first run fills the executor's caches)
    mgr = ex.mgr
    live = set()
    alloc, free = mgr.allocateDeviceMem, mgr.freeDeviceMem

    def tracked_alloc(num_bytes, device_num):
        p = alloc(num_bytes, device_num)
        live.add(p)
        return p

    def tracked_free(ptr):
        live.discard(ptr)
        return free(ptr)

    mgr.allocateDeviceMem, mgr.freeDeviceMem = tracked_alloc, tracked_free
    try:
        got = ex.execute(q, result="columns")
        assert 0 < got.num_rows <= 50
        assert live == {got.block.ptr}
        cols = ex.execute(dataclasses.replace(q, having=[], order_by=[], limit=None), result="columns")
        rolled = cols.group_by(["dx"], [("id", "dx", None), ("count", None, "groups")])
        assert live == {got.block.ptr, cols.block.ptr, rolled.block.ptr}
        for c in (got, cols, rolled):
            c.free()
        assert not live
    finally:
        del mgr.allocateDeviceMem, mgr.freeDeviceMem
