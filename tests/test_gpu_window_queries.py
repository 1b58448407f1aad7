"""Window functions through the query path: QueryUnit.windows applied by Executor.execute(result="columns") after HAVING
and before ORDER BY / LIMIT, and DeviceColumns.window on its own.  Everything is compared with SQLite on the same data:
the GROUP BY as a common table expression, the window functions over it."""
import dataclasses
import sqlite3

import numpy as np
import pytest

from hdk_amd.ir import Agg, Cmp, ColRef, KeyRef, Lit, OrderEntry, QueryUnit, TargetRef, Window

pytestmark = pytest.mark.gpu

N = 6_000


def _columns():
    rng = np.random.default_rng(2032)
    k1 = rng.integers(0, 20, N).astype(np.int64)
    k2 = rng.integers(0, 15, N).astype(np.int64)  # 300 groups of about 20 rows
    v = rng.integers(0, 4, N).astype(np.int64)  # small: the groups' sums tie
    x = rng.integers(0, 12, N).astype(np.int64)
    f = rng.integers(1, 1000, N) / 4.0
    return {"k1": k1, "k2": k2, "v": v, "x": x, "f": f}


@pytest.fixture(scope="module")
def table():
    return _columns()


@pytest.fixture(scope="module")
def storage(table):
    from hdk_amd.storage import ArrowStorage
    st = ArrowStorage()
    st.import_numpy("t", table, fragment_size=2_500)
    return st


@pytest.fixture(scope="module")
def db(table):
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE t (k1 INTEGER, k2 INTEGER, v INTEGER, x INTEGER, f REAL)")
    con.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?)", list(zip(*[table[c].tolist() for c in ("k1", "k2", "v", "x", "f")])))
    return con


GROUPS = "WITH g AS (SELECT k1, k2, COUNT(*) AS n, SUM(v) AS s, SUM(f) AS sf, COUNT(DISTINCT x) AS dx FROM t GROUP BY k1, k2) "
TARGETS = [KeyRef(0, "k1"), KeyRef(1, "k2"), Agg("count", None, "n"), Agg("sum", ColRef("v"), "s"), Agg("sum", ColRef("f"), "sf")]
BY_K1 = ("k1",)


def _unit(windows, **kw):
    return QueryUnit("t", groupby=[ColRef("k1"), ColRef("k2")], targets=TARGETS, windows=windows, **kw)


def _rows(cols, names, ordered=False):
    rows = list(zip(*[cols[c] for c in names]))
    return rows if ordered else sorted(rows)


def _check(ex, db, q, names, sql, approx=(), ordered=False):
    got = ex.execute(q, result="columns")
    try:
        cols = got.to_columns()
        assert list(cols)[:-len(q.windows)] == [t.name for t in q.targets]  # the window columns come last
        want = [tuple(r) for r in db.execute(GROUPS + sql)]
        if not ordered:
            want.sort()
        rows = _rows(cols, names, ordered)
        assert len(rows) == len(want) > 0
        for a, b in zip(rows, want):
            for name, p, w in zip(names, a, b):
                if name in approx and p is not None and w is not None:
                    assert abs(p - w) <= 1e-6 * abs(w), (name, a, b)
                else:
                    assert p == w, (name, a, b)
        return cols
    finally:
        got.free()


def test_rank_over_a_group_by(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    by = (OrderEntry("s", desc=True),)
    q = _unit([Window("rank", partition_by=BY_K1, order_by=by, name="r"), Window("dense_rank", partition_by=BY_K1, order_by=by),
               Window("row_number", partition_by=BY_K1, order_by=by + (OrderEntry("k2"),), name="rn"),
               Window("cume_dist", partition_by=BY_K1, order_by=by, name="cd"),
               Window("percent_rank", partition_by=BY_K1, order_by=by, name="pr")])
    w = "OVER (PARTITION BY k1 ORDER BY s DESC)"
    cols = _check(ex, db, q, ["k1", "k2", "s", "r", "dense_rank_6", "cd", "pr", "rn"],
                  f"SELECT k1, k2, s, RANK() {w}, DENSE_RANK() {w}, CUME_DIST() {w}, PERCENT_RANK() {w}, "
                  "ROW_NUMBER() OVER (PARTITION BY k1 ORDER BY s DESC, k2) FROM g")
    assert max(cols["r"]) > max(cols["dense_rank_6"])  # the sums tie
    assert list(cols) == ["k1", "k2", "n", "s", "sf", "r", "dense_rank_6", "cd", "pr", "rn"]  # by specification, first appearance first


def test_running_sum_share_of_the_partition_and_lag(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    by = (OrderEntry("s", desc=True), OrderEntry("k2"))
    q = _unit([Window("sum", "n", BY_K1, by, frame="rows", name="running"), Window("sum", TargetRef("n"), BY_K1, by[:1], name="upto_peers"),
               Window("avg", "sf", BY_K1, by, name="avg_sf"), Window("lag", "s", BY_K1, by, name="before"),
               Window("lead", "k2", BY_K1, by, param=2, name="after"), Window("max", "sf", BY_K1, by, name="mx")])
    w = "OVER (PARTITION BY k1 ORDER BY s DESC, k2"
    rows = "ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW)"
    _check(ex, db, q, ["k1", "k2", "running", "avg_sf", "before", "after", "mx", "upto_peers"],
           f"SELECT k1, k2, SUM(n) {w} {rows}, AVG(sf) {w}), LAG(s) {w}), LEAD(k2, 2) {w}), MAX(sf) {w} {rows}, "
           "SUM(n) OVER (PARTITION BY k1 ORDER BY s DESC) FROM g", approx=("avg_sf",))
    # share of the partition total: SUM over the whole partition beside the row's own value
    q = _unit([Window("sum", "s", BY_K1, name="total"), Window("count", None, BY_K1, name="groups"), Window("sum", "sf", BY_K1, name="tf")])
    cols = _check(ex, db, q, ["k1", "k2", "s", "total", "groups", "tf"],
                  "SELECT k1, k2, s, SUM(s) OVER (PARTITION BY k1), COUNT(*) OVER (PARTITION BY k1), SUM(sf) OVER (PARTITION BY k1) FROM g",
                  approx=("tf",))
    for k in range(20):
        share = [s / t for s, t, k1 in zip(cols["s"], cols["total"], cols["k1"]) if k1 == k]
        assert abs(sum(share) - 1.0) < 1e-9 and len(share) == cols["groups"][cols["k1"].index(k)]


def test_having_then_a_window_then_order_by_the_window_column(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    q = _unit([Window("rank", partition_by=BY_K1, order_by=(OrderEntry("s", desc=True),), name="r")],
              having=[Cmp(TargetRef("n"), ">", Lit(18))], order_by=[OrderEntry("r"), OrderEntry("k1"), OrderEntry("k2")], limit=25, offset=3)
    cols = _check(ex, db, q, ["k1", "k2", "n", "r"],
                  "SELECT k1, k2, n, RANK() OVER (PARTITION BY k1 ORDER BY s DESC) AS r FROM g WHERE n > 18 ORDER BY r, k1, k2 "
                  "LIMIT 25 OFFSET 3", ordered=True)
    assert len(cols["r"]) == 25 and min(cols["n"]) > 18  # the ranks are those among the groups that passed


def test_two_window_specifications_in_one_query(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    q = _unit([Window("rank", partition_by=BY_K1, order_by=(OrderEntry("n"),), name="by_n"),
               Window("rank", partition_by=("k2",), order_by=(OrderEntry("s", desc=True),), name="by_s"),
               Window("count", None, BY_K1, (OrderEntry("n"),), name="upto"), Window("row_number", name="pos")],
              order_by=[OrderEntry("pos")])
    cols = _check(ex, db, q, ["k1", "k2", "by_n", "upto", "by_s"],
                  "SELECT k1, k2, RANK() OVER (PARTITION BY k1 ORDER BY n), COUNT(*) OVER (PARTITION BY k1 ORDER BY n), "
                  "RANK() OVER (PARTITION BY k2 ORDER BY s DESC) FROM g")
    assert cols["pos"] == list(range(1, 301))  # no partition keys, no order entries: one partition in the rows' order


def test_a_window_over_count_distinct(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    q = QueryUnit("t", groupby=[ColRef("k1"), ColRef("k2")],
                  targets=[KeyRef(0, "k1"), KeyRef(1, "k2"), Agg("count_distinct", ColRef("x"), "dx"), Agg("count", None, "n")],
                  having=[Cmp(TargetRef("n"), ">=", Lit(15))],
                  windows=[Window("rank", partition_by=BY_K1, order_by=(OrderEntry("dx", desc=True),), name="r"),
                           Window("sum", "dx", BY_K1, name="total")],
                  order_by=[OrderEntry("k1"), OrderEntry("r"), OrderEntry("k2")], limit=40)
    _check(ex, db, q, ["k1", "k2", "dx", "r", "total"],
           "SELECT k1, k2, dx, RANK() OVER (PARTITION BY k1 ORDER BY dx DESC) AS r, SUM(dx) OVER (PARTITION BY k1) FROM g "
           "WHERE n >= 15 ORDER BY k1, r, k2 LIMIT 40", ordered=True)


def test_window_on_columns_that_are_sorted_already(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    src = ex.execute(_unit([], order_by=[OrderEntry("k1"), OrderEntry("n"), OrderEntry("k2")]), result="columns")
    try:
        before = src.to_columns()
        outs = [Window("row_number", name="rn"), Window("rank"), Window("sum", "n", name="upto"), Window("first_value", "k2", name="first"),
                Window("last_value", "k2", frame="partition", name="last"), Window("ntile", param=4, name="quart")]
        got = src.window(["k1"], [OrderEntry("n")], outs, presorted=True)
        # sorted by the call itself; more outs than one library call takes
        again = src.window([TargetRef("k1")], [OrderEntry("n")], outs + [dataclasses.replace(o, name=None) for o in outs])
        try:
            assert src.block is not None and src.block.ptr and src.to_columns() == before  # the receiver stays valid
            cols = got.to_columns()
            assert [d.name for d in got.columns()] == ["k1", "k2", "n", "s", "sf", "rn", "rank_6", "upto", "first", "last", "quart"]
            assert {c: cols[c] for c in before} == before  # presorted: the rows as they were
            w = "OVER (PARTITION BY k1 ORDER BY n"
            want = db.execute(GROUPS + f"SELECT k1, k2, ROW_NUMBER() {w}, k2), RANK() {w}), SUM(n) {w}), FIRST_VALUE(k2) {w}, k2), "
                              f"LAST_VALUE(k2) {w}, k2 ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING) FROM g "
                              "ORDER BY k1, n, k2").fetchall()
            assert _rows(cols, ["k1", "k2", "rn", "rank_6", "upto", "first", "last"], ordered=True) == [tuple(r) for r in want]
            sizes = np.bincount(cols["k1"])
            assert cols["quart"] == [(rn - 1) // -(-int(sizes[k]) // 4) + 1 for rn, k in zip(cols["rn"], cols["k1"])]
            twice = again.to_columns()
            assert len(twice) == 5 + 12 and again.num_rows == 300
            for a, b in (("rank_6", "rank_12"), ("upto", "sum_13"), ("quart", "ntile_16")):
                assert sorted(zip(twice["k1"], twice["k2"], twice[a])) == sorted(zip(twice["k1"], twice["k2"], twice[b]))
            assert sorted(zip(twice["k1"], twice["k2"], twice["rank_6"])) == sorted(zip(cols["k1"], cols["k2"], cols["rank_6"]))
            # a windowed result carries its schema through sort() and filter()
            top = got.sort([OrderEntry("upto", desc=True)], limit=3)
            kept = got.filter([Cmp(TargetRef("rn"), "=", Lit(1))])
            try:
                assert top.to_columns()["upto"] == sorted(cols["upto"], reverse=True)[:3]
                assert kept.num_rows == 20 and kept.to_columns()["rank_6"] == [1] * 20
            finally:
                top.free()
                kept.free()
        finally:
            got.free()
            again.free()
        empty = src.filter([Cmp(TargetRef("n"), "<", Lit(0))])
        none = empty.window(["k1"], [], [Window("rank", name="r")])
        assert none.num_rows == 0 and [d.name for d in none.columns()][-1] == "r" and none.to_columns()["r"] == []
    finally:
        src.free()
    with pytest.raises(ValueError, match="freed"):
        src.window(["k1"], [], [Window("rank")])


def test_every_intermediate_block_is_freed(gpu_executor_factory, storage):
    ex = gpu_executor_factory(storage)
    q = _unit([Window("rank", partition_by=BY_K1, order_by=(OrderEntry("s"),), name="r"), Window("sum", "n", ("k2",), name="t")],
              having=[Cmp(TargetRef("n"), ">", Lit(10))], order_by=[OrderEntry("r")], limit=50)
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
        assert got.num_rows == 50 and live == {got.block.ptr}
        more = got.window([], [], [Window("row_number")])
        assert live == {got.block.ptr, more.block.ptr}
        got.free()
        more.free()
        assert not live
    finally:
        del mgr.allocateDeviceMem, mgr.freeDeviceMem


def test_windows_need_columns(gpu_executor_factory, storage):
    ex = gpu_executor_factory(storage)
    with pytest.raises(ValueError, match="windows"):
        ex.execute(_unit([Window("rank", partition_by=BY_K1)]))
    with pytest.raises(ValueError, match="windows"):
        ex.execute(dataclasses.replace(_unit([Window("rank")]), order_by=[]), result="buffer")
