"""Device projection through the query path: QueryUnit.select applied by Executor.execute(result="columns") after HAVING
and the windows and before ORDER BY / LIMIT, and DeviceColumns.project on its own.  Every projected word is compared with
tests/project_expect.py applied to the unprojected to_host() columns; whole queries also with SQLite on the same data."""
import dataclasses
import sqlite3

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import HdkHipError
from hdk_amd.ir import FP64, Agg, Case, Cast, Cmp, ColRef, IsNull, KeyRef, Lit, OrderEntry, Proj, QueryUnit, TargetRef, Window
from hdk_amd.plan import resolve_select_columns

import project_expect as PE

pytestmark = pytest.mark.gpu

N = 6_000


def _columns():
    rng = np.random.default_rng(2033)
    k1 = rng.integers(0, 20, N).astype(np.int64)
    k2 = rng.integers(0, 15, N).astype(np.int64)  # 300 groups of about 20 rows
    v = rng.integers(-50, 200, N).astype(np.int64)
    x = rng.integers(0, 12, N).astype(np.int32)
    x[rng.random(N) < 0.3] = A.NULL_INT
    x[k2 == 3] = A.NULL_INT  # whole groups without an x: COUNT(x) = 0, SUM(x) NULL
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
    x = [None if t == A.NULL_INT else t for t in table["x"].tolist()]
    con.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?)",
                    list(zip(table["k1"].tolist(), table["k2"].tolist(), table["v"].tolist(), x, table["f"].tolist())))
    return con


GROUPS = ("WITH g AS (SELECT k1, k2, COUNT(*) AS n, SUM(v) AS s, SUM(x) AS sx, COUNT(x) AS nx, SUM(f) AS sf, COUNT(DISTINCT x) AS dx "
          "FROM t GROUP BY k1, k2) ")
TARGETS = [KeyRef(0, "k1"), KeyRef(1, "k2"), Agg("count", None, "n"), Agg("sum", ColRef("v"), "s"), Agg("sum", ColRef("x"), "sx"),
           Agg("count", ColRef("x"), "nx"), Agg("sum", ColRef("f"), "sf")]
s, n, sx, nx, sf = (TargetRef(t) for t in ("s", "n", "sx", "nx", "sf"))
GUARDED = Case([(Cmp(nx, "=", Lit(0)), Lit(None))], sx / nx)


def _unit(**kw):
    return QueryUnit("t", groupby=[ColRef("k1"), ColRef("k2")], targets=TARGETS, **kw)


def _expected(base, select):
    """the select list over the DeviceColumns `base`, by the evaluator -> (int64 words per out, the error code)"""
    programs, _ = resolve_select_columns(base.columns(), select)
    cols = [np.ascontiguousarray(c).view(np.int64) for c in base.to_host()]
    ops, outs = [], []
    for p in programs:
        outs.append((len(ops), len(p.ops), p.is_fp, p.nullable, p.null_bits))
        ops += list(p.ops)
    words, _, err = PE.evaluate(cols, ops, outs)
    return words, err


def _words(cols):
    return [np.ascontiguousarray(c).view(np.int64) for c in cols.to_host()]


def _check_against_the_evaluator(ex, q):
    """q without its select list, projected by DeviceColumns.project: word for word what the evaluator gives; then q itself:
    the same rows.  -> the projected columns as python lists"""
    base = ex.execute(dataclasses.replace(q, select=[], order_by=[], limit=None, offset=0), result="columns")
    try:
        want, err = _expected(base, q.select)
        assert err == 0
        got = base.project(q.select)
        try:
            assert got.num_rows == base.num_rows > 0 and got.num_cols == len(q.select) and got.capacity == got.num_rows
            for j, (a, b) in enumerate(zip(_words(got), want)):
                assert np.array_equal(a, b), j
            assert base.to_host()[0].size == base.num_rows  # the source stays valid
        finally:
            got.free()
    finally:
        base.free()
    full = ex.execute(q, result="columns")
    try:
        assert [c.name for c in full.columns()] == [p.name for p in q.select]
        rows = list(zip(*[w.tolist() for w in _words(full)]))
        all_rows = list(zip(*[w.tolist() for w in want]))
        if q.limit is None:
            assert sorted(rows) == sorted(all_rows)
        else:
            assert len(rows) == q.limit and set(rows) <= set(all_rows)
        return full.to_columns()
    finally:
        full.free()


def _close(a, b):
    return (a is None and b is None) or (a is not None and b is not None and abs(a - b) <= 1e-9 * max(abs(a), abs(b), 1.0))


def test_ratio_guarded_ratio_and_share_of_the_partition(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    q = _unit(windows=[Window("sum", "s", ("k1",), name="tot")],
              select=[Proj(TargetRef("k1"), "k1"), Proj(TargetRef("k2"), "k2"), Proj(s / n, "mean"), Proj(Cast(s, FP64) / n, "fmean"),
                      Proj(GUARDED, "xmean"), Proj(Lit(100.0) * s / TargetRef("tot"), "share"), Proj(sf * 2 - n, "e"),
                      Proj(Case([(IsNull(sx), Lit(-1))], sx % 7), "m")])
    cols = _check_against_the_evaluator(ex, q)
    want = {(r[0], r[1]): r[2:] for r in db.execute(
        GROUPS + "SELECT k1, k2, s / n, CAST(s AS REAL) / n, CASE WHEN nx = 0 THEN NULL ELSE sx / nx END, "
        "100.0 * s / SUM(s) OVER (PARTITION BY k1), sf * 2 - n, CASE WHEN sx IS NULL THEN -1 ELSE sx % 7 END FROM g")}
    assert len(want) == len(cols["k1"]) == 300
    assert sum(v is None for v in cols["xmean"]) == 20  # the groups without an x: guarded, not raised
    for i, key in enumerate(zip(cols["k1"], cols["k2"])):
        w = want[key]
        assert (cols["mean"][i], cols["xmean"][i], cols["m"][i]) == (w[0], w[2], w[5]), key
        assert _close(cols["fmean"][i], w[1]) and _close(cols["share"][i], w[3]) and _close(cols["e"][i], w[4]), key


def test_order_by_a_computed_column_with_having(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    q = _unit(having=[Cmp(n, ">", Lit(15))],
              select=[Proj(TargetRef("k1"), "k1"), Proj(TargetRef("k2"), "k2"), Proj(Cast(s, FP64) / n, "ratio"), Proj(n, "n")],
              order_by=[OrderEntry("ratio", desc=True), OrderEntry("k1"), OrderEntry("k2")], limit=10)
    cols = _check_against_the_evaluator(ex, q)
    want = list(db.execute(GROUPS + "SELECT k1, k2, CAST(s AS REAL) / n AS ratio, n FROM g WHERE n > 15 "
                                    "ORDER BY ratio DESC, k1, k2 LIMIT 10"))
    assert list(zip(cols["k1"], cols["k2"], cols["n"])) == [(r[0], r[1], r[3]) for r in want]
    assert all(_close(a, r[2]) for a, r in zip(cols["ratio"], want)) and min(cols["n"]) > 15
    assert cols["ratio"] == sorted(cols["ratio"], reverse=True)


def test_select_on_a_count_distinct_unit(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    q = QueryUnit("t", groupby=[ColRef("k1"), ColRef("k2")],
                  targets=[KeyRef(0, "k1"), KeyRef(1, "k2"), Agg("count_distinct", ColRef("x"), "dx"), Agg("count", None, "n"),
                           Agg("sum", ColRef("v"), "s")],
                  select=[Proj(TargetRef("k1"), "k1"), Proj(TargetRef("k2"), "k2"),
                          Proj(Case([(Cmp(TargetRef("dx"), "=", Lit(0)), Lit(None))], s / TargetRef("dx")), "per"),
                          Proj(Cast(TargetRef("dx"), FP64) / n, "density")],
                  order_by=[OrderEntry("density", desc=True), OrderEntry("k1"), OrderEntry("k2")], limit=30)
    got = ex.execute(q, result="columns")
    try:
        cols = got.to_columns()
    finally:
        got.free()
    want = list(db.execute(GROUPS + "SELECT k1, k2, CASE WHEN dx = 0 THEN NULL ELSE s / dx END, CAST(dx AS REAL) / n AS density "
                                    "FROM g ORDER BY density DESC, k1, k2 LIMIT 30"))
    assert list(cols) == ["k1", "k2", "per", "density"]
    assert list(zip(cols["k1"], cols["k2"], cols["per"])) == [r[:3] for r in want]
    assert all(_close(a, r[3]) for a, r in zip(cols["density"], want))
    # the unprojected regrouped columns through the evaluator
    base = ex.execute(dataclasses.replace(q, select=[], order_by=[], limit=None), result="columns")
    try:
        words, err = _expected(base, q.select)
        proj = base.project(q.select)
        try:
            assert err == 0 and all(np.array_equal(a, b) for a, b in zip(_words(proj), words))
        finally:
            proj.free()
    finally:
        base.free()


def test_a_long_select_list_goes_through_several_calls(gpu_executor_factory, storage):
    ex = gpu_executor_factory(storage)
    select = [Proj(s * (j + 1) + n, f"e{j}") for j in range(11)] + [Proj(TargetRef("k2"), "k2")]
    base = ex.execute(_unit(), result="columns")
    try:
        words, err = _expected(base, select)
        got = base.project(select)
        try:
            assert got.num_cols == 12 and err == 0
            assert all(np.array_equal(a, b) for a, b in zip(_words(got), words))
        finally:
            got.free()
        empty = base.sort([], limit=0).project(select)
        assert empty.num_rows == 0 and [c.name for c in empty.columns()] == [p.name for p in select]
    finally:
        base.free()


def test_a_zero_count_without_a_guard_raises_and_leaks_nothing(gpu_executor_factory, storage):
    ex = gpu_executor_factory(storage)
    # (SUM(x) / COUNT(x) would not do: the sum of no value is NULL, and NULL / 0 is NULL)
    q = _unit(select=[Proj(TargetRef("k1"), "k1"), Proj(s / nx, "per_x")])
    ok = _unit(select=[Proj(TargetRef("k1"), "k1"), Proj(GUARDED, "xmean")])
    ex.execute(ok, result="columns").free()  # (the first run fills the executor's caches)
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
        with pytest.raises(HdkHipError) as e:
            ex.execute(q, result="columns")
        assert e.value.code == A.ERR_DIV_BY_ZERO
        assert not live
        got = ex.execute(ok, result="columns")
        assert live == {got.block.ptr}
        got.free()
        assert not live
    finally:
        del mgr.allocateDeviceMem, mgr.freeDeviceMem


def test_select_needs_columns(gpu_executor_factory, storage):
    ex = gpu_executor_factory(storage)
    q = _unit(select=[Proj(s / n, "mean")])
    with pytest.raises(ValueError, match="select"):
        ex.execute(q)
    with pytest.raises(ValueError, match="select"):
        ex.execute(q, result="buffer")
