"""Scanning a device result: Executor.register_columns and a QueryUnit whose table is a QueryUnit (a FROM-subquery), on the
device.  Every outer unit over the registered table is held to the same unit over a host table imported from the result's
host copy -- the path the oracle tests cover -- and to SQLite's answer to the whole nested statement."""
import dataclasses
import math
import sqlite3

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import storage as S
from hdk_amd._lib import HdkHipError
from hdk_amd.ir import (Agg, BinOp, Cmp, ColRef, JoinSpec, KeyRef, Lit, Or, OrderEntry, Proj, QueryMustRunOnCpu, QueryUnit,
                        TargetRef, Type)

import chunk_expect as E

pytestmark = pytest.mark.gpu

N, NG, FRAG = 9_000, 300, 128
WORDS = ["ant", "bee", "cat", "dog", "eel"]


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(416)
    g = rng.integers(0, NG, N).astype(np.int32)
    g[rng.random(N) < 0.03] = A.NULL_INT
    v = rng.integers(-500, 500, N).astype(np.int32)
    v[rng.random(N) < 0.1] = A.NULL_INT
    x = (rng.integers(-400, 400, N) / 4.0).astype(np.float32)
    x[rng.random(N) < 0.3] = np.array([A.NULL_FLOAT_BITS], dtype=np.int32).view(np.float32)[0]
    x[g % 50 == 7] = np.array([A.NULL_FLOAT_BITS], dtype=np.int32).view(np.float32)[0]  # whole groups without an x
    return {"g": g, "v": v, "x": x, "f": rng.integers(0, 21, N) / 2.0, "w": rng.integers(0, len(WORDS), N).astype(np.int32)}


@pytest.fixture(scope="module")
def dim():
    dk = np.arange(0, NG, 2, dtype=np.int32)  # every other key
    return {"dk": dk, "dval": (dk.astype(np.int64) * 3 - 100)}


@pytest.fixture()
def ex(gpu_executor_factory, table, dim):
    st = S.ArrowStorage()
    t = st.import_numpy("t", table, fragment_size=4_000, types={"w": Type("dict", 4, True)})
    t.columns["w"].dictionary = list(WORDS)
    st.import_numpy("dim", dim)
    ex = gpu_executor_factory(st)
    yield ex
    for name, tb in list(st.tables.items()):
        if isinstance(tb, S.DeviceTable):
            ex.drop_registered(name)
    ex.cache.clear()


def _opt(a, null):
    return [None if z else v for v, z in zip(a.tolist(), (a == null).tolist())]


@pytest.fixture(scope="module")
def db(table, dim):
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE t (g INTEGER, v INTEGER, x REAL, f REAL, w TEXT)")
    xnull = table["x"].view(np.int32) == A.NULL_FLOAT_BITS
    con.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?)",
                    zip(_opt(table["g"], A.NULL_INT), _opt(table["v"], A.NULL_INT),
                        [None if z else float(v) for v, z in zip(table["x"].tolist(), xnull.tolist())], table["f"].tolist(),
                        [WORDS[i] for i in table["w"]]))
    con.execute("CREATE TABLE dim (dk INTEGER, dval INTEGER)")
    con.executemany("INSERT INTO dim VALUES (?, ?)", zip(dim["dk"].tolist(), dim["dval"].tolist()))
    return con


G, V, X, F = ColRef("g"), ColRef("v"), ColRef("x"), ColRef("f")
INNER = QueryUnit("t", groupby=[G], targets=[KeyRef(0, "k"), Agg("sum", V, "s"), Agg("count", None, "c"), Agg("min", F, "mf"),
                                             Agg("max", X, "mx")])
INNER_SQL = "SELECT g AS k, SUM(v) AS s, COUNT(*) AS c, MIN(f) AS mf, MAX(x) AS mx FROM t GROUP BY g"
K, SS, CC, MF, MX = ColRef("k"), ColRef("s"), ColRef("c"), ColRef("mf"), ColRef("mx")


def outer_units(table):
    return {
        "perfect_mod": (QueryUnit(table, groupby=[BinOp("%", K, Lit(8))],
                                  targets=[KeyRef(0, "b"), Agg("sum", SS, "s"), Agg("count", None, "n"), Agg("min", MF, "lo"),
                                           Agg("max", MX, "hi")]),
                        "SELECT k % 8, SUM(s), COUNT(*), MIN(mf), MAX(mx) FROM ({inner}) GROUP BY k % 8"),
        "perfect_key": (QueryUnit(table, groupby=[K], targets=[KeyRef(0, "k"), Agg("sum", CC, "n"), Agg("max", MX, "hi")]),
                        "SELECT k, SUM(c), MAX(mx) FROM ({inner}) GROUP BY k"),
        "baseline_fp": (QueryUnit(table, groupby=[MF], targets=[KeyRef(0, "mf"), Agg("sum", CC, "n"), Agg("count", None, "g")]),
                        "SELECT mf, SUM(c), COUNT(*) FROM ({inner}) GROUP BY mf"),
        "filter_project": (QueryUnit(table, quals=[Or(Cmp(K, "<", Lit(5)), Cmp(SS, ">", Lit(900)))],
                                     targets=[Proj(K, "k"), Proj(SS, "s"), Proj(MX, "mx")]),
                           "SELECT k, s, mx FROM ({inner}) WHERE k < 5 OR s > 900"),
        "non_grouped": (QueryUnit(table, targets=[Agg("sum", SS, "s"), Agg("count", None, "n"), Agg("min", MF, "lo"),
                                                  Agg("max", MX, "hi"), Agg("avg", MF, "a"), Agg("count", K, "nk")]),
                        "SELECT SUM(s), COUNT(*), MIN(mf), MAX(mx), AVG(mf), COUNT(k) FROM ({inner})"),
        "join": (QueryUnit(table, joins=[JoinSpec("dim", K, "dk")], groupby=[K],
                           targets=[KeyRef(0, "k"), Agg("sum", BinOp("+", SS, ColRef("dval", "dim")), "sd")]),
                 "SELECT k, SUM(s + dval) FROM ({inner}) JOIN dim ON k = dk GROUP BY k"),
    }


def rows_of(columns):
    """{name: list} -> the rows as a sorted list of tuples (None first)"""
    rows = list(zip(*columns.values()))
    return sorted(rows, key=lambda r: tuple((v is not None, v if v is not None else 0) for v in r))


def same_rows(got, want):
    """bit-exact for integers and strings, 1e-6 relative for doubles (the project's rule)"""
    if len(got) != len(want):
        return False
    for a, b in zip(got, want):
        if len(a) != len(b):
            return False
        for p, q in zip(a, b):
            if isinstance(p, float) or isinstance(q, float):
                if p is None or q is None or not math.isclose(p, q, rel_tol=1e-6, abs_tol=1e-12):
                    return False
            elif p != q:
                return False
    return True


def run_rows(ex, q, result="buffer"):
    res = ex.execute(q, result=result)
    try:
        return rows_of(res.to_columns())
    finally:
        if result == "columns":
            res.free()


def host_twin(ex, cols, reg, name, fragment_size):
    """the registered table's values imported from the host copy of the columns: the sentinel rewrite stated by chunk_expect"""
    sel = [(j, d.is_fp, d.nullable, d.null_bits, reg.columns[d.name].type.null_value()) for j, d in enumerate(cols.schema)]
    words = E.copy([w.view(np.int64) for w in cols.to_host()], cols.num_rows, sel)
    types = {d.name: reg.columns[d.name].type for d in cols.schema}
    arrays = {d.name: (w.view(np.float64) if types[d.name].is_fp else w) for d, w in zip(cols.schema, words)}
    h = ex.storage.import_numpy(name, arrays, fragment_size=fragment_size, types=types)
    for d in cols.schema:
        h.columns[d.name].dictionary = d.dictionary
    return h


def test_round_trip_and_statistics(ex):
    cols = ex.execute(INNER, result="columns")
    try:
        assert cols.num_rows == NG + 1 and [d.name for d in cols.schema] == ["k", "s", "c", "mf", "mx"]
        assert cols.schema[0].null_bits == A.NULL_INT  # a 4-byte slot: the sentinel sign-extended
        before = [w.copy() for w in cols.to_host()]
        reg = ex.register_columns("r", cols, fragment_size=FRAG - 5)  # (rounded up to 128)
        assert isinstance(reg, S.DeviceTable) and ex.storage.get("r") is reg
        assert reg.fragment_rows == FRAG and reg.frag_rows == [128, 128, 45] and reg.num_rows == NG + 1
        assert [reg.columns[n].type for n in reg.column_order] == [Type("int", 8, True), Type("int", 8, True), Type("int", 8, False),
                                                                    Type("fp", 8, True), Type("fp", 8, True)]
        assert all(reg.device_chunk(n, f) % 256 == 0 for n in reg.column_order for f in range(3))
        for a, b in zip(before, cols.to_host()):
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), "the columns were modified"
        h = host_twin(ex, cols, reg, "h", FRAG)
        for n in reg.column_order:
            assert reg.columns[n].stats == h.columns[n].stats, n
            assert [type(s.min) for s in reg.columns[n].stats] == [type(s.min) for s in h.columns[n].stats], n
        assert reg.columns["k"].table_stats().has_nulls and reg.columns["mx"].table_stats().has_nulls
        star = QueryUnit("r", targets=[Proj(ColRef(n), n) for n in reg.column_order])
        assert same_rows(run_rows(ex, star), rows_of(cols.to_columns()))
        with pytest.raises(ValueError, match="already a table"):
            ex.register_columns("r", cols)
        with pytest.raises(QueryMustRunOnCpu, match="outer table"):
            ex.execute(QueryUnit("dim", joins=[JoinSpec("r", ColRef("dk"), "k")], targets=[Agg("sum", ColRef("s", "r"), "x")]))
    finally:
        cols.free()


def test_a_selection_and_a_dictionary_column(ex):
    inner = QueryUnit("t", groupby=[ColRef("w")], targets=[KeyRef(0, "w"), Agg("count", None, "c"), Agg("sum", V, "s")])
    cols = ex.execute(inner, result="columns")
    try:
        reg = ex.register_columns("r", cols, columns=["c", 0])
        assert reg.column_order == ["c", "w"] and reg.columns["w"].type == Type("dict", 8, True)
        got = run_rows(ex, QueryUnit("r", targets=[Proj(ColRef("c"), "c"), Proj(ColRef("w"), "w")]))
        full = cols.to_columns()
        assert got == rows_of({"c": full["c"], "w": full["w"]}) and {r[1] for r in got} == set(WORDS)
        # the ids still group, and come back as strings
        again = run_rows(ex, QueryUnit("r", groupby=[ColRef("w")], targets=[KeyRef(0, "w"), Agg("sum", ColRef("c"), "n")]))
        assert again == rows_of({"w": full["w"], "n": full["c"]})
    finally:
        cols.free()


@pytest.mark.parametrize("unit", ["perfect_mod", "perfect_key", "baseline_fp", "filter_project", "non_grouped", "join"])
def test_outer_units_over_the_registered_table(ex, db, unit):
    cols = ex.execute(INNER, result="columns")
    try:
        reg = ex.register_columns("r", cols, fragment_size=FRAG)
        host_twin(ex, cols, reg, "h", FRAG)
    finally:
        cols.free()
    q_dev, sql = outer_units("r")[unit]
    q_host, _ = outer_units("h")[unit]
    a, b = ex.prepare(q_dev), ex.prepare(q_host)
    try:
        assert a.kernel_names() == b.kernel_names()  # the same fast kernels on both paths
        assert bytes(a.cp.plan) == bytes(b.cp.plan)
    finally:
        a.free()
        b.free()
    got, twin = run_rows(ex, q_dev), run_rows(ex, q_host)
    assert same_rows(got, twin), (got[:3], twin[:3])
    want = sorted(db.execute(sql.format(inner=INNER_SQL)).fetchall(),
                  key=lambda r: tuple((v is not None, v if v is not None else 0) for v in r))
    assert same_rows(got, want), (got[:3], want[:3])
    # and as one nested unit
    nested, _ = outer_units(INNER)[unit]
    assert same_rows(run_rows(ex, nested), want)
    assert sorted(ex.storage.tables) == ["dim", "h", "r", "t"]


def test_nested_units(ex, db):
    level1 = QueryUnit("t", groupby=[G, ColRef("w")], targets=[KeyRef(0, "g"), KeyRef(1, "w"), Agg("sum", V, "s"), Agg("count", None, "c")])
    level2 = QueryUnit(level1, groupby=[ColRef("g")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("s"), "s"), Agg("sum", ColRef("c"), "c")],
                       having=[Cmp(TargetRef("c"), ">", Lit(25))], order_by=[OrderEntry("s", desc=True), OrderEntry("k")], limit=40)
    level3 = QueryUnit(level2, targets=[Agg("sum", ColRef("s"), "s"), Agg("count", None, "n"), Agg("min", ColRef("k"), "lo"),
                                        Agg("sum", ColRef("c"), "c")])
    sql = ("SELECT SUM(s), COUNT(*), MIN(k), SUM(c) FROM (SELECT g AS k, SUM(s) AS s, SUM(c) AS c FROM "
           "(SELECT g, w, SUM(v) AS s, COUNT(*) AS c FROM t GROUP BY g, w) GROUP BY g HAVING SUM(c) > 25 "
           "ORDER BY s DESC, k LIMIT 40)")
    want = db.execute(sql).fetchall()
    assert want[0][1] == 40
    assert same_rows(run_rows(ex, level3), want)
    assert same_rows(run_rows(ex, level3, result="columns"), want)
    # the outer's own stages over a grouped outer unit
    outer = QueryUnit(level2, groupby=[BinOp("/", ColRef("k"), Lit(100))], targets=[KeyRef(0, "b"), Agg("sum", ColRef("c"), "c")],
                      order_by=[OrderEntry("b")])
    res = ex.execute(outer, result="columns")
    try:
        got = list(zip(*res.to_columns().values()))
    finally:
        res.free()
    assert got == db.execute("SELECT k / 100, SUM(c) FROM (SELECT g AS k, SUM(c) AS c, SUM(s) AS s FROM (SELECT g, w, SUM(v) AS s, "
                             "COUNT(*) AS c FROM t GROUP BY g, w) GROUP BY g HAVING SUM(c) > 25 ORDER BY s DESC, k LIMIT 40) "
                             "GROUP BY k / 100 ORDER BY 1").fetchall()
    assert sorted(ex.storage.tables) == ["dim", "t"]
    with pytest.raises(ValueError, match="execute"):
        ex.compile(level3)


def test_an_inner_result_of_no_rows(ex):
    inner = dataclasses.replace(INNER, quals=[Cmp(V, ">", Lit(10**6))])
    q = QueryUnit(inner, targets=[Agg("count", None, "n"), Agg("sum", ColRef("s"), "s")])
    assert run_rows(ex, q) == [(0, None)]
    assert sorted(ex.storage.tables) == ["dim", "t"]


def test_a_raising_outer_step_leaves_nothing_behind(ex):
    inner = dataclasses.replace(INNER, targets=INNER.targets + [Agg("sum", BinOp("-", V, V), "z")])  # z: 0, or NULL
    ok = QueryUnit(inner, targets=[Agg("sum", BinOp("/", SS, CC), "q")])
    run_rows(ex, ok)  # (whatever the first use of the tables uploads is there before the level is taken)
    level = ex.cache.nbytes()
    bad = QueryUnit(inner, targets=[Agg("sum", BinOp("/", SS, ColRef("z")), "q")])
    with pytest.raises(HdkHipError) as e:
        ex.execute(bad)
    assert e.value.code == A.ERR_DIV_BY_ZERO == 1
    assert sorted(ex.storage.tables) == ["dim", "t"] and ex.cache.nbytes() == level
    assert run_rows(ex, ok)  # and the executor still works


def test_lifecycle(ex):
    first = ex.execute(INNER, result="columns")
    second = ex.execute(dataclasses.replace(INNER, quals=[Cmp(G, "<", Lit(10))]), result="columns")
    try:
        q = QueryUnit("r", targets=[Agg("count", None, "n"), Agg("sum", ColRef("c"), "c")])
        ex.register_columns("r", first)
        assert run_rows(ex, q) == [(NG + 1, N)]
        ex.drop_registered("r")
        assert "r" not in ex.storage.tables
        reg = ex.register_columns("r", second)  # the same name, other data: nothing stale is served
        want = int(np.count_nonzero((first.to_host()[0] >= 0) & (first.to_host()[0] < 10)))
        assert want == 10 and run_rows(ex, q)[0][0] == want
        ex.drop_registered("r")
        ex.cache.clear()  # (the cache never owned the block: nothing is freed twice)
        ex.cache.clear()
        assert reg.block is None
        with pytest.raises(ValueError, match="not a registered result"):
            ex.drop_registered("r")
        assert first.num_rows == NG + 1 and first.to_host()[2].sum() == N  # the columns outlive their tables
    finally:
        first.free()
        second.free()
