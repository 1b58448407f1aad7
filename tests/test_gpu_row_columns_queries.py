"""Dense device columns of projections and non-grouped results through the executor: PreparedStep.fetch_columns against
fetch() of the same launch, and Executor.execute(result="columns") with the stages that a projection could not reach
before -- ORDER BY / LIMIT, windows, select, result_joins, DeviceColumns.group_by -- against SQLite on the same data and the
numpy evaluators of the window and projection stages."""
import dataclasses
import sqlite3

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd.ir import (Agg, Case, Cmp, ColRef, JoinSpec, KeyRef, Lit, OrderEntry, Proj, QueryMustRunOnCpu, QueryUnit, ResultJoin,
                        TargetRef, Type, Window)
from hdk_amd.plan import resolve_select_columns

import project_expect as PE
import window_expect as WE

pytestmark = pytest.mark.gpu

N = 20_000
ND = 300
WORDS = ["ash", "birch", "cedar", "elm", "fir"]


def _columns():
    rng = np.random.default_rng(2034)
    g = rng.integers(0, 7, N).astype(np.int64)
    g[rng.random(N) < 0.05] = A.NULL_BIGINT
    v = rng.integers(-500, 500, N).astype(np.int32)
    v[rng.random(N) < 0.1] = A.NULL_INT
    return {"rid": np.arange(N, dtype=np.int64), "g": g, "v": v, "k": rng.integers(0, ND, N).astype(np.int64),
            "w": rng.integers(0, len(WORDS), N).astype(np.int32), "d": rng.integers(-1000, 1000, N) / 8.0,
            "s": rng.integers(-100, 100, N).astype(np.int16)}


@pytest.fixture(scope="module")
def table():
    return _columns()


@pytest.fixture(scope="module")
def dim():
    rng = np.random.default_rng(7)
    return {"key": rng.permutation(ND).astype(np.int64), "x": rng.integers(0, 100, ND).astype(np.int64)}


@pytest.fixture(scope="module")
def storage(table, dim):
    from hdk_amd.storage import ArrowStorage
    st = ArrowStorage()
    t = st.import_numpy("t", table, fragment_size=7_000, types={"w": Type("dict", 4, True), "rid": Type("int", 8, False)})
    t.columns["w"].dictionary = list(WORDS)
    assert t.num_fragments == 3
    st.import_numpy("dim", dim)
    return st


def _opt(a, null):
    return [None if x == null else x for x in a.tolist()]


@pytest.fixture(scope="module")
def db(table, dim):
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE t (rid INTEGER, g INTEGER, v INTEGER, k INTEGER, w TEXT, d REAL, s INTEGER)")
    con.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?, ?, ?)",
                    zip(table["rid"].tolist(), _opt(table["g"], A.NULL_BIGINT), _opt(table["v"], A.NULL_INT), table["k"].tolist(),
                        [WORDS[i] for i in table["w"]], table["d"].tolist(), table["s"].tolist()))
    con.execute("CREATE TABLE dim (key INTEGER, x INTEGER)")
    con.executemany("INSERT INTO dim VALUES (?, ?)", zip(dim["key"].tolist(), dim["x"].tolist()))
    return con


WHERE = [Cmp(ColRef("v"), ">", Lit(100))]  # about 36 % of the rows; a NULL v does not pass
TARGETS = [Proj(ColRef("rid"), "rid"), Proj(ColRef("g"), "g"), Proj(ColRef("v"), "v"), Proj(ColRef("w"), "w"), Proj(ColRef("d"), "d"),
           Proj(ColRef("s"), "s")]
NAMES = [t.name for t in TARGETS]
PASSING = "SELECT rid, g, v, w, d, s FROM t WHERE v > 100"


def _unit(**kw):
    return QueryUnit("t", quals=WHERE, targets=TARGETS, **kw)


def _rows(cols, names=None):
    c = cols if isinstance(cols, dict) else cols.to_columns()
    return [tuple(r) for r in zip(*[c[x] for x in (names or list(c))])]


def _words(cols):
    return [np.ascontiguousarray(c).view(np.int64) for c in cols.to_host()]


def _key(row):
    return tuple((x is None, x) for x in row)


# ---- fetch_columns against fetch() of the same launch -------------------------------------------------------------------------
FORMS = {"plain": {}, "sparse": {"HDK_HIP_PROJECT_WRITER": "sparse"}, "dense": {"HDK_HIP_PROJECT_WRITER": "dense"}, "join": {}}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
def test_fetch_columns_is_the_fetched_buffer_row_by_row(gpu_executor_factory, storage, monkeypatch, columnar, form):
    for name, value in FORMS[form].items():
        monkeypatch.setenv(name, value)
    q = _unit(output_columnar=columnar)
    if form == "join":
        q = dataclasses.replace(q, joins=[JoinSpec("dim", ColRef("k"), "key")], targets=TARGETS + [Proj(ColRef("x", "dim"), "x")])
    ex = gpu_executor_factory(storage)
    step = ex.prepare(q)
    try:
        assert "hdk_scan_project" in step.kernel_names()
        step.enqueue()
        cols = step.fetch_columns(positions=True)
        plain = step.fetch_columns()
        res = step.fetch()
    finally:
        step.free()
    try:
        cp, total = step.cp, res.total_matched
        assert cols.error_code == res.error_code == 0
        assert cols.num_rows == plain.num_rows == total == res.row_count() > 5000
        pos, want = rs.projection_arrays(cp, res.buffer, total)
        got = _words(cols)
        assert len(got) == len(want) + 1 and cols.columns()[-1].name == "__pos"
        for t, (a, b) in enumerate(zip(got, want + [pos])):
            assert np.array_equal(a, b), t
        assert len(set(got[0].tolist())) == total  # rid: every row once
        assert plain.to_columns() == res.to_columns()
        assert plain.to_arrow().schema == res.to_arrow().schema and plain.to_arrow().equals(res.to_arrow())
        assert [d.name for d in plain.columns()] == [t.name for t in q.targets]
    finally:
        cols.free()
        plain.free()


def test_fetch_columns_of_a_non_grouped_step(gpu_executor_factory, storage, db):
    q = QueryUnit("t", quals=WHERE, targets=[Agg("count", None, "n"), Agg("sum", ColRef("v"), "s"), Agg("avg", ColRef("d"), "m"),
                                             Agg("min", ColRef("s"), "lo"), Agg("count", ColRef("g"), "ng")])
    ex = gpu_executor_factory(storage)
    step = ex.prepare(q)
    try:
        step.enqueue()
        cols = step.fetch_columns()
        res = step.fetch()
        with pytest.raises(ValueError, match="positions"):
            step.fetch_columns(positions=True)
    finally:
        step.free()
    try:
        assert cols.num_rows == cols.capacity == 1
        assert [w.tolist() for w in _words(cols)] == [w.tolist() for w in rs.rows_to_dense(step.cp, res.buffer)]
        assert cols.to_columns() == res.to_columns()
        assert cols.to_arrow().schema == res.to_arrow().schema
        n, s, m, lo, ng = db.execute("SELECT COUNT(*), SUM(v), AVG(d), MIN(s), COUNT(g) FROM t WHERE v > 100").fetchone()
        got = cols.to_columns()
        assert (got["n"], got["s"], got["lo"], got["ng"]) == ([n], [s], [lo], [ng]) and abs(got["m"][0] - m) <= 1e-9 * abs(m)
    finally:
        cols.free()


# ---- the stages above a projection ------------------------------------------------------------------------------------------------
def test_order_by_limit_offset(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    q = _unit(order_by=[OrderEntry("v", desc=True), OrderEntry("rid")], limit=10, offset=3)
    out = ex.execute(q, result="columns")
    try:
        want = db.execute(PASSING + " ORDER BY v DESC, rid LIMIT 10 OFFSET 3").fetchall()
        assert _rows(out, NAMES) == [tuple(r) for r in want] and out.num_rows == 10
    finally:
        out.free()
    with pytest.raises(QueryMustRunOnCpu, match="dictionary"):  # id order is not string order
        ex.execute(_unit(order_by=[OrderEntry("w")]), result="columns")
    with pytest.raises(ValueError, match="columns"):
        ex.execute(q)


def test_a_window_and_a_guarded_division_over_projected_rows(gpu_executor_factory, storage):
    ex = gpu_executor_factory(storage)
    base = ex.execute(_unit(), result="columns")
    try:
        windows = [Window("row_number", partition_by=["g"], order_by=[OrderEntry("v"), OrderEntry("rid")], name="rn")]
        out = ex.execute(_unit(windows=windows), result="columns")
        try:
            assert [d.name for d in out.columns()] == NAMES + ["rn"] and out.num_rows == base.num_rows
            words = _words(out)
            ig, iv, irid = NAMES.index("g"), NAMES.index("v"), NAMES.index("rid")
            want = WE.window(words[:-1], out.num_rows, [ig], [iv, irid], [WE.WOut("row_number")])[0]
            assert np.array_equal(words[-1], want) and want.max() > 100
            assert sorted(_rows(out, NAMES), key=_key) == sorted(_rows(base), key=_key)  # every projected row once
            # partitions ascend with the NULL partition last, rows inside by v, rid
            g = [r[ig] for r in _rows(out, NAMES)]
            assert g == sorted(g, key=lambda x: (x is None, x)) and g[-1] is None
        finally:
            out.free()
        v, s = TargetRef("v"), TargetRef("s")
        select = [Proj(TargetRef("rid"), "rid"), Proj(Case([(Cmp(s, "=", Lit(0)), Lit(None))], v / s), "ratio"), Proj(TargetRef("d") * Lit(2.0), "dd")]
        programs, _ = resolve_select_columns(base.columns(), select)
        ops, outs = [], []
        for p in programs:
            outs.append((len(ops), len(p.ops), p.is_fp, p.nullable, p.null_bits))
            ops += list(p.ops)
        want, _, err = PE.evaluate(_words(base), ops, outs)
        out = ex.execute(_unit(select=select), result="columns")
        try:
            assert err == 0 and [d.name for d in out.columns()] == ["rid", "ratio", "dd"]
            for j, (a, b) in enumerate(zip(_words(out), want)):
                assert np.array_equal(a, b), j
            assert any(x is None for x in out.to_columns()["ratio"])
        finally:
            out.free()
    finally:
        base.free()


def test_a_group_by_result_semi_joined_against_a_filtered_projection(gpu_executor_factory, storage, db):
    """SELECT k, COUNT(*), SUM(v) FROM t GROUP BY k HAVING k IN (SELECT key FROM dim WHERE x < 30)"""
    ex = gpu_executor_factory(storage)
    keys = ex.execute(QueryUnit("dim", quals=[Cmp(ColRef("x"), "<", Lit(30))], targets=[Proj(ColRef("key"), "k")]), result="columns")
    try:
        assert 0 < keys.num_rows < ND
        q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("count", None, "n"), Agg("sum", ColRef("v"), "sv")],
                      result_joins=[ResultJoin(keys, ["k"], type="semi")], order_by=[OrderEntry("k")])
        out = ex.execute(q, result="columns")
        try:
            want = db.execute("SELECT k, COUNT(*), SUM(v) FROM t WHERE k IN (SELECT key FROM dim WHERE x < 30) GROUP BY k ORDER BY k").fetchall()
            assert _rows(out) == [tuple(r) for r in want] and len(want) == keys.num_rows
        finally:
            out.free()
        # and a projection as the LEFT side of a result join, under a sort
        q = _unit(result_joins=[ResultJoin(keys, ["rid"], ["k"], type="semi")], order_by=[OrderEntry("rid")])
        out = ex.execute(q, result="columns")
        try:
            want = db.execute(PASSING + " AND rid IN (SELECT key FROM dim WHERE x < 30) ORDER BY rid").fetchall()
            assert _rows(out, NAMES) == [tuple(r) for r in want] and want
        finally:
            out.free()
        assert keys.block is not None  # `right` is not consumed
    finally:
        keys.free()


def test_distinct_over_a_projection(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    cols = ex.execute(_unit(), result="columns")
    try:
        out = cols.group_by(["g"], [("id", "g", "g"), ("count", None, "n"), ("max", "v", "hi")])
        try:
            want = db.execute("SELECT g, COUNT(*), MAX(v) FROM t WHERE v > 100 GROUP BY g").fetchall()
            assert sorted(_rows(out), key=_key) == sorted((tuple(r) for r in want), key=_key) and len(want) == 8
        finally:
            out.free()
    finally:
        cols.free()


def test_limit_without_order_by_stops_the_scan(gpu_executor_factory, storage, table):
    ex = gpu_executor_factory(storage)
    for columnar in (False, True):
        out = ex.execute(_unit(limit=25, offset=5, output_columnar=columnar), result="columns")
        try:
            assert out.num_rows == 25 and out.error_code <= 0
            assert out.compiled.plan.entry_count == 30  # the buffer is sized by the limit
            rows = _rows(out, NAMES)
            assert len({r[0] for r in rows}) == 25
            for rid, g, v, w, d, s in rows:
                assert v > 100 and v == table["v"][rid] and w == WORDS[table["w"][rid]] and d == table["d"][rid] and s == table["s"][rid]
        finally:
            out.free()
    out = ex.execute(_unit(limit=0), result="columns")
    assert out.num_rows == 0
    out.free()


def test_a_select_over_a_non_grouped_unit(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    q = QueryUnit("t", quals=WHERE, targets=[Agg("sum", ColRef("v"), "s"), Agg("count", None, "n")],
                  select=[Proj(TargetRef("s") / TargetRef("n"), "mean"), Proj(TargetRef("n"), "n")])
    out = ex.execute(q, result="columns")
    try:
        want = db.execute("SELECT SUM(v) / COUNT(*), COUNT(*) FROM t WHERE v > 100").fetchall()
        assert _rows(out) == [tuple(r) for r in want]
    finally:
        out.free()


# ---- sizing and ownership -----------------------------------------------------------------------------------------------------
def test_fetch_columns_counts_first_above_the_threshold(gpu_executor_factory, storage, monkeypatch):
    from hdk_amd.executor import PreparedStep
    ex = gpu_executor_factory(storage)
    for columnar in (False, True):
        step = ex.prepare(_unit(output_columnar=columnar))
        try:
            step.enqueue()
            one = step.fetch_columns(positions=True)
            assert one.capacity == step.cp.entry_count == N > one.num_rows
            one_call = PreparedStep.COLUMNS_ONE_CALL_BYTES
            monkeypatch.setattr(PreparedStep, "COLUMNS_ONE_CALL_BYTES", 1024)
            two = step.fetch_columns(positions=True)
            monkeypatch.setattr(PreparedStep, "COLUMNS_ONE_CALL_BYTES", one_call)
            assert two.capacity == two.num_rows == one.num_rows
            assert all(np.array_equal(a, b) for a, b in zip(_words(one), _words(two)))
            assert two.to_columns() == one.to_columns()
            one.free()
            two.free()
        finally:
            step.free()


def test_every_block_is_handed_back(gpu_executor_factory, storage):
    ex = gpu_executor_factory(storage)
    q = _unit(windows=[Window("row_number", partition_by=["g"], order_by=[OrderEntry("rid")], name="rn")],
              select=[Proj(TargetRef("rid"), "rid"), Proj(TargetRef("rn"), "rn")], order_by=[OrderEntry("rn"), OrderEntry("rid")], limit=50)
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
        assert live == {got.block.ptr} and got.num_rows == 50
        got.free()
        assert not live
        got = ex.execute(QueryUnit("t", targets=[Agg("sum", ColRef("v"), "s"), Agg("count", None, "n")],
                                   select=[Proj(TargetRef("s") / TargetRef("n"), "mean")]), result="columns")
        assert live == {got.block.ptr}
        got.free()
        with pytest.raises(QueryMustRunOnCpu):
            ex.execute(_unit(order_by=[OrderEntry("w")]), result="columns")  # the sort refuses: the projected block goes back
        assert not live
    finally:
        del mgr.allocateDeviceMem, mgr.freeDeviceMem
