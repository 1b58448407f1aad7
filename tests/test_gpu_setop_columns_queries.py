"""The device set operations through the query path: DeviceColumns.union / intersect / except_ of two GROUP BY results and
of a projection's columns (fp and dictionary columns presented through to_columns()), QueryUnit.result_setops followed by
ORDER BY ... LIMIT, and UNION ALL + group_by as the merge of two partial results.  The reference is SQLite over the same
data; the ALL forms, which SQLite lacks, are collections.Counter arithmetic over SQLite's rows of each side
(tests/setop_expect.counter_setop, which test_setop_columns_cpu.py checks against SQLite's ROW_NUMBER form)."""
import collections
import dataclasses
import sqlite3

import numpy as np
import pytest

from hdk_amd.ir import Agg, Cmp, ColRef, KeyRef, Lit, OrderEntry, Proj, QueryUnit, ResultSetOp, TargetRef

import setop_expect as E

pytestmark = pytest.mark.gpu

N = 30_000
WORDS = ["ash", "birch", "cedar", "elm", "fir"]
EVERY_OP = [("union", True), ("union", False), ("intersect", False), ("intersect", True), ("except", False), ("except", True)]


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(78)
    return {"k": rng.integers(0, 200, N).astype(np.int64), "g": rng.integers(0, 4, N).astype(np.int64),
            "v": rng.integers(-1000, 1000, N).astype(np.int64), "x": rng.integers(-4, 5, N) * 0.5,
            "s": rng.integers(0, len(WORDS), N)}


@pytest.fixture(scope="module")
def storage(table):
    import pyarrow as pa
    from hdk_amd.storage import ArrowStorage
    st = ArrowStorage()
    words = pa.array([WORDS[i] for i in table["s"]]).dictionary_encode()
    st.import_arrow(pa.table({"k": pa.array(table["k"]), "g": pa.array(table["g"]), "v": pa.array(table["v"]),
                              "x": pa.array(table["x"]), "s": words}), "t")
    return st


@pytest.fixture(scope="module")
def db(table):
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE t (k INTEGER, g INTEGER, v INTEGER, x REAL, s TEXT)")
    con.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?)",
                    zip(table["k"].tolist(), table["g"].tolist(), table["v"].tolist(), table["x"].tolist(), [WORDS[i] for i in table["s"]]))
    return con


def counts_unit(cond):
    """SELECT k, COUNT(*) n FROM t WHERE <cond> GROUP BY k"""
    return QueryUnit("t", quals=[cond], groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("count", None, "n")])


# the two ranges of k overlap in [80, 120): those groups are the same rows on both sides
LOW, HIGH = Cmp(ColRef("k"), "<", Lit(120)), Cmp(ColRef("k"), ">=", Lit(80))
LOW_SQL, HIGH_SQL = "SELECT k, COUNT(*) n FROM t WHERE k < 120 GROUP BY k", "SELECT k, COUNT(*) n FROM t WHERE k >= 80 GROUP BY k"


def rows_of(cols):
    c = cols.to_columns()
    return [tuple(r) for r in zip(*[c[x] for x in c])]


def check_setop(left, right, lrows, rrows, op, all, names):
    before = rows_of(left), rows_of(right)
    out = {"union": left.union, "intersect": left.intersect, "except": left.except_}[op](right, all=all)
    try:
        assert [d.name for d in out.columns()] == names and [d.target_idx for d in out.columns()] == list(range(len(names)))
        got = rows_of(out)
        want = E.counter_setop(collections.Counter(lrows), collections.Counter(rrows), op, all)
        assert collections.Counter(got) == want, (op, all)
        assert out.num_rows == sum(want.values())
        assert out.num_rows == 0 or (out.block is not None and out.capacity >= out.num_rows)
        if op == "union" and all:
            assert got == before[0] + before[1]  # the left rows, then the right rows, each in its order
        else:
            raw = list(zip(*[c.tolist() for c in out.to_host()]))  # (a dictionary column orders by its ids)
            assert raw == sorted(raw)  # ascending over all columns (no NULLs here)
    finally:
        out.free()
    assert (rows_of(left), rows_of(right)) == before, "an input changed"


@pytest.mark.parametrize("op,all", EVERY_OP)
def test_two_group_by_results(gpu_executor_factory, storage, db, op, all):
    ex = gpu_executor_factory(storage)
    low, high = ex.execute(counts_unit(LOW), result="columns"), ex.execute(counts_unit(HIGH), result="columns")
    try:
        lrows, rrows = db.execute(LOW_SQL).fetchall(), db.execute(HIGH_SQL).fetchall()
        check_setop(low, high, lrows, rrows, op, all, ["k", "n"])
        if not all and op != "union":  # SQLite's own word for it
            word = {"intersect": "INTERSECT", "except": "EXCEPT"}[op]
            want = db.execute(f"{LOW_SQL} {word} {HIGH_SQL}").fetchall()
            out = low.setop(high, op)
            try:
                assert sorted(rows_of(out)) == sorted(want) and 0 < len(want) < len(lrows)
            finally:
                out.free()
        # one column of each, where rows repeat: the ALL forms differ from the plain ones
        ln, hn = low.project([Proj(TargetRef("n"), "n")]), high.project([Proj(TargetRef("n"), "n")])
        try:
            check_setop(ln, hn, [r[1:] for r in lrows], [r[1:] for r in rrows], op, all, ["n"])
            # an empty side, either way round, and both
            none = ln.filter([Cmp(TargetRef("n"), "<", Lit(0))])
            try:
                assert none.num_rows == 0
                check_setop(ln, none, [r[1:] for r in lrows], [], op, all, ["n"])
                check_setop(none, hn, [], [r[1:] for r in rrows], op, all, ["n"])
                check_setop(none, none, [], [], op, all, ["n"])
            finally:
                none.free()
        finally:
            ln.free()
            hn.free()
    finally:
        low.free()
        high.free()


def test_a_projections_columns_with_fp_and_dictionary_columns(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    targets = [Proj(ColRef("g"), "g"), Proj(ColRef("x"), "x"), Proj(ColRef("s"), "s")]
    a = ex.execute(QueryUnit("t", quals=[Cmp(ColRef("v"), "<", Lit(-990))], targets=targets), result="columns")
    b = ex.execute(QueryUnit("t", quals=[Cmp(ColRef("v"), ">", Lit(985))], targets=targets), result="columns")
    try:
        arows = db.execute("SELECT g, x, s FROM t WHERE v < -990").fetchall()
        brows = db.execute("SELECT g, x, s FROM t WHERE v > 985").fetchall()
        assert a.columns()[1].is_fp and a.columns()[2].dictionary is not None
        for op, all in EVERY_OP:
            check_setop(a, b, arows, brows, op, all, ["g", "x", "s"])
        want = db.execute("SELECT g, x, s FROM t WHERE v < -990 INTERSECT SELECT g, x, s FROM t WHERE v > 985").fetchall()
        out = a.intersect(b)
        try:
            assert sorted(rows_of(out)) == sorted(want) and 0 < len(want) < len(set(arows))
        finally:
            out.free()
        # the same through the unit: a projection with result_setops, ordered afterwards
        q = QueryUnit("t", quals=[Cmp(ColRef("v"), "<", Lit(-990))], targets=targets, result_setops=[ResultSetOp(b, "except")],
                      order_by=[OrderEntry("x", desc=True), OrderEntry("g")])
        out = ex.execute(q, result="columns")
        try:
            want = db.execute("SELECT * FROM (SELECT g, x, s FROM t WHERE v < -990 EXCEPT SELECT g, x, s FROM t WHERE v > 985) "
                              "ORDER BY x DESC, g").fetchall()
            got = rows_of(out)
            # (the strings of equal (x, g) follow their dictionary ids, not the alphabet)
            assert [r[:2] for r in got] == [r[:2] for r in want] and sorted(got) == sorted(want) and len(want) > 7
        finally:
            out.free()
        assert b.block is not None and sorted(rows_of(b)) == sorted(brows)  # `right` is not consumed
        with pytest.raises(ValueError, match="floating-point"):
            a.union(a.project([Proj(TargetRef("x"), "x"), Proj(TargetRef("g"), "g"), Proj(TargetRef("s"), "s")]))
    finally:
        a.free()
        b.free()


def test_result_setops_then_order_by_and_limit(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)
    high = ex.execute(counts_unit(HIGH), result="columns")
    try:
        for op, word in (("union", "UNION"), ("intersect", "INTERSECT"), ("except", "EXCEPT")):
            q = dataclasses.replace(counts_unit(LOW), result_setops=[ResultSetOp(high, op)],
                                    order_by=[OrderEntry("n", desc=True), OrderEntry("k")], limit=12, offset=1)
            out = ex.execute(q, result="columns")
            try:
                want = db.execute(f"SELECT * FROM ({LOW_SQL} {word} {HIGH_SQL}) ORDER BY n DESC, k LIMIT 12 OFFSET 1").fetchall()
                assert rows_of(out) == want and len(want) == 12, op
            finally:
                out.free()
        assert high.block is not None and high.num_rows == 120  # `right` is not consumed
        # two in a row, HAVING below them: (low HAVING n > 150) UNION ALL high EXCEPT high = nothing of high's rows
        q = dataclasses.replace(counts_unit(LOW), having=[Cmp(TargetRef("n"), ">", Lit(150))],
                                result_setops=[ResultSetOp(high, "union", True), ResultSetOp(high, "except")], order_by=[OrderEntry("k")])
        out = ex.execute(q, result="columns")
        try:
            want = db.execute(f"SELECT * FROM (SELECT * FROM ({LOW_SQL}) WHERE n > 150 EXCEPT {HIGH_SQL}) ORDER BY k").fetchall()
            assert rows_of(out) == want and 0 < len(want) < 80
        finally:
            out.free()
        # a count_distinct unit hands them to its regroup step
        q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("count_distinct", ColRef("v"), "n")],
                      result_setops=[ResultSetOp(high, "union")], order_by=[OrderEntry("k"), OrderEntry("n")], limit=30)
        out = ex.execute(q, result="columns")
        try:
            want = db.execute(f"SELECT * FROM (SELECT k, COUNT(DISTINCT v) n FROM t GROUP BY k UNION {HIGH_SQL}) ORDER BY k, n LIMIT 30").fetchall()
            assert rows_of(out) == want
        finally:
            out.free()
        with pytest.raises(ValueError, match="columns"):
            ex.execute(dataclasses.replace(counts_unit(LOW), result_setops=[ResultSetOp(high, "union")]))  # result="buffer"
        with pytest.raises(ValueError, match="union, intersect or except"):
            ex.execute(dataclasses.replace(counts_unit(LOW), result_setops=[ResultSetOp(high, "minus")]), result="columns")
    finally:
        high.free()


def test_union_all_then_group_by_merges_two_partial_results(gpu_executor_factory, storage, db):
    ex = gpu_executor_factory(storage)

    def partial(cond):
        return QueryUnit("t", quals=[cond], groupby=[ColRef("k")],
                         targets=[KeyRef(0, "k"), Agg("count", None, "n"), Agg("sum", ColRef("v"), "sv"), Agg("min", ColRef("x"), "lo")])

    a = ex.execute(partial(Cmp(ColRef("g"), "<", Lit(2))), result="columns")
    b = ex.execute(partial(Cmp(ColRef("g"), ">=", Lit(2))), result="columns")
    try:
        both = a.union(b, all=True)
        try:
            assert both.num_rows == a.num_rows + b.num_rows and both.capacity == both.num_rows
            merged = both.group_by(["k"], [("id", "k", "k"), ("sum", "n", "n"), ("sum", "sv", "sv"), ("min", "lo", "lo")])
            try:
                want = db.execute("SELECT k, COUNT(*), SUM(v), MIN(x) FROM t GROUP BY k ORDER BY k").fetchall()
                assert rows_of(merged) == want and len(want) == 200
            finally:
                merged.free()
        finally:
            both.free()
    finally:
        a.free()
        b.free()
