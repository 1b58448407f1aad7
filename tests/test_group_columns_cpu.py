"""hdk_hip_group_columns without a device: the numpy expectation of the GPU tests (group_expect.py) against SQLite and the
rules SQLite cannot show, the host arithmetic and the argument checks of the C ABI, the resolution of
DeviceColumns.group_by's arguments, and the rewrite of a count_distinct unit into an inner unit and a regroup."""
import ctypes as C
import sqlite3

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import lib
from hdk_amd.ir import FP64, INT64, Agg, Cmp, ColRef, KeyRef, Lit, OrderEntry, QueryMustRunOnCpu, QueryUnit, TargetRef, Type
from hdk_amd.plan import (ColumnDesc, compile_query, describe_columns, has_count_distinct, regroup_columns,
                          resolve_having_columns, resolve_order_by, split_count_distinct)
from hdk_amd.storage import ArrowStorage

import group_expect as G
from group_expect import NULL_F64_BITS, NULL_I64, Out, bits

INT_NULLABLE = (False, True, NULL_I64)
FP_NULLABLE = (True, True, NULL_F64_BITS)


# ---- the evaluator against SQLite ------------------------------------------------------------------------------------
def _table(seed, n=400):
    """k1, k2 keys (k2 nullable), a nullable int column, a nullable real column of one sign; sorted by the keys.  Group
    k1 == 0 has no value in either column."""
    rng = np.random.default_rng(seed)
    k1 = rng.integers(0, 6, n).astype(np.int64)
    k2 = rng.integers(0, 4, n).astype(np.int64)
    k2[rng.random(n) < 0.2] = NULL_I64
    iv = rng.integers(-50, 50, n).astype(np.int64)
    iv[rng.random(n) < 0.3] = NULL_I64
    fv = rng.integers(1, 400, n) / 8.0
    fw = bits(fv).copy()
    fw[rng.random(n) < 0.3] = NULL_F64_BITS
    iv[k1 == 0] = NULL_I64
    fw[k1 == 0] = NULL_F64_BITS
    order = np.lexsort((k2, k1))  # (NULL_I64 sorts first: any order will do, equal keys only have to be adjacent)
    return [c[order] for c in (k1, k2, iv, fw)]


def _sqlite(cols):
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE t (k1 INTEGER, k2 INTEGER, iv INTEGER, fv REAL)")
    k1, k2, iv, fw = cols
    rows = [(int(a), None if b == NULL_I64 else int(b), None if c == NULL_I64 else int(c),
             None if d == NULL_F64_BITS else float(np.int64(d).view(np.float64))) for a, b, c, d in zip(k1, k2, iv, fw)]
    db.executemany("INSERT INTO t VALUES (?, ?, ?, ?)", rows)
    return db


def _unword(w, nullable, null_bits, is_fp):
    if nullable and w == null_bits:
        return None
    return float(np.int64(w).view(np.float64)) if is_fp else int(w)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("keys", [[0], [0, 1]])
def test_evaluator_agrees_with_sqlite(seed, keys):
    cols = _table(seed)
    outs = [Out("id", k, False, k == 1, NULL_I64) for k in keys]
    outs += [Out("count", -1), Out("count", 2, *INT_NULLABLE), Out("sum", 2, *INT_NULLABLE), Out("min", 2, *INT_NULLABLE),
             Out("max", 2, *INT_NULLABLE), Out("count", 3, *FP_NULLABLE), Out("sum", 3, *FP_NULLABLE), Out("min", 3, *FP_NULLABLE),
             Out("max", 3, *FP_NULLABLE)]
    got, runs = G.group(cols, len(cols[0]), keys, outs)
    names = ", ".join(f"k{k + 1}" for k in keys)
    sql = (f"SELECT {names}, COUNT(*), COUNT(iv), SUM(iv), MIN(iv), MAX(iv), COUNT(fv), SUM(fv), MIN(fv), MAX(fv) FROM t "
           f"GROUP BY {names}")
    want = {r[:len(keys)]: r[len(keys):] for r in _sqlite(cols).execute(sql)}
    assert runs == len(want)
    saw_all_null = False
    for r in range(runs):
        row = [_unword(got[j][r], o.nullable and o.kind != "count", o.null_bits, o.is_fp and o.kind != "count") for j, o in enumerate(outs)]
        w = want[tuple(row[:len(keys)])]
        for j, (a, b) in enumerate(zip(row[len(keys):], w)):
            if outs[len(keys) + j].kind == "sum" and outs[len(keys) + j].is_fp and a is not None:
                assert b is not None and abs(a - b) <= 1e-6 * abs(b)
            else:
                assert a == b, (r, j, a, b)
        saw_all_null = saw_all_null or (row[len(keys) + 2] is None and row[len(keys) + 1] == 0)
    assert saw_all_null  # SUM of a group without a value is NULL, its COUNT 0


@pytest.mark.parametrize("seed", [4, 5])
def test_count_distinct_as_two_group_bys(seed):
    """COUNT(DISTINCT x) GROUP BY k == GROUP BY k, x then GROUP BY k, COUNT(x): a NULL x is an inner group that is not counted"""
    k1, k2, iv, _ = _table(seed)
    order = np.lexsort((iv, k1))
    inner_cols = [k1[order], iv[order]]
    inner, _ = G.group(inner_cols, len(k1), [0, 1], [Out("id", 0), Out("id", 1), Out("count", -1), Out("count", 1, *INT_NULLABLE)])
    outer, runs = G.group(inner, len(inner[0]), [0], [Out("id", 0), Out("count", 1, *INT_NULLABLE), Out("sum", 2), Out("sum", 3)])
    want = _sqlite([k1, k2, iv, np.zeros_like(iv)]).execute(
        "SELECT k1, COUNT(DISTINCT iv), COUNT(*), COUNT(iv) FROM t GROUP BY k1 ORDER BY k1").fetchall()
    assert [tuple(int(c[r]) for c in outer) for r in range(runs)] == want
    assert want[0][1] == 0  # the group whose arguments are all NULL


# ---- the rules SQLite cannot show -------------------------------------------------------------------------------------
def test_int_sum_wraps():
    big = (1 << 62) + 1
    cols = [np.zeros(4, dtype=np.int64), np.array([big, big, big, NULL_I64], dtype=np.int64)]
    got, runs = G.group(cols, 4, [0], [Out("sum", 1, *INT_NULLABLE), Out("sum", 1)])
    assert runs == 1
    assert int(got[0][0]) == (3 * big + (1 << 63)) % (1 << 64) - (1 << 63)
    assert int(got[1][0]) == (3 * big + NULL_I64 + (1 << 63)) % (1 << 64) - (1 << 63)  # not nullable: the sentinel is a value


def test_signed_zeros_are_two_runs_and_null_keys_one():
    k = bits([0.0, 0.0, -0.0, -0.0, 0.0])
    got, runs = G.group([k], 5, [0], [Out("id", 0), Out("count", -1)])
    assert runs == 3 and got[1].tolist() == [2, 2, 1]
    k = np.array([NULL_I64, NULL_I64, 3], dtype=np.int64)
    assert G.group([k], 3, [0], [Out("count", -1)])[0][0].tolist() == [2, 1]


def test_a_column_that_cannot_be_null_holds_the_sentinel():
    cols = [np.zeros(3, dtype=np.int64), np.array([NULL_I64, 5, 7], dtype=np.int64)]
    got, _ = G.group(cols, 3, [0], [Out("count", 1), Out("min", 1), Out("count", 1, *INT_NULLABLE), Out("min", 1, *INT_NULLABLE)])
    assert [int(c[0]) for c in got] == [3, NULL_I64, 2, 5]
    allnull = [np.zeros(2, dtype=np.int64), np.full(2, NULL_I64, dtype=np.int64)]
    got, _ = G.group(allnull, 2, [0], [Out("sum", 1, *INT_NULLABLE), Out("max", 1, *INT_NULLABLE), Out("count", 1, *INT_NULLABLE)])
    assert [int(c[0]) for c in got] == [NULL_I64, NULL_I64, 0]


def test_unsorted_input_makes_every_run_a_row():
    k = np.array([1, 2, 1, 1], dtype=np.int64)
    got, runs = G.group([k], 4, [0], [Out("id", 0), Out("count", -1)])
    assert runs == 3 and got[0].tolist() == [1, 2, 1] and got[1].tolist() == [1, 1, 2]
    assert G.group([k], 0, [0], [Out("id", 0)])[1] == 0


# ---- the C ABI's host side -------------------------------------------------------------------------------------------
TILE = 4096
# section 2's needs: a 32-bit count per tile, and per out and tile an 8-byte partial and a 4-byte non-NULL count
WS_BYTES_PER_TILE = lambda outs: 4 + 12 * outs  # noqa: E731
WS_HEAD = lambda outs: WS_BYTES_PER_TILE(outs) + 4 + 3 * 256  # noqa: E731  (a partly filled last tile, the total, three regions rounded to 256 bytes)


def test_workspace_is_monotone_and_bounded():
    L = lib()
    for outs in (1, 2, 16):
        last = 0
        for n in [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 10 * TILE, 200_003, 1_100_003, 100_000_000, 2**32 - 1]:
            b = L.hdk_hip_group_columns_workspace_bytes(n, outs)
            assert b >= last and b % 8 == 0
            assert b <= (n / TILE) * WS_BYTES_PER_TILE(outs) + WS_HEAD(outs), (n, outs)
            assert b >= (n // TILE) * WS_BYTES_PER_TILE(outs)
            last = b
        assert L.hdk_hip_group_columns_workspace_bytes(10 * TILE, outs) >= L.hdk_hip_group_columns_workspace_bytes(10 * TILE, 1)


def _outs(*specs):
    arr = (A.GroupOut * max(len(specs), 1))()
    for i, (col, kind) in enumerate(specs):
        arr[i] = A.GroupOut(col, kind, 0, 0, 0, 0)
    return arr


def test_invalid_arguments_come_back_before_any_device():
    L = lib()
    ok_ptr = 4096  # (never dereferenced: every check comes first)
    key0 = (C.c_int32 * 8)(0, 1, 0, 0, 0, 0, 0, 0)

    def call(cols=ok_ptr, capacity=100, num_cols=2, num_rows=100, keys=key0, num_keys=1, outs=_outs((0, A.AGG_ID)), num_outs=1,
             out=1 << 30, out_capacity=100, row_count=8192, ws=None, ws_bytes=0):
        st = L.hdk_hip_group_columns(cols, capacity, num_cols, num_rows, keys, num_keys, outs, num_outs, out, out_capacity,
                                     row_count, ws, ws_bytes, 0, None)
        return st, (L.hdk_hip_last_error() or b"").decode()

    for kw in ({"cols": None}, {"keys": None}, {"outs": None}, {"row_count": None}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "NULL" in msg, kw
    for k in (0, 9, -1):
        st, msg = call(num_keys=k)
        assert st == A.ERR_INVALID_ARG and "num_keys" in msg
    for k in (0, 17, -1):
        st, msg = call(num_outs=k)
        assert st == A.ERR_INVALID_ARG and "num_outs" in msg
    for c in (-1, 2):
        st, msg = call(keys=(C.c_int32 * 1)(c))
        assert st == A.ERR_INVALID_ARG and "key" in msg and "column" in msg
    for kind in (A.AGG_SUM, A.AGG_MIN, A.AGG_MAX, A.AGG_ID):
        for c in (-1, 2):
            st, msg = call(outs=_outs((c, kind)))
            assert st == A.ERR_INVALID_ARG and "column" in msg, (kind, c)
    st, msg = call(outs=_outs((2, A.AGG_COUNT)))
    assert st == A.ERR_INVALID_ARG and "column" in msg
    st, msg = call(outs=_outs((1, A.AGG_ID)))  # column 1 is no key
    assert st == A.ERR_INVALID_ARG and "not a key" in msg
    for kind in (A.AGG_AVG, A.AGG_SINGLE_VALUE, 7, 200):
        st, msg = call(outs=_outs((0, kind)))
        assert st == A.ERR_INVALID_ARG and "kind" in msg
    st, msg = call(num_rows=101)
    assert st == A.ERR_INVALID_ARG and "capacity" in msg
    st, msg = call(num_rows=2**32, capacity=2**33)
    assert st == A.ERR_INVALID_ARG and "32-bit" in msg
    st, msg = call(out=ok_ptr + 8)
    assert st == A.ERR_INVALID_ARG and "overlap" in msg
    st, msg = call(out=ok_ptr - 8, out_capacity=2)
    assert st == A.ERR_INVALID_ARG and "overlap" in msg
    need = L.hdk_hip_group_columns_workspace_bytes(100, 1)
    st, msg = call(ws=1 << 20, ws_bytes=need - 1)
    assert st == A.ERR_INVALID_ARG and "workspace" in msg
    st, msg = call(ws=(1 << 20) + 4, ws_bytes=need)
    assert st == A.ERR_INVALID_ARG and "aligned" in msg
    # every pair of blocks: cols [4096, 5696), out_cols 800 bytes, row_count 8 bytes, the workspace `need` bytes
    for kw, names in (({"row_count": ok_ptr + 16}, ("row_count", "cols")), ({"row_count": (1 << 30) + 792}, ("row_count", "out_cols")),
                      ({"ws": ok_ptr + 1024, "ws_bytes": need}, ("workspace", "cols")),
                      ({"ws": (1 << 30) - 8, "ws_bytes": need}, ("workspace", "out_cols")),
                      ({"ws": 8192 - need + 8, "ws_bytes": need}, ("workspace", "row_count"))):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "overlap" in msg and all(x in msg for x in names), (kw, msg)


def test_the_struct_mirrors_the_header():
    assert C.sizeof(A.GroupOut) == lib().hdk_hip_sizeof_group_out() == 16
    assert A.MAX_GROUP_KEYS == 8 and A.MAX_GROUP_OUTS == 16


# ---- DeviceColumns.group_by's arguments ------------------------------------------------------------------------------
def _storage():
    import pyarrow as pa
    st = ArrowStorage()
    n = 120
    st.import_arrow(pa.table({
        "k": pa.array((np.arange(n) % 10).astype(np.int64)),
        "x": pa.array([None if i % 7 == 0 else i % 5 for i in range(n)], type=pa.int64()),
        "v": pa.array(np.arange(n, dtype=np.int64)),
        "f": pa.array(np.arange(n, dtype=np.float64)),
        "s": pa.array(["a", "b", "c"] * (n // 3)).dictionary_encode()}), "t")
    return st


def _describe(targets, groupby=("k", "s")):
    st = _storage()
    q = QueryUnit("t", groupby=[ColRef(c) for c in groupby], targets=targets)
    return describe_columns(compile_query(st, q))


def test_a_plan_describes_its_columns():
    d = _describe([KeyRef(0), KeyRef(1), Agg("count"), Agg("sum", ColRef("x"), "sx"), Agg("min", ColRef("f"), "mf")])
    assert [c.name for c in d] == ["k", "s", "count_2", "sx", "mf"] and [c.target_idx for c in d] == list(range(5))
    assert [c.kind for c in d] == ["key", "key", "agg", "agg", "agg"]
    assert d[1].dictionary is not None and d[0].dictionary is None
    assert (d[2].is_fp, d[2].nullable) == (False, False)
    assert (d[3].is_fp, d[3].nullable, d[3].null_bits) == (False, True, NULL_I64)
    assert (d[4].is_fp, d[4].null_bits) == (True, NULL_F64_BITS)


def test_regroup_resolves_keys_outs_types_and_names():
    d = _describe([KeyRef(0), KeyRef(1), Agg("count", None, "n"), Agg("sum", ColRef("x"), "sx"), Agg("min", ColRef("f"), "mf")])
    keys, spec, out = regroup_columns(d, ["k"], [("id", "k", None), ("sum", "n", "rows"), ("sum", 3, None), ("min", "mf", "mf"),
                                                   ("max", "s", "last_s"), ("count", None, None), ("count", "sx", "nx")])
    assert keys == [0]
    assert spec == [("id", 0), ("sum", 2), ("sum", 3), ("min", 4), ("max", 1), ("count", -1), ("count", 3)]
    assert [c.name for c in out] == ["k", "rows", "sum_2", "mf", "last_s", "count_5", "nx"]
    assert [c.target_idx for c in out] == list(range(7))
    assert out[0].kind == "key" and out[0].type == d[0].type
    assert (out[1].nullable, out[1].is_fp, out[1].type.size) == (False, False, 8)  # SUM of a COUNT: an int64 that is never NULL
    assert (out[2].nullable, out[2].null_bits) == (True, NULL_I64)
    assert (out[3].is_fp, out[3].nullable, out[3].null_bits) == (True, d[4].nullable, NULL_F64_BITS)
    assert out[4].dictionary is d[1].dictionary  # MAX of a string id stays a string id
    for c in (out[5], out[6]):
        assert (c.is_fp, c.nullable, c.type) == (False, False, Type("int", 8, False)) and c.agg == "count"
    # what sort() and filter() read of a regrouped result
    assert resolve_order_by(out, len(out), [OrderEntry("rows", True), OrderEntry(3)]) == [(1, True, False), (3, False, False)]
    with pytest.raises(QueryMustRunOnCpu):
        resolve_order_by(out, len(out), [OrderEntry("last_s")])
    hv = resolve_having_columns(out, [Cmp(TargetRef("rows"), ">", Lit(3)), Cmp(TargetRef("mf"), "<", Lit(2.5))])
    assert [(lf.lhs_col, lf.cmp_fp, lf.lhs_nullable) for lf in hv.leaves] == [(1, False, False), (3, True, True)]


def test_regroup_refuses_what_it_cannot_do():
    d = _describe([KeyRef(0), KeyRef(1), Agg("count", None, "n")])
    for keys, outs in (([], [("count", None, None)]), (["k"], []), (["nope"], [("count", None, None)]), ([3], [("count", None, None)]),
                       (["k"], [("id", "s", None)]), (["k"], [("sum", "s", None)]), (["k"], [("avg", "n", None)]),
                       (["k"], [("sum", None, None)]), (["k"], [("count", "nope", None)])):
        with pytest.raises(ValueError):
            regroup_columns(d, keys, outs)
    with pytest.raises(QueryMustRunOnCpu):
        regroup_columns(d, ["k"], [("count", None, None)] * 17)
    dec = [ColumnDesc("k", False, False, 0, INT64, 0, "key"),
           ColumnDesc("d", False, True, NULL_I64, Type("decimal", 8, True, 2), 1, "agg", "sum", None, 2)]
    out = regroup_columns(dec, [0], [("sum", "d", None), ("min", "d", None), ("count", "d", None)])[2]
    assert [c.scale for c in out] == [2, 2, 0] and out[0].type.kind == "decimal"  # SUM of a decimal keeps its scale


# ---- the rewrite of count_distinct -----------------------------------------------------------------------------------
def test_count_distinct_splits_into_an_inner_unit_and_a_regroup():
    q = QueryUnit("t", quals=[Cmp(ColRef("v"), ">", Lit(5))], groupby=[ColRef("k"), ColRef("s")],
                  targets=[Agg("count_distinct", ColRef("x"), "dx"), KeyRef(1), Agg("count"), Agg("sum", ColRef("v"), "sv"),
                           Agg("count_distinct", ColRef("x")), Agg("min", ColRef("f")), KeyRef(0, "key"), Agg("max", ColRef("v"))],
                  having=[Cmp(TargetRef("dx"), ">", Lit(1))], order_by=[OrderEntry("dx", True)], limit=3, offset=1)
    assert has_count_distinct(q)
    inner, rg = split_count_distinct(q)
    assert inner.table == "t" and inner.quals == q.quals and inner.joins == q.joins
    assert inner.groupby == [ColRef("k"), ColRef("s"), ColRef("x")]
    assert inner.targets[:3] == [KeyRef(0, "__key0"), KeyRef(1, "__key1"), KeyRef(2, "__distinct")]
    assert [(t.kind, t.arg) for t in inner.targets[3:]] == [("count", None), ("sum", ColRef("v")), ("min", ColRef("f")),
                                                            ("max", ColRef("v"))]
    assert not inner.having and not inner.order_by and inner.limit is None and inner.offset == 0
    assert rg.keys == [0, 1]
    assert rg.outs == [("count", 2, "dx"), ("id", 1, "s"), ("sum", 3, "count_2"), ("sum", 4, "sv"), ("count", 2, "count_distinct_4"),
                       ("min", 5, "min_5"), ("id", 0, "key"), ("max", 6, "max_7")]
    assert (rg.having, rg.order_by, rg.limit, rg.offset) == (q.having, q.order_by, 3, 1)
    # the inner unit is an ordinary plan, and its columns regroup under the unit's names in the unit's order
    cp = compile_query(_storage(), inner)
    _, _, out = regroup_columns(describe_columns(cp), rg.keys, rg.outs)
    assert [c.name for c in out] == ["dx", "s", "count_2", "sv", "count_distinct_4", "min_5", "key", "max_7"]
    assert (out[0].nullable, out[0].is_fp, out[0].agg) == (False, False, "count")
    assert out[1].dictionary is not None
    assert not has_count_distinct(inner)


def test_count_distinct_that_must_run_elsewhere():
    k, x, v = ColRef("k"), ColRef("x"), ColRef("v")
    for q, word in ((QueryUnit("t", groupby=[k], targets=[Agg("count_distinct", x), Agg("count_distinct", v)]), "different"),
                    (QueryUnit("t", groupby=[k], targets=[Agg("count_distinct", x), Agg("avg", v)]), "avg"),
                    (QueryUnit("t", groupby=[k], targets=[Agg("count_distinct", x), Agg("single_value", v)]), "single_value"),
                    (QueryUnit("t", targets=[Agg("count_distinct", x)]), "GROUP BY")):
        with pytest.raises(QueryMustRunOnCpu, match=word):
            split_count_distinct(q)
    q = QueryUnit("t", groupby=[k], targets=[KeyRef(0), Agg("count_distinct", x)])
    with pytest.raises(ValueError, match="split_count_distinct"):
        compile_query(_storage(), q)
    with pytest.raises(ValueError):
        split_count_distinct(QueryUnit("t", groupby=[k], targets=[Agg("count_distinct", None)]))
    # result="buffer" is refused before anything is prepared (no device is touched)
    from hdk_amd.executor import Executor
    ex = Executor.__new__(Executor)
    with pytest.raises(ValueError, match="columns"):
        Executor.execute(ex, q, result="buffer")
