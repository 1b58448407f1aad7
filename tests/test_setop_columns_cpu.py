"""The host side of the device set operations over dense result columns (hdk_hip_concat_columns, hdk_hip_setop_columns,
DeviceColumns.union / intersect / except_): the numpy evaluator of their contracts (tests/setop_expect.py) against SQLite
and against collections.Counter, the C ABI's argument checks, which come back before any device is touched, the
workspace arithmetic, plan.resolve_setop_columns -- the schema rule -- and the refusals of a unit that carries
result_setops.  No GPU."""
import collections
import ctypes as C
import dataclasses
import sqlite3

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import lib
from hdk_amd.ir import QueryMustRunOnCpu, Type
from hdk_amd.plan import SETOP_CODES, ColumnDesc, resolve_setop_columns

import setop_expect as E
from setop_expect import NULL_I32, NULL_I64

EVERY_OP = [("union", True), ("union", False), ("intersect", False), ("intersect", True), ("except", False), ("except", True)]


def make_case(seed, nc, ln, rn):
    """few distinct values, so that duplicates on both sides, rows on one side only and NULLs all occur; the left NULL is
    INT32_MIN sign-extended and the right one INT64_MIN, the output's INT64_MIN"""
    rng = np.random.default_rng(seed)
    lcols = [rng.integers(0, 4, ln).astype(np.int64) for _ in range(nc)]
    rcols = [rng.integers(1, 5, rn).astype(np.int64) for _ in range(nc)]
    for j in range(nc):
        lcols[j][rng.random(ln) < 0.2] = NULL_I32
        rcols[j][rng.random(rn) < 0.2] = NULL_I64
    pairs = [(j, j, True, True, int(NULL_I32), int(NULL_I64), int(NULL_I64)) for j in range(nc)]
    return lcols, rcols, pairs


def sqlite_rows(lcols, ln, rcols, rn, nc, op, all):
    db = sqlite3.connect(":memory:")
    names = ", ".join(f"c{j}" for j in range(nc))
    for t in ("l", "r"):
        db.execute(f"CREATE TABLE {t} ({', '.join(f'c{j} INTEGER' for j in range(nc))})")
    val = lambda v, null: None if v == null else int(v)  # noqa: E731
    marks = ", ".join("?" * nc)
    db.executemany(f"INSERT INTO l VALUES ({marks})", [tuple(val(lcols[j][i], NULL_I32) for j in range(nc)) for i in range(ln)])
    db.executemany(f"INSERT INTO r VALUES ({marks})", [tuple(val(rcols[j][i], NULL_I64) for j in range(nc)) for i in range(rn)])
    word = {"union": "UNION", "intersect": "INTERSECT", "except": "EXCEPT"}[op]
    if op == "union":
        sql = f"SELECT {names} FROM l UNION {'ALL ' if all else ''}SELECT {names} FROM r"
    elif not all:
        sql = f"SELECT {names} FROM l {word} SELECT {names} FROM r"
    else:
        # SQLite has no INTERSECT ALL / EXCEPT ALL: number the copies of a row on each side and drop the number
        num = f"SELECT {names}, ROW_NUMBER() OVER (PARTITION BY {names}) AS rn FROM"
        sql = f"SELECT {names} FROM ({num} l {word} {num} r)"
    return collections.Counter(db.execute(sql).fetchall())


@pytest.mark.parametrize("op,all", EVERY_OP)
@pytest.mark.parametrize("nc,ln,rn", [(1, 60, 45), (2, 70, 50), (1, 0, 30), (2, 40, 0), (1, 0, 0)])
def test_the_evaluator_against_sqlite_and_counter(op, all, nc, ln, rn):
    for seed in range(4):
        lcols, rcols, pairs = make_case(100 * seed + nc, nc, ln, rn)
        got = E.method(lcols, ln, rcols, rn, pairs, [False] * nc, op, all)
        assert len(got) == nc
        rows = E.multiset(got, [NULL_I64] * nc)
        assert rows == sqlite_rows(lcols, ln, rcols, rn, nc, op, all), (seed, op, all)
        want = E.counter_setop(E.multiset(lcols, [NULL_I32] * nc), E.multiset(rcols, [NULL_I64] * nc), op, all)
        assert rows == want
        if not (op == "union" and all) and len(got[0]):
            # the rows ascend in the sort's order, NULLs last
            order = [(j, False, False, False, True, int(NULL_I64)) for j in range(nc)]
            assert np.array_equal(E.S.expected_perm(got, order), np.arange(len(got[0])))


def test_the_keep_rule_on_one_run_for_every_l_and_r():
    """a run of r right rows followed by l left rows between two other runs: UNION 1, INTERSECT min(1, l, r), INTERSECT ALL
    min(l, r), EXCEPT l > 0 and r == 0, EXCEPT ALL max(l - r, 0)"""
    for r in range(4):
        for l in range(4):
            if l + r == 0:
                continue
            key = np.array([1] + [5] * (r + l) + [9], dtype=np.int64)
            tag = np.array([1] + [7] * r + [0] * l + [0], dtype=np.int64)  # (any non-zero word marks a right row)
            n = len(key)
            inside = slice(1, 1 + r + l)
            want = {E.UNION: 1, E.INTERSECT: int(l > 0 and r > 0), E.INTERSECT_ALL: min(l, r), E.EXCEPT: int(l > 0 and r == 0),
                    E.EXCEPT_ALL: max(l - r, 0)}
            for op, count in want.items():
                m = E.keep([key, tag], n, [0], 1, op)
                assert int(m[inside].sum()) == count, (op, l, r)


def test_concat_translates_each_sides_null_and_tags_the_sides():
    l = [np.array([1, int(NULL_I32), 3], dtype=np.int64)]
    r = [np.array([int(NULL_I64), int(NULL_I32)], dtype=np.int64)]
    out = E.concat(l, 3, r, 2, [(0, 0, True, True, int(NULL_I32), int(NULL_I64), -5)], 1)
    assert out[0].tolist() == [1, -5, 3, -5, int(NULL_I32)] and out[1].tolist() == [0, 0, 0, 1, 1]
    out = E.concat(l, 3, r, 2, [(0, 0, False, True, int(NULL_I32), int(NULL_I64), -5)], 0, True)
    assert out[1].tolist() == [1, int(NULL_I32), 3, -5, int(NULL_I32)] and out[0].tolist() == [1, 1, 1, 0, 0]


# ---- the C ABI: argument errors before any device, workspace arithmetic -------------------------------------------------
def _pairs(*specs):
    arr = (A.SetopCol * max(len(specs), 1))()
    for i, (lc, rc) in enumerate(specs):
        arr[i] = A.SetopCol(lc, rc, 1, 1, (C.c_uint8 * 6)(), A.NULL_BIGINT, A.NULL_BIGINT, A.NULL_BIGINT)
    return arr


def _idx(*cols):
    return (C.c_int32 * max(len(cols), 1))(*cols)


def test_concat_invalid_arguments_come_back_before_any_device():
    L = lib()
    # (never dereferenced: every check comes first) left [4096, 5696), right [1 << 20, + 2400), out 3 x 200 words at 1 << 30
    def call(lcols=4096, lcap=100, lnc=2, ln=100, rcols=1 << 20, rcap=100, rnc=3, rn=100, pairs=_pairs((0, 0), (1, 2)), nc=2,
             side=2, flags=0, out=1 << 30, ocap=200, device=0):
        st = L.hdk_hip_concat_columns(lcols, lcap, lnc, ln, rcols, rcap, rnc, rn, pairs, nc, side, flags, out, ocap, device, None)
        return st, (L.hdk_hip_last_error() or b"").decode()

    for kw in ({"lcols": None}, {"rcols": None}, {"pairs": None}, {"out": None}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "NULL" in msg, kw
    for kw in ({"lnc": 0}, {"rnc": 0}, {"nc": 0}, {"nc": 9}, {"nc": -1}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "num_cols" in msg, kw
    for spec, side in (((-1, 0), "left"), ((2, 0), "left"), ((0, -1), "right"), ((0, 3), "right")):
        st, msg = call(pairs=_pairs(spec, (0, 0)))
        assert st == A.ERR_INVALID_ARG and "pair 0" in msg and side in msg, spec
    st, msg = call(side=3)
    assert st == A.ERR_INVALID_ARG and "side_col" in msg
    for flags in (2, 3, 0x80000000):
        st, msg = call(flags=flags)
        assert st == A.ERR_INVALID_ARG and "flags" in msg
    for kw in ({"ln": 2**32, "lcap": 2**33}, {"rn": 2**32, "rcap": 2**33},
               {"ln": 2**31, "lcap": 2**31, "rn": 2**31, "rcap": 2**31, "ocap": 2**33}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "32-bit" in msg, kw
    for kw in ({"ln": 101}, {"rn": 101}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "capacit" in msg, kw
    st, msg = call(ocap=199)
    assert st == A.ERR_INVALID_ARG and "out_capacity" in msg
    for kw, name in (({"out": 4096 + 8}, "lcols"), ({"out": (1 << 20) + 2392}, "rcols")):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "overlap" in msg and name in msg, (kw, msg)
    # the inputs are only read and may be one block; a side without rows has no bytes and its columns may be NULL.  Such calls
    # pass every check of their arguments, so they are given a device that does not exist: where there is a device, a call
    # with these made-up addresses must never get as far as a launch
    for kw in ({"rcols": 4096, "rnc": 2, "pairs": _pairs((0, 0), (1, 1))}, {"lcols": None, "ln": 0, "ocap": 100},
               {"rcols": None, "rn": 0, "side": -1}, {"lcols": None, "ln": 0, "rcols": None, "rn": 0, "ocap": 0}):
        st, msg = call(device=-1, **kw)
        assert st == A.ERR_INVALID_ARG and msg == "device -1 out of range", (kw, msg)


def test_setop_invalid_arguments_come_back_before_any_device():
    L = lib()
    # (never dereferenced) cols 3 x 100 words at 4096, out 2 x 100 words at 1 << 30, row_count at 8192
    def call(cols=4096, cap=100, nc=3, n=100, keys=_idx(0, 1), nkeys=2, tag=2, op=A.SETOP_UNION, outs=_idx(0, 1), nouts=2,
             out=1 << 30, ocap=100, row_count=8192, ws=None, ws_bytes=0, device=0):
        st = L.hdk_hip_setop_columns(cols, cap, nc, n, keys, nkeys, tag, op, outs, nouts, out, ocap, row_count, ws, ws_bytes,
                                     device, None)
        return st, (L.hdk_hip_last_error() or b"").decode()

    for kw in ({"cols": None}, {"keys": None}, {"outs": None}, {"row_count": None}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "NULL" in msg, kw
    st, msg = call(nc=0)
    assert st == A.ERR_INVALID_ARG and "num_cols" in msg
    for k in (0, 9, -1):
        st, msg = call(nkeys=k)
        assert st == A.ERR_INVALID_ARG and "num_keys" in msg
    for k in (0, 17, -1):
        st, msg = call(nouts=k)
        assert st == A.ERR_INVALID_ARG and "num_outs" in msg
    for op in (-1, 5, 100):
        st, msg = call(op=op)
        assert st == A.ERR_INVALID_ARG and "op" in msg
    for tag in (-1, 3):
        st, msg = call(tag=tag)
        assert st == A.ERR_INVALID_ARG and "tag_col" in msg
    for tag in (0, 1):
        st, msg = call(tag=tag)
        assert st == A.ERR_INVALID_ARG and "tag column" in msg
    for keys in (_idx(-1, 0), _idx(0, 3)):
        st, msg = call(keys=keys)
        assert st == A.ERR_INVALID_ARG and "key" in msg
    for outs in (_idx(-1, 0), _idx(0, 3)):
        st, msg = call(outs=outs)
        assert st == A.ERR_INVALID_ARG and "out" in msg
    st, msg = call(n=2**32, cap=2**33)
    assert st == A.ERR_INVALID_ARG and "32-bit" in msg
    st, msg = call(n=101)
    assert st == A.ERR_INVALID_ARG and "capacity" in msg
    need = L.hdk_hip_setop_columns_workspace_bytes(100)
    st, msg = call(ws=1 << 24, ws_bytes=need - 1)
    assert st == A.ERR_INVALID_ARG and "workspace" in msg
    st, msg = call(ws=(1 << 24) + 4, ws_bytes=need)
    assert st == A.ERR_INVALID_ARG and "aligned" in msg
    for kw, names in (({"out": 4096 + 8}, ("out_cols", "cols")), ({"row_count": 4096 + 16}, ("row_count", "cols")),
                      ({"row_count": (1 << 30) + 800}, ("row_count", "out_cols")),
                      ({"ws": 4096 + 1024, "ws_bytes": need}, ("workspace", "cols")),
                      ({"ws": 8192 - need + 8, "ws_bytes": need}, ("workspace", "row_count"))):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "overlap" in msg and all(x in msg for x in names), (kw, msg)
    # the tag and a subset of the keys are valid outs, and the out_cols of a count-only call has no bytes and overlaps nothing
    for kw in ({"outs": _idx(2, 1), "device": -1}, {"outs": _idx(1), "nouts": 1, "device": -1}, {"out": 4096, "ocap": 0, "device": -1},
               {"out": None, "device": -1}, {"n": 0, "ws": 1 << 24, "ws_bytes": 512, "device": -1}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and msg == "device -1 out of range", (kw, msg)


def test_workspace_arithmetic():
    L = lib()
    align = lambda x: (x + 255) & ~255  # noqa: E731
    for n in (0, 1, 4096, 4097, 10**6, 2**32 - 1):
        tiles = (n + 4095) // 4096
        want = 2 * align(4 * (tiles + 1)) + align(8 * tiles) + align(4 * tiles) + 512 * tiles
        assert L.hdk_hip_setop_columns_workspace_bytes(n) == want, n
    # one bit per row and 20 bytes per tile, plus at most 1.5 KiB
    n = 100_000_000
    assert L.hdk_hip_setop_columns_workspace_bytes(n) <= n // 8 + 512 + 20 * (n // 4096 + 1) + 1536


def test_the_struct_and_constants_mirror_the_header():
    L = lib()
    assert C.sizeof(A.SetopCol) == L.hdk_hip_sizeof_setop_col() == 40
    assert A.MAX_SETOP_COLUMNS == 8 and A.MAX_SETOP_OUTS == 16 and A.CONCAT_TAG_FIRST == 1
    assert (A.SETOP_UNION, A.SETOP_INTERSECT, A.SETOP_INTERSECT_ALL, A.SETOP_EXCEPT, A.SETOP_EXCEPT_ALL) == (0, 1, 2, 3, 4)
    assert (E.UNION, E.INTERSECT, E.INTERSECT_ALL, E.EXCEPT, E.EXCEPT_ALL) == (0, 1, 2, 3, 4)
    assert SETOP_CODES == {k: v for k, v in E.OPS.items()}
    from hdk_amd import _lib
    assert {"hdk_hip_concat_columns", "hdk_hip_setop_columns", "hdk_hip_setop_columns_workspace_bytes"} <= set(_lib.SIGNATURES)


# ---- plan.resolve_setop_columns: the schema rule ------------------------------------------------------------------------
INT = Type("int", 8, True)
INT_NN = Type("int", 8, False)
FP = Type("fp", 8, True)
FP_NN = Type("fp", 8, False)
DICT = Type("dict", 4, True)
WORDS, OTHER_WORDS = ["a", "b"], ["b", "a"]


def desc(name, type=INT, idx=0, dictionary=None, scale=0, null=None, kind="key"):
    if null is None:
        null = A.NULL_DOUBLE_BITS if type.is_fp else A.NULL_BIGINT
    return ColumnDesc(name, type.is_fp, type.nullable, null if type.nullable else 0, type, idx, kind, "", dictionary, scale)


def test_resolve_setop_columns_pairs_by_position_and_presents_like_the_left():
    left = [desc("k", INT, 0), desc("x", FP, 1), desc("s", DICT, 2, WORDS), desc("d", Type("decimal", 8, True, 2), 3, scale=2)]
    right = [desc("a", INT, 0, kind="proj"), desc("b", FP, 1), desc("c", DICT, 2, list(WORDS)),
             desc("e", Type("decimal", 8, True, 2), 3, scale=2)]
    pairs, descs = resolve_setop_columns(left, right)
    assert [(p[0], p[1]) for p in pairs] == [(0, 0), (1, 1), (2, 2), (3, 3)]
    assert [d.name for d in descs] == ["k", "x", "s", "d"] and [d.target_idx for d in descs] == [0, 1, 2, 3]
    assert descs[2].dictionary is WORDS and descs[3].scale == 2 and descs[0].kind == "key" and descs[1].is_fp
    assert all(d.nullable and A.to_i64(d.null_bits) == A.to_i64(l.null_bits) for d, l in zip(descs, left))
    assert all(p[6] == A.to_i64(l.null_bits) for p, l in zip(pairs, left))


def test_resolve_setop_columns_chooses_the_sentinel():
    i32 = A.to_i64(A.NULL_INT)
    # both nullable, the same sentinel: the left's
    pairs, descs = resolve_setop_columns([desc("k", INT, null=i32)], [desc("k", INT, null=i32)])
    assert pairs[0] == (0, 0, True, True, i32, i32, i32) and descs[0].null_bits == i32 and descs[0].nullable
    # both nullable, different sentinels: the 8-byte type's
    pairs, descs = resolve_setop_columns([desc("k", INT, null=i32)], [desc("k", INT)])
    assert pairs[0] == (0, 0, True, True, i32, A.NULL_BIGINT, A.NULL_BIGINT) and descs[0].null_bits == A.NULL_BIGINT
    pairs, descs = resolve_setop_columns([desc("x", FP, null=77)], [desc("x", FP)])
    assert pairs[0][6] == A.NULL_DOUBLE_BITS and descs[0].null_bits == A.NULL_DOUBLE_BITS and descs[0].is_fp
    # only the left is nullable: the left's
    pairs, descs = resolve_setop_columns([desc("k", INT, null=i32)], [desc("k", INT_NN)])
    assert pairs[0] == (0, 0, True, False, i32, 0, i32) and descs[0].nullable and descs[0].null_bits == i32
    # only the right is nullable: the 8-byte type's, and the output becomes nullable
    pairs, descs = resolve_setop_columns([desc("k", INT_NN)], [desc("k", INT, null=i32)])
    assert pairs[0] == (0, 0, False, True, 0, i32, A.NULL_BIGINT)
    assert descs[0].nullable and descs[0].type.nullable and descs[0].null_bits == A.NULL_BIGINT
    pairs, descs = resolve_setop_columns([desc("x", FP_NN)], [desc("x", FP)])
    assert pairs[0][6] == A.NULL_DOUBLE_BITS and descs[0].nullable
    # neither
    pairs, descs = resolve_setop_columns([desc("k", INT_NN)], [desc("k", INT_NN)])
    assert not descs[0].nullable and not pairs[0][2] and not pairs[0][3]


def test_resolve_setop_columns_errors():
    k, x = desc("k", INT), desc("x", FP)
    with pytest.raises(ValueError, match="number of columns"):
        resolve_setop_columns([k, x], [k])
    with pytest.raises(ValueError, match="number of columns"):
        resolve_setop_columns([], [])
    with pytest.raises(ValueError, match="floating-point"):
        resolve_setop_columns([k], [x])
    with pytest.raises(ValueError, match="floating-point"):
        resolve_setop_columns([x], [k])
    with pytest.raises(ValueError, match="scale"):
        resolve_setop_columns([desc("d", Type("decimal", 8, True, 2), scale=2)], [desc("d", Type("decimal", 8, True, 3), scale=3)])
    with pytest.raises(ValueError, match="scale"):
        resolve_setop_columns([desc("d", Type("decimal", 8, True, 2), scale=2)], [k])
    with pytest.raises(ValueError, match="dictionary"):
        resolve_setop_columns([desc("s", DICT, 0, WORDS)], [desc("s", DICT, 0, OTHER_WORDS)])
    with pytest.raises(ValueError, match="dictionary"):
        resolve_setop_columns([desc("s", DICT, 0, WORDS)], [k])
    with pytest.raises(ValueError, match="dictionary"):
        resolve_setop_columns([k], [desc("s", DICT, 0, WORDS)])
    many = [desc(f"c{i}", INT, i) for i in range(9)]
    with pytest.raises(QueryMustRunOnCpu):
        resolve_setop_columns(many, many)
    assert len(resolve_setop_columns(many[:8], many[:8])[0]) == 8


# ---- a unit that carries result_setops ---------------------------------------------------------------------------------
def test_result_setops_default_to_empty_and_are_refused_below_the_columns():
    from hdk_amd.executor import Executor
    from hdk_amd.ir import Agg, ColRef, KeyRef, QueryUnit, ResultSetOp
    from hdk_amd.plan import compile_query
    from hdk_amd.storage import ArrowStorage
    names = [f.name for f in dataclasses.fields(QueryUnit)]
    assert "result_setops" in names[-2:] and QueryUnit("t").result_setops == []
    so = ResultSetOp(None, "union")
    assert (so.right, so.op, so.all) == (None, "union", False)
    st = ArrowStorage()
    st.import_numpy("t", {"k": np.arange(10, dtype=np.int64) % 3, "v": np.arange(10, dtype=np.int64)})
    q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s")], result_setops=[so])
    with pytest.raises(ValueError, match="result_setops"):
        compile_query(st, q)
    ex = Executor.__new__(Executor)  # (the refusals come before anything of the executor is used)
    with pytest.raises(ValueError, match="result_setops need result='columns'"):
        ex.execute(q)
    with pytest.raises(ValueError, match="result_setops need result='columns'"):
        ex.execute(q, result="buffer")
