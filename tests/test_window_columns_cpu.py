"""hdk_hip_window_columns without a device: the numpy expectation of the GPU tests (window_expect.py) against SQLite and
the rules SQLite cannot show, the host arithmetic and the argument checks of the C ABI, and the resolution of ir.Window
against a result's columns."""
import ctypes as C
import os
import sqlite3

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import lib
from hdk_amd.ir import Agg, BinOp, ColRef, KeyRef, Lit, OrderEntry, QueryMustRunOnCpu, QueryUnit, TargetRef, Type, Window
from hdk_amd.plan import (ColumnDesc, compile_query, default_window_frame, describe_columns, group_windows,
                          resolve_window_columns, split_count_distinct)
from hdk_amd.storage import ArrowStorage

import window_expect as W
from window_expect import FRAMES, KINDS, NULL_F64_BITS, NULL_I64, WOut, bits

INT_NULLABLE = (False, True, NULL_I64)
FP_NULLABLE = (True, True, NULL_F64_BITS)


# ---- the evaluator against SQLite ------------------------------------------------------------------------------------
def _table(seed, nparts, norder, n=300):
    """k1, k2 partition keys (k2 nullable), o1, o2 order keys with ties (o1 nullable), a nullable int column, a nullable
    real column of one sign; sorted by the partition keys, then the order keys, NULLs last.  Partition k1 == 0 has no
    value in either column."""
    rng = np.random.default_rng(seed)
    k1 = rng.integers(0, 6, n).astype(np.int64)
    k2 = rng.integers(0, 3, n).astype(np.int64)
    k2[rng.random(n) < 0.2] = NULL_I64
    o1 = rng.integers(0, 5, n).astype(np.int64)
    o1[rng.random(n) < 0.15] = NULL_I64
    o2 = rng.integers(0, 3, n).astype(np.int64)
    iv = rng.integers(-50, 50, n).astype(np.int64)
    iv[rng.random(n) < 0.3] = NULL_I64
    fw = bits(rng.integers(1, 400, n) / 8.0).copy()
    fw[rng.random(n) < 0.3] = NULL_F64_BITS
    iv[k1 == 0] = NULL_I64
    fw[k1 == 0] = NULL_F64_BITS
    cols = [k1, k2, o1, o2, iv, fw]
    sort_by = [0, 1][:nparts] + [2, 3][:norder]
    order = sorted(range(n), key=lambda r: tuple((cols[c][r] == NULL_I64, cols[c][r]) for c in sort_by))
    return [c[order] for c in cols]


def _sqlite(cols):
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE t (pos INTEGER, k1 INTEGER, k2 INTEGER, o1 INTEGER, o2 INTEGER, iv INTEGER, fv REAL)")
    rows = []
    for r in range(len(cols[0])):
        ints = [None if cols[c][r] == NULL_I64 else int(cols[c][r]) for c in range(5)]
        f = cols[5][r]
        rows.append((r, *ints, None if f == NULL_F64_BITS else float(np.int64(f).view(np.float64))))
    db.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?, ?, ?)", rows)
    return db


def _unword(w, nullable, null_bits, is_fp):
    if nullable and w == null_bits:
        return None
    return float(np.int64(w).view(np.float64)) if is_fp else int(w)


UPTO_ROW = "ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW"
UPTO_PEERS = "RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW"
WHOLE = "ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING"


def _cases(nparts, norder):
    """[(WOut, SQL expression, how to read SQLite's answer)] over every kind with every frame it reads.  Peers are the
    rows with equal order keys; where the contract speaks of ROWS, SQLite orders by the order keys and then by the row's
    position in the input, which is the order the evaluator sees."""
    part = "PARTITION BY " + ", ".join(["k1", "k2"][:nparts])
    peers = "ORDER BY " + ", ".join(f"{c} NULLS LAST" for c in ["o1", "o2"][:norder])
    rows = peers + ", pos"
    res = [(WOut("row_number"), f"ROW_NUMBER() OVER ({part} {rows})", "int")]
    for kind in ("rank", "dense_rank"):
        res.append((WOut(kind), f"{kind.upper()}() OVER ({part} {peers})", "int"))
    for kind in ("percent_rank", "cume_dist"):
        res.append((WOut(kind), f"{kind.upper()}() OVER ({part} {peers})", "fp"))
    for col, null, sql_col in ((4, INT_NULLABLE, "iv"), (5, FP_NULLABLE, "fv")):
        how = "fp" if null[0] else "int"
        for k in (0, 1, 2, 7):
            res.append((WOut("lag", col, "rows", *null, k), f"LAG({sql_col}, {k}) OVER ({part} {rows})", how))
            res.append((WOut("lead", col, "rows", *null, k), f"LEAD({sql_col}, {k}) OVER ({part} {rows})", how))
        res.append((WOut("first_value", col, "rows", *null), f"FIRST_VALUE({sql_col}) OVER ({part} {rows})", how))
        res.append((WOut("last_value", col, "rows", *null), f"LAST_VALUE({sql_col}) OVER ({part} {rows} {UPTO_ROW})", how))
        res.append((WOut("last_value", col, "partition", *null), f"LAST_VALUE({sql_col}) OVER ({part} {rows} {WHOLE})", how))
        # (which of several peers SQLite takes for the last is its own business: it names the row, the word is looked up)
        res.append((WOut("last_value", col, "range", *null), f"MAX(pos) OVER ({part} {peers} {UPTO_PEERS})", "row of " + str(col)))
        windows = {"rows": f"({part} {rows} {UPTO_ROW})", "range": f"({part} {peers} {UPTO_PEERS})", "partition": f"({part})"}
        for frame, over in windows.items():
            for kind in ("count", "sum", "min", "max", "avg"):
                h = "int" if kind == "count" else "sum" if null[0] and kind in ("sum", "avg") else "fp" if kind == "avg" else how
                res.append((WOut(kind, col, frame, *null), f"{kind.upper()}({sql_col}) OVER {over}", h))
    for frame, over in windows.items():
        res.append((WOut("count", -1, frame), f"COUNT(*) OVER {over}", "int"))
    return res


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("nparts", [1, 2])
@pytest.mark.parametrize("norder", [1, 2])
def test_evaluator_agrees_with_sqlite(seed, nparts, norder):
    cols = _table(seed, nparts, norder)
    n = len(cols[0])
    cases = _cases(nparts, norder)
    assert {c[0].kind for c in cases} == set(KINDS) - {"ntile"}
    for kind in ("count", "sum", "min", "max", "avg", "last_value"):
        assert {c[0].frame for c in cases if c[0].kind == kind} == set(FRAMES)
    got = W.window(cols, n, [0, 1][:nparts], [2, 3][:norder], [c[0] for c in cases])
    want = _sqlite(cols).execute("SELECT " + ", ".join(c[1] for c in cases) + " FROM t ORDER BY pos").fetchall()
    assert len(want) == n
    saw_null_sum = saw_peers = False
    for j, (o, sql, how) in enumerate(cases):
        is_fp_word = how in ("fp", "sum")
        nullable = o.kind not in ("count", "row_number", "rank", "dense_rank", "percent_rank", "cume_dist")
        null_bits = NULL_F64_BITS if o.kind == "avg" else o.null_bits
        for r in range(n):
            b = want[r][j]
            if how.startswith("row of"):
                assert got[j][r] == cols[o.col][b], (sql, r)
                saw_peers = saw_peers or b > r
                continue
            a = _unword(got[j][r], nullable, null_bits, is_fp_word)
            if how == "sum" and a is not None:
                assert b is not None and abs(a - b) <= 1e-6 * abs(b), (sql, r, a, b)
            else:
                assert a == b, (sql, r, a, b)
            saw_null_sum = saw_null_sum or (o.kind == "sum" and a is None)
    assert saw_null_sum and saw_peers


@pytest.mark.parametrize("seed", [4, 5])
def test_ntile_is_the_references_rule(seed):
    cols = _table(seed, 1, 1)
    n = len(cols[0])
    db = _sqlite(cols)
    sizes = {k: c for k, c in db.execute("SELECT k1, COUNT(*) FROM t GROUP BY k1")}
    for nt in (1, 2, 3, 7, 1000):
        got = W.window(cols, n, [0], [2], [WOut("ntile", param=nt), WOut("row_number")])
        for r in range(n):
            size = sizes[int(cols[0][r])]
            per = (size + nt - 1) // nt  # index_to_ntile, QE/WindowContext.cpp:194-206
            assert got[0][r] == (got[1][r] - 1) // per + 1
        want = db.execute(f"SELECT k1, NTILE({nt}) OVER (PARTITION BY k1 ORDER BY o1 NULLS LAST, pos) FROM t ORDER BY pos").fetchall()
        checked = 0
        for r, (k, tile) in enumerate(want):
            if sizes[k] % nt == 0:  # (the standard spreads a remainder over the first tiles: SQLite does, the reference does not)
                assert got[0][r] == tile
                checked += 1
        assert checked or nt > 3


# ---- the rules SQLite cannot show -------------------------------------------------------------------------------------
def test_signed_zeros_split_peer_groups_and_null_keys_do_not():
    part = np.zeros(5, dtype=np.int64)
    o = bits([0.0, 0.0, -0.0, -0.0, 0.0])
    got = W.window([part, o], 5, [0], [1], [WOut("rank"), WOut("dense_rank"), WOut("count", -1, "range")])
    assert got[0].tolist() == [1, 1, 3, 3, 5] and got[1].tolist() == [1, 1, 2, 2, 3] and got[2].tolist() == [2, 2, 4, 4, 5]
    o = np.array([NULL_I64, NULL_I64, 3], dtype=np.int64)
    assert W.window([part[:3], o], 3, [0], [1], [WOut("rank")])[0].tolist() == [1, 1, 3]
    assert W.window([o], 3, [0], [], [WOut("row_number")])[0].tolist() == [1, 2, 1]  # NULL partition keys: one partition


def test_int_sum_wraps_and_a_sum_equal_to_the_sentinel_stays_a_value():
    big = (1 << 62) + 1
    cols = [np.zeros(4, dtype=np.int64), np.array([big, big, big, NULL_I64], dtype=np.int64)]
    got = W.window(cols, 4, [0], [], [WOut("sum", 1, "rows", *INT_NULLABLE), WOut("sum", 1, "partition")])
    wrap = lambda x: (x + (1 << 63)) % (1 << 64) - (1 << 63)  # noqa: E731
    assert [int(x) for x in got[0]] == [big, wrap(2 * big), wrap(3 * big), wrap(3 * big)]
    assert int(got[1][0]) == wrap(3 * big + NULL_I64)  # not nullable: the sentinel is a value
    # -2^62 twice is the sentinel: a value, then a value again
    cols = [np.zeros(3, dtype=np.int64), np.array([-(1 << 62), -(1 << 62), 5], dtype=np.int64)]
    got = W.window(cols, 3, [0], [], [WOut("sum", 1, "rows", *INT_NULLABLE), WOut("count", 1, "rows", *INT_NULLABLE)])
    assert [int(x) for x in got[0]] == [-(1 << 62), NULL_I64, NULL_I64 + 5] and got[1].tolist() == [1, 2, 3]


def test_lag_zero_is_the_row_itself_and_the_word_is_copied_unexamined():
    cols = [np.array([1, 1, 1, 2], dtype=np.int64), np.array([7, NULL_I64, 9, 4], dtype=np.int64)]
    got = W.window(cols, 4, [0], [], [WOut("lag", 1, "rows", False, True, -1, 0), WOut("lag", 1, "rows", False, True, -1, 1),
                                      WOut("lead", 1, "rows", False, True, -1, 2), WOut("lead", 1, "rows", False, True, -1, 10**12)])
    assert got[0].tolist() == cols[1].tolist()
    assert got[1].tolist() == [-1, 7, NULL_I64, -1] and got[2].tolist() == [9, -1, -1, -1] and got[3].tolist() == [-1] * 4


def test_unsorted_input_makes_every_stretch_a_partition():
    k = np.array([1, 2, 1, 1], dtype=np.int64)
    got = W.window([k], 4, [0], [], [WOut("row_number"), WOut("count", -1, "partition")])
    assert got[0].tolist() == [1, 1, 1, 2] and got[1].tolist() == [1, 1, 2, 2]
    assert W.window([k], 0, [0], [], [WOut("row_number")])[0].tolist() == []
    assert W.window([k], 4, [], [], [WOut("row_number")])[0].tolist() == [1, 2, 3, 4]


# ---- the C ABI's host side -------------------------------------------------------------------------------------------
TILE = 4096
# per row the directory's three 32-bit entries; per tile two 32-bit counts and per out an 8-byte partial and a 4-byte count
WS_BYTES = lambda n, outs: 12 * n + (n / TILE) * (8 + 12 * outs)  # noqa: E731
WS_HEAD = lambda outs: (8 + 12 * outs) + 8 + 7 * 256  # noqa: E731  (a partly filled last tile, the totals, seven regions rounded to 256 bytes)


def test_the_struct_mirrors_the_header():
    assert C.sizeof(A.WindowOut) == lib().hdk_hip_sizeof_window_out() == 24
    offs = {f[0]: getattr(A.WindowOut, f[0]).offset for f in A.WindowOut._fields_}
    assert offs == {"col": 0, "kind": 4, "frame": 5, "is_fp": 6, "nullable": 7, "null_bits": 8, "param": 16}
    assert A.MAX_WINDOW_KEYS == 8 and A.MAX_WINDOW_OUTS == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hdk_hip.h")).read()
    for i, k in enumerate(KINDS):
        assert getattr(A, "WIN_" + k.upper()) == i and f"HDK_WIN_{k.upper()} = {i}" in hdr
    for i, f in enumerate(FRAMES):
        assert getattr(A, "FRAME_" + f.upper()) == i and f"HDK_FRAME_{f.upper()} = {i}" in hdr
    assert "#define HDK_HIP_MAX_WINDOW_OUTS 8" in hdr and "#define HDK_HIP_MAX_WINDOW_KEYS 8" in hdr


def test_workspace_is_monotone_and_bounded():
    L = lib()
    for outs in (1, 2, 8):
        last = 0
        for n in [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 10 * TILE, 200_003, 1_100_003, 100_000_000, 2**32 - 1]:
            b = L.hdk_hip_window_columns_workspace_bytes(n, outs)
            assert b >= last and b % 8 == 0
            assert b <= WS_BYTES(n, outs) + WS_HEAD(outs), (n, outs)
            assert b >= 12 * n + (n // TILE) * (8 + 12 * outs)
            last = b
        assert L.hdk_hip_window_columns_workspace_bytes(10 * TILE, outs) >= L.hdk_hip_window_columns_workspace_bytes(10 * TILE, 1)


def _outs(*specs):
    arr = (A.WindowOut * max(len(specs), 1))()
    for i, s in enumerate(specs):
        col, kind, frame, param = (list(s) + [0, 0])[:4]
        arr[i] = A.WindowOut(col, kind, frame, 0, 0, 0, param)
    return arr


def test_invalid_arguments_come_back_before_any_device():
    L = lib()
    ok_ptr = 4096  # (never dereferenced: every check comes first)
    key0 = (C.c_int32 * 8)(0, 1, 0, 0, 0, 0, 0, 0)

    def call(cols=ok_ptr, capacity=100, num_cols=2, num_rows=100, part=key0, num_part=1, order=key0, num_order=1,
             outs=_outs((0, A.WIN_SUM)), num_outs=1, out=1 << 30, out_capacity=100, ws=None, ws_bytes=0):
        st = L.hdk_hip_window_columns(cols, capacity, num_cols, num_rows, part, num_part, order, num_order, outs, num_outs, out,
                                      out_capacity, ws, ws_bytes, 0, None)
        return st, (L.hdk_hip_last_error() or b"").decode()

    for kw in ({"cols": None}, {"outs": None}, {"out": None}, {"part": None}, {"order": None}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "NULL" in msg, kw
    for k in (9, -1):
        st, msg = call(num_part=k)
        assert st == A.ERR_INVALID_ARG and "num_part" in msg
        st, msg = call(num_order=k)
        assert st == A.ERR_INVALID_ARG and "num_order" in msg
    for k in (0, 9, -1):
        st, msg = call(num_outs=k)
        assert st == A.ERR_INVALID_ARG and "num_outs" in msg
    st, msg = call(num_cols=0)
    assert st == A.ERR_INVALID_ARG and "num_cols" in msg
    for c in (-1, 2):
        st, msg = call(part=(C.c_int32 * 1)(c))
        assert st == A.ERR_INVALID_ARG and "partition key" in msg and "column" in msg
        st, msg = call(order=(C.c_int32 * 1)(c))
        assert st == A.ERR_INVALID_ARG and "order key" in msg and "column" in msg
    for kind in (A.WIN_SUM, A.WIN_MIN, A.WIN_MAX, A.WIN_AVG, A.WIN_LAG, A.WIN_LEAD, A.WIN_FIRST_VALUE, A.WIN_LAST_VALUE):
        for c in (-1, 2):
            st, msg = call(outs=_outs((c, kind)))
            assert st == A.ERR_INVALID_ARG and "column" in msg, (kind, c)
    st, msg = call(outs=_outs((2, A.WIN_COUNT)))
    assert st == A.ERR_INVALID_ARG and "column" in msg
    for kind in (15, 200):
        st, msg = call(outs=_outs((0, kind)))
        assert st == A.ERR_INVALID_ARG and "kind" in msg
    for frame in (3, 255):
        st, msg = call(outs=_outs((0, A.WIN_SUM, frame)))
        assert st == A.ERR_INVALID_ARG and "frame" in msg
    for kind in (A.WIN_LAG, A.WIN_LEAD, A.WIN_NTILE, A.WIN_SUM):
        st, msg = call(outs=_outs((0, kind, 0, -1)))
        assert st == A.ERR_INVALID_ARG and "param" in msg
    st, msg = call(outs=_outs((0, A.WIN_NTILE, 0, 0)))
    assert st == A.ERR_INVALID_ARG and "NTILE" in msg
    st, msg = call(num_rows=101, out_capacity=200)
    assert st == A.ERR_INVALID_ARG and "capacity" in msg
    st, msg = call(out_capacity=99)
    assert st == A.ERR_INVALID_ARG and "out_capacity" in msg
    st, msg = call(num_rows=2**32, capacity=2**33, out_capacity=2**33)
    assert st == A.ERR_INVALID_ARG and "32-bit" in msg
    st, msg = call(out=ok_ptr + 8)
    assert st == A.ERR_INVALID_ARG and "overlap" in msg
    st, msg = call(out=ok_ptr - 8)
    assert st == A.ERR_INVALID_ARG and "overlap" in msg
    need = L.hdk_hip_window_columns_workspace_bytes(100, 1)
    st, msg = call(ws=1 << 20, ws_bytes=need - 1)
    assert st == A.ERR_INVALID_ARG and "workspace" in msg
    st, msg = call(ws=(1 << 20) + 4, ws_bytes=need)
    assert st == A.ERR_INVALID_ARG and "aligned" in msg
    for kw, names in (({"ws": ok_ptr + 1024, "ws_bytes": need}, ("workspace", "cols")),
                      ({"ws": (1 << 30) - 8, "ws_bytes": need}, ("workspace", "out_cols"))):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "overlap" in msg and all(x in msg for x in names), (kw, msg)
    # what is allowed: no keys at all, the ranking kinds with any column, COUNT(*); no rows is no work and no device
    assert call(num_rows=0, part=None, num_part=0, order=None, num_order=0,
                outs=_outs((-1, A.WIN_COUNT), (-7, A.WIN_RANK), (99, A.WIN_NTILE, 0, 4)), num_outs=3)[0] == A.OK


# ---- ir.Window against a result's columns ----------------------------------------------------------------------------
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


def _describe():
    q = QueryUnit("t", groupby=[ColRef("k"), ColRef("s")],
                  targets=[KeyRef(0), KeyRef(1), Agg("count", None, "n"), Agg("sum", ColRef("x"), "sx"), Agg("min", ColRef("f"), "mf")])
    return describe_columns(compile_query(_storage(), q))


def test_default_frames():
    for kind in KINDS:
        assert default_window_frame(kind, False) == "partition"
    assert [default_window_frame(k, True) for k in ("count", "sum", "avg", "min", "max", "last_value")] == \
        ["range", "range", "range", "rows", "rows", "rows"]
    d = _describe()
    by = [OrderEntry("sx", True)]
    outs = [Window("sum", "n"), Window("min", "n"), Window("last_value", "n"), Window("sum", "n", frame="rows"),
            Window("count"), Window("avg", TargetRef("sx"))]
    assert [s.frame for s in resolve_window_columns(d, ["k"], by, outs)[2]] == [A.FRAME_RANGE, A.FRAME_ROWS, A.FRAME_ROWS,
                                                                               A.FRAME_ROWS, A.FRAME_RANGE, A.FRAME_RANGE]
    assert {s.frame for s in resolve_window_columns(d, ["k"], [], outs[:3] + outs[4:])[2]} == {A.FRAME_PARTITION}


def test_windows_resolve_columns_types_names_and_nullability():
    d = _describe()
    outs = [Window("rank"), Window("row_number", name="rn"), Window("percent_rank"), Window("cume_dist"), Window("ntile", param=4),
            Window("count"), Window("count", "sx"), Window("avg", "n"), Window("lag", "n"), Window("lead", "mf", param=Lit(3)),
            Window("first_value", "sx"), Window("last_value", "n"), Window("sum", 3), Window("min", "mf"), Window("max", "s"),
            Window("sum", "n", name="total"), Window("dense_rank")]
    part, order, spec, out = resolve_window_columns(d, ["k", TargetRef(1)], [OrderEntry("sx", True), OrderEntry(2, False, True)], outs)
    assert part == [0, 1] and order == [(3, True, False), (2, False, True)]
    assert [(s.kind, s.col, s.param) for s in spec] == [
        (A.WIN_RANK, -1, 0), (A.WIN_ROW_NUMBER, -1, 0), (A.WIN_PERCENT_RANK, -1, 0), (A.WIN_CUME_DIST, -1, 0), (A.WIN_NTILE, -1, 4),
        (A.WIN_COUNT, -1, 0), (A.WIN_COUNT, 3, 0), (A.WIN_AVG, 2, 0), (A.WIN_LAG, 2, 1), (A.WIN_LEAD, 4, 3), (A.WIN_FIRST_VALUE, 3, 0),
        (A.WIN_LAST_VALUE, 2, 0), (A.WIN_SUM, 3, 0), (A.WIN_MIN, 4, 0), (A.WIN_MAX, 1, 0), (A.WIN_SUM, 2, 0), (A.WIN_DENSE_RANK, -1, 0)]
    assert [c.name for c in out] == ["rank_5", "rn", "percent_rank_7", "cume_dist_8", "ntile_9", "count_10", "count_11", "avg_12",
                                     "lag_13", "lead_14", "first_value_15", "last_value_16", "sum_17", "min_18", "max_19", "total",
                                     "dense_rank_21"]
    assert [c.target_idx for c in out] == list(range(5, 22))
    int64 = Type("int", 8, False)
    for j in (0, 1, 4, 5, 6, 16):  # ranking kinds and counts: int64, never NULL
        assert (out[j].is_fp, out[j].nullable, out[j].type) == (False, False, int64), j
    for j in (2, 3):
        assert (out[j].is_fp, out[j].nullable, out[j].type) == (True, False, Type("fp", 8, False))
    assert (out[7].is_fp, out[7].nullable, out[7].null_bits) == (True, True, NULL_F64_BITS)  # AVG
    assert (out[8].is_fp, out[8].nullable, out[8].null_bits, out[8].type) == (False, True, NULL_I64, d[2].type)  # LAG of a count
    assert (out[9].is_fp, out[9].nullable, out[9].null_bits, out[9].type) == (True, True, NULL_F64_BITS, d[4].type)
    assert (out[10].nullable, out[10].null_bits, out[10].type) == (d[3].nullable, d[3].null_bits, d[3].type)  # FIRST_VALUE: as the argument
    assert (out[11].nullable, out[11].type) == (False, d[2].type)
    assert (out[12].is_fp, out[12].nullable, out[12].null_bits, out[12].type.size) == (False, True, NULL_I64, 8)
    assert (out[13].is_fp, out[13].nullable, out[13].null_bits) == (True, True, NULL_F64_BITS)
    assert out[14].dictionary is d[1].dictionary and out[14].nullable  # MAX of a string id stays a string id
    assert (out[15].nullable, out[15].null_bits) == (True, NULL_I64)  # SUM of a count: nullable by rule, never NULL in fact
    dec = [ColumnDesc("k", False, False, 0, Type("int", 8, False), 0, "key"),
           ColumnDesc("d", False, True, NULL_I64, Type("decimal", 8, True, 2), 1, "agg", "sum", None, 2)]
    out = resolve_window_columns(dec, [0], [], [Window("sum", "d"), Window("avg", "d"), Window("count", "d"), Window("lag", "d")])[3]
    assert [c.scale for c in out] == [2, 2, 0, 2] and out[0].type.kind == "decimal"


def test_windows_refuse_what_they_cannot_do():
    d = _describe()
    for part, order, outs in (([BinOp("+", ColRef("k"), Lit(1))], [], [Window("rank")]),
                              (["k"], [], [Window("sum", ColRef("x"))]),  # an input column is no output column
                              (["k"], [], [Window("sum", BinOp("+", TargetRef("n"), Lit(1)))]),
                              (["k"], [], [Window("lag", "n", param=TargetRef("n"))]),  # a lag that is no constant
                              (["k"], [], [Window("lag", "n", param=1.5)]),
                              (["k"], [], [Window("ntile", param=ColRef("v"))]),
                              (["k"] * 9, [], [Window("rank")]),
                              (["k"], [OrderEntry("n")] * 9, [Window("rank")]),
                              (["k"], [OrderEntry("s")], [Window("rank")])):  # id order is not string order
        with pytest.raises(QueryMustRunOnCpu):
            resolve_window_columns(d, part, order, outs)
    for part, order, outs in ((["nope"], [], [Window("rank")]), ([7], [], [Window("rank")]), (["k"], [OrderEntry("nope")], [Window("rank")]),
                              (["k"], [], []), (["k"], [], [Window("median", "n")]), (["k"], [], [Window("sum", "n", frame="groups")]),
                              (["k"], [], [Window("sum")]), (["k"], [], [Window("rank", "n")]), (["k"], [], [Window("sum", "s")]),
                              (["k"], [], [Window("avg", "s")]), (["k"], [], [Window("ntile")]), (["k"], [], [Window("lag", "n", param=-1)]),
                              (["k"], [], [Window("sum", "nope")]), (["k"], [], [Window("rank", name="n")]),
                              (["k"], [], [("rank", None, None)])):
        with pytest.raises(ValueError):
            resolve_window_columns(d, part, order, outs)
    assert resolve_window_columns(d, ["s"], [], [Window("rank")])[0] == [1]  # a partition key may be dictionary-encoded


def test_a_units_windows_group_by_specification_and_leave_the_plan_alone():
    by = (OrderEntry("sx", True),)
    ws = [Window("rank", partition_by=("k",), order_by=by), Window("sum", "n", partition_by=("k",)),
          Window("lag", "n", partition_by=["k"], order_by=list(by)), Window("count", partition_by=("k",))]
    assert group_windows(ws) == [(("k",), by, [0, 2]), (("k",), (), [1, 3])]
    with pytest.raises(ValueError):
        group_windows([("rank",)])
    assert QueryUnit("t").windows == []
    # ORDER BY may name a window column: the plan leaves the entries to the windowed columns
    q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0), Agg("count", None, "n")],
                  windows=[Window("rank", order_by=[OrderEntry("n")], name="r")], order_by=[OrderEntry("r")])
    assert compile_query(_storage(), q).order_by == []
    with pytest.raises(ValueError):
        compile_query(_storage(), QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0)], order_by=[OrderEntry("r")]))
    with pytest.raises(QueryMustRunOnCpu):
        compile_query(_storage(), QueryUnit("t", targets=[Agg("count")], windows=[Window("rank")]))
    # a count_distinct unit hands its windows to the regroup step
    q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0), Agg("count_distinct", ColRef("x"), "dx")],
                  windows=[Window("rank", order_by=[OrderEntry("dx", True)])])
    inner, rg = split_count_distinct(q)
    assert inner.windows == [] and rg.windows == q.windows
    # result="buffer" is refused before anything is prepared (no device is touched)
    from hdk_amd.executor import Executor
    ex = Executor.__new__(Executor)
    for unit in (q, dataclass_replace(q, targets=[KeyRef(0)])):
        with pytest.raises(ValueError, match="windows"):
            Executor.execute(ex, unit, result="buffer")


def dataclass_replace(q, **kw):
    import dataclasses
    return dataclasses.replace(q, **kw)
