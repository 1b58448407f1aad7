"""The host side of scanning a device result (hdk_hip_chunk_columns, storage.DeviceTable, Executor.register_columns, a
QueryUnit whose table is a QueryUnit): the numpy evaluator of the call's contract (tests/chunk_expect.py) against the
storage layer's own statistics, the C ABI's argument checks, which come back before any device is touched, the workspace
arithmetic, the plans a DeviceTable compiles to -- byte for byte those of a host table with the same values -- and the
refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import storage as S
from hdk_amd._lib import lib
from hdk_amd.executor import BufferCache, DeviceColumns, Executor
from hdk_amd.ir import Agg, BinOp, Cmp, ColRef, JoinSpec, KeyRef, Lit, Or, Proj, QueryMustRunOnCpu, QueryUnit, Type
from hdk_amd.plan import ColumnDesc, compile_query

import chunk_expect as E
from chunk_expect import NULL_DOUBLE_BITS, NULL_FLOAT_WIDE_BITS, NULL_I32, NULL_I64


def make_columns(n, seed=7):
    """an int column with 4-byte NULLs, a double column with negative values and widened-float NULLs, a NOT NULL int"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-50, 50, n).astype(np.int64)
    a[rng.random(n) < 0.2] = NULL_I32
    d = (rng.random(n) * 200 - 100).view(np.int64).copy() if n else np.zeros(0, np.int64)
    d[rng.random(n) < 0.2] = NULL_FLOAT_WIDE_BITS
    b = rng.integers(0, 1000, n).astype(np.int64)
    sel = [(0, False, True, int(NULL_I32), int(NULL_I64)), (1, True, True, int(NULL_FLOAT_WIDE_BITS), int(NULL_DOUBLE_BITS)),
           (2, False, False, 0, int(NULL_I64))]
    types = [Type("int", 8, True), Type("fp", 8, True), Type("int", 8, False)]
    return [a, d, b], sel, types


# ---- the evaluator against the storage layer -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,frag", [(0, 32), (1, 32), (100, 32), (97, 64), (300, 4128), (3 * 4096 + 1, 4096)])
def test_evaluator_stats_equal_the_storage_layers(n, frag):
    cols, sel, types = make_columns(n)
    if n >= 64:
        cols[0][32:64] = NULL_I32  # an all-NULL fragment at frag 32
    out = E.copy(cols, n, sel)
    st = E.stats(out, sel, n, frag)
    host = {f"c{j}": (w.view(np.float64) if s[1] else w) for j, (w, s) in enumerate(zip(out, sel))}
    t = S.ArrowStorage().import_numpy("t", host, fragment_size=frag, types={f"c{j}": ty for j, ty in enumerate(types)})
    assert t.num_fragments == E.num_fragments(n, frag)
    for j, ty in enumerate(types):
        for f in range(t.num_fragments):
            mn, mx, nulls, values = st[j][f]
            rec = S.stats_from_record(ty, 0 if mn is None else mn, 0 if mx is None else mx, nulls, values)
            want = t.columns[f"c{j}"].stats[f]
            assert rec == want and type(rec.min) is type(want.min) and type(rec.max) is type(want.max), (j, f, rec, want)
            assert nulls + values == t.frag_rows[f]


def test_evaluator_rewrites_only_nullable_columns_and_keeps_nans_out_of_min_max():
    nan = np.array([np.nan], dtype=np.float64).view(np.int64)[0]
    d = np.array([-1.5, np.nan, 2.0, -0.0], dtype=np.float64).view(np.int64)
    cols = [np.array([1, int(NULL_I32), 3, int(NULL_I64)], dtype=np.int64), d]
    sel = [(0, False, True, int(NULL_I32), int(NULL_I64)), (0, False, False, int(NULL_I32), int(NULL_I64)),
           (1, True, True, int(NULL_FLOAT_WIDE_BITS), int(NULL_DOUBLE_BITS))]
    out = E.copy(cols, 4, sel)
    assert out[0].tolist() == [1, int(NULL_I64), 3, int(NULL_I64)] and out[1].tolist() == cols[0].tolist()
    st = E.stats(out, sel, 4, 32)
    assert st[0][0] == (1, 3, 2, 2)  # (a word that equals out_null_bits already reads as NULL afterwards)
    assert st[1][0] == (int(NULL_I64), 3, 0, 4)
    assert st[2][0][2:] == (0, 4) and np.array(st[2][0][:2], dtype=np.int64).view(np.float64).tolist() == [-1.5, 2.0]
    only_nan = E.stats([np.array([nan, nan], dtype=np.int64)], [sel[2]], 2, 32)
    assert only_nan[0][0] == (None, None, 0, 2)
    assert S.stats_from_record(Type("fp", 8), int(E.POS_INF_BITS), int(E.NEG_INF_BITS), 0, 2) == S.ChunkStats(None, None, False)


# ---- the C ABI: argument errors before any device, workspace arithmetic -------------------------------------------------
def _sel(*cols):
    arr = (A.ChunkCol * max(len(cols), 1))()
    for i, c in enumerate(cols):
        arr[i] = A.ChunkCol(c, 0, 1, (C.c_uint8 * 2)(), int(NULL_I32), int(NULL_I64))
    return arr


def test_invalid_arguments_come_back_before_any_device():
    L = lib()
    # (never dereferenced: every check comes first) cols 3 x 100 words at 4096, out 2 x 128 words at 1 << 30, stats at 1 << 20
    def call(cols=4096, cap=100, ncin=3, n=100, sel=_sel(0, 2), nc=2, frag=32, out=1 << 30, ocap=128, stats=1 << 20, ws=None,
             ws_bytes=0, device=0):
        st = L.hdk_hip_chunk_columns(cols, cap, ncin, n, sel, nc, frag, out, ocap, stats, ws, ws_bytes, device, None)
        return st, (L.hdk_hip_last_error() or b"").decode()

    for kw in ({"cols": None}, {"sel": None}, {"out": None}, {"stats": None}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "NULL" in msg, kw
    for nc in (0, 17, -1):
        st, msg = call(nc=nc, sel=_sel(*([0] * 17)))
        assert st == A.ERR_INVALID_ARG and "num_cols" in msg, nc
    for sel in (_sel(-1, 0), _sel(0, 3)):
        st, msg = call(sel=sel)
        assert st == A.ERR_INVALID_ARG and "names column" in msg
    for frag in (0, 31, 33, 4100):
        st, msg = call(frag=frag)
        assert st == A.ERR_INVALID_ARG and "fragment_rows" in msg, frag
    st, msg = call(n=2**32, cap=2**33, ocap=2**33)
    assert st == A.ERR_INVALID_ARG and "32-bit" in msg
    for kw in ({"n": 101, "ocap": 128}, {"n": 100, "ocap": 96}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "capacity" in msg, kw
    st, msg = call(ocap=100)
    assert st == A.ERR_INVALID_ARG and "out_capacity" in msg and "multiple of 32" in msg
    need = L.hdk_hip_chunk_columns_workspace_bytes(100, 32, 2)
    assert need > 0
    st, msg = call(ws=1 << 24, ws_bytes=need - 1)
    assert st == A.ERR_INVALID_ARG and "workspace" in msg
    st, msg = call(ws=(1 << 24) + 4, ws_bytes=need)
    assert st == A.ERR_INVALID_ARG and "aligned" in msg
    for kw, names in (({"out": 4096 + 8}, ("out_cols", "cols")), ({"stats": 4096 + 16}, ("stats", "cols")),
                      ({"stats": (1 << 30) + 800}, ("stats", "out_cols")),
                      ({"ws": 4096 + 1024, "ws_bytes": need}, ("workspace", "cols"))):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "overlap" in msg and all(x in msg for x in names), (kw, msg)
    # valid calls: one output column needs no aligned capacity, a column may be selected twice, no rows need no cols.  They are
    # given a device that does not exist: with these made-up addresses a call must never get as far as a launch
    for kw in ({"sel": _sel(1), "nc": 1, "ocap": 100}, {"sel": _sel(1, 1)}, {"cols": None, "n": 0, "cap": 0},
               {"sel": _sel(*range(3), *([0] * 13)), "nc": 16}, {"frag": 4128}):
        st, msg = call(device=-1, **kw)
        assert st == A.ERR_INVALID_ARG and msg == "device -1 out of range", (kw, msg)


def test_workspace_arithmetic():
    L = lib()
    for n in (0, 1, 4096, 4097):
        for frag in (32, 4128):
            for nc in (1, 2, 16):
                assert L.hdk_hip_chunk_columns_workspace_bytes(n, frag, nc) == E.workspace_bytes(n, frag, nc), (n, frag, nc)
    # spelled out: 4 097 rows in fragments of 32 are 129 tiles (one per fragment), in fragments of 4 128 two (4 096 + 1 rows)
    assert L.hdk_hip_chunk_columns_workspace_bytes(4097, 32, 1) == (129 * 32 + 255) // 256 * 256
    assert L.hdk_hip_chunk_columns_workspace_bytes(4097, 4128, 2) == 256
    assert L.hdk_hip_chunk_columns_workspace_bytes(4129, 4128, 1) == 256  # 2 tiles of fragment 0, 1 of fragment 1: 96 bytes
    assert L.hdk_hip_chunk_columns_workspace_bytes(0, 32, 1) == 0
    # partials are negligible next to the data: 32 bytes per column and 32 KiB tile
    assert L.hdk_hip_chunk_columns_workspace_bytes(100_000_000, 32_000_000, 2) <= 2 * 100_000_000 * 8 // 1000


def test_the_structs_and_constants_mirror_the_header():
    L = lib()
    assert C.sizeof(A.ChunkCol) == L.hdk_hip_sizeof_chunk_col() == 24
    assert C.sizeof(A.ChunkStatsRecord) == L.hdk_hip_sizeof_chunk_stats() == 32
    assert A.MAX_CHUNK_COLUMNS == 16


# ---- a DeviceTable compiles to the plan of a host table with the same values ---------------------------------------------
class FakeBlock:
    def __init__(self, ptr):
        self.ptr, self.freed = ptr, 0

    def free(self):
        self.freed += 1
        self.ptr = 0


def both_tables(n=1000, frag=320):
    """-> (storage with the DeviceTable "t" and the dimension "dim", storage with the same values imported from the host)"""
    rng = np.random.default_rng(3)
    k = rng.integers(0, 40, n).astype(np.int64)
    k[rng.random(n) < 0.1] = NULL_I32
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    x = np.round(rng.random(n) * 20 - 10, 1).view(np.int64).copy()
    x[rng.random(n) < 0.1] = NULL_FLOAT_WIDE_BITS
    sel = [(0, False, True, int(NULL_I32), int(NULL_I64)), (1, False, False, 0, int(NULL_I64)),
           (2, True, True, int(NULL_FLOAT_WIDE_BITS), int(NULL_DOUBLE_BITS))]
    names, types = ["k", "v", "x"], [Type("int", 8, True), Type("int", 8, False), Type("fp", 8, True)]
    out = E.copy([k, v, x], n, sel)
    st = E.stats(out, sel, n, frag)
    dim = {"dk": np.arange(40, dtype=np.int32), "dval": (np.arange(40, dtype=np.int64) * 3)}
    host = S.ArrowStorage()
    host.import_numpy("t", {nm: (w.view(np.float64) if ty.is_fp else w) for nm, w, ty in zip(names, out, types)},
                      fragment_size=frag, types=dict(zip(names, types)))
    host.import_numpy("dim", dim)
    dev = S.ArrowStorage()
    dev.import_numpy("dim", dim)
    cols = [S.Column(nm, ty, [], [S.stats_from_record(ty, r[0] or 0, r[1] or 0, r[2], r[3]) for r in st[j]])
            for j, (nm, ty) in enumerate(zip(names, types))]
    frag_rows = [min(frag, n - b) for b in range(0, n, frag)]
    dev.add_table(S.DeviceTable("t", cols, frag_rows, FakeBlock(1 << 30), 1024, frag))
    return dev, host


UNITS = {
    "perfect": QueryUnit("t", groupby=[ColRef("k")],
                         targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s"), Agg("count", None, "c"), Agg("min", ColRef("x"), "mn")]),
    "baseline": QueryUnit("t", groupby=[ColRef("x")], targets=[KeyRef(0, "x"), Agg("sum", ColRef("v"), "s")]),
    "filter_project": QueryUnit("t", quals=[Or(Cmp(ColRef("k"), "<", Lit(5)), Cmp(ColRef("v"), ">", Lit(900)))],
                                targets=[Proj(ColRef("k"), "k"), Proj(BinOp("+", ColRef("v"), Lit(1)), "v1")]),
    "non_grouped": QueryUnit("t", targets=[Agg("sum", ColRef("v"), "s"), Agg("count", None, "c"), Agg("max", ColRef("x"), "mx"),
                                           Agg("avg", ColRef("x"), "a")]),
    "join": QueryUnit("t", joins=[JoinSpec("dim", ColRef("k"), "dk")], groupby=[ColRef("k")],
                      targets=[KeyRef(0, "k"), Agg("sum", BinOp("+", ColRef("v"), ColRef("dval", "dim")), "s")]),
}


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_a_device_table_compiles_to_the_plan_of_the_host_table(unit):
    dev, host = both_tables()
    a, b = compile_query(dev, UNITS[unit]), compile_query(host, UNITS[unit])
    assert bytes(a.plan) == bytes(b.plan)
    assert a.entry_count == b.entry_count and a.buffer_bytes == b.buffer_bytes
    assert a.input_cols == b.input_cols and a.slot_widths == b.slot_widths


def test_device_table_addresses_and_the_cache_that_stores_nothing():
    dev, _ = both_tables()
    t = dev.get("t")
    assert t.num_rows == 1000 and t.num_fragments == 4 and t.frag_rows[-1] == 40
    assert all(c.fragments == [] for c in t.columns.values())
    assert t.device_column("k") == 1 << 30 and t.device_column("x") == (1 << 30) + 2 * 1024 * 8
    assert t.device_chunk("v", 3) == (1 << 30) + 1024 * 8 + 3 * 320 * 8
    assert all(t.device_chunk(c, f) % 256 == 0 for c in t.column_order for f in range(4))
    with pytest.raises(IndexError):
        t.device_chunk("k", 4)
    cache = BufferCache(None, 0)  # (no manager: a view needs none)
    view = cache.chunk(t, "v", 3)
    assert (view.ptr, view.nbytes) == (t.device_chunk("v", 3), 40 * 8)
    assert cache.linearized(t, "x").ptr == t.device_column("x") and cache.linearized(t, "x").nbytes == 8000
    assert cache.nbytes() == 0 and not cache._chunks
    view.free()
    cache.clear()
    assert t.block.freed == 0 and t.block.ptr == 1 << 30
    # another table under the same name: the cache answers from the table at hand, never from the name
    other = S.DeviceTable("t", list(t.columns.values()), t.frag_rows, FakeBlock(1 << 40), 1024, 320)
    assert cache.chunk(other, "v", 3).ptr == (1 << 40) + 1024 * 8 + 3 * 320 * 8
    t.free()
    t.free()
    assert t.block is None
    with pytest.raises(ValueError, match="freed"):
        t.device_chunk("k", 0)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_a_registered_table_cannot_be_the_inner_table():
    dev, _ = both_tables()
    q = QueryUnit("dim", joins=[JoinSpec("t", ColRef("dk"), "k")], targets=[Agg("sum", ColRef("v", "t"), "s")])
    with pytest.raises(QueryMustRunOnCpu, match="a registered result can only be scanned as the outer table"):
        compile_query(dev, q)


def _executor(storage=None):
    return Executor(storage or S.ArrowStorage(), 0, mgr=object())  # (every refusal comes before the manager is asked)


def _columns(descs, rows=0, error_code=0, block=None):
    return DeviceColumns(None, None, 0, block, rows, rows, error_code, descs)


def _desc(name, ty=Type("int", 8, True), **kw):
    return ColumnDesc(name, ty.is_fp, ty.nullable, A.to_i64(ty.null_as_int64_or_double_bits()), ty, **kw)


def test_compile_refuses_a_nested_unit():
    inner = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("count", None, "c")])
    with pytest.raises(ValueError, match="execute"):
        _executor().compile(QueryUnit(inner, targets=[Agg("sum", ColRef("c"), "s")]))


def test_register_columns_refusals():
    dev, _ = both_tables()
    ex = _executor(dev)
    ok = [_desc("a"), _desc("b")]
    with pytest.raises(ValueError, match="already a table"):
        ex.register_columns("t", _columns(ok))
    with pytest.raises(ValueError, match="not unique"):
        ex.register_columns("r", _columns([_desc("a"), _desc("a")]))
    with pytest.raises(ValueError, match="empty"):
        ex.register_columns("r", _columns([_desc("a"), _desc("")]))
    with pytest.raises(ValueError, match="error code 1"):
        ex.register_columns("r", _columns(ok, error_code=1))
    with pytest.raises(ValueError, match="error code -1"):
        ex.register_columns("r", _columns(ok, error_code=-1))
    with pytest.raises(ValueError, match="17 columns"):
        ex.register_columns("r", _columns([_desc(f"c{i}") for i in range(17)]))
    with pytest.raises(ValueError, match="freed"):
        ex.register_columns("r", _columns(ok, rows=5))
    with pytest.raises(ValueError, match="names no column"):
        ex.register_columns("r", _columns(ok), columns=["a", "z"])
    with pytest.raises(ValueError, match="outside"):
        ex.register_columns("r", _columns(ok), columns=[2])
    with pytest.raises(ValueError, match="not unique"):
        ex.register_columns("r", _columns(ok), columns=["a", 0])
    with pytest.raises(ValueError, match="positive"):
        ex.register_columns("r", _columns(ok), fragment_size=-1)
    assert "r" not in dev.tables
    with pytest.raises(ValueError, match="not a registered result"):
        ex.drop_registered("dim")


def test_the_type_rule():
    T = S.registered_column_type
    assert T(_desc("a", Type("int", 4, True))) == Type("int", 8, True)
    assert T(_desc("a", Type("int", 2, False))) == Type("int", 8, False)
    assert T(_desc("a", Type("decimal", 8, True, scale=2))) == Type("decimal", 8, True, scale=2)
    assert T(_desc("a", Type("timestamp", 8, True, unit="ms"))) == Type("timestamp", 8, True, unit="ms")
    assert T(_desc("a", Type("date", 8, True, unit="s"))) == Type("date", 8, True, unit="s")
    assert T(_desc("a", Type("fp", 4, True))) == Type("fp", 8, True)
    assert T(ColumnDesc("avg", True, True, int(NULL_DOUBLE_BITS), Type("int", 4), agg="avg")) == Type("fp", 8, True)
    assert T(ColumnDesc("c", False, False, 0, Type("dict", 4), agg="count")) == Type("int", 8, False)
    assert T(_desc("s", Type("dict", 4, True), dictionary=["x", "y"])) == Type("dict", 8, True)
    assert T(_desc("a", Type("int", 4, True))).null_value() == int(NULL_I64)
    for ty, what in ((Type("bool", 1, True), "bool"), (Type("date", 4, True, unit="d"), "DATE in days")):
        with pytest.raises(ValueError, match=f"'flag'.*{what}.*columns="):
            T(_desc("flag", ty))
    # and through the executor, where the remedy works
    ex = _executor()
    with pytest.raises(ValueError, match="columns="):
        ex.register_columns("r", _columns([_desc("a"), _desc("flag", Type("bool", 1, True))]))
