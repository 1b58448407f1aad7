"""Device-side columnar results for projections and non-grouped results (hdk_hip_columnarize_rows), the ABI directly: a
buffer in the plan's layout is made in numpy (random words plus planted extremes), uploaded and columnarized; every word is
compared with result_set.rows_to_dense on the host copy.  The routine moves and widens, it never rounds: all comparisons
are exact."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd._lib import check, lib
from hdk_amd.ir import Agg, ColRef, KeyRef, Proj, QueryUnit, Type
from hdk_amd.plan import columnar_slot_offsets, compile_query
from hdk_amd.storage import ArrowStorage

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A5A5A5A5A
SLACK = 8  # poisoned words behind the output block
TILE = 4096  # rows per tile (hdk_amd/csrc/row_columns.hip: kRwTile)
TOTALS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17]


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


# ---- plans ------------------------------------------------------------------------------------------------------------------
def rowwise_plan(ntargets, entry_count):
    st = ArrowStorage()
    st.import_numpy("t", {f"c{i}": np.arange(4, dtype=np.int64) for i in range(ntargets)})
    cp = compile_query(st, QueryUnit("t", targets=[Proj(ColRef(f"c{i}"), f"c{i}") for i in range(ntargets)], scan_limit=entry_count))
    p = cp.plan
    assert p.query_kind == A.Q_PROJECTION and not p.output_columnar and p.row_size_quad == ntargets + 1 and p.entry_count == entry_count
    return cp


WIDTHS = [("i8", 1), ("i16", 2), ("i32", 4), ("i64", 8)]


def columnar_plan(entry_count, nullable=True):
    """1-, 2-, 4- and 8-byte integer columns and a double, all in one plan"""
    st = ArrowStorage()
    cols = {"i8": np.zeros(4, np.int8), "i16": np.zeros(4, np.int16), "i32": np.zeros(4, np.int32), "i64": np.zeros(4, np.int64),
            "d": np.zeros(4, np.float64)}
    types = {"d": Type("fp", 8, nullable)}
    types.update({name: Type("int", w, nullable) for name, w in WIDTHS})
    st.import_numpy("t", cols, types=types)
    cp = compile_query(st, QueryUnit("t", targets=[Proj(ColRef(c), c) for c in cols], output_columnar=True, scan_limit=entry_count))
    p = cp.plan
    assert p.query_kind == A.Q_PROJECTION and p.output_columnar and cp.slot_widths == [1, 2, 4, 8, 8] and p.entry_count == entry_count
    return cp


def random_buffer(cp, seed):
    """the plan's buffer filled with random words, padding included"""
    rng = np.random.default_rng(seed)
    return rng.integers(-2**63, 2**63 - 1, max(cp.buffer_bytes // 8, 1), dtype=np.int64, endpoint=True)


def plant_extremes(cp, buf, rows):
    """minimum, -1, 0, maximum and the NULL sentinel of every integer column of columnar_plan, at both ends of the rows"""
    n = int(cp.plan.entry_count)
    raw = buf.view(np.uint8)
    for (name, w), off in zip(WIDTHS, columnar_slot_offsets(cp, n)):
        dt = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[w]
        col = raw[off:off + n * w].view(dt)
        ii = np.iinfo(dt)
        vals = np.array([ii.min, -1, 0, ii.max, Type("int", w).null_value()], dtype=dt)
        k = min(len(vals), rows)
        col[:k] = vals[:k]
        if rows >= 2 * len(vals):
            col[rows - len(vals):rows] = vals[::-1]


# ---- the call -------------------------------------------------------------------------------------------------------------
def columnarize_rows(mgr, cp, d_buf_ptr, entry_count, total, capacity=None, count_only=False, positions=False, total_ptr="own"):
    """-> (status, row_count, the output block as (num_targets, capacity) int64, the positions block, the slack) with poison
    where nothing was written"""
    L = lib()
    nt = int(cp.plan.num_targets)
    cap = int(entry_count if capacity is None else capacity)
    block = np.full(nt * cap + SLACK, POISON, dtype=np.int64)
    pos = np.full(cap + SLACK, POISON, dtype=np.int64)
    d_out, d_pos = mgr.to_device(block, 0), mgr.to_device(pos, 0)
    d_rows = mgr.to_device(np.array([POISON], dtype=np.uint64), 0)
    d_total = mgr.to_device(np.array([0 if total is None else total, 0], dtype=np.int32), 0)
    try:
        tp = (None if total is None else d_total.ptr) if total_ptr == "own" else total_ptr
        st = L.hdk_hip_columnarize_rows(C.byref(cp.plan), d_buf_ptr, entry_count, tp, None if count_only else d_out.ptr, cap,
                                        d_pos.ptr if positions else None, d_rows.ptr, 0, None)
        mgr.synchronizeStream(0)
        rows = int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0])
        got = mgr.to_host(d_out.ptr, block.nbytes, 0, np.int64)
        got_pos = mgr.to_host(d_pos.ptr, pos.nbytes, 0, np.int64)
    finally:
        for d in (d_out, d_pos, d_rows, d_total):
            d.free()
    return st, rows, got[:nt * cap].reshape(nt, cap), got_pos[:cap], np.concatenate([got[nt * cap:], got_pos[cap:]])


def check_buffer(mgr, cp, buf, total, **kw):
    """Upload a host buffer, columnarize it, compare with rows_to_dense: the count, the exact prefix of every column and
    of the positions, and the poison everywhere else."""
    n = 1 if cp.plan.query_kind == A.Q_NON_GROUPED else int(cp.plan.entry_count)
    projection = cp.plan.query_kind == A.Q_PROJECTION
    positions = bool(kw.get("positions"))
    want = rs.rows_to_dense(cp, buf, total, positions=positions)
    want_rows = len(want[0])
    d_buf = mgr.to_device(np.ascontiguousarray(buf), 0)
    try:
        st, rows, got, got_pos, slack = columnarize_rows(mgr, cp, d_buf.ptr, n, total if projection else None, **kw)
    finally:
        d_buf.free()
    assert st == A.OK, lib().hdk_hip_last_error()
    assert rows == want_rows
    cap = got.shape[1]
    m = 0 if kw.get("count_only") else min(rows, cap)
    for t in range(cp.plan.num_targets):
        assert np.array_equal(got[t, :m], want[t][:m]), f"target {t}"
        assert (got[t, m:] == POISON).all(), f"target {t}: written past row {m}"
    if positions:
        assert np.array_equal(got_pos[:m], want[-1][:m])
        assert (got_pos[m:] == POISON).all()
    else:
        assert (got_pos == POISON).all()
    assert (slack == POISON).all()
    return rows, got


def _odd(n):
    return n if n % 2 else n + 1


# ---- 1. geometry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", TOTALS)
def test_geometry_row_wise(mgr, total):
    cp = rowwise_plan(2, max(total, 1))
    check_buffer(mgr, cp, random_buffer(cp, total), total, positions=True)


@pytest.mark.parametrize("total", TOTALS)
def test_geometry_columnar(mgr, total):
    """entry_count odd: a narrow column's end is no multiple of 16, and the next starts after padding"""
    cp = columnar_plan(_odd(max(total, 1)))
    buf = random_buffer(cp, total)
    plant_extremes(cp, buf, total)
    check_buffer(mgr, cp, buf, total, positions=True)


@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
def test_fewer_rows_than_entries(mgr, columnar):
    total = 3 * TILE + 17
    cp = columnar_plan(_odd(total + 1000)) if columnar else rowwise_plan(3, total + 1000)
    check_buffer(mgr, cp, random_buffer(cp, 1), total, positions=True)


@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
def test_total_matched_outside_the_buffer(mgr, columnar):
    n = TILE + 33
    cp = columnar_plan(n) if columnar else rowwise_plan(3, n)
    buf = random_buffer(cp, 2)
    rows, _ = check_buffer(mgr, cp, buf, n + 5000, positions=True)  # the step ran out of output rows: every entry is a row
    assert rows == n
    rows, _ = check_buffer(mgr, cp, buf, 2**31 - 1)
    assert rows == n
    for total in (0, -1, -2**31):  # nothing matched / a count below zero: no row, nothing read into the (poisoned) block
        rows, _ = check_buffer(mgr, cp, buf, total, positions=True)
        assert rows == 0


# ---- 2. capacity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["row16", "rowwise", "columnar"])
def test_capacity(mgr, layout):
    total = TILE + 101
    cp = columnar_plan(_odd(total)) if layout == "columnar" else rowwise_plan(1 if layout == "row16" else 4, total)
    buf = random_buffer(cp, 3)
    rows, _ = check_buffer(mgr, cp, buf, total, count_only=True, positions=True)  # writes nothing: the block is compared whole
    assert rows == total
    for cap in (total - 1, 1, TILE, total + 7):
        rows, got = check_buffer(mgr, cp, buf, total, capacity=cap, positions=True)
        assert rows == total and got.shape[1] == cap  # the true count whatever the capacity


# ---- 3. widths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nullable", [True, False], ids=["nullable", "not_null"])
def test_narrow_columns_are_sign_extended(mgr, nullable):
    total = 2 * TILE + 5  # two full tiles through the 8-byte groups, the rest per value
    cp = columnar_plan(total, nullable)
    buf = random_buffer(cp, 4)
    plant_extremes(cp, buf, total)
    rows, got = check_buffer(mgr, cp, buf, total)
    for t, (name, w) in enumerate(WIDTHS):
        lo, hi, null = -2**(8 * w - 1), 2**(8 * w - 1) - 1, Type("int", w).null_value()
        assert got[t, :5].tolist() == [lo, -1, 0, hi, null] and got[t, total - 5:total].tolist() == [null, hi, 0, -1, lo]
        assert got[t, :total].min() >= lo and got[t, :total].max() <= hi
    # the schema names the sign-extended sentinel
    from hdk_amd.plan import describe_columns
    for d, (name, w) in zip(describe_columns(cp), WIDTHS):
        assert d.nullable == nullable and d.null_bits == Type("int", w).null_value() == got[WIDTHS.index((name, w)), 4]


# ---- 4. row-wise widths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, "walk", "lds"])
@pytest.mark.parametrize("total", [4097, 3 * 4096 + 17])
@pytest.mark.parametrize("ntargets", [1, 2, 3, 5, 8])
def test_row_wise_widths(mgr, monkeypatch, ntargets, total, variant):
    """rows of 2, 3, 4, 6 and 9 words: the register path, an odd and an even LDS pitch, the widest row; through the
    kernel the library picks and through each of the two it has"""
    if variant:
        monkeypatch.setenv("HDK_HIP_ROWS_VARIANT", variant)
    from hdk_amd._lib import sync_switches
    sync_switches()
    cp = rowwise_plan(ntargets, total)
    buf = random_buffer(cp, ntargets * total)
    check_buffer(mgr, cp, buf, total, positions=True)
    check_buffer(mgr, cp, buf, total)  # pos_out = NULL leaves its block untouched
    # a buffer that starts 8 bytes off a 16-byte boundary takes 8-byte loads
    d_buf = mgr.alloc(buf.nbytes + 8, 0)
    try:
        mgr.copyHostToDevice(d_buf.ptr + 8, buf, buf.nbytes, 0)
        st, rows, got, got_pos, slack = columnarize_rows(mgr, cp, d_buf.ptr + 8, total, total, positions=True)
    finally:
        d_buf.free()
    want = rs.rows_to_dense(cp, buf, total, positions=True)
    assert st == A.OK and rows == total and np.array_equal(got, np.stack(want[:-1])) and np.array_equal(got_pos, want[-1])


# ---- 5. beyond 4 GiB -----------------------------------------------------------------------------------------------------------
def test_offsets_beyond_4_gib(mgr):
    """300 M rows of 16 bytes: row 2^28 starts at byte 2^32.  The buffer is set on the device and three rows are planted
    with small copies; only they and their neighbours are read back."""
    n = 300_000_000
    cp = rowwise_plan(1, n)
    L = lib()
    d_buf = mgr.alloc(n * 16, 0)
    d_out = mgr.alloc(2 * n * 8, 0)
    d_rows = mgr.to_device(np.array([POISON], dtype=np.uint64), 0)
    d_total = mgr.to_device(np.array([n, 0], dtype=np.int32), 0)
    try:
        mgr.setDeviceMem(d_buf.ptr, 0x11, n * 16, 0)
        mgr.setDeviceMem(d_out.ptr, 0x5A, 2 * n * 8, 0)
        planted = [(0, 11, -5), (2**28, 22, 6), (n - 1, 33, 2**40)]
        for e, pos, val in planted:
            mgr.copyHostToDevice(d_buf.ptr + e * 16, np.array([pos, val], dtype=np.int64), 16, 0)
        check(L.hdk_hip_columnarize_rows(C.byref(cp.plan), d_buf.ptr, n, d_total.ptr, d_out.ptr, n, d_out.ptr + n * 8, d_rows.ptr, 0, None))
        mgr.synchronizeStream(0)
        assert int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0]) == n
        fill = 0x1111111111111111
        for e, pos, val in planted:
            lo, hi = max(e - 2, 0), min(e + 3, n)
            want_v, want_p = [fill] * (hi - lo), [fill] * (hi - lo)
            want_v[e - lo], want_p[e - lo] = val, pos
            assert mgr.to_host(d_out.ptr + lo * 8, (hi - lo) * 8, 0, np.int64).tolist() == want_v, e
            assert mgr.to_host(d_out.ptr + (n + lo) * 8, (hi - lo) * 8, 0, np.int64).tolist() == want_p, e
    finally:
        for d in (d_buf, d_out, d_rows, d_total):
            d.free()


# ---- 6. non-grouped ------------------------------------------------------------------------------------------------------------
def _agg_plan(targets):
    st = ArrowStorage()
    st.import_numpy("t", {"v": np.arange(4, dtype=np.int64), "w": np.arange(4, dtype=np.int32), "f": np.zeros(4, np.float32),
                          "d": np.zeros(4, np.float64)})
    cp = compile_query(st, QueryUnit("t", targets=targets))
    assert cp.plan.query_kind == A.Q_NON_GROUPED and set(cp.slot_widths) == {8}  # (the plan compiler makes no 4-byte slots here)
    return cp


def _f32(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def test_non_grouped_every_aggregate_kind(mgr):
    cp = _agg_plan([Agg("count", None, "n"), Agg("count", ColRef("w"), "nw"), Agg("sum", ColRef("v"), "s"), Agg("min", ColRef("w"), "lo"),
                    Agg("max", ColRef("v"), "hi"), Agg("avg", ColRef("v"), "m"), Agg("single_value", ColRef("v"), "one"),
                    Agg("sum", ColRef("d"), "sd")])
    buf = np.array([7, 5, -2**62, A.NULL_INT, 2**63 - 1, 2**62 + 12345, 3, A.NULL_BIGINT, np.float64(-0.1).view(np.int64)], dtype=np.int64)
    rows, got = check_buffer(mgr, cp, buf, None)
    assert rows == 1
    assert got[5, 0] == int((np.float64(2**62 + 12345) / np.float64(3)).view(np.int64))  # a sum beyond 2^53: one double division
    assert got[:5, 0].tolist() == buf[:5].tolist() and got[6, 0] == A.NULL_BIGINT
    buf[6] = 0  # AVG at count 0
    rows, got = check_buffer(mgr, cp, buf, None)
    assert got[5, 0] == A.NULL_DOUBLE_BITS


def test_non_grouped_float_accumulators(mgr):
    cp = _agg_plan([Agg("sum", ColRef("f"), "s"), Agg("min", ColRef("f"), "lo"), Agg("avg", ColRef("f"), "m"), Agg("avg", ColRef("d"), "md"),
                    Agg("count", ColRef("f"), "n"), Agg("max", ColRef("f"), "hi")])
    junk = 0x7777 << 32  # the high half of a float slot is not the value's
    buf = np.array([_f32(1.7) | junk, A.NULL_FLOAT_BITS | junk, _f32(-3.25) | junk, 4, np.float64(2.5).view(np.int64), 7, 9,
                    _f32(-0.0)], dtype=np.int64)
    rows, got = check_buffer(mgr, cp, buf, None)
    f = np.float32
    assert got[0, 0] == int(np.float64(f(1.7)).view(np.int64)) and got[1, 0] == A.NULL_DOUBLE_BITS
    assert got[2, 0] == int((np.float64(f(-3.25)) / np.float64(4)).view(np.int64))
    assert got[3, 0] == int((np.float64(2.5) / np.float64(7)).view(np.int64)) and got[4, 0] == 9
    buf[3] = buf[5] = 0
    rows, got = check_buffer(mgr, cp, buf, None)
    assert got[2, 0] == got[3, 0] == A.NULL_DOUBLE_BITS
    check_buffer(mgr, cp, buf, None, count_only=True)
    check_buffer(mgr, cp, buf, None, capacity=3)


# ---- 7. rejections -------------------------------------------------------------------------------------------------------------
def _status(mgr, cp, *, buf=8, entry_count=None, total=8, rows=8):
    """the status and message of a call with small integers for the device pointers (no call gets as far as a launch)"""
    L = lib()
    n = int(cp.plan.entry_count) if entry_count is None else entry_count
    st = L.hdk_hip_columnarize_rows(C.byref(cp.plan), buf, n, total, None, 0, None, rows, 0, None)
    return st, (L.hdk_hip_last_error() or b"").decode()


def test_rejections(mgr):
    st = ArrowStorage()
    st.import_numpy("t", {"k": np.arange(50, dtype=np.int64), "v": np.arange(50, dtype=np.int64)})
    grouped = compile_query(st, QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s")]))
    code, msg = _status(mgr, grouped)
    assert code == A.ERR_UNSUPPORTED and "hdk_hip_columnarize_result" in msg
    proj = rowwise_plan(2, 100)
    agg = _agg_plan([Agg("sum", ColRef("v"), "s")])
    for cp in (proj, agg):
        code, msg = _status(mgr, cp, buf=None, entry_count=1 if cp is agg else None, total=None if cp is agg else 8)
        assert code == A.ERR_INVALID_ARG and "buf" in msg
        code, msg = _status(mgr, cp, rows=None, entry_count=1 if cp is agg else None, total=None if cp is agg else 8)
        assert code == A.ERR_INVALID_ARG and "row_count" in msg
    code, msg = _status(mgr, proj, total=None)
    assert code == A.ERR_INVALID_ARG and "total_matched" in msg
    for n in (0, 2, 100):
        code, msg = _status(mgr, agg, entry_count=n, total=None)
        assert code == A.ERR_INVALID_ARG and "entry_count" in msg
    assert lib().hdk_hip_columnarize_rows(None, 8, 1, None, None, 0, None, 8, 0, None) == A.ERR_INVALID_ARG


# ---- 8. a second call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["rowwise", "columnar"])
def test_a_second_call_is_byte_identical(mgr, layout):
    total = 2 * TILE + 77
    cp = columnar_plan(_odd(total)) if layout == "columnar" else rowwise_plan(5, total)
    buf = random_buffer(cp, 9)
    d_buf = mgr.to_device(buf, 0)
    try:
        first = columnarize_rows(mgr, cp, d_buf.ptr, int(cp.plan.entry_count), total, positions=True)
        second = columnarize_rows(mgr, cp, d_buf.ptr, int(cp.plan.entry_count), total, positions=True)
        assert np.array_equal(mgr.to_host(d_buf.ptr, buf.nbytes, 0, np.int64), buf)  # the input is not modified
    finally:
        d_buf.free()
    assert first[0] == second[0] == A.OK and first[1] == second[1] == total
    for a, b in zip(first[2:], second[2:]):
        assert a.tobytes() == b.tobytes()
