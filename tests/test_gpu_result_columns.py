"""Device-side columnar results (hdk_hip_columnarize_result): a group-by buffer in HBM becomes one dense 8-byte column
per target, rows in entry order.  Every expectation comes from code that is not under test: the host reader
(hdk_amd/result_set.py: non_empty_mask / _slot_arrays / _key_arrays) applied to the same buffer, with the value table of
include/hdk_hip.h restated in numpy.  Most cases need no GPU query: the oracle gives a host buffer in the plan's layout,
which is uploaded and columnarized."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd._lib import check, lib
from hdk_amd.ir import FP64, Agg, Cast, Cmp, ColRef, KeyRef, Lit, Proj, QueryUnit
from hdk_amd.plan import compact_init_vals, compile_query
from hdk_amd.storage import ArrowStorage

from util import oracle_init_buffer, run_oracle

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


# ---- the expectation: the host reader + the value table in numpy ---------------------------------------------------------
def expected_columns(cp, buf, entry_count=None):
    """(row count, [int64 bit patterns per target]) of the non-empty entries of a host buffer, in entry order."""
    p = cp.plan
    n = int(entry_count if entry_count is not None else p.entry_count)
    buf = np.ascontiguousarray(buf)
    mask = rs.non_empty_mask(cp, buf, n)
    slots = rs._slot_arrays(cp, buf, n)
    keys = rs._key_arrays(cp, buf, n)
    out, s = [], 0
    for t in range(p.num_targets):
        tg = p.targets[t]
        a = (slots[s] if slots[s] is not None else keys[tg.key_idx])[mask].astype(np.int64)
        lo = (a & 0xFFFFFFFF).astype(np.uint32)
        if tg.agg == A.AGG_AVG:  # pair_to_double
            cnt = slots[s + 1][mask].astype(np.int64)
            if tg.arg_is_fp == A.FP_SLOT_FLOAT:
                dividend = lo.view(np.float32).astype(np.float64)
            elif tg.arg_is_fp:
                dividend = a.view(np.float64)
            else:
                dividend = a.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                bits = (dividend / cnt.astype(np.float64)).view(np.int64).copy()
            bits[cnt == 0] = A.NULL_DOUBLE_BITS
        elif tg.arg_is_fp == A.FP_SLOT_FLOAT and tg.agg not in (A.AGG_COUNT, A.AGG_ID):
            bits = lo.view(np.float32).astype(np.float64).view(np.int64).copy()
            if tg.skip_null:
                bits[lo == np.uint32(A.NULL_FLOAT_BITS)] = A.NULL_DOUBLE_BITS
        else:
            bits = a
        out.append(bits)
        s += 2 if tg.agg == A.AGG_AVG else 1
    return int(mask.sum()), out


# ---- the call -------------------------------------------------------------------------------------------------------------
def columnarize(mgr, cp, d_buf_ptr, entry_count, capacity=None, count_only=False, pool_workspace=False):
    """-> (row_count, the whole output block as (num_targets, capacity) int64, poison where nothing was written)."""
    L = lib()
    nt = int(cp.plan.num_targets)
    cap = int(entry_count if capacity is None else capacity)
    block = np.full(max(nt * cap, 1), POISON, dtype=np.int64)
    d_out = mgr.to_device(block, 0)
    d_rows = mgr.to_device(np.array([POISON], dtype=np.uint64), 0)
    iv = np.ascontiguousarray(cp.init_vals, dtype=np.int64)
    ws_bytes = L.hdk_hip_result_columns_workspace_bytes(entry_count)
    d_ws = None if pool_workspace else mgr.alloc(ws_bytes, 0)
    try:
        check(L.hdk_hip_columnarize_result(C.byref(cp.plan), d_buf_ptr, entry_count, iv.ctypes.data,
                                           None if count_only else d_out.ptr, cap, d_rows.ptr,
                                           d_ws.ptr if d_ws else None, ws_bytes if d_ws else 0, 0, None))
        mgr.synchronizeStream(0)
        rows = int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0])
        got = mgr.to_host(d_out.ptr, block.nbytes, 0, np.int64)[:nt * cap].reshape(nt, cap)
    finally:
        d_out.free()
        d_rows.free()
        if d_ws:
            d_ws.free()
    return rows, got


def check_buffer(mgr, cp, buf, entry_count=None, **kw):
    """Upload a host buffer, columnarize it, compare with the host reader: the count, the exact prefix of every column,
    and the poison everywhere else."""
    n = int(entry_count if entry_count is not None else cp.plan.entry_count)
    want_rows, want = expected_columns(cp, buf, n)
    d_buf = mgr.to_device(np.ascontiguousarray(buf), 0)
    try:
        rows, got = columnarize(mgr, cp, d_buf.ptr, n, **kw)
    finally:
        d_buf.free()
    assert rows == want_rows
    cap = got.shape[1]
    m = 0 if kw.get("count_only") else min(rows, cap)
    for t in range(cp.plan.num_targets):
        assert np.array_equal(got[t, :m], want[t][:m]), f"target {t}"
        assert (got[t, m:] == POISON).all(), f"target {t}: written past row {m}"
    return rows, got


# ---- 1. occupancy geometry ------------------------------------------------------------------------------------------------
def _occupancy_buffer(oracle, n, pattern, nullable_v):
    """Perfect hash, GROUP BY k, SUM(v), row-wise, entry_count n.  nullable_v: v has NULLs, so the table is keyed (3 quads
    a row); without them it is keyless with 16-byte rows (get_keyless_info), the rows one 16-byte load reads."""
    k = np.arange(n, dtype=np.int64)
    if pattern == "full" or pattern == "none":
        keep = np.ones(n, dtype=bool)
    else:  # alternating occupied and empty runs of `pattern` entries; both ends kept so that the key range stays [0, n)
        keep = (k // int(pattern)) % 2 == 0
        keep[0] = keep[-1] = True
    k = k[keep]
    rng = np.random.default_rng(n + len(k))
    v = rng.integers(-10**6, 10**6, len(k), dtype=np.int64)
    if nullable_v and len(k) > 1:
        v[1] = A.NULL_BIGINT
    st = ArrowStorage()
    st.import_numpy("t", {"k": k, "v": v})
    quals = [Cmp(ColRef("v"), "<", Lit(-10**7))] if pattern == "none" else []
    cp, buf, err = run_oracle(oracle, st, QueryUnit("t", quals=quals, groupby=[ColRef("k")],
                                                    targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s")]))
    assert err == 0
    p = cp.plan
    assert p.query_kind == A.Q_PERFECT_HASH and not p.output_columnar and p.entry_count == n
    return cp, buf, int(keep.sum()) if pattern != "none" else 0


_GEOMETRY = [(n, pat) for n in (1, 63, 64, 65, 200_003) for pat in ("none", "full")] + \
            [(200_003, run) for run in (1, 64, 256, 4096, 65536)]


@pytest.mark.parametrize("nullable_v", [False, True], ids=["keyless16", "keyed24"])
@pytest.mark.parametrize("n,pattern", _GEOMETRY)
def test_occupancy_geometry(oracle, mgr, n, pattern, nullable_v):
    cp, buf, groups = _occupancy_buffer(oracle, n, pattern, nullable_v)
    if n > 2:
        assert bool(cp.plan.keyless) == (not nullable_v) and cp.plan.row_size_quad == (3 if nullable_v else 2)
    rows, _ = check_buffer(mgr, cp, buf)
    assert rows == groups


# ---- 2. capacity and count-only -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs256(oracle):
    return _occupancy_buffer(oracle, 200_003, 256, False)


def test_count_only_writes_nothing(mgr, runs256):
    cp, buf, groups = runs256
    rows, got = check_buffer(mgr, cp, buf, count_only=True, pool_workspace=True)
    assert rows == groups and (got == POISON).all()


@pytest.mark.parametrize("cap", ["rows-1", 1])
def test_capacity_limits_the_rows_written_not_the_count(mgr, runs256, cap):
    cp, buf, groups = runs256
    cap = groups - 1 if cap == "rows-1" else cap
    rows, got = check_buffer(mgr, cp, buf, capacity=cap, pool_workspace=True)
    assert rows == groups and got.shape[1] == cap and not (got == POISON).any()


# ---- 3. layout matrix -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matrix_table():
    rng = np.random.default_rng(7)
    n = 30_000
    v = rng.integers(-10**9, 10**9, n, dtype=np.int64)
    v[rng.random(n) < 0.05] = A.NULL_BIGINT
    st = ArrowStorage()
    st.import_numpy("t", {
        "k": rng.integers(0, 9000, n).astype(np.int64) * 3,          # sparse perfect-hash range: two thirds empty
        "k32": rng.integers(-500, 7000, n).astype(np.int32),
        "b": rng.integers(0, 70, n).astype(np.int32),
        "c": rng.integers(0, 90, n).astype(np.int32),
        "v": v,
        "vnn": rng.integers(1, 10**6, n, dtype=np.int64),            # no NULLs: keyless plans
    }, fragment_size=11_000)
    return st


# (no COUNT(*) and only nullable arguments: nothing get_keyless_info could use, so the perfect-hash table stays keyed)
_AGGS = [Agg("sum", ColRef("v"), "s"), Agg("count", ColRef("v"), "c"), Agg("avg", ColRef("v"), "a"), Agg("min", ColRef("v"), "mn")]


@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
@pytest.mark.parametrize("baseline", [False, True], ids=["perfect", "baseline"])
def test_layout_matrix(oracle, mgr, matrix_table, columnar, baseline):
    q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k")] + _AGGS, output_columnar=columnar,
                  force_baseline=baseline, baseline_entry_count=20_011 if baseline else None)
    cp, buf, err = run_oracle(oracle, matrix_table, q)
    p = cp.plan
    assert err == 0 and p.query_kind == (A.Q_BASELINE_HASH if baseline else A.Q_PERFECT_HASH)
    assert bool(p.output_columnar) == columnar and not p.keyless
    assert p.targets[0].slot_width == (0 if baseline else 8)  # baseline: the projected key has no slot of its own
    rows, _ = check_buffer(mgr, cp, buf)
    assert 5000 < rows < 9000


@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
@pytest.mark.parametrize("second", ["sum", "avg"])
def test_keyless_perfect_hash(oracle, mgr, matrix_table, columnar, second):
    """Keyless: emptiness is the slot idx_target_as_key still holding its init value -- a SUM slot, or AVG's count slot
    (the second slot of its target)."""
    q = QueryUnit("t", groupby=[ColRef("k")], output_columnar=columnar,
                  targets=[KeyRef(0, "k"), Agg(second, ColRef("vnn"), "x"), Agg("max", ColRef("v"), "mx")])
    cp, buf, err = run_oracle(oracle, matrix_table, q)
    p = cp.plan
    assert err == 0 and p.keyless == 1 and bool(p.output_columnar) == columnar
    assert p.idx_target_as_key == (2 if second == "avg" else 1)
    check_buffer(mgr, cp, buf)


def test_keyless_four_byte_key_slot(oracle, mgr, matrix_table):
    """COUNT(*) alone: 4-byte slots (pick_target_compact_width), a row of 8 bytes, emptiness read from a 4-byte slot."""
    cp, buf, err = run_oracle(oracle, matrix_table, QueryUnit("t", groupby=[ColRef("k32")],
                                                              targets=[KeyRef(0, "k"), Agg("count", None, "c")]))
    p = cp.plan
    assert err == 0 and p.keyless == 1 and cp.slot_widths == [4, 4] and p.row_size_quad == 1
    check_buffer(mgr, cp, buf)


@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
def test_four_byte_slots_in_a_baseline_table(oracle, mgr, matrix_table, columnar):
    q = QueryUnit("t", groupby=[ColRef("k32")], force_baseline=True, baseline_entry_count=16_001, output_columnar=columnar,
                  targets=[KeyRef(0, "k"), Agg("count", None, "c")])
    cp, buf, err = run_oracle(oracle, matrix_table, q)
    p = cp.plan
    assert err == 0 and p.targets[1].slot_width == 4 and p.targets[0].slot_width == 0
    assert p.key_width == (8 if columnar else 4)
    check_buffer(mgr, cp, buf)


def test_four_byte_keys_and_two_key_columns_baseline(oracle, mgr, matrix_table):
    q = QueryUnit("t", groupby=[ColRef("b"), ColRef("c")], force_baseline=True, baseline_entry_count=12_007,
                  targets=[KeyRef(1, "c"), Agg("avg", ColRef("v"), "a"), KeyRef(0, "b"), Agg("sum", ColRef("v"), "s")])
    cp, buf, err = run_oracle(oracle, matrix_table, q)
    p = cp.plan
    assert err == 0 and p.key_width == 4 and p.key_count == 2
    assert p.targets[0].slot_width == 0 and p.targets[0].key_idx == 1 and p.targets[2].slot_width == 0
    rows, _ = check_buffer(mgr, cp, buf)
    assert rows > 4000


@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
def test_two_key_columns_perfect(oracle, mgr, matrix_table, columnar):
    q = QueryUnit("t", groupby=[ColRef("b"), ColRef("c")], output_columnar=columnar,
                  targets=[KeyRef(0, "b"), KeyRef(1, "c"), Agg("sum", ColRef("v"), "s"), Agg("count", ColRef("v"), "cv")])
    cp, buf, err = run_oracle(oracle, matrix_table, q)
    p = cp.plan
    assert err == 0 and p.query_kind == A.Q_PERFECT_HASH and p.key_count == 2 and p.entry_count == 70 * 90
    check_buffer(mgr, cp, buf)


# ---- 4. values ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def values_table():
    rng = np.random.default_rng(11)
    n = 6000
    k = rng.integers(0, 300, n).astype(np.int64)
    null_f = np.array([A.NULL_FLOAT_BITS], dtype=np.int32).view(np.float32)[0]
    null_d = np.array([A.NULL_DOUBLE_BITS], dtype=np.int64).view(np.float64)[0]
    f = (rng.normal(size=n) * 30).astype(np.float32)
    f[rng.random(n) < 0.1] = null_f
    f[k == 17] = null_f                       # a group whose FLOAT values are all NULL
    d = rng.normal(size=n) * 1e3
    d[rng.random(n) < 0.1] = null_d
    d[k == 23] = null_d
    big = rng.integers(2**51, 2**52, n, dtype=np.int64)   # ~20 rows a group: sums beyond 2^53
    big[rng.random(n) < 0.05] = A.NULL_BIGINT
    st = ArrowStorage()
    st.import_numpy("t", {"k": k, "f": f, "d": d, "big": big, "allnull": np.full(n, A.NULL_BIGINT, dtype=np.int64),
                          "sv": k * 7 - 100, "x": rng.integers(0, 40, n).astype(np.int64)})
    return st


def _target(cp, name):
    return next(oc.target_idx for oc in cp.out_cols if oc.name == name)


def test_avg_of_all_null_and_of_sums_beyond_2_53(oracle, mgr, values_table):
    q = QueryUnit("t", groupby=[ColRef("k")],
                  targets=[KeyRef(0, "k"), Agg("avg", ColRef("allnull"), "an"), Agg("avg", ColRef("big"), "ab"),
                           Agg("sum", ColRef("big"), "sb"), Agg("single_value", ColRef("sv"), "sv"), Agg("count", None, "c")])
    cp, buf, err = run_oracle(oracle, values_table, q)
    assert err == 0 and cp.plan.targets[_target(cp, "sv")].agg == A.AGG_SINGLE_VALUE
    rows, got = check_buffer(mgr, cp, buf)
    assert rows == 300
    assert (got[_target(cp, "an"), :rows] == A.NULL_DOUBLE_BITS).all()
    # AVG over an int64 sum that a double cannot hold exactly: double(sum) / double(count), as pair_to_double computes it
    slots = rs._slot_arrays(cp, buf, cp.plan.entry_count)
    mask = rs.non_empty_mask(cp, buf, cp.plan.entry_count)
    s, c = slots[3][mask], slots[4][mask]  # slots: k, an (2), ab (2), ...
    assert (s > 2**53).any()
    assert np.array_equal(got[_target(cp, "ab"), :rows].view(np.float64), s.astype(np.float64) / c.astype(np.float64))
    assert np.array_equal(got[_target(cp, "sv"), :rows], got[_target(cp, "k"), :rows] * 7 - 100)


@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
def test_float_and_double_accumulators(oracle, mgr, values_table, columnar):
    q = QueryUnit("t", groupby=[ColRef("k")], output_columnar=columnar,
                  targets=[KeyRef(0, "k"), Agg("avg", ColRef("f"), "af"), Agg("sum", ColRef("f"), "sf"),
                           Agg("min", ColRef("f"), "mf"), Agg("avg", ColRef("d"), "ad"), Agg("min", ColRef("d"), "md"),
                           Agg("max", ColRef("d"), "xd")])
    cp, buf, err = run_oracle(oracle, values_table, q)
    p = cp.plan
    assert err == 0
    for name in ("af", "sf", "mf"):  # float accumulators in 8-byte padded slots
        assert p.targets[_target(cp, name)].arg_is_fp == A.FP_SLOT_FLOAT and p.targets[_target(cp, name)].slot_width == 8
    for name in ("ad", "md", "xd"):
        assert p.targets[_target(cp, name)].arg_is_fp == A.FP_SLOT_DOUBLE
    rows, got = check_buffer(mgr, cp, buf)
    keys = got[_target(cp, "k"), :rows]
    all_null_f, all_null_d = int(np.nonzero(keys == 17)[0][0]), int(np.nonzero(keys == 23)[0][0])
    for name in ("af", "sf", "mf"):  # the group whose FLOAT values are all NULL: NULL_FLOAT -> NULL_DOUBLE
        assert got[_target(cp, name), all_null_f] == A.NULL_DOUBLE_BITS
        assert got[_target(cp, name), all_null_d] != A.NULL_DOUBLE_BITS
    for name in ("ad", "md", "xd"):
        assert got[_target(cp, name), all_null_d] == A.NULL_DOUBLE_BITS
    # and the host tail turns the device columns into the rows the host reader gives
    dense = rs.dense_to_columns(cp, [got[t, :rows] for t in range(p.num_targets)])
    assert dense == rs.to_columns(cp, buf)


def test_cast_to_double_key_keeps_its_bit_pattern(oracle, mgr, values_table):
    q = QueryUnit("t", groupby=[Cast(ColRef("x"), FP64)], targets=[KeyRef(0, "k"), Agg("sum", ColRef("sv"), "s")])
    cp, buf, err = run_oracle(oracle, values_table, q)
    assert err == 0 and cp.key_types[0].is_fp
    rows, got = check_buffer(mgr, cp, buf)
    assert rows == 40
    assert sorted(got[0, :rows].view(np.float64).tolist()) == [float(i) for i in range(40)]


# ---- 5. foreign entry count -----------------------------------------------------------------------------------------------
def test_reduced_table_with_a_foreign_entry_count(oracle, mgr, matrix_table):
    """A columnar baseline partial re-inserted into a fresh table of twice the entries (hdk_hip_reduce_buffers): the
    column offsets of the bigger table are not the plan's."""
    q = QueryUnit("t", groupby=[ColRef("k")], force_baseline=True, baseline_entry_count=20_011, output_columnar=True,
                  targets=[KeyRef(0, "k")] + _AGGS)
    cp, partial, err = run_oracle(oracle, matrix_table, q)
    p = cp.plan
    assert err == 0 and p.query_kind == A.Q_BASELINE_HASH and p.output_columnar
    n2 = 2 * int(p.entry_count)
    fresh = oracle_init_buffer(oracle, cp, entry_count=n2)
    d_this, d_that = mgr.to_device(fresh, 0), mgr.to_device(partial, 0)
    d_err = mgr.to_device(np.zeros(1, dtype=np.int32), 0)
    that = (C.c_void_p * 1)(d_that.ptr)
    counts = (C.c_uint32 * 1)(p.entry_count)
    iv = np.ascontiguousarray(cp.init_vals, dtype=np.int64)
    check(lib().hdk_hip_reduce_buffers(C.byref(p), d_this.ptr, n2, that, counts, 1, iv.ctypes.data, d_err.ptr, 0, None))
    mgr.synchronizeStream(0)
    assert int(mgr.to_host(d_err.ptr, 4, 0, np.int32)[0]) == 0
    reduced = mgr.to_host(d_this.ptr, fresh.nbytes, 0, np.int64)
    rows, got = columnarize(mgr, cp, d_this.ptr, n2)
    for d in (d_this, d_that, d_err):
        d.free()
    # in order: the host reader on the same reduced buffer
    want_rows, want = expected_columns(cp, reduced, n2)
    assert rows == want_rows
    for t in range(p.num_targets):
        assert np.array_equal(got[t, :rows], want[t]) and (got[t, rows:] == POISON).all()
    # as a set of rows: what the host reader gives for the partial table
    part_rows, part = expected_columns(cp, partial)
    assert rows == part_rows
    assert sorted(zip(*[g[:rows].tolist() for g in got])) == sorted(zip(*[c.tolist() for c in part]))


# ---- 6. offsets beyond 4 GiB ----------------------------------------------------------------------------------------------
def test_offsets_beyond_4_gib(oracle, mgr):
    """300 M entries of 16 bytes: entry 2^28 + 1 starts past 4 GiB.  The table is initialised on the device and three
    rows are planted with small copies; no host copy of the table exists."""
    st = ArrowStorage()
    st.import_numpy("t", {"k": np.arange(50, dtype=np.int64) * 10_000_000_019, "v": np.arange(50, dtype=np.int64)})
    cp = compile_query(st, QueryUnit("t", groupby=[ColRef("k")], force_baseline=True, baseline_entry_count=128,
                                     targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s")]))
    p = cp.plan
    assert p.query_kind == A.Q_BASELINE_HASH and not p.output_columnar and p.row_size_quad == 2 and p.key_width == 8
    n = 300_000_000
    L = lib()
    d_buf = mgr.alloc(n * 16, 0)
    d_init = mgr.to_device(compact_init_vals(cp), 0)
    try:
        check(L.hdk_hip_init_group_by_buffer(d_buf.ptr, d_init.ptr, n, 1, 8, 2, 0, 1, 256, 1024, 0, None))
        mgr.synchronizeStream(0)
        planted = [(0, 11, -5), (2**28 + 1, 22, 6), (n - 1, 33, 2**40)]
        for e, key, val in planted:
            mgr.copyHostToDevice(d_buf.ptr + e * 16, np.array([key, val], dtype=np.int64), 16, 0)
        rows, got = columnarize(mgr, cp, d_buf.ptr, n, capacity=16)
    finally:
        d_buf.free()
        d_init.free()
    assert rows == 3
    assert got[0, :3].tolist() == [11, 22, 33] and got[1, :3].tolist() == [-5, 6, 2**40]
    assert (got[:, 3:] == POISON).all()


# ---- 6b. more tiles than one trip of the scan -------------------------------------------------------------------------------
SCAN_TRIP = 4096  # tile counts hdk_counts_scan<4> takes per trip (1 024 threads x 4): 16.8 M entries
TILE = 4096  # entries per tile (hdk_amd/csrc/result_columns.hip: kRcTile)


def test_more_tiles_than_one_scan_trip(mgr):
    """4 098 tiles: the scan's carry crosses a trip boundary with groups in the tiles on both sides of it -- the last
    three entries of tile 4095 (the last counter of the first trip) and every third entry of tile 4096 (the first
    counter of the second).  A columnar perfect-hash table of one key and one slot column, built as a raw buffer."""
    n = SCAN_TRIP * TILE + TILE + 1
    st = ArrowStorage()
    st.import_numpy("t", {"k": np.array([0, n - 1], dtype=np.int64), "v": np.array([A.NULL_BIGINT, 1], dtype=np.int64)})
    cp = compile_query(st, QueryUnit("t", groupby=[ColRef("k")], output_columnar=True, targets=[Agg("sum", ColRef("v"), "s")]))
    p = cp.plan
    assert p.query_kind == A.Q_PERFECT_HASH and p.output_columnar and not p.keyless and p.entry_count == n
    assert p.key_count == 1 and cp.slot_widths == [8] and p.num_targets == 1
    kept = np.concatenate([np.arange(SCAN_TRIP * TILE - 3, SCAN_TRIP * TILE), np.arange(SCAN_TRIP * TILE, (SCAN_TRIP + 1) * TILE, 3)])
    buf = np.empty(2 * n, dtype=np.int64)  # [key column | slot column], n * 8 bytes each
    buf[:n] = A.EMPTY_KEY_64
    buf[n:] = int(cp.init_vals[0])
    buf[kept] = kept
    buf[n + kept] = kept * 7 - 3
    cap = 2048
    d_buf = mgr.to_device(buf, 0)
    try:
        rows, got = columnarize(mgr, cp, d_buf.ptr, n, capacity=cap)
    finally:
        d_buf.free()
    assert rows == len(kept) == 3 + 1366
    assert np.array_equal(got[0, :rows], kept * 7 - 3)
    assert (got[0, rows:] == POISON).all()


# ---- 7. rejections --------------------------------------------------------------------------------------------------------
def test_rejections(mgr, matrix_table):
    L = lib()
    d = mgr.alloc(1 << 16, 0)
    d_rows = mgr.alloc(8, 0)
    iv = np.zeros(16, dtype=np.int64)

    def call(plan, rows_ptr=d_rows.ptr, ws=None, ws_bytes=0, n=100):
        st = L.hdk_hip_columnarize_result(C.byref(plan), d.ptr, n, iv.ctypes.data, None, 0, rows_ptr, ws, ws_bytes, 0, None)
        return st, (L.hdk_hip_last_error() or b"").decode()

    try:
        non_grouped = compile_query(matrix_table, QueryUnit("t", targets=[Agg("sum", ColRef("v"), "s")]))
        assert non_grouped.plan.query_kind == A.Q_NON_GROUPED
        st, msg = call(non_grouped.plan)
        assert st == A.ERR_UNSUPPORTED and "non-grouped" in msg
        proj = compile_query(matrix_table, QueryUnit("t", quals=[Cmp(ColRef("b"), "<", Lit(3))], targets=[Proj(ColRef("v"), "v")]))
        assert proj.plan.query_kind == A.Q_PROJECTION
        st, msg = call(proj.plan)
        assert st == A.ERR_UNSUPPORTED and "projection" in msg
        grouped = compile_query(matrix_table, QueryUnit("t", groupby=[ColRef("b")], targets=[KeyRef(0), Agg("count")]))
        st, msg = call(grouped.plan, rows_ptr=None)
        assert st == A.ERR_INVALID_ARG and "row_count" in msg
        need = L.hdk_hip_result_columns_workspace_bytes(100)
        st, msg = call(grouped.plan, ws=d.ptr, ws_bytes=need - 1)
        assert st == A.ERR_INVALID_ARG and "workspace" in msg
        st, msg = call(grouped.plan, ws=d.ptr, ws_bytes=need, n=int(grouped.plan.entry_count))
        assert st == A.OK, msg
        mgr.synchronizeStream(0)
    finally:
        d.free()
        d_rows.free()


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def test_execute_with_result_columns(gpu_executor_factory, matrix_table):
    """Executor.execute(result="columns") and Engine.run(..., result="columns") give what the default path gives."""
    q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k")] + _AGGS)
    ex = gpu_executor_factory(matrix_table)
    want = ex.execute(q)
    cols = ex.execute(q, result="columns")
    try:
        assert cols.row_count() == cols.num_rows == want.row_count()
        assert cols.to_columns() == want.to_columns()
        assert cols.to_arrow().equals(want.to_arrow())
        assert cols.device_ptr(1) == cols.device_ptr(0) + cols.capacity * 8
        host = cols.to_host()
        assert [a.dtype for a in host] == [np.int64, np.int64, np.int64, np.float64, np.int64]
    finally:
        cols.free()
    with pytest.raises(ValueError):
        ex.execute(q, result="rows")


def test_fetch_columns_counts_first_above_the_threshold(gpu_executor_factory, matrix_table, monkeypatch):
    """Above COLUMNS_ONE_CALL_BYTES the block is sized by a count-only call: capacity == num_rows."""
    from hdk_amd.executor import PreparedStep
    q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k")] + _AGGS)
    ex = gpu_executor_factory(matrix_table)
    step = ex.prepare(q)
    try:
        step.enqueue()
        one = step.fetch_columns()
        assert one.capacity == step.cp.entry_count > one.num_rows
        monkeypatch.setattr(PreparedStep, "COLUMNS_ONE_CALL_BYTES", 1024)
        two = step.fetch_columns()
        assert two.capacity == two.num_rows == one.num_rows
        assert two.to_columns() == one.to_columns() == step.fetch().to_columns()
        one.free()
        two.free()
    finally:
        step.free()
