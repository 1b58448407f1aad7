"""hdk_hip_group_columns on raw uploaded columns: GROUP BY over dense 8-byte columns in HBM.  The expectation is
tests/group_expect.py (numpy, checked against SQLite in test_group_columns_cpu.py).  Every case asserts row_count, every
output column, the poison beyond the output rows and in a guard column, and an untouched input.  Everything is compared
word for word, except a SUM of doubles: 1e-6 relative, on positive values (its association is unspecified)."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import check, lib

import group_expect as G
from group_expect import NULL_F64_BITS, NULL_I64, Out, bits

pytestmark = pytest.mark.gpu

POISON64 = np.uint64(0x5A5A5A5A5A5A5A5A)
TILE = 4096  # rows per tile (hdk_amd/csrc/group_columns.hip: kGcTile); a wave owns 1024 of them, an item 64
TRIP = 4096  # tiles per trip of hdk_counts_scan<4> and of the carry scan (kGcCarryTrip)
N = 200_003
KIND = {"id": A.AGG_ID, "count": A.AGG_COUNT, "sum": A.AGG_SUM, "min": A.AGG_MIN, "max": A.AGG_MAX}


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


def run_group(mgr, cols, key_cols, outs, out_capacity=None, give_workspace=False, count_only=False):
    """-> (row_count, out[(nouts + 1), ocap])"""
    L = lib()
    n, nc, no = len(cols[0]), len(cols), len(outs)
    cap = n + 3
    host_in = np.full((nc, cap), 0x1111111111111111, dtype=np.int64)
    for t, c in enumerate(cols):
        host_in[t, :n] = c
    ocap = n + 5 if out_capacity is None else out_capacity
    d_in = mgr.to_device(host_in.reshape(-1), 0)
    d_out = mgr.to_device(np.full((no + 1) * max(ocap, 1), POISON64, dtype=np.uint64), 0)
    d_rows = mgr.to_device(np.full(1, POISON64, dtype=np.uint64), 0)
    keys = (C.c_int32 * len(key_cols))(*key_cols)
    arr = (A.GroupOut * no)()
    for i, o in enumerate(outs):
        arr[i] = A.GroupOut(o.col, KIND[o.kind], int(o.is_fp), int(o.nullable), 0, A.to_i64(o.null_bits))
    ws = None
    if give_workspace:
        ws = mgr.alloc(L.hdk_hip_group_columns_workspace_bytes(n, no), 0)
    try:
        check(L.hdk_hip_group_columns(d_in.ptr, cap, nc, n, keys, len(key_cols), arr, no, None if count_only else d_out.ptr, ocap,
                                      d_rows.ptr, ws.ptr if ws else None, ws.nbytes if ws else 0, 0, None))
        mgr.synchronizeStream(0)
        rows = int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0])
        out = mgr.to_host(d_out.ptr, (no + 1) * max(ocap, 1) * 8, 0, np.uint64).reshape(no + 1, max(ocap, 1))
        back = mgr.to_host(d_in.ptr, nc * cap * 8, 0, np.int64).reshape(nc, cap)
    finally:
        for b in (d_in, d_out, d_rows, ws):
            if b is not None:
                b.free()
    assert np.array_equal(back, host_in), "the input was modified"
    return rows, out


def check_case(mgr, cols, key_cols, outs, out_capacity=None, give_workspace=False):
    cols = [np.ascontiguousarray(c).view(np.int64) for c in cols]
    n = len(cols[0])
    want, runs = G.group(cols, n, key_cols, outs)
    rows, out = run_group(mgr, cols, key_cols, outs, out_capacity, give_workspace)
    assert rows == runs
    w = runs if out_capacity is None else min(runs, out_capacity)
    for j, o in enumerate(outs):
        got = out[j, :w].view(np.int64)
        if o.kind == "sum" and o.is_fp:
            null = want[j][:w] == np.int64(o.null_bits)
            assert np.array_equal(got == np.int64(o.null_bits), null), (j, o)
            assert np.allclose(got.view(np.float64)[~null], want[j][:w].view(np.float64)[~null], rtol=1e-6, atol=0), (j, o)
        else:
            assert np.array_equal(got, want[j][:w]), (j, o, np.flatnonzero(got != want[j][:w])[:5])
        assert (out[j, w:] == POISON64).all(), (j, o)
    assert (out[len(outs)] == POISON64).all(), "guard column"
    return runs


def keys_from_tails(n, tails):
    """a key column whose runs end exactly at the rows `tails` (and at n - 1)"""
    head = np.zeros(n, dtype=np.int64)
    t = np.asarray(sorted(set(int(x) for x in tails if 0 <= x < n - 1)), dtype=np.int64)
    head[t + 1] = 1
    return np.cumsum(head) * 3 - 11


def run_keys(n, mode, rng):
    if mode == "one":
        return np.full(n, 42, dtype=np.int64)
    if mode == "distinct":
        return np.arange(n, dtype=np.int64) * 5 - 1000
    mean = 3 if mode == "r3" else 300
    lens = rng.integers(1, 2 * mean, 2 * n // mean + 2)  # (twice as many runs as n rows need on average)
    keys = np.repeat(np.arange(len(lens), dtype=np.int64), lens)[:n]
    assert len(keys) == n
    return keys


def int_values(n, rng, null_share=0.3):
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    v[rng.random(n) < null_share] = NULL_I64
    return v


def fp_values(n, rng, null_share=0.3):
    v = bits(rng.integers(1, 4000, n) / 4.0).copy()  # positive: no cancellation in a sum, no -0.0 beside +0.0
    v[rng.random(n) < null_share] = NULL_F64_BITS
    return v


# key column 0, a nullable int column 1 and a nullable double column 2: every kind on both
EVERY_KIND = [Out("id", 0), Out("count", -1), Out("count", 1, False, True, NULL_I64), Out("sum", 1, False, True, NULL_I64),
              Out("min", 1, False, True, NULL_I64), Out("max", 1, False, True, NULL_I64),
              Out("count", 2, True, True, NULL_F64_BITS), Out("sum", 2, True, True, NULL_F64_BITS),
              Out("min", 2, True, True, NULL_F64_BITS), Out("max", 2, True, True, NULL_F64_BITS)]


def every_kind_case(mgr, keys, seed, **kw):
    rng = np.random.default_rng(seed)
    n = len(keys)
    return check_case(mgr, [keys, int_values(n, rng), fp_values(n, rng)], [0], EVERY_KIND, **kw)


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, N])
def test_sizes_and_run_lengths(mgr, n):
    for mode in ("one", "distinct", "r3", "r300"):
        rng = np.random.default_rng(n * 7 + len(mode))
        runs = every_kind_case(mgr, run_keys(n, mode, rng), n + len(mode))
        assert runs == (1 if mode == "one" else n if mode == "distinct" else runs)


@pytest.mark.parametrize("edge", [63, 64, 1023, 1024, 4095, 4096])
def test_runs_that_end_at_an_item_wave_or_tile_boundary(mgr, edge):
    n = 3 * TILE + 77
    tails = [t * TILE + edge for t in range(3)] + [t * TILE + edge - 1 for t in (0, 2)] + [5]
    every_kind_case(mgr, keys_from_tails(n, tails), edge)


def test_a_run_over_three_whole_tiles(mgr):
    n = 5 * TILE + 9
    every_kind_case(mgr, keys_from_tails(n, [TILE - 1, 4 * TILE - 1]), 1)  # exactly tiles 1..3
    every_kind_case(mgr, keys_from_tails(n, [7, 4 * TILE + 700]), 2)  # from tile 0 into tile 4, no tail in 1..3


def test_the_carry_resets_after_a_run_that_ends_with_its_tile(mgr):
    n = 2 * TILE + 100
    every_kind_case(mgr, keys_from_tails(n, [TILE - 1, TILE]), 3)
    every_kind_case(mgr, keys_from_tails(n, [10, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE]), 4)


def test_the_last_row_alone_in_its_tile(mgr):
    n = 2 * TILE + 1
    every_kind_case(mgr, keys_from_tails(n, [100, 2 * TILE - 1]), 5)  # a run of its own
    every_kind_case(mgr, keys_from_tails(n, [100]), 6)  # the end of a run that began in tile 0
    every_kind_case(mgr, np.zeros(n, dtype=np.int64), 7)


def test_no_value_yet_survives_the_tile_carry(mgr):
    n = 2 * TILE
    keys = keys_from_tails(n, [9, n - 6])  # one run from row 10 across both tiles
    rng = np.random.default_rng(11)
    for where in ("first_null", "second_null", "all_null"):
        iv, fv = int_values(n, rng, 0.0), fp_values(n, rng, 0.0)
        lo, hi = {"first_null": (0, TILE), "second_null": (TILE, n), "all_null": (10, n - 5)}[where]
        iv[lo:hi] = NULL_I64
        fv[lo:hi] = NULL_F64_BITS
        check_case(mgr, [keys, iv, fv], [0], EVERY_KIND)
    # a run whose only value is the last row of the second tile, and one whose only value is the first row of the first
    iv = np.full(n, NULL_I64, dtype=np.int64)
    iv[n - 1] = 5
    iv[0] = -7
    check_case(mgr, [np.zeros(n, dtype=np.int64), iv, bits(np.ones(n))], [0], EVERY_KIND)


def test_a_column_that_cannot_be_null_holds_the_sentinel(mgr):
    n = TILE + 50
    rng = np.random.default_rng(12)
    keys = run_keys(n, "r3", rng)
    iv = rng.integers(-5, 5, n).astype(np.int64)
    iv[::4] = NULL_I64
    fv = bits(rng.integers(1, 100, n) / 2.0).copy()
    fv[::5] = NULL_F64_BITS  # DBL_MIN as a value
    outs = [Out("id", 0), Out("count", 1), Out("sum", 1), Out("min", 1), Out("max", 1), Out("count", 2, True), Out("min", 2, True),
            Out("max", 2, True), Out("sum", 2, True)]
    check_case(mgr, [keys, iv, fv], [0], outs)


def test_several_keys_null_keys_and_signed_zeros(mgr):
    n = 2 * TILE + 33
    rng = np.random.default_rng(13)
    k0 = np.full(n, 7, dtype=np.int64)
    k1 = np.repeat(np.arange(n // 50 + 1, dtype=np.int64), 50)[:n]
    k1[(k1 % 7) == 3] = NULL_I64  # NULL keys: NULL equals NULL
    k2 = bits(np.where((np.arange(n) // 5) % 2 == 0, 0.0, -0.0)).copy()  # -0.0 and +0.0 are two keys
    v = int_values(n, rng)
    val = Out("sum", 3, False, True, NULL_I64)
    assert check_case(mgr, [k0, k1, k2, v], [0, 1], [Out("id", 0), Out("id", 1), val]) < n // 40
    assert check_case(mgr, [k0, k1, k2, v], [0, 1, 2], [Out("id", 2), val, Out("id", 0), Out("count", -1), Out("id", 1)]) >= n // 5
    # a key that is not projected; the outs in another order than the columns
    check_case(mgr, [k0, k1, k2, v], [2, 1], [Out("max", 3, False, True, NULL_I64), Out("count", 3, False, True, NULL_I64),
                                              Out("id", 1), Out("min", 3, False, True, NULL_I64)])
    check_case(mgr, [k2], [0], [Out("id", 0)])  # SELECT DISTINCT over adjacent rows


def test_scan_trips(mgr):
    """one more tile than a trip of both scans, plus a one-row tile: a long run across the trip boundary, sparse tails
    beyond it, tile indices >= 4096.  One column: key and argument."""
    n = (TRIP + 1) * TILE + 1
    key = np.arange(n, dtype=np.int64) // 10_007  # runs of 10 007 rows: two tiles and a bit, most tiles with one tail or none
    a, b = 4000 * TILE + 17, TRIP * TILE + 100
    key[a:b] = -5  # 96 tiles and a bit, ending in the first tile of the second trip
    key[b:n - 1] = np.int64(1) << 40  # the rest of the second trip but the last row: its tail is the last row of tile TRIP
    key[b + 2000] = 3  # ... but for two one-row runs in it
    key[n - 1] = 9  # the one-row tile
    nullable = (False, True, int(key[123_456]))  # (the run of that key is all NULL)
    outs = [Out("id", 0), Out("count", -1), Out("sum", 0), Out("min", 0), Out("count", 0, *nullable), Out("max", 0, *nullable)]
    check_case(mgr, [key], [0], outs)


def test_calling_variants(mgr):
    rng = np.random.default_rng(14)
    n = 3 * TILE + 5
    keys = run_keys(n, "r3", rng)
    cols = [keys, int_values(n, rng), fp_values(n, rng)]
    runs = G.group(cols, n, [0], [Out("id", 0)])[1]
    for cap in (1, runs // 2, runs - 1, runs):
        check_case(mgr, cols, [0], EVERY_KIND, out_capacity=cap)
    check_case(mgr, cols, [0], EVERY_KIND, give_workspace=True)
    rows, out = run_group(mgr, cols, [0], EVERY_KIND, count_only=True)
    assert rows == runs and (out == POISON64).all()
    rows, out = run_group(mgr, cols, [0], EVERY_KIND, out_capacity=0)
    assert rows == runs and (out == POISON64).all()


def test_no_rows(mgr):
    L = lib()
    d_in = mgr.to_device(np.zeros(8, dtype=np.int64), 0)
    d_rows = mgr.to_device(np.full(1, POISON64, dtype=np.uint64), 0)
    keys = (C.c_int32 * 1)(0)
    arr = (A.GroupOut * 1)(A.GroupOut(0, A.AGG_ID, 0, 0, 0, 0))
    try:
        check(L.hdk_hip_group_columns(d_in.ptr, 4, 2, 0, keys, 1, arr, 1, None, 0, d_rows.ptr, None, 0, 0, None))
        mgr.synchronizeStream(0)
        assert int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0]) == 0
    finally:
        d_in.free()
        d_rows.free()


def test_int_sum_wraps(mgr):
    n = TILE + 300
    rng = np.random.default_rng(15)
    keys = np.arange(n, dtype=np.int64) // 3  # runs of three: 3 * (2^62 + odd) wraps to an odd word, never the sentinel
    v = (np.int64(1) << 62) + 2 * rng.integers(0, 1000, n).astype(np.int64) + 1
    v[rng.random(n) < 0.5] *= -1
    outs = [Out("sum", 1, False, True, NULL_I64), Out("id", 0), Out("sum", 1)]
    check_case(mgr, [keys, v], [0], outs)
    check_case(mgr, [np.zeros(n, dtype=np.int64), v], [0], outs[1:])  # one run: the sum wraps many times over
