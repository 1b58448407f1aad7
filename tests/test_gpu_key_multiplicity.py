"""hdk_hip_key_multiplicity on the device, through the C ABI, against its numpy statement (tests/multiplicity_expect.py):
both routes at the tile seams, the wave-uniform add, the NULL rules, rows out of range, and what the call leaves alone."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import check, lib

import multiplicity_expect as M
from multiplicity_expect import NULL_I64

pytestmark = pytest.mark.gpu

POISON64 = np.uint64(0x5A5A5A5A5A5A5A5A)
FILL = 0x1111111111111111  # what lies in the capacity behind the rows
TILE = 4096
ROWS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1]
NULL = int(NULL_I64)
DAY = 86400


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


def run(mgr, cols, n, keys, entry_count=0, bucket=1, nulls_match=False, cap_extra=0, own_workspace=False):
    """-> the record (max_matches, occupied, rows_filed, rows_out_of_range); a guard word lies behind the record and the
    workspace, and the input is compared on the way out"""
    L = lib()
    nc = len(cols)
    cap = n + cap_extra
    host = np.full((nc, max(cap, 1)), FILL, dtype=np.int64)
    for t, c in enumerate(cols):
        host[t, :n] = c[:n]
    arr = (A.MultiplicityKey * len(keys))()
    for i, (col, nullable, null_bits, mn, mx, tr) in enumerate(keys):
        arr[i] = A.MultiplicityKey(col, int(nullable), (C.c_uint8 * 3)(), A.to_i64(null_bits), A.to_i64(mn), A.to_i64(mx), A.to_i64(tr))
    flags = A.KEYS_NULLS_MATCH if nulls_match else 0
    d_in = mgr.to_device(host.reshape(-1), 0)
    d_rec = mgr.to_device(np.full(5, POISON64, dtype=np.uint64), 0)
    need = L.hdk_hip_key_multiplicity_workspace_bytes(n, arr, len(keys), entry_count)
    d_ws = mgr.to_device(np.full(need // 8 + 1, POISON64, dtype=np.uint64), 0) if own_workspace else None
    try:
        check(L.hdk_hip_key_multiplicity(d_in.ptr if n else None, cap, nc, n, arr, len(keys), entry_count, bucket, flags, d_rec.ptr,
                                         d_ws.ptr if d_ws else None, need if d_ws else 0, 0, None))
        mgr.synchronizeStream(0)
        rec = mgr.to_host(d_rec.ptr, 40, 0, np.uint64)
        assert rec[4] == POISON64, "the word behind the record"
        assert np.array_equal(mgr.to_host(d_in.ptr, host.size * 8, 0, np.int64).reshape(host.shape), host), "the input was modified"
        if d_ws:
            assert mgr.to_host(d_ws.ptr + need, 8, 0, np.uint64)[0] == POISON64, "the word behind the workspace"
    finally:
        for b in (d_in, d_rec, d_ws):
            if b is not None:
                b.free()
    return tuple(int(x) for x in rec[:4])


def check_call(mgr, cols, n, keys, entry_count=0, bucket=1, nulls_match=False, **kw):
    want = M.expect(cols, n, keys, entry_count, bucket, nulls_match)
    got = run(mgr, cols, n, keys, entry_count, bucket, nulls_match, **kw)
    assert got == want, (n, entry_count, got, want)
    return got


def keyed_column(n, lo, hi, seed, nulls=0.1):
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, hi + 1, n).astype(np.int64)
    a[rng.random(n) < nulls] = NULL_I64
    return a


# ---- both routes at every row count ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_perfect_route_row_counts(mgr, n):
    """a payload column in front of the key, 300 slots; the capacity equal to the rows, then larger with a workspace of the
    caller's; n == 0 leaves an all-zero record"""
    cols = [np.arange(n, dtype=np.int64), keyed_column(n, -100, 199, n + 1)]
    k = M.key(1, True, NULL, -100, 199)
    got = check_call(mgr, cols, n, [k], 300)
    assert got == check_call(mgr, cols, n, [k], 300, cap_extra=7 if n % 2 == 0 else 8, own_workspace=True)
    check_call(mgr, cols, n, [k], 301, nulls_match=True, own_workspace=True)
    if n == 0:
        assert got == (0, 0, 0, 0)


@pytest.mark.parametrize("n", ROWS)
def test_sorted_route_row_counts(mgr, n):
    """input in random order; one component, then two with NULLs in either"""
    cols = [keyed_column(n, 0, 40, n + 2), np.arange(n, dtype=np.int64), keyed_column(n, -2, 2, n + 3)]
    one = check_call(mgr, cols, n, [M.key(0)])
    assert one == check_call(mgr, cols, n, [M.key(0)], cap_extra=9, own_workspace=True)
    check_call(mgr, cols, n, [M.key(2), M.key(0)], own_workspace=True)
    if n == 0:
        assert one == (0, 0, 0, 0)


# ---- the perfect route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entries", [1, 2, 33, 100_000])
def test_perfect_route_entry_counts(mgr, entries):
    n = 2 * TILE + 77
    cols = [keyed_column(n, 5, 5 + entries - 1, entries)]
    got = check_call(mgr, cols, n, [M.key(0, True, NULL, 5, 5 + entries - 1)], entries)
    assert got[3] == 0 and got[1] <= entries
    if entries == 1:
        assert got[0] == got[2] and got[1] == 1


def test_one_key_in_every_row_is_one_add_per_wave(mgr):
    """10 000 rows of one key: every wave item is uniform; max_matches counts them all"""
    n = 10_000
    got = check_call(mgr, [np.full(n, 42, dtype=np.int64)], n, [M.key(0, True, NULL, 0, 99)], 100)
    assert got == (n, 1, n, 0)


def test_a_wave_in_which_all_lanes_but_one_agree(mgr):
    """rows r0 .. r0 + 63 are one wave's item: 63 of them name slot 7, one another slot, a NULL or a word out of range"""
    n = TILE + 500
    for odd_at, odd in ((0, 8), (17, 3), (63, 99), (17, NULL), (5, 1000)):
        a = np.full(n, 7, dtype=np.int64)
        a[256 + odd_at] = odd  # (item 1 of wave 0: rows 256 .. 319)
        a[TILE + 64 + odd_at] = odd
        got = check_call(mgr, [a], n, [M.key(0, True, NULL, 0, 99)], 100)
        assert got[0] == n - 2
    # and a uniform wave whose leading lanes do not file at all
    a = np.full(n, 7, dtype=np.int64)
    a[256:300] = NULL
    assert check_call(mgr, [a], n, [M.key(0, True, NULL, 0, 99)], 100) == (n - 44, 1, n - 44, 0)


def test_sorted_input_with_long_equal_runs(mgr):
    n = 3 * TILE + 1
    a = np.sort(keyed_column(n, 0, 9, 3, nulls=0))
    got = check_call(mgr, [a], n, [M.key(0, True, NULL, 0, 9)], 10)
    assert got[1] == 10 and got[2] == n


def test_all_rows_null(mgr):
    n = TILE + 3
    a = np.full(n, NULL, dtype=np.int64)
    assert check_call(mgr, [a], n, [M.key(0, True, NULL, 0, 9)], 10) == (0, 0, 0, 0)
    assert check_call(mgr, [a], n, [M.key(0, True, NULL, 0, 9)], 11, nulls_match=True) == (n, 1, n, 0)


def test_nulls_filed_under_max_plus_one(mgr):
    n = 5000
    a = keyed_column(n, 10, 20, 9, nulls=0.3)
    nulls = int((a == NULL_I64).sum())
    got = check_call(mgr, [a], n, [M.key(0, True, NULL, 10, 20)], 12, nulls_match=True)
    assert got[0] == nulls and got[2] == n and got[1] == 12
    # a table without the slot for them: the NULLs are out of range, as the build would report
    assert check_call(mgr, [a], n, [M.key(0, True, NULL, 10, 20)], 11, nulls_match=True)[3] == nulls


def test_date_bucket_with_negative_seconds(mgr):
    n = TILE + 100
    rng = np.random.default_rng(4)
    a = (rng.integers(-20, 11, n) * DAY + rng.integers(0, DAY, n)).astype(np.int64)
    a[rng.random(n) < 0.1] = NULL_I64
    vals = a[a != NULL_I64]
    mn, mx = int(vals.min()), int(vals.max())
    entries = -(-(mx - mn + 1) // DAY)
    got = check_call(mgr, [a], n, [M.key(0, True, NULL, mn, mx)], entries, bucket=DAY)
    assert got[3] == 0 and 25 <= got[1] <= entries
    entries = -(-(mx - mn + 2) // DAY)
    check_call(mgr, [a], n, [M.key(0, True, NULL, mn, mx)], entries, bucket=DAY, nulls_match=True)


def test_three_rows_out_of_range(mgr):
    """one word below min_val, one above max_val, one in range whose slot is entry_count"""
    n = 1000
    a = keyed_column(n, 100, 150, 8)
    a[3], a[500], a[999] = 99, 201, 160
    got = check_call(mgr, [a], n, [M.key(0, True, NULL, 100, 200)], 60)
    assert got[3] == 3
    assert got[2] == n - 3 - int((a == NULL_I64).sum())


def test_a_not_nullable_column_holding_the_sentinel(mgr):
    n = 300
    a = np.arange(n, dtype=np.int64)
    a[7] = a[9] = NULL
    # not nullable: the word is a value, and one below min_val
    assert check_call(mgr, [a], n, [M.key(0, False, NULL, 0, n - 1)], n) == (1, n - 2, n - 2, 2)
    assert check_call(mgr, [a], n, [M.key(0, True, NULL, 0, n - 1)], n) == (1, n - 2, n - 2, 0)
    # ... or the smallest value of the range itself
    assert check_call(mgr, [a], n, [M.key(0, False, NULL, NULL, NULL + 10)], 11)[:2] == (2, 1)
    # the sorted route: a value like any other, two equal rows
    assert check_call(mgr, [a], n, [M.key(0, False, NULL)]) == (2, n - 1, n, 0)
    assert check_call(mgr, [a], n, [M.key(0, True, NULL)]) == (1, n - 2, n - 2, 0)


# ---- the sorted route -----------------------------------------------------------------------------------------------------
def test_a_run_that_spans_three_tiles(mgr):
    run_len = 2 * TILE + 10
    n = 3 * TILE + 500
    a = np.arange(n, dtype=np.int64) + 1000  # distinct, all above the run's key
    a[:run_len] = 5  # sorted first: tiles 0 and 1 hold nothing else, tile 2 its last 10 rows
    got = check_call(mgr, [a], n, [M.key(0)])
    assert got == (run_len, n - run_len + 1, n, 0)
    rng = np.random.default_rng(1)
    assert check_call(mgr, [rng.permutation(a)], n, [M.key(0)]) == got
    # the same run at the END of the sorted order: it begins in the middle of a tile
    b = a.copy()
    b[:run_len] = 10**9
    assert check_call(mgr, [rng.permutation(b)], n, [M.key(0)]) == got


def test_a_run_that_ends_at_a_tile_seam(mgr):
    n = 2 * TILE + 7
    a = np.arange(n, dtype=np.int64) + 10_000
    a[:100] = 1  # sorted: rows 0 .. 99
    a[100:TILE] = 2  # rows 100 .. 4095: ends with the tile
    a[TILE:TILE + 64] = 3  # begins with the next, ends with a wave's item
    got = check_call(mgr, [np.random.default_rng(2).permutation(a)], n, [M.key(0)])
    assert got[0] == TILE - 100 and got[1] == 3 + n - TILE - 64


def test_every_row_distinct_and_every_row_equal(mgr):
    n = 2 * TILE + 65
    distinct = np.random.default_rng(6).permutation(n).astype(np.int64)
    assert check_call(mgr, [distinct], n, [M.key(0)]) == (1, n, n, 0)
    assert check_call(mgr, [np.full(n, -3, dtype=np.int64)], n, [M.key(0)]) == (n, 1, n, 0)
    assert check_call(mgr, [np.full(n, NULL, dtype=np.int64)], n, [M.key(0)]) == (0, 0, 0, 0)


def test_the_longest_run_carries_a_null(mgr):
    """the most frequent (a, b) holds a NULL in b: the answer is the next longest"""
    n = TILE + 900
    rng = np.random.default_rng(12)
    a = rng.integers(0, 50, n).astype(np.int64)
    b = rng.integers(0, 3, n).astype(np.int64)
    a[:700], b[:700] = 9, NULL
    a[700:1100], b[700:1100] = 9, 1
    p = rng.permutation(n)
    got = check_call(mgr, [a[p], b[p]], n, [M.key(0), M.key(1)])
    assert 400 <= got[0] < 700 and got[2] == n - 700
    # with b not nullable the NULL word is a value and the 700 rows are the answer
    assert check_call(mgr, [a[p], b[p]], n, [M.key(0), M.key(1, False)])[0] == 700


@pytest.mark.parametrize("nk", [1, 2, 3])
def test_component_counts(mgr, nk):
    """the key columns in any order among others; a key that differs only in its last component is another key"""
    n = 2 * TILE + 333
    rng = np.random.default_rng(20 + nk)
    cols = [keyed_column(n, 0, 3, 30 + j, nulls=0.05) for j in range(3)] + [rng.integers(0, 2**40, n).astype(np.int64)]
    order = [2, 0, 1][:nk]
    got = check_call(mgr, cols, n, [M.key(c) for c in order])
    assert got[1] <= 4 ** nk
    assert got == check_call(mgr, cols, n, [M.key(c) for c in order], own_workspace=True, cap_extra=31)


def test_a_single_key_with_a_range_beyond_a_perfect_table(mgr):
    n = TILE + 1
    a = np.random.default_rng(7).integers(-2**62, 2**62, n).astype(np.int64)
    a[1::2] = a[0]
    assert check_call(mgr, [a], n, [M.key(0)])[0] == 1 + n // 2
