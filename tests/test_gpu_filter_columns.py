"""hdk_hip_filter_columns on raw uploaded columns: HAVING over dense 8-byte columns in HBM.  The expectation is
tests/having_expect.py (numpy, checked against SQLite and the truth tables in test_filter_columns_cpu.py).  Every case
asserts row_count, every output column, perm_out, the poison beyond the output rows and in a guard column, and an
untouched input -- exactly."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import check, lib

import having_expect as H
from having_expect import INT64_MAX, INT64_MIN, NULL_DOUBLE_BITS, col_leaf, dbits, lit_leaf

pytestmark = pytest.mark.gpu

POISON64 = np.uint64(0x5A5A5A5A5A5A5A5A)
POISON32 = np.uint32(0x5A5A5A5A)
TILE = 4096  # rows per tile (hdk_amd/csrc/filter_columns.hip: kFcTile)
N = 200_003
INT = (False, False, 0)


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


def run_filter(mgr, cols, leaves, prog, out_capacity=None, give_workspace=False, count_only=False):
    """-> (row_count, out[(nc + 1), ocap] or None, perm[ocap] or None)"""
    L = lib()
    n, nc = len(cols[0]), len(cols)
    cap = n + 3
    host_in = np.full((nc, cap), 0x1111111111111111, dtype=np.int64)
    for t, c in enumerate(cols):
        host_in[t, :n] = c
    ocap = n + 5 if out_capacity is None else out_capacity
    d_in = mgr.to_device(host_in.reshape(-1), 0)
    d_out = mgr.to_device(np.full((nc + 1) * max(ocap, 1), POISON64, dtype=np.uint64), 0)
    d_perm = mgr.to_device(np.full(max(ocap, 1), POISON32, dtype=np.uint32), 0)
    d_rows = mgr.to_device(np.full(1, POISON64, dtype=np.uint64), 0)
    arr = (A.HavingLeaf * len(leaves))()
    for i, lf in enumerate(leaves):
        arr[i] = A.HavingLeaf(lf.lhs_col, lf.rhs_col, lf.cmp, int(lf.rhs_is_col), int(lf.cmp_fp), int(lf.lhs_is_fp),
                              int(lf.lhs_nullable), int(lf.rhs_is_fp), int(lf.rhs_nullable), 0, A.to_i64(lf.lhs_null_bits),
                              A.to_i64(lf.rhs_null_bits), A.to_i64(lf.rhs_lit))
    ops = (C.c_uint8 * max(len(prog), 1))(*prog)
    ws = None
    if give_workspace:
        ws = mgr.alloc(L.hdk_hip_filter_columns_workspace_bytes(n), 0)
    try:
        check(L.hdk_hip_filter_columns(d_in.ptr, cap, nc, n, arr, len(leaves), ops, len(prog), None if count_only else d_out.ptr,
                                       ocap, d_rows.ptr, None if count_only else d_perm.ptr, ws.ptr if ws else None,
                                       ws.nbytes if ws else 0, 0, None))
        mgr.synchronizeStream(0)
        rows = int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0])
        out = mgr.to_host(d_out.ptr, (nc + 1) * max(ocap, 1) * 8, 0, np.uint64).reshape(nc + 1, max(ocap, 1))
        perm = mgr.to_host(d_perm.ptr, max(ocap, 1) * 4, 0, np.uint32)
        back = mgr.to_host(d_in.ptr, nc * cap * 8, 0, np.int64).reshape(nc, cap)
    finally:
        for b in (d_in, d_out, d_perm, d_rows, ws):
            if b is not None:
                b.free()
    assert np.array_equal(back, host_in), "the input was modified"
    return rows, out, perm


def check_case(mgr, cols, leaves, prog, out_capacity=None, give_workspace=False, want=None):
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in cols]
    if want is None:
        want = H.expected_rows(cols, leaves, prog)
    rows, out, perm = run_filter(mgr, cols, leaves, prog, out_capacity, give_workspace)
    assert rows == len(want)
    w = len(want) if out_capacity is None else min(len(want), out_capacity)
    assert np.array_equal(perm[:w], want[:w])
    assert (perm[w:] == POISON32).all()
    for t, c in enumerate(cols):
        assert np.array_equal(out[t, :w].view(np.int64), c[want[:w]]), t
        assert (out[t, w:] == POISON64).all(), t
    assert (out[len(cols)] == POISON64).all(), "guard column"
    return want


def _selectivity_case(n, sel):
    """two columns and one leaf on the first with the wanted selectivity"""
    rng = np.random.default_rng(n * 31 + len(sel))
    k = rng.integers(0, 1000, n).astype(np.int64)
    v = np.arange(n, dtype=np.int64) * 3 - 7
    if sel == "none":
        lf = lit_leaf(0, A.CMP_LT, 0)
    elif sel == "all":
        lf = lit_leaf(0, A.CMP_GE, 0)
    elif sel == "half":
        lf = lit_leaf(0, A.CMP_LT, 500)
    elif sel == "thousandth":
        lf = lit_leaf(0, A.CMP_EQ, 7)
    else:  # exactly one tile in the middle has passing rows
        mid = (n // TILE) // 2
        k[:] = 5
        k[mid * TILE:(mid + 1) * TILE][::3] = 2000
        lf = lit_leaf(0, A.CMP_GT, 1000)
    return [k, v], [lf]


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, N, 1_100_003])
def test_sizes_and_selectivities(mgr, n):
    for sel in ("none", "all", "half", "thousandth", "one_tile"):
        cols, leaves = _selectivity_case(n, sel)
        want = check_case(mgr, cols, leaves, [])
        if sel == "none":
            assert len(want) == 0
        if sel == "all":
            assert len(want) == n
        if sel == "one_tile" and n > 3 * TILE:
            assert 0 < len(want) <= TILE and want[0] // TILE == want[-1] // TILE == (n // TILE) // 2


SCAN_TRIP = 4096  # tile counts hdk_counts_scan<4> takes per trip (1 024 threads x kFcScanPer): 16.7 M rows


@pytest.mark.parametrize("sel", ["sparse", "one_tile_in_the_second_trip", "last_rows_only"])
def test_more_tiles_than_one_scan_trip(mgr, sel):
    """A whole trip of the one-block scan plus two tiles, the second of them holding one row: the carry from trip to
    trip, the tail of the later trip, and tile indices at and beyond 4096 in the count and compact passes."""
    n = SCAN_TRIP * TILE + TILE + 1
    rng = np.random.default_rng(len(sel))
    if sel == "sparse":  # about one row in 1000, in every tile, the very last row among them
        k = rng.integers(0, 1000, n).astype(np.int64)
        k[-1] = 7
        cols, leaf = [k, np.arange(n, dtype=np.int64) * 5 - 11], lit_leaf(0, A.CMP_EQ, 7)
    elif sel == "one_tile_in_the_second_trip":  # every tile before it is skipped unread by the compact pass
        k = np.full(n, 5, dtype=np.int64)
        k[SCAN_TRIP * TILE:(SCAN_TRIP + 1) * TILE][::3] = 2000
        cols, leaf = [k], lit_leaf(0, A.CMP_GT, 1000)
    else:  # a few rows at the end of the first trip's last tile, and the single row of the last tile
        k = np.full(n, 5, dtype=np.int64)
        k[SCAN_TRIP * TILE - 3:SCAN_TRIP * TILE] = 2000
        k[-1] = 2000
        cols, leaf = [k], lit_leaf(0, A.CMP_GT, 1000)
    want = H.expected_rows(cols, [leaf], [])
    assert 0 < len(want) < n // 500 and want[-1] == n - 1 or sel == "one_tile_in_the_second_trip"
    assert want[-1] >= SCAN_TRIP * TILE  # (kept rows beyond the first trip)
    check_case(mgr, cols, [leaf], [], out_capacity=len(want) + 5, want=want)


@pytest.mark.parametrize("n", [65, TILE + 1, N])
def test_out_capacity_below_the_passing_rows(mgr, n):
    cols, leaves = _selectivity_case(n, "half")
    want = H.expected_rows(cols, leaves, [])
    for ocap in sorted({0, 1, len(want) // 2, len(want) - 1}):
        if 0 <= ocap < len(want):
            check_case(mgr, cols, leaves, [], out_capacity=ocap, want=want)


@pytest.mark.parametrize("n", [1, TILE + 1, N])
def test_count_only_and_workspace(mgr, n):
    for sel in ("half", "one_tile", "none"):
        cols, leaves = _selectivity_case(n, sel)
        want = check_case(mgr, cols, leaves, [])
        assert np.array_equal(check_case(mgr, cols, leaves, [], give_workspace=True), want)
        for give in (False, True):
            rows, out, perm = run_filter(mgr, cols, leaves, [], give_workspace=give, count_only=True)
            assert rows == len(want)
            assert (out == POISON64).all() and (perm == POISON32).all()


def test_zero_rows_store_a_zero_count(mgr):
    L = lib()
    d_rows = mgr.to_device(np.full(1, POISON64, dtype=np.uint64), 0)
    d_in = mgr.to_device(np.zeros(8, dtype=np.int64), 0)
    arr = (A.HavingLeaf * 1)(A.HavingLeaf(0, 0, A.CMP_GT, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5))
    try:
        check(L.hdk_hip_filter_columns(d_in.ptr, 4, 2, 0, arr, 1, None, 0, None, 0, d_rows.ptr, None, None, 0, 0, None))
        mgr.synchronizeStream(0)
        assert int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0]) == 0
    finally:
        d_rows.free()
        d_in.free()


_INTS = [INT64_MIN, INT64_MIN + 1, -2, -1, 0, 1, 2, (1 << 53), (1 << 53) + 1, INT64_MAX - 1, INT64_MAX, NULL_DOUBLE_BITS]
_FPS = [0.0, -0.0, 1.0, -1.0, 0.5, float("inf"), float("-inf"), float("nan"), -float("nan"), 1e300, 9.007199254740992e15,
        -9.223372036854775808e18, 9.223372036854775808e18, float(np.int64(NULL_DOUBLE_BITS).view(np.float64))]


def _cross(kind_l, kind_r):
    """every value of the left pool against every value of the right pool, as two columns (+ a payload)"""
    lv = np.array(_INTS, dtype=np.int64) if kind_l == "int" else np.array(_FPS, dtype=np.float64).view(np.int64)
    rv = np.array(_INTS, dtype=np.int64) if kind_r == "int" else np.array(_FPS, dtype=np.float64).view(np.int64)
    a = np.repeat(lv, len(rv))
    b = np.tile(rv, len(lv))
    return [a, b, np.arange(len(a), dtype=np.int64)], rv


@pytest.mark.parametrize("kinds", [("int", "int"), ("fp", "fp"), ("int", "fp"), ("fp", "int")])
def test_every_cmp_nullability_and_kind(mgr, kinds):
    """every cmp x {int, fp, mixed} x {nullable lhs, nullable rhs, both, neither}, column and literal right-hand sides.  A
    non-nullable column holds the NULL sentinels as ordinary values."""
    kl, kr = kinds
    cols, rvals = _cross(kl, kr)
    null_of = {"int": INT64_MIN, "fp": NULL_DOUBLE_BITS}
    for cmp in range(A.CMP_EQ, A.CMP_GE + 1):
        for ln in (False, True):
            li = (kl == "fp", ln, null_of[kl])
            for rn in (False, True):
                ri = (kr == "fp", rn, null_of[kr])
                check_case(mgr, cols, [col_leaf(0, cmp, 1, li, ri)], [])
            # literals: three a call (the middle one negated), so that every value of the right pool is a literal once
            lits = [float(np.int64(v).view(np.float64)) if kr == "fp" else int(v) for v in rvals]
            for i in range(0, len(lits), 3):
                leaves = [lit_leaf(0, cmp, x, li) for x in lits[i:i + 3]]
                prog = {1: [0], 2: [0, 1, A.F_NOT, A.F_OR], 3: [0, 1, A.F_NOT, A.F_OR, 2, A.F_OR]}[len(leaves)]
                check_case(mgr, cols, leaves, prog)


def test_signed_zeros_and_nans_follow_the_c_operators(mgr):
    nan = float("nan")
    c = np.array([0.0, -0.0, nan, float("inf"), -float("inf"), 1.0], dtype=np.float64).view(np.int64)
    info = (True, False, 0)
    for cmp, lit, want in ((A.CMP_EQ, -0.0, [0, 1]), (A.CMP_EQ, 0.0, [0, 1]), (A.CMP_NE, nan, [0, 1, 2, 3, 4, 5]), (A.CMP_EQ, nan, []),
                           (A.CMP_LE, nan, []), (A.CMP_GE, nan, []), (A.CMP_LT, 1.0, [0, 1, 4]), (A.CMP_NE, 1.0, [0, 1, 2, 3, 4])):
        got = check_case(mgr, [c], [lit_leaf(0, cmp, lit, info)], [])
        assert got.tolist() == want, (cmp, lit)
    # the column against itself: NaN <> NaN, everything else equal
    assert check_case(mgr, [c], [col_leaf(0, A.CMP_NE, 0, info, info)], []).tolist() == [2]


def _program_cols(n):
    rng = np.random.default_rng(4242)
    cols = [rng.integers(-4, 5, n).astype(np.int64) for _ in range(3)]
    cols[1][rng.random(n) < 0.25] = INT64_MIN  # nullable
    cols.append((rng.integers(-4, 5, n) / 2).astype(np.float64).view(np.int64))
    cols[3][rng.random(n) < 0.25] = NULL_DOUBLE_BITS
    return cols


@pytest.mark.parametrize("name", ["conjunction", "a_or_b", "not_a", "not_a_and_b_or_c", "eight_leaves", "eight_leaves_program",
                                  "same_column_twice"])
def test_programs(mgr, name):
    n = 3 * TILE + 77
    cols = _program_cols(n)
    nul = (False, True, INT64_MIN)
    fnul = (True, True, NULL_DOUBLE_BITS)
    a, b, c = lit_leaf(0, A.CMP_GT, 0), lit_leaf(1, A.CMP_LE, 1, nul), lit_leaf(3, A.CMP_LT, 0.5, fnul)
    eight = [a, b, c, lit_leaf(2, A.CMP_NE, 3), col_leaf(0, A.CMP_GE, 2), col_leaf(1, A.CMP_NE, 3, nul, fnul), lit_leaf(0, A.CMP_LT, 4),
             lit_leaf(3, A.CMP_GE, -1.5, fnul)]
    leaves, prog = {
        "conjunction": ([a, b, c], []),
        "a_or_b": ([a, b], [0, 1, A.F_OR]),
        "not_a": ([b], [0, A.F_NOT]),
        "not_a_and_b_or_c": ([a, b, c], [0, 1, A.F_AND, A.F_NOT, 2, A.F_OR]),
        "eight_leaves": (eight, []),
        # all eight pushed before the first operator: the deepest stack a program can ask for
        "eight_leaves_program": (eight, [0, 1, 2, 3, 4, 5, 6, 7, A.F_OR, A.F_AND, A.F_OR, A.F_AND, A.F_OR, A.F_AND, A.F_OR, A.F_NOT]),
        # leaves on one column that are not neighbours in the caller's order
        "same_column_twice": ([lit_leaf(0, A.CMP_GT, -2), b, lit_leaf(0, A.CMP_LT, 3)], [0, 1, A.F_OR, 2, A.F_AND]),
    }[name]
    want = check_case(mgr, cols, leaves, prog)
    if name != "eight_leaves":
        assert 0 < len(want) < n


@pytest.mark.parametrize("seed", range(20))
def test_fuzz(mgr, seed):
    rng = np.random.default_rng(7700 + seed)
    n = 50_000 + int(rng.integers(0, 100))
    cols, infos, leaves, tree, prog = H.random_case(rng, n, ncols=int(rng.integers(1, 6)))
    check_case(mgr, cols, leaves, prog, give_workspace=bool(seed % 2))
