"""hdk_hip_sort_columns on raw uploaded columns: ORDER BY / LIMIT / OFFSET over dense 8-byte columns in HBM.  The
expectation is tests/sort_expect.py (stable numpy, checked against the reference's comparator in
test_sort_columns_cpu.py).  Every case runs with the top-N selection allowed and with HDK_HIP_SORT_NO_SELECT, and asserts
the permutation and every output column exactly, the poison beyond out_rows and in a guard column, and an untouched
input."""
import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import check, lib

from sort_expect import INT64_MAX, INT64_MIN, NULL_DOUBLE_BITS, dbits, expected_perm, out_rows_of

pytestmark = pytest.mark.gpu

POISON64 = np.uint64(0x5A5A5A5A5A5A5A5A)
POISON32 = np.uint32(0x5A5A5A5A)
TILE = 4096  # rows per tile of the sort kernels (hdk_amd/csrc/sort_columns.hip: kScTile)
N = 200_003


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


def run_sort(mgr, cols, order, limit, offset, flags, give_workspace=False):
    L = lib()
    n, nc = len(cols[0]), len(cols)
    cap = n + 3
    host_in = np.full((nc, cap), 0x1111111111111111, dtype=np.int64)
    for t, c in enumerate(cols):
        host_in[t, :n] = c
    out_rows = out_rows_of(n, limit, offset)
    ocap = out_rows + 5
    d_in = mgr.to_device(host_in.reshape(-1), 0)
    d_out = mgr.to_device(np.full((nc + 1) * ocap, POISON64, dtype=np.uint64), 0)
    d_perm = mgr.to_device(np.full(ocap, POISON32, dtype=np.uint32), 0)
    arr = (A.OrderEntry * len(order))()
    for i, (col, desc, nulls_first, is_fp, nullable, null_bits) in enumerate(order):
        arr[i] = A.OrderEntry(col, int(desc), int(nulls_first), int(is_fp), int(nullable), A.to_i64(null_bits))
    ws = None
    if give_workspace:
        nb = L.hdk_hip_sort_columns_workspace_bytes(n, len(order))
        ws = mgr.alloc(nb, 0)
    try:
        check(L.hdk_hip_sort_columns(d_in.ptr, cap, nc, n, arr, len(order), offset, limit, flags, d_out.ptr, ocap, d_perm.ptr,
                                     ws.ptr if ws else None, ws.nbytes if ws else 0, 0, None))
        mgr.synchronizeStream(0)
        out = mgr.to_host(d_out.ptr, (nc + 1) * ocap * 8, 0, np.uint64).reshape(nc + 1, ocap)
        perm = mgr.to_host(d_perm.ptr, ocap * 4, 0, np.uint32)
        back = mgr.to_host(d_in.ptr, nc * cap * 8, 0, np.int64).reshape(nc, cap)
    finally:
        for b in (d_in, d_out, d_perm, ws):
            if b is not None:
                b.free()
    assert np.array_equal(back, host_in), "the input was modified"
    return out, perm, out_rows


def check_case(mgr, cols, order, limit=0, offset=0, give_workspace=False, want_perm=None):
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in cols]
    full = expected_perm(cols, order) if want_perm is None else want_perm
    for flags in (0, A.SORT_NO_SELECT):
        out, perm, out_rows = run_sort(mgr, cols, order, limit, offset, flags, give_workspace)
        want = full[offset:offset + out_rows]
        assert len(want) == out_rows
        assert np.array_equal(perm[:out_rows], want), (flags, limit, offset)
        assert (perm[out_rows:] == POISON32).all(), flags
        for t, c in enumerate(cols):
            assert np.array_equal(out[t, :out_rows].view(np.int64), c[want]), (flags, t)
            assert (out[t, out_rows:] == POISON64).all(), (flags, t)
        assert (out[len(cols)] == POISON64).all(), "guard column"


def asc(col=0, nullable=False, null_bits=INT64_MIN):
    return (col, False, False, False, nullable, null_bits)


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, N, 1_100_003])
def test_sizes(mgr, n):
    rng = np.random.default_rng(n)
    k = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
    v = np.arange(n, dtype=np.int64) * 3
    full = expected_perm([k, v], [asc()])
    check_case(mgr, [k, v], [asc()], want_perm=full)
    check_case(mgr, [k, v], [asc()], limit=max(1, n // 16), want_perm=full)  # (small enough for the selection)


def _shapes():
    rng = np.random.default_rng(77)
    r = rng.integers(0, 256, N).astype(np.int64)
    return {
        "all_equal": np.full(N, 42, dtype=np.int64),
        "sorted": np.arange(N, dtype=np.int64) - 1000,
        "reversed": (np.arange(N, dtype=np.int64) - 1000)[::-1].copy(),
        "full_range": rng.integers(INT64_MIN, INT64_MAX, N, dtype=np.int64, endpoint=True),
        "top_byte": (r - 128) << 56,
        "middle_byte": (r << 24) + 5,
        "below_2_24_ties": rng.integers(0, 1 << 24, N // 50).astype(np.int64)[rng.integers(0, N // 50, N)],
    }


@pytest.mark.parametrize("shape", ["all_equal", "sorted", "reversed", "full_range", "top_byte", "middle_byte", "below_2_24_ties"])
def test_key_shapes(mgr, shape):
    k = _shapes()[shape]
    v = np.arange(N, dtype=np.int64)[::-1].copy()
    full = expected_perm([k, v], [asc()])
    if shape in ("all_equal", "sorted"):
        assert np.array_equal(full, np.arange(N, dtype=np.uint32))  # no live digit / nothing to move: the identity
    check_case(mgr, [k, v], [asc()], want_perm=full)
    check_case(mgr, [k, v], [asc()], limit=10, want_perm=full)
    check_case(mgr, [k, v], [(0, True, False, False, False, 0)], limit=10, offset=7)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
def test_int_extremes_next_to_nulls(mgr, desc, nulls_first):
    rng = np.random.default_rng(5)
    k = rng.integers(-5, 5, N).astype(np.int64)
    k[rng.random(N) < 0.1] = INT64_MAX
    k[rng.random(N) < 0.1] = INT64_MIN + 1
    k[rng.random(N) < 0.1] = INT64_MIN  # NULL
    k[rng.random(N) < 0.05] = INT64_MAX - 1
    order = [(0, desc, nulls_first, False, True, INT64_MIN)]
    full = expected_perm([k], order)
    check_case(mgr, [k], order, want_perm=full)
    # a LIMIT that ends inside the first class and one that ends inside the last
    check_case(mgr, [k], order, limit=100, want_perm=full)
    check_case(mgr, [k], order, limit=N // 10, offset=11, want_perm=full)


def _doubles(rng, n):
    d = rng.normal(size=n) * 1e6
    d[rng.random(n) < 0.05] = np.inf
    d[rng.random(n) < 0.05] = -np.inf
    d[rng.random(n) < 0.05] = 5e-324
    d[rng.random(n) < 0.05] = -5e-324
    d[rng.random(n) < 0.1] = 2.2250738585072014e-308  # NULL_DOUBLE, or DBL_MIN as a value
    d[d == 0] = 3.0
    return d.view(np.int64).copy()


@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("desc,nulls_first", [(False, False), (True, True), (True, False)])
def test_doubles(mgr, nullable, desc, nulls_first):
    d = _doubles(np.random.default_rng(9), N)
    order = [(0, desc, nulls_first, True, nullable, NULL_DOUBLE_BITS)]
    full = expected_perm([d], order)
    check_case(mgr, [d], order, want_perm=full)
    check_case(mgr, [d], order, limit=10, offset=3, want_perm=full)


def test_signed_zero_and_nan_take_the_documented_order(mgr):
    """include/hdk_hip.h: -0.0 before +0.0; NaNs by bit pattern beyond the infinities (sign set: before -inf; clear: after
    +inf).  Ties in ascending row."""
    classes = [dbits(np.nan) | (1 << 63), dbits(-np.inf), dbits(-1.0), dbits(-0.0), dbits(0.0), dbits(1.0), dbits(np.inf),
               dbits(np.nan)]
    classes = [A.to_i64(c) for c in classes]
    rng = np.random.default_rng(3)
    which = rng.integers(0, len(classes), 10_007)
    d = np.array(classes, dtype=np.int64)[which]
    asc_perm = np.argsort(which, kind="stable").astype(np.uint32)
    desc_perm = np.argsort(-which, kind="stable").astype(np.uint32)
    check_case(mgr, [d], [(0, False, False, True, False, 0)], want_perm=asc_perm)
    check_case(mgr, [d], [(0, True, False, True, False, 0)], want_perm=desc_perm)
    check_case(mgr, [d], [(0, False, False, True, False, 0)], limit=10, want_perm=asc_perm)


def _three(rng, n):
    a = rng.integers(0, 7, n).astype(np.int64)           # heavy primary ties
    a[rng.random(n) < 0.1] = INT64_MIN
    d = _doubles(rng, n)
    c = rng.integers(-1000, 1000, n).astype(np.int64)
    return [a, d, c]


@pytest.mark.parametrize("give_workspace", [False, True])
def test_two_and_three_entries(mgr, give_workspace):
    cols = _three(np.random.default_rng(21), N)
    two = [(0, True, False, False, True, INT64_MIN), (1, False, True, True, True, NULL_DOUBLE_BITS)]
    three = [(0, False, True, False, True, INT64_MIN), (2, True, False, False, False, 0), (1, True, False, True, True, NULL_DOUBLE_BITS)]
    for order in (two, three):
        full = expected_perm(cols, order)
        check_case(mgr, cols, order, give_workspace=give_workspace, want_perm=full)
        check_case(mgr, cols, order, limit=10, give_workspace=give_workspace, want_perm=full)


@pytest.mark.parametrize("limit", ["1", "10", "n", "n+5"])
def test_limits_and_offsets(mgr, limit):
    n = 5003
    cols = _three(np.random.default_rng(22), n)
    order = [(0, False, False, False, True, INT64_MIN), (2, True, False, False, False, 0)]
    full = expected_perm(cols, order)
    lim = {"1": 1, "10": 10, "n": n, "n+5": n + 5}[limit]
    for offset in (0, 7, n - 1, n, n + 1):
        check_case(mgr, cols, order, limit=lim, offset=offset, want_perm=full)
    # a limit over keys without any sortable difference: the first rows as they are
    same = [np.full(n, 9, dtype=np.int64), cols[2]]
    check_case(mgr, same, [asc()], limit=lim, offset=7, want_perm=np.arange(n, dtype=np.uint32))


def test_ties_at_the_threshold_go_to_the_second_entry(mgr):
    """5 rows below, then 1 000 rows that share the 10th primary key: the second entry decides who is in."""
    rng = np.random.default_rng(31)
    a = rng.integers(100, 1 << 40, N).astype(np.int64)
    where = rng.permutation(N)
    a[where[:5]] = 0
    a[where[5:1005]] = 1
    b = rng.integers(-50, 50, N).astype(np.int64)
    order = [asc(0), (1, True, False, False, False, 0)]
    full = expected_perm([a, b], order)
    assert (a[full[5:1005]] == 1).all()
    check_case(mgr, [a, b], order, limit=10, want_perm=full)
    check_case(mgr, [a, b], order, limit=10, offset=3, want_perm=full)


def test_eight_columns_three_entries(mgr):
    rng = np.random.default_rng(41)
    n = 50_021
    cols = _three(rng, n) + [rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64) for _ in range(5)]
    order = [(2, False, False, False, False, 0), (0, True, True, False, True, INT64_MIN), (1, False, False, True, True, NULL_DOUBLE_BITS)]
    full = expected_perm(cols, order)
    check_case(mgr, cols, order, want_perm=full)
    check_case(mgr, cols, order, limit=10, offset=7, want_perm=full)
