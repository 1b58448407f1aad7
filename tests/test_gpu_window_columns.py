"""hdk_hip_window_columns on raw uploaded columns: window functions over dense 8-byte columns in HBM.  The expectation is
tests/window_expect.py (numpy, checked against SQLite in test_window_columns_cpu.py).  Every case asserts every output
column, the poison beyond num_rows and in a guard column, and an untouched input.  Everything is compared word for word
(PERCENT_RANK and CUME_DIST too: a double division without fast-math is correctly rounded), except a SUM or AVG of
doubles: 1e-6 relative, on positive values (the association of the sum is unspecified).  RANGE and PARTITION outputs must
in addition be bit-identical across their peer group or partition."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import check, lib

import window_expect as W
from window_expect import FRAMES, KINDS, NULL_F64_BITS, NULL_I64, WOut, bits

pytestmark = pytest.mark.gpu

POISON64 = np.uint64(0x5A5A5A5A5A5A5A5A)
TILE = 4096  # rows per tile (hdk_amd/csrc/column_segments.h: kGcTile); a wave owns 1024 of them, an item 64
TRIP = 4096  # tiles per trip of hdk_counts_scan<4> and of the carry scan (kGcCarryTrip)
N = 200_003
INT_NULLABLE = (False, True, NULL_I64)
FP_NULLABLE = (True, True, NULL_F64_BITS)


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


def run_window(mgr, cols, part_cols, order_cols, outs, extra_capacity=5, give_workspace=False):
    """-> out[(nouts + 1), ocap]"""
    L = lib()
    n, nc, no = len(cols[0]), len(cols), len(outs)
    cap = n + 3
    host_in = np.full((nc, cap), 0x1111111111111111, dtype=np.int64)
    for t, c in enumerate(cols):
        host_in[t, :n] = c
    ocap = n + extra_capacity
    d_in = mgr.to_device(host_in.reshape(-1), 0)
    d_out = mgr.to_device(np.full((no + 1) * max(ocap, 1), POISON64, dtype=np.uint64), 0)
    pc = (C.c_int32 * max(len(part_cols), 1))(*part_cols)
    oc = (C.c_int32 * max(len(order_cols), 1))(*order_cols)
    arr = (A.WindowOut * no)()
    for i, o in enumerate(outs):
        arr[i] = A.WindowOut(o.col, KINDS.index(o.kind), FRAMES.index(o.frame), int(o.is_fp), int(o.nullable), A.to_i64(o.null_bits),
                             int(o.param))
    ws = None
    if give_workspace:
        ws = mgr.alloc(L.hdk_hip_window_columns_workspace_bytes(n, no), 0)
    try:
        check(L.hdk_hip_window_columns(d_in.ptr, cap, nc, n, pc if part_cols else None, len(part_cols), oc if order_cols else None,
                                       len(order_cols), arr, no, d_out.ptr, ocap, ws.ptr if ws else None, ws.nbytes if ws else 0, 0,
                                       None))
        mgr.synchronizeStream(0)
        out = mgr.to_host(d_out.ptr, (no + 1) * max(ocap, 1) * 8, 0, np.uint64).reshape(no + 1, max(ocap, 1))
        back = mgr.to_host(d_in.ptr, nc * cap * 8, 0, np.int64).reshape(nc, cap)
    finally:
        for b in (d_in, d_out, ws):
            if b is not None:
                b.free()
    assert np.array_equal(back, host_in), "the input was modified"
    return out


def check_case(mgr, cols, part_cols, order_cols, outs, **kw):
    cols = [np.ascontiguousarray(c).view(np.int64) for c in cols]
    n = len(cols[0])
    want = W.window(cols, n, part_cols, order_cols, outs)
    # the first row of every row's partition and peer group, for the bit-identity of RANGE and PARTITION outputs
    firsts = {"partition": W.window(cols, n, part_cols, [], [WOut("row_number")])[0],
              "range": W.window(cols, n, part_cols + order_cols, [], [WOut("row_number")])[0]}
    for lo in range(0, len(outs), A.MAX_WINDOW_OUTS):  # (a call takes eight outs)
        part = outs[lo:lo + A.MAX_WINDOW_OUTS]
        out = run_window(mgr, cols, part_cols, order_cols, part, **kw)
        for j, o in enumerate(part):
            got, exp = out[j, :n].view(np.int64), want[lo + j]
            if o.kind in ("sum", "avg") and o.is_fp:
                null_bits = np.int64(NULL_F64_BITS if o.kind == "avg" else o.null_bits)
                null = exp == null_bits
                assert np.array_equal(got == null_bits, null), (j, o)
                assert np.allclose(got.view(np.float64)[~null], exp.view(np.float64)[~null], rtol=1e-6, atol=0), (j, o)
            else:
                assert np.array_equal(got, exp), (lo + j, o, np.flatnonzero(got != exp)[:5])
            if o.kind in W.AGGREGATES and o.frame != "rows":
                head = np.arange(n) - (firsts[o.frame] - 1)
                assert np.array_equal(got, got[head]), (j, o, "not one word per " + o.frame)
            assert (out[j, n:] == POISON64).all(), (j, o)
        assert (out[len(part)] == POISON64).all(), "guard column"


def keys_from_tails(n, tails):
    """a key column whose stretches end exactly at the rows `tails` (and at n - 1)"""
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
    lens = rng.integers(1, 2 * mean, 2 * n // mean + 2)  # (twice as many stretches as n rows need on average)
    keys = np.repeat(np.arange(len(lens), dtype=np.int64), lens)[:n]
    assert len(keys) == n
    return keys


def order_with_ties(part, rng, mean=2):
    """an order key that is sorted inside every partition of `part` and has ties: peer groups of about `mean` rows"""
    n = len(part)
    step = (rng.random(n) < 1.0 / mean).astype(np.int64)
    return np.cumsum(step)  # (non-decreasing over the whole input: sorted inside every partition)


def int_values(n, rng, null_share=0.3):
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    v[rng.random(n) < null_share] = NULL_I64
    return v


def fp_values(n, rng, null_share=0.3):
    v = bits(rng.integers(1, 4000, n) / 4.0).copy()  # positive: no cancellation in a sum, no -0.0 beside +0.0
    v[rng.random(n) < null_share] = NULL_F64_BITS
    return v


# partition key column 0, order key column 1, a nullable int column 2 and a nullable double column 3: every kind on both,
# with every frame it reads
EVERY_KIND = [WOut("row_number"), WOut("rank"), WOut("dense_rank"), WOut("percent_rank"), WOut("cume_dist"), WOut("ntile", param=3)]
for _col, _null in ((2, INT_NULLABLE), (3, FP_NULLABLE)):
    EVERY_KIND += [WOut("lag", _col, "rows", *_null, 1), WOut("lead", _col, "rows", *_null, 2), WOut("first_value", _col, "rows", *_null)]
    for _frame in FRAMES:
        EVERY_KIND += [WOut(k, _col, _frame, *_null) for k in ("last_value", "count", "sum", "min", "max", "avg")]
EVERY_KIND += [WOut("count", -1, f) for f in FRAMES]


def every_kind_case(mgr, part, seed, order=None, outs=EVERY_KIND, **kw):
    rng = np.random.default_rng(seed)
    n = len(part)
    order = order_with_ties(part, rng) if order is None else order
    check_case(mgr, [part, order, int_values(n, rng), fp_values(n, rng)], [0], [1], outs, **kw)


def test_the_out_list_covers_every_kind_and_frame():
    assert {o.kind for o in EVERY_KIND} == set(KINDS)
    for kind in ("last_value",) + W.AGGREGATES:
        assert {o.frame for o in EVERY_KIND if o.kind == kind} == set(FRAMES)


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, N])
def test_sizes_and_run_lengths(mgr, n):
    for mode in ("one", "distinct", "r3", "r300"):
        rng = np.random.default_rng(n * 7 + len(mode))
        every_kind_case(mgr, run_keys(n, mode, rng), n + len(mode))


@pytest.mark.parametrize("edge", [63, 64, 1023, 1024, 4095, 4096])
def test_partitions_and_peer_groups_that_end_at_an_item_wave_or_tile_boundary(mgr, edge):
    n = 3 * TILE + 77
    tails = [t * TILE + edge for t in range(3)] + [t * TILE + edge - 1 for t in (0, 2)] + [5]
    every_kind_case(mgr, keys_from_tails(n, tails), edge)
    # the same rows as peer-group ends inside one partition, and inside partitions that end elsewhere
    every_kind_case(mgr, np.zeros(n, dtype=np.int64), edge + 1, order=keys_from_tails(n, tails))
    every_kind_case(mgr, keys_from_tails(n, [700, TILE + 3000]), edge + 2, order=keys_from_tails(n, tails))


def test_a_partition_over_three_whole_tiles(mgr):
    n = 5 * TILE + 9
    every_kind_case(mgr, keys_from_tails(n, [TILE - 1, 4 * TILE - 1]), 1)  # exactly tiles 1..3
    every_kind_case(mgr, keys_from_tails(n, [7, 4 * TILE + 700]), 2)  # from tile 0 into tile 4, no tail in 1..3


def test_the_carry_resets_after_a_partition_that_ends_with_its_tile(mgr):
    n = 2 * TILE + 100
    every_kind_case(mgr, keys_from_tails(n, [TILE - 1, TILE]), 3)
    every_kind_case(mgr, keys_from_tails(n, [10, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE]), 4)


def test_the_last_row_alone_in_its_tile(mgr):
    n = 2 * TILE + 1
    every_kind_case(mgr, keys_from_tails(n, [100, 2 * TILE - 1]), 5)  # a partition of its own
    every_kind_case(mgr, keys_from_tails(n, [100]), 6)  # the end of a partition that began in tile 0
    every_kind_case(mgr, np.zeros(n, dtype=np.int64), 7)


def test_a_peer_group_that_straddles_a_tile_boundary(mgr):
    n = 2 * TILE + 50
    part = keys_from_tails(n, [99])
    order = keys_from_tails(n, [99, TILE - 30, TILE + 40, 2 * TILE - 1])  # peers [TILE - 29, TILE + 40] and up to the tile's end
    every_kind_case(mgr, part, 8, order=order)
    every_kind_case(mgr, part, 9, order=keys_from_tails(n, [99, TILE - 1, 2 * TILE + 3]))  # one peer group is all of tile 1


def test_no_value_yet_survives_the_tile_carry(mgr):
    n = 2 * TILE
    part = keys_from_tails(n, [9, n - 6])  # one partition from row 10 across both tiles
    rng = np.random.default_rng(11)
    order = order_with_ties(part, rng, 5)
    for where in ("first_null", "second_null", "all_null"):
        iv, fv = int_values(n, rng, 0.0), fp_values(n, rng, 0.0)
        lo, hi = {"first_null": (0, TILE), "second_null": (TILE, n), "all_null": (10, n - 5)}[where]
        iv[lo:hi] = NULL_I64
        fv[lo:hi] = NULL_F64_BITS
        check_case(mgr, [part, order, iv, fv], [0], [1], EVERY_KIND)
    # a partition whose only value is the last row of the second tile, and one whose only value is its first row
    for at, val in ((n - 1, 5), (0, -7)):
        iv = np.full(n, NULL_I64, dtype=np.int64)
        iv[at] = val
        fv = np.full(n, NULL_F64_BITS, dtype=np.int64)
        fv[at] = bits([2.5])[0]
        check_case(mgr, [np.zeros(n, dtype=np.int64), order, iv, fv], [0], [1], EVERY_KIND)


def test_lag_and_lead_distances(mgr):
    n = 3 * TILE + 500
    rng = np.random.default_rng(12)
    iv, fv = int_values(n, rng), fp_values(n, rng)
    outs = []
    for k in (0, 1, 63, 64, 4096, 5000, n + 10, 1 << 40):
        outs += [WOut("lag", 2, "rows", *INT_NULLABLE, k), WOut("lead", 3, "rows", *FP_NULLABLE, k)]
    # partitions shorter and longer than every k: mean 3, mean 300, one of 9 000 rows, one partition
    long_one = keys_from_tails(n, [200, 9200])
    for part in (run_keys(n, "r3", rng), run_keys(n, "r300", rng), long_one, np.zeros(n, dtype=np.int64)):
        check_case(mgr, [part, order_with_ties(part, rng), iv, fv], [0], [1], outs)


def test_ntile(mgr):
    n = 2 * TILE + 77
    rng = np.random.default_rng(13)
    outs = [WOut("ntile", param=p) for p in (1, 3, 4, 100, 10_000, (1 << 63) - 1)] + [WOut("row_number")]
    for part in (run_keys(n, "r3", rng), run_keys(n, "r300", rng), keys_from_tails(n, [5, 5005]), np.zeros(n, dtype=np.int64)):
        check_case(mgr, [part, order_with_ties(part, rng), part, part], [0], [1], outs)


def test_no_partition_keys_no_order_keys_and_neither(mgr):
    n = TILE + 900
    rng = np.random.default_rng(14)
    part = run_keys(n, "r300", rng)
    cols = [part, order_with_ties(part, rng, 4), int_values(n, rng), fp_values(n, rng)]
    check_case(mgr, cols, [], [1], EVERY_KIND)  # one partition, peers by the order key
    check_case(mgr, cols, [0], [], EVERY_KIND)  # every row of a partition a peer: RANGE is PARTITION
    check_case(mgr, cols, [], [], EVERY_KIND)


def test_several_keys_null_keys_and_signed_zeros(mgr):
    n = 2 * TILE + 33
    rng = np.random.default_rng(15)
    k0 = np.full(n, 7, dtype=np.int64)
    k1 = np.repeat(np.arange(n // 50 + 1, dtype=np.int64), 50)[:n]
    k1[(k1 % 7) == 3] = NULL_I64  # NULL keys: NULL equals NULL
    k2 = bits(np.where((np.arange(n) // 5) % 2 == 0, 0.0, -0.0)).copy()  # -0.0 and +0.0 are two keys
    o = np.arange(n, dtype=np.int64) // 2
    o[(o % 5) == 1] = NULL_I64  # NULL order keys are peers of each other
    iv, fv = int_values(n, rng), fp_values(n, rng)
    outs = [x for x in EVERY_KIND if x.col < 0] + [WOut(x.kind, x.col + 2, x.frame, *x[3:]) for x in EVERY_KIND if x.col >= 0]
    check_case(mgr, [k0, k1, k2, o, iv, fv], [0, 1], [2, 3], outs)  # signed zeros split peer groups
    check_case(mgr, [k0, k1, k2, o, iv, fv], [1, 2, 0], [3], outs)  # ... and partitions
    check_case(mgr, [k0, k1, k2, o, iv, fv], [2], [1, 3, 0], outs[:8])


def test_scan_trips(mgr):
    """one more tile than a trip of both scans, plus a one-row tile: a long partition across the trip boundary, sparse
    tails beyond it, tile indices >= 4096.  One column: partition key and argument."""
    n = (TRIP + 1) * TILE + 1
    key = np.arange(n, dtype=np.int64) // 10_007  # partitions of 10 007 rows: two tiles and a bit
    a, b = 4000 * TILE + 17, TRIP * TILE + 100
    key[a:b] = -5  # 96 tiles and a bit, ending in the first tile of the second trip
    key[b:n - 1] = np.int64(1) << 40  # the rest of the second trip but the last row
    key[b + 2000] = 3  # ... but for a one-row partition in it
    key[n - 1] = 9  # the one-row tile
    check_case(mgr, [key], [0], [], [WOut("row_number"), WOut("sum", 0, "rows"), WOut("count", 0, "partition")], extra_capacity=0)


def test_calling_variants(mgr):
    rng = np.random.default_rng(16)
    n = 3 * TILE + 5
    part = run_keys(n, "r3", rng)
    cols = [part, order_with_ties(part, rng), int_values(n, rng), fp_values(n, rng)]
    check_case(mgr, cols, [0], [1], EVERY_KIND[:8], give_workspace=True)
    check_case(mgr, cols, [0], [1], EVERY_KIND[8:16], extra_capacity=0)
    check_case(mgr, cols, [0], [1], EVERY_KIND[16:24], extra_capacity=TILE + 1)


def test_a_column_that_cannot_be_null_holds_the_sentinel(mgr):
    n = TILE + 50
    rng = np.random.default_rng(17)
    part = run_keys(n, "r3", rng)
    iv = rng.integers(-5, 5, n).astype(np.int64)
    iv[::4] = NULL_I64
    fv = bits(rng.integers(1, 100, n) / 2.0).copy()
    fv[::5] = NULL_F64_BITS  # DBL_MIN as a value
    outs = [WOut(k, 2, f) for f in FRAMES for k in ("count", "min", "max")] + [WOut("sum", 2, "rows"), WOut("avg", 3, "range", True),
                                                                               WOut("min", 3, "rows", True), WOut("sum", 3, "partition", True)]
    check_case(mgr, [part, order_with_ties(part, rng), iv, fv], [0], [1], outs)


def test_int_sum_wraps(mgr):
    n = TILE + 300
    rng = np.random.default_rng(18)
    part = np.arange(n, dtype=np.int64) // 3
    v = (np.int64(1) << 62) + 2 * rng.integers(0, 1000, n).astype(np.int64) + 1
    v[rng.random(n) < 0.5] *= -1
    outs = [WOut("sum", 1, f, *INT_NULLABLE) for f in FRAMES] + [WOut("sum", 1, "rows")]
    check_case(mgr, [part, v], [0], [], outs)
    check_case(mgr, [np.zeros(n, dtype=np.int64), v], [0], [], outs[3:])  # one partition: the sum wraps many times over


def test_no_rows(mgr):
    L = lib()
    d_in = mgr.to_device(np.zeros(8, dtype=np.int64), 0)
    d_out = mgr.to_device(np.full(8, POISON64, dtype=np.uint64), 0)
    keys = (C.c_int32 * 1)(0)
    arr = (A.WindowOut * 1)(A.WindowOut(0, A.WIN_SUM, A.FRAME_PARTITION, 0, 0, 0, 0))
    try:
        check(L.hdk_hip_window_columns(d_in.ptr, 4, 2, 0, keys, 1, keys, 1, arr, 1, d_out.ptr, 4, None, 0, 0, None))
        mgr.synchronizeStream(0)
        assert (mgr.to_host(d_out.ptr, 64, 0, np.uint64) == POISON64).all()
    finally:
        d_in.free()
        d_out.free()
