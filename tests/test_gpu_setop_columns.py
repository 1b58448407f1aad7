"""hdk_hip_setop_columns and hdk_hip_concat_columns on raw uploaded columns.  The expectation is tests/setop_expect.py
(numpy, checked against SQLite and collections.Counter in test_setop_columns_cpu.py).  Every case asserts row_count, every
output column word for word, the poison beyond the output rows and in a guard column, and an untouched input."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import check, lib

import setop_expect as E
from setop_expect import NULL_F64_BITS, NULL_I32, NULL_I64

pytestmark = pytest.mark.gpu

POISON64 = np.uint64(0x5A5A5A5A5A5A5A5A)
FILL = 0x1111111111111111  # what lies in the capacity behind the rows
TILE = 4096  # rows per tile (hdk_amd/csrc/column_segments.h: kGcTile); a wave owns 1024 of them, an item 64
TRIP = 4096  # tiles per trip of hdk_counts_scan<4> and of the carry scan (kGcCarryTrip)
EVERY_OP = (E.UNION, E.INTERSECT, E.INTERSECT_ALL, E.EXCEPT, E.EXCEPT_ALL)
RIGHT_WORDS = np.array([1, -1, 1 << 32, 7 << 40, -(1 << 63), 3], dtype=np.int64)  # a non-zero tag word, its low half 0 included


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


class Block:
    """input columns uploaded once (capacity n + 3), any number of calls over them, the input compared on the way out"""

    def __init__(self, mgr, cols):
        self.mgr, self.n, self.nc = mgr, len(cols[0]), len(cols)
        self.cap = self.n + 3
        self.host = np.full((self.nc, self.cap), FILL, dtype=np.int64)
        for t, c in enumerate(cols):
            self.host[t, :self.n] = c
        self.d_in = mgr.to_device(self.host.reshape(-1), 0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                back = self.mgr.to_host(self.d_in.ptr, self.nc * self.cap * 8, 0, np.int64).reshape(self.nc, self.cap)
                assert np.array_equal(back, self.host), "the input was modified"
        finally:
            self.d_in.free()

    def run(self, key_cols, tag_col, op, outs, ocap, give_workspace=False, count_only=False, n=None):
        """-> (row_count, out[(nouts + 1), ocap])"""
        L, mgr = lib(), self.mgr
        n = self.n if n is None else n
        no = len(outs)
        d_out = mgr.to_device(np.full((no + 1) * max(ocap, 1), POISON64, dtype=np.uint64), 0)
        d_rows = mgr.to_device(np.full(1, POISON64, dtype=np.uint64), 0)
        ws = mgr.alloc(L.hdk_hip_setop_columns_workspace_bytes(n), 0) if give_workspace else None
        try:
            check(L.hdk_hip_setop_columns(self.d_in.ptr, self.cap, self.nc, n, (C.c_int32 * len(key_cols))(*key_cols), len(key_cols),
                                          tag_col, op, (C.c_int32 * no)(*outs), no, None if count_only else d_out.ptr, ocap,
                                          d_rows.ptr, ws.ptr if ws else None, ws.nbytes if ws else 0, 0, None))
            mgr.synchronizeStream(0)
            rows = int(mgr.to_host(d_rows.ptr, 8, 0, np.uint64)[0])
            out = mgr.to_host(d_out.ptr, (no + 1) * max(ocap, 1) * 8, 0, np.uint64).reshape(no + 1, max(ocap, 1))
        finally:
            for b in (d_out, d_rows, ws):
                if b is not None:
                    b.free()
        return rows, out


def check_block(mgr, cols, key_cols, tag_col, ops=EVERY_OP, outs=None, out_capacity=None, give_workspace=False):
    """every op over one uploaded block -> the kept counts by op"""
    cols = [np.ascontiguousarray(c).view(np.int64) for c in cols]
    n = len(cols[0])
    outs = list(key_cols) if outs is None else outs
    counters = E.counters(cols, n, key_cols, tag_col)
    counts = {}
    with Block(mgr, cols) as blk:
        for op in ops:
            m = E.keep_of(*counters, op)
            kept = int(m.sum())
            ocap = kept + 5 if out_capacity is None else out_capacity
            rows, out = blk.run(key_cols, tag_col, op, outs, ocap, give_workspace)
            assert rows == kept, (op, rows, kept)
            w = min(kept, ocap)
            for j, t in enumerate(outs):
                got, want = out[j, :w].view(np.int64), cols[t][m][:w]
                assert np.array_equal(got, want), (op, j, np.flatnonzero(got != want)[:5])
                assert (out[j, w:] == POISON64).all(), (op, j)
            assert (out[len(outs)] == POISON64).all(), "guard column"
            counts[op] = kept
    return counts


def runs_block(rights, lefts, rng=None):
    """one key column and a tag: run i has rights[i] right rows (tag != 0) followed by lefts[i] left rows (tag 0); the keys
    ascend by run"""
    rights, lefts = np.asarray(rights, dtype=np.int64), np.asarray(lefts, dtype=np.int64)
    lens = rights + lefts
    key = np.repeat(np.arange(len(lens), dtype=np.int64) * 3 - 11, lens)
    first = np.repeat(np.cumsum(lens) - lens, lens)
    pos = np.arange(len(key)) - first  # the row's place in its run
    is_right = pos < np.repeat(rights, lens)
    words = RIGHT_WORDS[(np.arange(len(key)) if rng is None else rng.integers(0, len(RIGHT_WORDS), len(key))) % len(RIGHT_WORDS)]
    return key, np.where(is_right, words, 0).astype(np.int64)


def short_runs(n, rng, most=3):
    """at least n rows of runs with 0..most right and 0..most left rows, never none of both"""
    m = n + 1
    r, l = rng.integers(0, most + 1, m), rng.integers(0, most + 1, m)
    l[(r + l) == 0] = 1
    return r, l


def random_block(n, rng, most=3):
    r, l = short_runs(n, rng, most)
    key, tag = runs_block(r, l, rng)
    return key[:n], tag[:n]  # (a run cut short still has its right rows in front)


def block_with(n, rng, special):
    """random short runs with the runs `special` = [(first row, right rows, left rows)] at their places -> key, tag of n rows"""
    rs, ls, at = [], [], 0
    for first, r, l in special:
        assert first >= at
        if first > at:  # filler of exactly first - at rows: short runs, the last one cut to fit
            fr, fl = short_runs(first - at, rng)
            lens = fr + fl
            k = int(np.searchsorted(np.cumsum(lens), first - at))
            fr, fl = fr[:k + 1].copy(), fl[:k + 1].copy()
            over = int((fr + fl).sum()) - (first - at)
            cut = min(over, int(fl[k]))
            fl[k] -= cut
            fr[k] -= over - cut
            keep = (fr + fl) > 0
            rs += fr[keep].tolist()
            ls += fl[keep].tolist()
        rs.append(r)
        ls.append(l)
        at = first + r + l
    assert at <= n
    if at < n:
        fr, fl = short_runs(n - at, rng)
        rs += fr.tolist()
        ls += fl.tolist()
    key, tag = runs_block(rs, ls, rng)
    assert len(key) >= n
    return key[:n], tag[:n]


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_sizes_with_random_short_runs(mgr, n):
    rng = np.random.default_rng(n)
    key, tag = random_block(n, rng)
    check_block(mgr, [key, tag], [0], 1)
    if n == 1:  # the one row as a right row, too
        check_block(mgr, [key, np.array([5], dtype=np.int64)], [0], 1)


@pytest.mark.parametrize("edge", [64, 1024, TILE])
def test_the_sides_switch_at_an_item_wave_or_tile_boundary(mgr, edge):
    """the right part of a run ends at row edge - 1 and its left part begins at row edge; then the same with the run's first
    and last row at the edge"""
    rng = np.random.default_rng(edge)
    n = 2 * TILE + 100
    for r, l in ((5, 5), (1, 3), (3, 1), (40, 2), (2, 40)):
        if r > edge:
            continue
        key, tag = block_with(n, rng, [(edge - r, r, l), (TILE + edge - r, r, l)])
        assert tag[edge - 1] != 0 and tag[edge] == 0 and key[edge - r] == key[edge + l - 1]
        check_block(mgr, [key, tag], [0], 1)
    key, tag = block_with(n, rng, [(edge - 4, 2, 2), (edge, 2, 2), (edge + 4, 0, 3)])  # runs that end and begin with the edge
    assert key[edge - 1] != key[edge]
    check_block(mgr, [key, tag], [0], 1)


def test_one_run_over_three_whole_tiles(mgr):
    """the switch from right to left rows in the middle tile: l > r, l == r and l < r over thousands of rows"""
    rng = np.random.default_rng(3)
    n = 5 * TILE + 9
    for r in (TILE + 1500, TILE + 2048, 2 * TILE - 1):
        key, tag = block_with(n, rng, [(TILE, r, 3 * TILE - r)])
        assert key[TILE] == key[4 * TILE - 1] and key[TILE - 1] != key[TILE] and key[4 * TILE] != key[TILE]
        counts = check_block(mgr, [key, tag], [0], 1)
        assert counts[E.UNION] < n
    # and a run of left rows only / right rows only over the three tiles
    for r, l in ((0, 3 * TILE), (3 * TILE, 0)):
        key, tag = block_with(n, rng, [(TILE, r, l)])
        check_block(mgr, [key, tag], [0], 1)


def test_the_carry_resets_after_a_run_that_ends_with_its_tile(mgr):
    """a run of right rows only fills tile 1; the run of left rows only that follows must not see them"""
    rng = np.random.default_rng(4)
    key, tag = block_with(4 * TILE, rng, [(TILE, TILE, 0), (2 * TILE, 0, TILE + 10)])
    counts = check_block(mgr, [key, tag], [0], 1)
    assert counts[E.EXCEPT_ALL] >= TILE + 10
    # the same with the sides swapped: the right rows of the second run see no left row of the first
    key, tag = block_with(4 * TILE, rng, [(TILE, 0, TILE), (2 * TILE, TILE + 10, 0)])
    check_block(mgr, [key, tag], [0], 1)


def test_the_last_row_alone_in_its_tile(mgr):
    rng = np.random.default_rng(5)
    n = 2 * TILE + 1
    for last in ((n - 1, 0, 1), (n - 1, 1, 0)):  # a run of its own: a left row, a right row
        key, tag = block_with(n, rng, [last])
        check_block(mgr, [key, tag], [0], 1)
    key, tag = block_with(n, rng, [(n - 40, 30, 10)])  # ... and the last left row of a run that began in the tile before
    check_block(mgr, [key, tag], [0], 1)
    key, tag = block_with(n, rng, [(n - 40, 39, 1)])
    check_block(mgr, [key, tag], [0], 1)


def test_every_relation_of_l_and_r_for_every_op(mgr):
    """runs with l > r, l == r, l < r, r == 0 and l == 0, short and longer than an item, next to each other"""
    rs, ls = [], []
    for r, l in ((1, 3), (2, 2), (3, 1), (0, 2), (2, 0), (0, 1), (1, 0), (1, 1), (70, 100), (100, 70), (90, 90), (0, 130), (130, 0)):
        rs += [r] * 3
        ls += [l] * 3
    key, tag = runs_block(rs * 4, ls * 4)
    counts = check_block(mgr, [key, tag], [0], 1)
    r, l = np.array(rs * 4), np.array(ls * 4)
    assert counts == {E.UNION: len(r), E.INTERSECT: int(((r > 0) & (l > 0)).sum()), E.INTERSECT_ALL: int(np.minimum(r, l).sum()),
                      E.EXCEPT: int(((r == 0) & (l > 0)).sum()), E.EXCEPT_ALL: int(np.maximum(l - r, 0).sum())}


def test_several_keys_null_keys_signed_zeros_and_nans(mgr):
    """1, 2 and 8 key columns; a run is bit-equality on all of them: NULL equals NULL, -0.0, +0.0 and two NaN patterns are
    four rows; outs that are a subset of the keys, in another order, and the tag"""
    rng = np.random.default_rng(6)
    n = TILE + 777
    key, tag = random_block(n, rng)
    run = (key + 11) // 3
    k0 = run // 4
    k1 = np.where(run % 4 == 3, NULL_I64, run % 4)  # a NULL key is a key like another
    fp = np.array([0.0, -0.0, np.nan, 1.5]).view(np.int64).copy()
    fp[2] = np.int64(0x7FF8000000000001)  # a NaN by another pattern than numpy's
    nan2 = np.float64(np.nan).view(np.int64)
    kf = np.where(run % 5 == 4, nan2, fp[run % 4])
    kf = np.where(run % 7 == 6, NULL_F64_BITS, kf)
    # (k0, k1) names the run, and so does (k0, kf): neighbouring runs differ in the fp word's bits alone
    check_block(mgr, [k0, k1, tag], [0, 1], 2)
    check_block(mgr, [tag, k0, kf], [1, 2], 0, outs=[2, 1])
    check_block(mgr, [k0, k1, tag, kf], [0, 1, 3], 2, outs=[1])                # a subset of the keys
    check_block(mgr, [k0, k1, tag, kf], [3, 0, 1], 2, outs=[2, 0, 3, 1])       # the tag leaves when asked for
    # eight keys: the run changes in the last one only, then in the first one only
    const = [np.full(n, 10 + i, dtype=np.int64) for i in range(7)]
    check_block(mgr, const + [key, tag], list(range(8)), 8, outs=[7, 0])
    check_block(mgr, [key] + const + [tag], list(range(8)), 8, ops=(E.UNION, E.INTERSECT_ALL, E.EXCEPT_ALL), outs=[0, 7])
    # -0.0 / +0.0 / NaN patterns adjacent, one row of each side per pattern: four runs, not one
    pat = np.array([0.0, -0.0, np.nan, np.nan]).view(np.int64).copy()
    pat[3] = np.int64(0x7FF8000000000001)
    counts = check_block(mgr, [np.repeat(pat, 2), np.tile(np.array([1, 0], dtype=np.int64), 4)], [0], 1)
    assert counts[E.UNION] == 4 and counts[E.INTERSECT] == 4 and counts[E.EXCEPT] == 0


def test_scan_trips(mgr):
    """more tiles than a trip of both scans: runs of length 3, one run that crosses from tile 4095 into tile 4096 and a
    one-row tile at the end.  One key column and the tag."""
    n = TRIP * TILE + TILE + 1
    rows = np.arange(n, dtype=np.int64)
    key = rows // 3
    tag = np.where(rows % 3 == 0, 1, 0).astype(np.int64)  # one right row, two left rows
    tag[(rows // 3) % 5 == 0] = 0  # every fifth run: left rows only
    tag[((rows // 3) % 5 == 1) & (rows % 3 == 1)] = 9  # ... and the next: two right rows, one left row
    a, b = TRIP * TILE - 1500, TRIP * TILE + 2500  # the long run: 1 700 right rows, then left rows across the trip boundary
    key[a:b] = -5
    tag[a:a + 1700] = 1 << 33
    tag[a + 1700:b] = 0
    key[n - 1] = -9  # the one-row tile: a run of its own
    tag[n - 1] = 0
    check_block(mgr, [key, tag], [0], 1, ops=(E.UNION, E.INTERSECT_ALL, E.EXCEPT_ALL))


def test_calling_variants(mgr):
    """count-only equals the materialised count; a capacity below the count writes nothing at or beyond it; a caller's
    workspace gives what the pool's gives"""
    rng = np.random.default_rng(14)
    n = 3 * TILE + 5
    key, tag = random_block(n, rng)
    cols = [key, tag]
    counts = check_block(mgr, cols, [0], 1)
    check_block(mgr, cols, [0], 1, give_workspace=True)
    for cap in (1, 1000, TILE + 1):
        check_block(mgr, cols, [0], 1, out_capacity=cap)
    check_block(mgr, cols, [0], 1, ops=(E.UNION,), out_capacity=counts[E.UNION] - 1)
    with Block(mgr, cols) as blk:
        for op in EVERY_OP:
            rows, out = blk.run([0], 1, op, [0, 1], 8, count_only=True)
            assert rows == counts[op] and (out == POISON64).all()
            rows, out = blk.run([0], 1, op, [0, 1], 0)
            assert rows == counts[op] and (out == POISON64).all()


def test_no_rows(mgr):
    with Block(mgr, [np.zeros(5, dtype=np.int64)] * 2) as blk:
        for op in EVERY_OP:
            rows, out = blk.run([0], 1, op, [0], 4, n=0)
            assert rows == 0 and (out == POISON64).all()


def test_a_block_that_violates_the_precondition_stays_inside_its_bounds(mgr):
    """left rows before right rows, equal rows apart: the rows are unspecified, the count is at most num_rows, and nothing
    outside the permitted range is written (the memory guards are what is checked)"""
    rng = np.random.default_rng(15)
    n = 2 * TILE + 333
    key = rng.integers(0, 50, n).astype(np.int64)
    tag = rng.integers(0, 2, n).astype(np.int64)
    with Block(mgr, [key, tag]) as blk:
        for op in EVERY_OP:
            for ocap in (n + 7, 100):
                rows, out = blk.run([0], 1, op, [0, 1], ocap)
                assert rows <= n
                w = min(rows, ocap)
                assert (out[:2, w:] == POISON64).all() and (out[2] == POISON64).all()
                assert np.isin(out[0, :w].view(np.int64), key).all()  # (every word written is a word of the input)


# ---- hdk_hip_concat_columns ------------------------------------------------------------------------------------------------
def run_concat(mgr, lcols, rcols, pairs, side_col=-1, flags=0, lcap_extra=3, rcap_extra=0):
    """-> out[(output columns + 1), ocap] with ocap = rows + 5; the inputs are compared on the way out"""
    L = lib()
    ln, rn = (len(lcols[0]) if lcols else 0), (len(rcols[0]) if rcols else 0)
    lnc = max(len(lcols), 1 + max(p[0] for p in pairs))  # (a side without rows still says how many columns it has)
    rnc = max(len(rcols), 1 + max(p[1] for p in pairs))
    lcap, rcap = ln + lcap_extra, rn + rcap_extra
    hl = np.full((lnc, max(lcap, 1)), FILL, dtype=np.int64)
    hr = np.full((rnc, max(rcap, 1)), FILL, dtype=np.int64)
    for t, c in enumerate(lcols):
        hl[t, :ln] = c
    for t, c in enumerate(rcols):
        hr[t, :rn] = c
    no = len(pairs) + (1 if side_col >= 0 else 0)
    ocap = ln + rn + 5
    arr = (A.SetopCol * len(pairs))()
    for j, (lc, rc, lnl, rnl, lnull, rnull, onull) in enumerate(pairs):
        arr[j] = A.SetopCol(lc, rc, int(lnl), int(rnl), (C.c_uint8 * 6)(), A.to_i64(int(lnull)), A.to_i64(int(rnull)), A.to_i64(int(onull)))
    d_l, d_r = mgr.to_device(hl.reshape(-1), 0), mgr.to_device(hr.reshape(-1), 0)
    d_out = mgr.to_device(np.full((no + 1) * ocap, POISON64, dtype=np.uint64), 0)
    try:
        check(L.hdk_hip_concat_columns(d_l.ptr if ln else None, lcap, lnc, ln, d_r.ptr if rn else None, rcap, rnc, rn, arr, len(pairs),
                                       side_col, flags, d_out.ptr, ocap, 0, None))
        mgr.synchronizeStream(0)
        out = mgr.to_host(d_out.ptr, (no + 1) * ocap * 8, 0, np.uint64).reshape(no + 1, ocap)
        assert np.array_equal(mgr.to_host(d_l.ptr, hl.size * 8, 0, np.int64).reshape(hl.shape), hl), "the left input was modified"
        assert np.array_equal(mgr.to_host(d_r.ptr, hr.size * 8, 0, np.int64).reshape(hr.shape), hr), "the right input was modified"
    finally:
        for b in (d_l, d_r, d_out):
            b.free()
    return out


def check_concat(mgr, lcols, rcols, pairs, side_col=-1, flags=0, **kw):
    ln, rn = (len(lcols[0]) if lcols else 0), (len(rcols[0]) if rcols else 0)
    want = E.concat(lcols, ln, rcols, rn, pairs, side_col, bool(flags & A.CONCAT_TAG_FIRST))
    out = run_concat(mgr, lcols, rcols, pairs, side_col, flags, **kw)
    assert len(want) + 1 == len(out)
    for j, w in enumerate(want):
        assert np.array_equal(out[j, :ln + rn].view(np.int64), w), (j, np.flatnonzero(out[j, :ln + rn].view(np.int64) != w)[:5])
        assert (out[j, ln + rn:] == POISON64).all(), j
    assert (out[len(want)] == POISON64).all(), "guard column"


def concat_side(n, rng, null):
    a = rng.integers(-5, 6, n).astype(np.int64)
    b = (rng.normal(size=n) * 10).view(np.int64).copy()
    c = rng.integers(-2**62, 2**62, n).astype(np.int64)
    a[rng.random(n) < 0.3] = null
    a[rng.random(n) < 0.1] = NULL_I64 if null == NULL_I32 else NULL_I32  # the OTHER side's sentinel is a value here
    b[rng.random(n) < 0.3] = NULL_F64_BITS
    return [a, b, c]


# the two sides use different sentinels in column 0; column 1 is nullable on the left only; column 2 on neither
PAIRS = [(0, 0, True, True, int(NULL_I32), int(NULL_I64), int(NULL_I64)),
         (1, 1, True, False, int(NULL_F64_BITS), 0, -77),
         (2, 2, False, False, 0, 0, 0)]


@pytest.mark.parametrize("ln,rn", [(1, 1), (63, 65), (64, 64), (1023, 1), (1024, 1025), (TILE - 1, 2), (TILE, TILE + 1),
                                   (3 * TILE + 17, 2 * TILE - 5)])
def test_concat_sizes_nulls_and_the_side_column(mgr, ln, rn):
    rng = np.random.default_rng(ln * 7 + rn)
    l, r = concat_side(ln, rng, NULL_I32), concat_side(rn, rng, NULL_I64)
    check_concat(mgr, l, r, PAIRS)
    check_concat(mgr, l, r, PAIRS, side_col=3)
    check_concat(mgr, l, r, PAIRS, side_col=0, flags=A.CONCAT_TAG_FIRST, lcap_extra=0, rcap_extra=9)
    # another column order on each side, a column twice, one pair
    check_concat(mgr, l, r, [(2, 0, False, True, 0, int(NULL_I64), 123), (0, 2, True, False, int(NULL_I32), 0, int(NULL_I64)),
                             (0, 0, False, False, 0, 0, 0)], side_col=1)
    check_concat(mgr, l, r, PAIRS[:1], side_col=1)


def test_concat_with_an_empty_side(mgr):
    rng = np.random.default_rng(8)
    side = concat_side(TILE + 9, rng, NULL_I32)
    swapped = [(lc, rc, rnl, lnl, rnull, lnull, onull) for lc, rc, lnl, rnl, lnull, rnull, onull in PAIRS]
    for sc, flags in ((-1, 0), (3, 0), (1, A.CONCAT_TAG_FIRST)):
        check_concat(mgr, side, [], PAIRS, sc, flags)
        check_concat(mgr, [], side, swapped, sc, flags)
    # both sides empty: nothing is launched, nothing is written
    out = run_concat(mgr, [], [], PAIRS[:1], 1)
    assert (out == POISON64).all()


def test_concat_then_setop_is_the_method(mgr):
    """the two calls in the order DeviceColumns uses them, the sort done here: the tag of CONCAT_TAG_FIRST is the tag the
    set operation expects"""
    rng = np.random.default_rng(9)
    l = [rng.integers(0, 40, 3000).astype(np.int64)]
    r = [rng.integers(20, 60, 2000).astype(np.int64)]
    pairs = [(0, 0, False, False, 0, 0, 0)]
    block = E.concat(r, 2000, l, 3000, pairs, 1, True)
    assert (block[1][:2000] == 1).all() and (block[1][2000:] == 0).all()
    check_concat(mgr, r, l, pairs, 1, A.CONCAT_TAG_FIRST)
    perm = np.argsort(block[0], kind="stable")
    counts = check_block(mgr, [block[0][perm], block[1][perm]], [0], 1)
    cl, cr = E.multiset(l), E.multiset(r)
    assert counts[E.INTERSECT_ALL] == sum((cl & cr).values()) and counts[E.EXCEPT_ALL] == sum((cl - cr).values())
    assert counts[E.UNION] == len(set(cl) | set(cr)) and counts[E.EXCEPT] == len(set(cl) - set(cr))
