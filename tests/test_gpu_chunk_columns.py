"""hdk_hip_chunk_columns on the device, through the C ABI, against its numpy statement (tests/chunk_expect.py): the copy with
the NULL rewrite, the per-fragment statistics at fragment and tile seams, the selection, and what the call leaves alone."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import check, lib

import chunk_expect as E
from chunk_expect import NULL_DOUBLE_BITS, NULL_FLOAT_WIDE_BITS, NULL_I32, NULL_I64

pytestmark = pytest.mark.gpu

POISON64 = np.uint64(0x5A5A5A5A5A5A5A5A)
FILL = 0x1111111111111111  # what lies in the capacity behind the rows
TILE = 4096  # rows per tile (hdk_amd/csrc/chunk_columns.hip: kCkTile)

INT_SEL = (False, True, int(NULL_I32), int(NULL_I64))
FP_SEL = (True, True, int(NULL_FLOAT_WIDE_BITS), int(NULL_DOUBLE_BITS))


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


def run(mgr, cols, n, sel, frag, cap_extra=0, ocap=None, own_workspace=False):
    """-> (out[(columns + 1), ocap] as uint64 with a guard column, stats[columns][fragments][4] as int64); the input is
    compared on the way out"""
    L = lib()
    ncin = len(cols)
    cap = n + cap_extra
    host = np.full((ncin, max(cap, 1)), FILL, dtype=np.int64)
    for t, c in enumerate(cols):
        host[t, :n] = c[:n]
    nc = len(sel)
    if ocap is None:
        ocap = (n + 31) // 32 * 32 + 32
    nf = E.num_fragments(n, frag)
    arr = (A.ChunkCol * nc)()
    for j, (col, is_fp, nullable, null_bits, out_null) in enumerate(sel):
        arr[j] = A.ChunkCol(col, int(is_fp), int(nullable), (C.c_uint8 * 2)(), A.to_i64(null_bits), A.to_i64(out_null))
    d_in = mgr.to_device(host.reshape(-1), 0)
    d_out = mgr.to_device(np.full((nc + 1) * ocap, POISON64, dtype=np.uint64), 0)
    d_stats = mgr.to_device(np.full((nc * nf + 1) * 4, POISON64, dtype=np.uint64), 0)
    need = L.hdk_hip_chunk_columns_workspace_bytes(n, frag, nc)
    d_ws = mgr.to_device(np.full(need // 8 + 1, POISON64, dtype=np.uint64), 0) if own_workspace else None
    try:
        check(L.hdk_hip_chunk_columns(d_in.ptr if n else None, cap, ncin, n, arr, nc, frag, d_out.ptr, ocap, d_stats.ptr,
                                      d_ws.ptr if d_ws else None, need if d_ws else 0, 0, None))
        mgr.synchronizeStream(0)
        out = mgr.to_host(d_out.ptr, (nc + 1) * ocap * 8, 0, np.uint64).reshape(nc + 1, ocap)
        st = mgr.to_host(d_stats.ptr, (nc * nf + 1) * 32, 0, np.int64)
        assert (st[nc * nf * 4:].view(np.uint64) == POISON64).all(), "the word behind the statistics"
        assert np.array_equal(mgr.to_host(d_in.ptr, host.size * 8, 0, np.int64).reshape(host.shape), host), "the input was modified"
        if d_ws:
            assert mgr.to_host(d_ws.ptr + need, 8, 0, np.uint64)[0] == POISON64, "the word behind the workspace"
    finally:
        for b in (d_in, d_out, d_stats, d_ws):
            if b is not None:
                b.free()
    return out, st[:nc * nf * 4].reshape(nc, nf, 4)


def check_call(mgr, cols, n, sel, frag, **kw):
    out, st = run(mgr, cols, n, sel, frag, **kw)
    want = E.copy(cols, n, sel)
    ws = E.stats(want, sel, n, frag)
    for j, w in enumerate(want):
        assert np.array_equal(out[j, :n].view(np.int64), w), (j, np.flatnonzero(out[j, :n].view(np.int64) != w)[:5])
        assert (out[j, n:] == POISON64).all(), (j, "rows behind num_rows")
        for f in range(len(ws[j])):
            if n == 0:
                assert (int(st[j, f, 2]), int(st[j, f, 3])) == (0, 0)
            else:
                assert E.same_stats(st[j, f], ws[j][f], sel[j][1]), (j, f, st[j, f].tolist(), ws[j][f])
    assert (out[len(want)] == POISON64).all(), "guard column"
    return out, st


def mixed(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(-1000, 1000, n).astype(np.int64)
    a[rng.random(n) < 0.2] = NULL_I32
    a[rng.random(n) < 0.05] = NULL_I64  # (reads as NULL afterwards)
    d = (rng.normal(size=n) * 100 - 20).view(np.int64).copy() if n else np.zeros(0, np.int64)
    d[rng.random(n) < 0.2] = NULL_FLOAT_WIDE_BITS
    b = rng.integers(-2**62, 2**62, n).astype(np.int64)
    return [a, d, b]


MIXED_SEL = [(0,) + INT_SEL, (1,) + FP_SEL, (2, False, False, 0, int(NULL_I64))]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
@pytest.mark.parametrize("frag", [32, TILE, 4128, 3 * TILE + 32])
def test_rows_and_fragment_sizes(mgr, n, frag):
    """fragments of one tile and less, of a tile and 32 rows (two tiles, the second short), larger than the rows; the input
    capacity equal to the rows, then odd and larger"""
    cols = mixed(n, n * 31 + frag)
    check_call(mgr, cols, n, MIXED_SEL, frag)
    check_call(mgr, cols, n, MIXED_SEL, frag, cap_extra=7 if n % 2 == 0 else 8, own_workspace=True)


def test_a_one_row_last_fragment_and_three_tiles(mgr):
    n = 3 * TILE + 1
    cols = mixed(n, 5)
    for frag in (TILE, 3 * TILE, 1024):
        out, st = check_call(mgr, cols, n, MIXED_SEL, frag, cap_extra=1)
        assert int(st[2, -1, 3]) == 1 and int(st[2, -1, 0]) == int(st[2, -1, 1]) == int(cols[2][n - 1])


@pytest.mark.parametrize("frag,seam", [(64, 64), (TILE, TILE), (4128, 4128), (3 * TILE, TILE), (3 * TILE, 2 * TILE)])
def test_minimum_and_maximum_do_not_leak_across_a_seam(mgr, frag, seam):
    """the column's only minimum in the last row before the seam, its only maximum in the first row after it: across a
    fragment boundary each fragment keeps its own; across a tile boundary inside a fragment the fragment has both"""
    n = 2 * TILE + 77 if seam >= TILE else 200
    a = np.arange(n, dtype=np.int64) % 97
    d = ((np.arange(n) % 89) * 0.5 - 3.0).view(np.int64).copy()
    a[seam - 1], a[seam] = -10**12, 10**12
    d[seam - 1], d[seam] = np.array([-1e300, 1e300]).view(np.int64)
    out, st = check_call(mgr, [a, d], n, [(0,) + INT_SEL, (1,) + FP_SEL], frag)
    f0, f1 = (seam - 1) // frag, seam // frag
    assert int(st[0, f0, 0]) == -10**12 and int(st[0, f1, 1]) == 10**12
    if f0 != f1:
        assert int(st[0, f0, 1]) < 97 and int(st[0, f1, 0]) >= 0
        assert st[1, f0, 1:2].view(np.float64)[0] < 100 and st[1, f1, 0:1].view(np.float64)[0] >= -3.0
    for f in range(st.shape[1]):
        if f not in (f0, f1):
            assert 0 <= int(st[0, f, 0]) <= int(st[0, f, 1]) < 97


def test_integers(mgr):
    n = 160
    a = np.arange(n, dtype=np.int64)
    a[3], a[40] = -2**63 + 1, 2**63 - 1
    a[5], a[41] = NULL_I32, NULL_I32
    a[64:96] = NULL_I32  # fragment 2 of 32 rows: NULLs only
    sel = [(0,) + INT_SEL, (0, False, False, int(NULL_I32), int(NULL_I64))]
    out, st = check_call(mgr, [a], n, sel, 32)
    assert int(st[0, 0, 0]) == -2**63 + 1 and int(st[0, 1, 1]) == 2**63 - 1
    assert out[0, 5].view(np.int64) == NULL_I64 and out[1, 5].view(np.int64) == NULL_I32  # rewritten / NOT NULL: left alone
    assert st[0, 2, 2:].tolist() == [32, 0] and st[1, 2, 2:].tolist() == [0, 32]
    assert st[1, 2, :2].tolist() == [int(NULL_I32), int(NULL_I32)] and int(st[1, 0, 0]) == -2**63 + 1
    assert st[0, :, 2].tolist() == [1, 1, 32, 0, 0] and st[1, :, 2].tolist() == [0] * 5


def test_doubles(mgr):
    n = 128
    d = np.linspace(-50.0, -1.0, n)  # negative: the bit patterns order the other way round
    d[7] = -0.0
    d[40] = np.nan
    d[33] = 7.5
    w = d.view(np.int64).copy()
    w[8] = NULL_FLOAT_WIDE_BITS
    w[96:128] = np.array([np.nan]).view(np.int64)[0]  # fragment 3: NaNs only
    w[64:96] = np.array([-0.0]).view(np.int64)[0]  # fragment 2: zeros only
    w[70] = 0
    out, st = check_call(mgr, [w], n, [(0,) + FP_SEL], 32)
    f = st[0, :, :2].copy().view(np.float64)
    assert f[0, 0] == -50.0 and f[0, 1] == 0.0 and f[1, 1] == 7.5  # (-0.0 is the largest of fragment 0)
    assert f[2, 0] == 0.0 and f[2, 1] == 0.0
    assert st[0, 0, 2:].tolist() == [1, 31] and st[0, 1, 2:].tolist() == [0, 32]  # the NaN is a value
    assert st[0, 3].tolist() == [int(E.POS_INF_BITS), int(E.NEG_INF_BITS), 0, 32]
    assert out[0, 8].view(np.int64) == NULL_DOUBLE_BITS


def test_selection(mgr):
    n = TILE + 100
    rng = np.random.default_rng(11)
    cols = [rng.integers(-100, 100, n).astype(np.int64) for _ in range(5)]
    cols[3] = (rng.normal(size=n)).view(np.int64).copy()
    cols[1][::7] = NULL_I32
    check_call(mgr, cols, n, [(1,) + INT_SEL, (3,) + FP_SEL], 1024, cap_extra=3)  # two of five
    check_call(mgr, cols, n, [(4,) + INT_SEL, (0,) + INT_SEL, (3,) + FP_SEL, (2,) + INT_SEL, (1,) + INT_SEL], 1024)  # reordered
    check_call(mgr, cols, n, [(1,) + INT_SEL, (1, False, False, 0, 0), (1,) + INT_SEL], 4128)  # one column three times
    check_call(mgr, cols, n, [(1,) + INT_SEL], 1024, ocap=n + 5)  # one output column needs no aligned capacity
    check_call(mgr, cols, n, [(t % 5,) + (FP_SEL if t % 5 == 3 else INT_SEL) for t in range(16)], 2048)  # the limit


def test_seventeen_columns_are_refused(mgr):
    L = lib()
    arr = (A.ChunkCol * 17)()
    d = mgr.to_device(np.zeros(64 * 18 + 64, dtype=np.int64), 0)
    try:
        st = L.hdk_hip_chunk_columns(d.ptr, 32, 1, 32, arr, 17, 32, d.ptr + 32 * 8, 32, d.ptr + 32 * 18 * 8, None, 0, 0, None)
        assert st == A.ERR_INVALID_ARG and b"num_cols" in L.hdk_hip_last_error()
    finally:
        d.free()
