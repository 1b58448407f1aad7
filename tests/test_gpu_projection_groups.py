"""The two-pass filter/project kernels in the form every large launch takes: a block's tiles in groups of four (one
block-wide scan and one barrier per group, hdk_amd/csrc/scan_project_fast.h).  A group needs more than 3 x grid tiles of
one fragment, so these tests pin the grid (Executor.prepare(grid=...)) and reach it with 86 K - 147 K rows: the tables,
queries and numpy expectations of projection_cases.py, which test_projection.py has checked against the oracle."""
import numpy as np
import pytest

import projection_cases as pc
from test_projection import run_projection_oracle

pytestmark = pytest.mark.gpu

WRITERS = (None, "sparse", "dense")  # HDK_HIP_PROJECT_WRITER: the device's choice, or either writing pass forced
POISON = 0x5A5A5A5A5A5A5A5A

_cases, _numpy, _oracle, _executors = {}, {}, {}, {}


def _case(layout):
    if layout not in _cases:
        _cases[layout] = pc.Case(layout)
    return _cases[layout]


def _want(layout, name, join=False):
    """the sorted numpy rows, once per layout and query"""
    key = (layout, name, join)
    if key not in _numpy:
        _numpy[key] = pc.expected_rows(_case(layout), name, join=join)
    return _numpy[key]


def _plan(oracle, layout, name, columnar, join=False):
    """(compiled plan, the oracle's sorted rows), once per layout, query and buffer form"""
    key = (layout, name, columnar, join)
    if key not in _oracle:
        cp, buf, err, n = run_projection_oracle(oracle, _case(layout).st, pc.query(name, columnar, join=join))
        assert err == 0
        _oracle[key] = (cp, pc.buffer_rows(cp, buf, n))
    return _oracle[key]


def _executor(factory, layout, fused=True):
    key = (layout, fused)
    if key not in _executors:
        _executors[key] = factory(_case(layout).st)
        _executors[key].fuse_join_tables = fused
    return _executors[key]


def _set_writer(monkeypatch, writer):
    if writer is None:
        monkeypatch.delenv("HDK_HIP_PROJECT_WRITER", raising=False)
    else:
        monkeypatch.setenv("HDK_HIP_PROJECT_WRITER", writer)


def _run_twice(ex, cp, grid, total_rows=None):
    """(result, kernel names) of a step run twice: the second run leaves the same bytes (the output
    order is a function of the input and the grid, not of the schedule)"""
    step = ex.prepare(cp, grid=grid)
    try:
        names = step.kernel_names()
        if total_rows is not None:
            step.ko.total_rows = total_rows
        res = step.run()
        again = step.run()
    finally:
        step.free()
    assert again.total_matched == res.total_matched and again.error_code == res.error_code
    assert np.array_equal(res.buffer, again.buffer), "a second run of the same step wrote other bytes"
    return res, names


@pytest.mark.parametrize("grid", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", list(pc.LAYOUTS))
def test_groups_match_numpy_and_oracle(oracle, gpu_executor_factory, monkeypatch, layout, grid):
    ex = _executor(gpu_executor_factory, layout)
    cells = [(w, {}, None) for w in WRITERS]
    if grid in (2, 3):
        # the one-pass kernel with one status word: it hands the launch to the two passes armed behind it, which then
        # run without a mask under the small grid
        cells.append((None, {"HDK_HIP_PROJECT_ONE_PASS": "1", "HDK_HIP_PROJECT_STATUS_SLACK": "0"}, 1))
    for writer, env, total_rows in cells:
        _set_writer(monkeypatch, writer)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for name in pc.FILTERS:
            want = _want(layout, name)
            for columnar in (False, True):
                cp, oracle_rows = _plan(oracle, layout, name, columnar)
                what = (layout, grid, writer, env, name, columnar)
                res, names = _run_twice(ex, cp, grid, total_rows)
                assert names.endswith("hdk_scan_project_direct"), what
                assert names.startswith("hdk_scan_project_stream") == bool(env), what
                assert res.error_code == 0 and res.total_matched == len(want), what
                got = pc.buffer_rows(cp, res.buffer, len(want))
                assert np.array_equal(got, want), what
                assert np.array_equal(got, oracle_rows), what
        for k in env:
            monkeypatch.delenv(k)


def _tiles_in_output_order(gpu_executor_factory, oracle, grid):
    case = _case("L2")
    cp, _ = _plan(oracle, "L2", "a32<600", True)
    res, _ = _run_twice(_executor(gpu_executor_factory, "L2"), cp, grid)
    rows = pc.buffer_rows(cp, res.buffer, res.total_matched, sort=False)
    tiles = case.tile_of_rid(rows[:, 1 + pc.TARGETS.index("rid")])
    first = np.concatenate([[True], tiles[1:] != tiles[:-1]])
    return case, tiles[first].tolist()


def test_a_callers_grid_is_honoured(oracle, gpu_executor_factory, monkeypatch):
    """The dense writing pass lays its rows out tile after tile, block after block, and block b takes the launch's tiles
    b, b + grid, ...: with two blocks the even tiles come out first, then the odd ones; with one block they ascend.  The
    rest of this file reaches the grouped form only as long as this holds."""
    _set_writer(monkeypatch, "dense")
    case, tiles = _tiles_in_output_order(gpu_executor_factory, oracle, 2)
    assert tiles == list(range(0, case.num_tiles, 2)) + list(range(1, case.num_tiles, 2))
    case, tiles = _tiles_in_output_order(gpu_executor_factory, oracle, 1)
    assert tiles == list(range(case.num_tiles))


def test_mask_ends_inside_a_group(gpu_executor_factory, monkeypatch):
    """1077 tiles against a selection mask of 1024 (total_rows = 1: the mask's slack alone, which is what forces this
    size): inside the fourth fragment (tiles 954..1076) a block goes from groups of masked tiles to single masked tiles to
    tiles that evaluate the filter again."""
    targets = ["rid", "a", "b"]
    case = pc.Case("mask", frag_rows=[1_300_007] * 3 + [499_979], columns=targets, seed=4200)
    assert case.num_tiles == 1077 and case.frag_tile_base[3] == 954
    ex = gpu_executor_factory(case.st)
    for name in ("a<37", "a<600"):
        keep = pc.keep_mask(case, name)
        want = np.stack([case.pos[keep]] + [case.cols[t][keep].astype(np.int64) for t in targets], axis=1)  # by rid
        cp = ex.compile(pc.query(name, True, targets=targets))
        for writer in ("sparse", "dense"):
            _set_writer(monkeypatch, writer)
            step = ex.prepare(cp, grid=3)
            step.ko.total_rows = 1
            res = step.run()
            step.free()
            assert res.error_code == 0 and res.total_matched == len(want), (name, writer)
            got = pc.buffer_rows(cp, res.buffer, len(want), sort=False)
            assert np.array_equal(got[np.argsort(got[:, 1], kind="stable")], want), (name, writer)


@pytest.mark.parametrize("grid", [0, 2])
def test_limit_rows_are_real_and_nothing_is_written_outside(gpu_executor_factory, monkeypatch, grid):
    """A LIMIT below the number of qualifying rows: the buffer holds `limit` distinct rows of the full result, the
    counter keeps counting, the error code is negative, and not a byte outside the caller's buffer changes."""
    import torch
    case = _case("L2")
    ex = _executor(gpu_executor_factory, "L2")
    dev = torch.device("cuda", 0)
    for name in ("a<600", "a32<600"):
        keep = pc.keep_mask(case, name)
        full = np.stack([case.pos[keep]] + [c[keep].view(np.int64) if c.dtype.kind == "f" else c[keep].astype(np.int64)
                                            for c in (case.cols[t] for t in pc.TARGETS)], axis=1)  # in rid order
        full_rid = full[:, 1]
        M = len(full)
        assert M >= 2
        for limit in (M, M - 1, M // 2 + 1, 1):
            for columnar in (False, True):
                cp = ex.compile(pc.query(name, columnar, scan_limit=limit))
                assert cp.entry_count == limit and cp.buffer_bytes % 8 == 0
                words = cp.buffer_bytes // 8
                for writer in ("sparse", "dense"):
                    what = (grid, name, limit, columnar, writer)
                    _set_writer(monkeypatch, writer)
                    out = torch.full((words + 1024,), POISON, dtype=torch.int64, device=dev)
                    torch.cuda.synchronize()
                    step = ex.prepare(cp, grid=grid, out_ptr=out.data_ptr() + 512 * 8)
                    res = step.run()
                    step.free()
                    host = out.cpu().numpy()
                    assert (host[:512] == POISON).all() and (host[512 + words:] == POISON).all(), what
                    assert res.total_matched == M, what
                    assert (res.error_code == 0) if limit >= M else (res.error_code < 0), what
                    assert res.row_count() == min(limit, M), what
                    got = pc.buffer_rows(cp, host[512:512 + words], min(limit, M), sort=False)
                    at = np.minimum(np.searchsorted(full_rid, got[:, 1]), M - 1)
                    assert np.array_equal(full[at], got), what  # each one a row of the full result (poison is none)
                    assert len(np.unique(got[:, 1])) == len(got), what


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("grid", [1, 3])
def test_join_through_groups(oracle, gpu_executor_factory, grid, fused):
    """One inner one-to-one join (NULL keys, keys without a partner): the counting pass probes, the sparse writing pass
    gathers the joined column, in groups of four tiles."""
    ex = _executor(gpu_executor_factory, "L2", fused)
    for name in pc.JOIN_FILTERS:
        want = _want("L2", name, join=True)
        for columnar in (False, True):
            cp, oracle_rows = _plan(oracle, "L2", name, columnar, join=True)
            res, names = _run_twice(ex, cp, grid)
            assert names.startswith("hdk_scan_project_count,hdk_scan_project_offsets"), names
            assert res.error_code == 0 and res.total_matched == len(want), (grid, fused, name, columnar)
            got = pc.buffer_rows(cp, res.buffer, len(want))
            assert np.array_equal(got, want), (grid, fused, name, columnar)
            assert np.array_equal(got, oracle_rows), (grid, fused, name, columnar)
