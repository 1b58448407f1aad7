"""Host-only parts of the device-side columnar results: the workspace arithmetic and the argument checks that come back
before any device is touched."""
import ctypes as C

import numpy as np

from hdk_amd import _abi as A
from hdk_amd._lib import lib
from hdk_amd.ir import Agg, ColRef, KeyRef, QueryUnit
from hdk_amd.plan import compile_query
from hdk_amd.storage import ArrowStorage


def test_workspace_bytes_is_host_arithmetic():
    f = lib().hdk_hip_result_columns_workspace_bytes
    assert f(1) > 0
    sizes = [f(n) for n in (0, 1, 4095, 4096, 4097, 10**6, 200_000_000, 2**31, 2**32 - 1)]
    assert sizes == sorted(sizes)
    assert f(200_000_000) >= 4 * (200_000_000 // 4096)   # one uint32 per tile of a few thousand entries
    assert f(2**32 - 1) <= 8 << 20                       # within a few MB even for the largest table


def _plan():
    st = ArrowStorage()
    st.import_numpy("t", {"k": np.arange(100, dtype=np.int64) % 10, "v": np.arange(100, dtype=np.int64)})
    return compile_query(st, QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0), Agg("sum", ColRef("v"))]))


def test_columnarize_checks_the_plan_before_any_device():
    L = lib()
    rows = C.c_uint64(0)
    iv = np.zeros(4, dtype=np.int64)
    # (the pointers are never dereferenced: the plan check comes first)
    assert L.hdk_hip_columnarize_result(None, 8, 10, iv.ctypes.data, None, 0, C.addressof(rows), None, 0, 0, None) == A.ERR_INVALID_ARG
    cp = _plan()
    bad = type(cp.plan).from_buffer_copy(cp.plan)
    bad.abi_version = 1
    st = L.hdk_hip_columnarize_result(C.byref(bad), 8, 10, iv.ctypes.data, None, 0, C.addressof(rows), None, 0, 0, None)
    assert st == A.ERR_INVALID_ARG and b"ABI" in L.hdk_hip_last_error()


def test_version_says_the_abi_grew():
    assert lib().hdk_hip_version() >= 1001


def test_dense_tail_gives_the_host_reader_rows(oracle):
    """The readers of dense columns (described_to_columns / described_to_arrow over describe_columns(cp): what
    DeviceColumns.to_columns() / to_arrow() call, and dense_to_columns) over the values the device writes (restated in numpy)
    equal the buffer's readers: names, order, None for NULL, AVG, decimal scale, and Arrow's names and types, a 4-byte
    COUNT's int32 among them."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from fuzz_queries import make_tables_wide, random_query_wide
    from hdk_amd.ir import QueryMustRunOnCpu
    from util import run_oracle
    rng = np.random.default_rng(5011)
    st = make_tables_wide(rng, 5000, 300)
    done = narrow_counts = 0
    for _ in range(30):
        q = random_query_wide(rng)
        try:
            cp, buf, err = run_oracle(oracle, st, q)
        except QueryMustRunOnCpu:
            continue
        if err or cp.plan.query_kind not in (A.Q_PERFECT_HASH, A.Q_BASELINE_HASH):
            continue
        narrow_counts += _assert_dense_readers_equal_the_buffers(cp, buf, q)
        done += 1
    assert done >= 15 and narrow_counts >= 1


def _assert_dense_readers_equal_the_buffers(cp, buf, q=None) -> bool:
    """-> whether the plan has a 4-byte COUNT"""
    from hdk_amd import result_set as rs
    from hdk_amd.plan import describe_columns
    dense = _device_values(cp, buf)
    schema = describe_columns(cp)
    want = rs.to_columns(cp, buf)
    got = rs.described_to_columns(schema, dense)
    assert got == want and list(got) == list(want), q
    assert rs.dense_to_columns(cp, dense) == want, q
    assert [rs.dense_column_null(cp, d.target_idx) for d in schema] == [(d.is_fp, d.nullable, d.null_bits) for d in schema]
    at, want_at = rs.described_to_arrow(schema, got), rs.columns_to_arrow(cp, want)
    assert at.schema == want_at.schema and at.equals(want_at), q
    return any(oc.agg == "count" and oc.type.size == 4 for oc in cp.out_cols)


def test_dictionary_keys_and_aggregates_read_as_the_buffer_does(oracle):
    """A dictionary-encoded key, and COUNT over a dictionary-encoded column (MIN / MAX over one the planner leaves to the
    CPU): names, values and Arrow types of the dense readers equal the buffer reader's."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pyarrow as pa
    import pytest
    from hdk_amd import result_set as rs
    from hdk_amd.ir import QueryMustRunOnCpu
    from util import run_oracle
    n = 600
    st = ArrowStorage()
    st.import_arrow(pa.table({"s": pa.array([("a", "b", None, "c")[i % 4] for i in range(n)]).dictionary_encode(),
                              "d": pa.array([("x", None, "y")[i % 3] for i in range(n)]).dictionary_encode(),
                              "v": pa.array(np.arange(n, dtype=np.int64) - 300)}), "t")
    for kind in ("min", "max"):
        with pytest.raises(QueryMustRunOnCpu):
            compile_query(st, QueryUnit("t", groupby=[ColRef("s")], targets=[KeyRef(0, "s"), Agg(kind, ColRef("d"))]))
    for bigint_count in (False, True):
        q = QueryUnit("t", groupby=[ColRef("s")], bigint_count=bigint_count,
                      targets=[KeyRef(0, "s"), Agg("count", ColRef("d"), "nd"), Agg("count", None, "n"), Agg("max", ColRef("v"), "mx")])
        cp, buf, err = run_oracle(oracle, st, q)
        assert err == 0
        assert _assert_dense_readers_equal_the_buffers(cp, buf, q) == (not bigint_count)
        cols = rs.to_columns(cp, buf)
        assert sorted(cols["s"], key=repr) == sorted(["a", "b", "c", None], key=repr) and sum(cols["nd"]) == 400


def _device_values(cp, buf):
    """The 8-byte value per target and non-empty entry, by the table of include/hdk_hip.h."""
    from hdk_amd import result_set as rs
    p = cp.plan
    n = int(p.entry_count)
    mask = rs.non_empty_mask(cp, buf, n)
    slots, keys = rs._slot_arrays(cp, buf, n), rs._key_arrays(cp, buf, n)
    out, s = [], 0
    for t in range(p.num_targets):
        tg = p.targets[t]
        a = (slots[s] if slots[s] is not None else keys[tg.key_idx])[mask].astype(np.int64)
        lo = (a & 0xFFFFFFFF).astype(np.uint32)
        if tg.agg == A.AGG_AVG:
            cnt = slots[s + 1][mask].astype(np.int64)
            dividend = lo.view(np.float32).astype(np.float64) if tg.arg_is_fp == A.FP_SLOT_FLOAT else \
                a.view(np.float64) if tg.arg_is_fp else a.astype(np.float64)
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
    return out


class _StubColumns:
    """Stands in for a DeviceColumns: every stage gives a new stub and is written into the shared log, as is free()."""

    def __init__(self, log, name="input", fail_at=None):
        self.log, self.name, self.fail_at, self.frees = log, name, fail_at, 0

    def _stage(self, what, *args):
        self.log.append((what, self.name) + args)
        if what == self.fail_at:
            raise RuntimeError(what)
        made = _StubColumns(self.log, what, self.fail_at)
        self.log.append(made)
        return made

    def filter(self, having):
        return self._stage("filter", having)

    def windows(self, windows):
        return self._stage("windows", windows)

    def project(self, outs):
        return self._stage("project", outs)

    def sort(self, order_by, limit=None, offset=0):
        return self._stage("sort", order_by, limit, offset)

    def free(self):
        self.frees += 1


def test_the_stage_pipeline_consumes_its_input():
    """executor.run_stages: HAVING, windows, select, sort in that order, each over the result of the one before; every
    block it no longer needs is freed exactly once, also when a stage raises; with no stage the input comes back as it is."""
    import pytest
    from hdk_amd.executor import run_stages
    log = []
    cols = _StubColumns(log)
    assert run_stages(cols) is cols and run_stages(cols, None, [], [], [], None, 0) is cols
    assert cols.frees == 0 and log == []

    got = run_stages(cols, "hv", ["w"], ["p"], ["o"], 5, 2)
    made = [x for x in log if isinstance(x, _StubColumns)]
    assert [x for x in log if not isinstance(x, _StubColumns)] == [
        ("filter", "input", "hv"), ("windows", "filter", ["w"]), ("project", "windows", ["p"]), ("sort", "project", ["o"], 5, 2)]
    assert got is made[-1] and got.name == "sort" and got.frees == 0
    assert cols.frees == 1 and [x.frees for x in made[:-1]] == [1, 1, 1]

    # a LIMIT or an OFFSET alone is a stage too
    for kw in ({"limit": 0}, {"offset": 3}):
        log.clear()
        cols = _StubColumns(log)
        got = run_stages(cols, **kw)
        assert got.name == "sort" and got.frees == 0 and cols.frees == 1
        assert log[0] == ("sort", "input", (), kw.get("limit"), kw.get("offset", 0))

    for fail_at, freed in (("filter", 0), ("windows", 1), ("project", 2), ("sort", 3)):
        log.clear()
        cols = _StubColumns(log, fail_at=fail_at)
        with pytest.raises(RuntimeError, match=fail_at):
            run_stages(cols, "hv", ["w"], ["p"], ["o"], 5, 2)
        made = [x for x in log if isinstance(x, _StubColumns)]
        assert cols.frees == 1 and [x.frees for x in made] == [1] * freed
