"""Host-only parts of the device ORDER BY / LIMIT: the expectation agrees with the reference's comparator, the workspace
arithmetic, the argument checks that come back before any device is touched, and the plan-level rejections."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd._lib import lib
from hdk_amd.ir import Agg, ColRef, KeyRef, OrderEntry, Proj, QueryMustRunOnCpu, QueryUnit
from hdk_amd.plan import compile_query
from hdk_amd.storage import ArrowStorage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sort_expect import comparator_perm, expected_perm, random_case  # noqa: E402


@pytest.mark.parametrize("seed", range(8))
def test_expectation_is_the_reference_comparator(seed):
    rng = np.random.default_rng(8100 + seed)
    cols, order = random_case(rng, 3000, 1 + seed % 3)
    assert np.array_equal(expected_perm(cols, order), comparator_perm(cols, order)), order


def test_workspace_bytes_is_host_arithmetic():
    f = lib().hdk_hip_sort_columns_workspace_bytes
    ns = (0, 1, 4095, 4096, 4097, 10**6, 100_000_000, 2**31, 2**32 - 1)
    sizes = [f(n, 1) for n in ns]
    assert sizes == sorted(sizes) and sizes[1] > 0
    for n, s in zip(ns, sizes):
        # two (8-byte key, 4-byte row) pairs a row, a quarter byte of digit counters, a fixed head
        assert 24 * n <= s <= 24.5 * n + (1 << 14), (n, s)
    assert f(10**6, 8) == f(10**6, 1)


def _entries(*es):
    arr = (A.OrderEntry * max(len(es), 1))()
    for i, e in enumerate(es):
        arr[i] = A.OrderEntry(*e)
    return arr


def test_invalid_arguments_come_back_before_any_device():
    L = lib()
    one = _entries((0, 0, 0, 0, 0, 0))
    ok_ptr = 4096  # (never dereferenced: every check comes first)

    def call(cols=ok_ptr, capacity=100, num_cols=2, num_rows=100, order=one, num_order=1, offset=0, limit=0, out=1 << 30,
             out_capacity=100):
        st = L.hdk_hip_sort_columns(cols, capacity, num_cols, num_rows, order, num_order, offset, limit, 0, out, out_capacity,
                                    None, None, 0, 0, None)
        return st, (L.hdk_hip_last_error() or b"").decode()

    for kw in ({"cols": None}, {"order": None}, {"out": None}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "NULL" in msg, kw
    for k in (0, 9, -1):
        st, msg = call(num_order=k)
        assert st == A.ERR_INVALID_ARG and "num_order" in msg
    for c in (-1, 2):
        st, msg = call(order=_entries((c, 0, 0, 0, 0, 0)))
        assert st == A.ERR_INVALID_ARG and "column" in msg
    st, msg = call(out_capacity=99)
    assert st == A.ERR_INVALID_ARG and "out_capacity" in msg
    # (5 rows remain after the offset of 95)
    st, msg = call(out_capacity=4, limit=10, offset=95)
    assert st == A.ERR_INVALID_ARG and "out_capacity" in msg
    st, msg = call(num_rows=101)
    assert st == A.ERR_INVALID_ARG and "capacity" in msg
    st, msg = call(num_rows=2**32, capacity=2**33, out_capacity=2**33)
    assert st == A.ERR_INVALID_ARG and "32-bit" in msg
    st, msg = call(out=ok_ptr + 8)
    assert st == A.ERR_INVALID_ARG and "overlap" in msg
    # nothing to do is not an error, and launches nothing
    assert call(num_rows=0)[0] == A.OK
    assert call(offset=100, out_capacity=0)[0] == A.OK
    assert call(offset=1000, limit=3, out_capacity=0)[0] == A.OK


def test_version_says_the_abi_grew():
    assert lib().hdk_hip_version() >= 1002


def _storage():
    st = ArrowStorage()
    st.import_numpy("t", {"k": np.arange(100, dtype=np.int64) % 10, "v": np.arange(100, dtype=np.int64)})
    st.import_arrow(__import__("pyarrow").table({"s": ["a", "b", "a", "c"], "v": [1, 2, 3, 4]}), "d")
    return st


def _q(**kw):
    return QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s"), Agg("count", name="n")], **kw)


def test_defaults_leave_the_compiled_plan_alone():
    st = _storage()
    base = compile_query(st, _q())
    assert base.order_by == [] and QueryUnit("t").order_by == [] and QueryUnit("t").limit is None and QueryUnit("t").offset == 0
    sorted_cp = compile_query(st, _q(order_by=[OrderEntry("n", desc=True), OrderEntry(0, nulls_first=True)], limit=3, offset=1))
    assert bytes(base.plan) == bytes(sorted_cp.plan)  # nothing of the plan changes: sorting happens on the result
    assert sorted_cp.order_by == [(2, True, False), (0, False, True)]
    assert np.array_equal(base.init_vals, sorted_cp.init_vals) and base.slot_widths == sorted_cp.slot_widths


def test_compile_query_rejections():
    st = _storage()
    with pytest.raises(ValueError):
        compile_query(st, _q(order_by=[OrderEntry("nope")]))
    with pytest.raises(ValueError):
        compile_query(st, _q(order_by=[OrderEntry(3)]))
    with pytest.raises(QueryMustRunOnCpu):
        compile_query(st, _q(order_by=[OrderEntry(i % 3) for i in range(9)]))
    with pytest.raises(QueryMustRunOnCpu):
        compile_query(st, QueryUnit("d", groupby=[ColRef("s")], targets=[KeyRef(0, "s"), Agg("count", name="n")],
                                    order_by=[OrderEntry("s")]))
    # (ordering such a result by its aggregate is fine)
    compile_query(st, QueryUnit("d", groupby=[ColRef("s")], targets=[KeyRef(0, "s"), Agg("count", name="n")],
                                order_by=[OrderEntry("n")]))
    with pytest.raises(QueryMustRunOnCpu):
        compile_query(st, QueryUnit("t", targets=[Proj(ColRef("v"), "v")], limit=5))
    with pytest.raises(QueryMustRunOnCpu):
        compile_query(st, QueryUnit("t", targets=[Agg("sum", ColRef("v"), "s")], order_by=[OrderEntry("s")]))
    with pytest.raises(QueryMustRunOnCpu):
        compile_query(st, QueryUnit("t", targets=[Agg("sum", ColRef("v"), "s")], offset=1))


def test_buffer_result_with_sort_info_is_an_error():
    from hdk_amd.executor import Executor
    ex = Executor.__new__(Executor)  # (the check comes before anything touches the device or the storage)
    for kw in ({"order_by": [OrderEntry("n")]}, {"limit": 3}, {"offset": 2}):
        with pytest.raises(ValueError, match="columns"):
            ex.execute(_q(**kw), result="buffer")
        with pytest.raises(ValueError, match="columns"):
            ex.execute(_q(**kw))


def test_dense_null_helper_agrees_with_the_dense_reader(oracle):
    """A value equal to dense_column_null's null_bits reads as None through dense_to_columns when the column is nullable,
    and as a value when it is not, over the wide fuzz plans."""
    from fuzz_queries import make_tables_wide, random_query_wide
    from util import run_oracle
    rng = np.random.default_rng(5011)
    st = make_tables_wide(rng, 5000, 300)
    done = 0
    for _ in range(30):
        q = random_query_wide(rng)
        try:
            cp, buf, err = run_oracle(oracle, st, q)
        except QueryMustRunOnCpu:
            continue
        if err or cp.plan.query_kind not in (A.Q_PERFECT_HASH, A.Q_BASELINE_HASH):
            continue
        nt = int(cp.plan.num_targets)
        infos = [rs.dense_column_null(cp, t) for t in range(nt)]
        dense = []
        for t, (is_fp, nullable, null_bits) in enumerate(infos):
            other = A.to_i64(int(np.float64(1.5).view(np.int64))) if is_fp else 1
            dense.append(np.array([A.to_i64(null_bits), other], dtype=np.int64))
        got = rs.dense_to_columns(cp, dense)
        for oc in cp.out_cols:
            is_fp, nullable, _ = infos[oc.target_idx]
            if oc.dictionary is not None:
                continue  # (ids index the dictionary: such a key is not sortable on the device anyway)
            assert (got[oc.name][0] is None) == nullable, (q, oc)
            assert got[oc.name][1] is not None
            assert isinstance(got[oc.name][1], float) == (is_fp or bool(oc.scale)), (q, oc)
        done += 1
    assert done >= 15
