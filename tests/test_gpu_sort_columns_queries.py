"""ORDER BY / LIMIT / OFFSET through the query path: Executor.execute(QueryUnit(order_by=...), result="columns"),
DeviceColumns.sort and Engine.run.  The expectation is sort_expect.expected_perm applied to the UNSORTED dense columns of
the same query."""
import dataclasses

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd.ir import FP64, Agg, ColRef, KeyRef, OrderEntry, QueryMustRunOnCpu, QueryUnit
from hdk_amd.plan import compile_query
from hdk_amd.storage import ArrowStorage

from fuzz_queries import make_tables_wide, random_query_wide
from sort_expect import expected_perm, out_rows_of

pytestmark = pytest.mark.gpu


def _entries(cp):
    return [(t, desc, nulls_first) + rs.dense_column_null(cp, t) for t, desc, nulls_first in cp.order_by]


def _take(columns, perm):
    return {name: [vals[i] for i in perm.tolist()] for name, vals in columns.items()}


def _expected(cp, unsorted, limit, offset):
    """to_columns() of the sorted result, from the unsorted DeviceColumns."""
    words = [c.view(np.int64) for c in unsorted.to_host()]
    perm = expected_perm(words, _entries(cp)) if cp.order_by else np.arange(unsorted.num_rows, dtype=np.uint32)
    out_rows = out_rows_of(unsorted.num_rows, limit or 0, offset)
    if limit == 0:
        out_rows = 0
    return _take(unsorted.to_columns(), perm[offset:offset + out_rows]), perm[offset:offset + out_rows]


def _storage():
    rng = np.random.default_rng(2026)
    n = 60_000
    k = rng.integers(0, 3000, n).astype(np.int64)
    k32 = rng.integers(-2000, 2000, n).astype(np.int32)
    k32[rng.random(n) < 0.01] = A.NULL_INT
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    w = rng.integers(-50, 50, n).astype(np.int64)
    w[rng.random(n) < 0.5] = A.NULL_BIGINT
    f = (rng.normal(size=n) * 10).astype(np.float32)
    # (+ 0.0 turns the -0.0 that rounding (-0.5, 0) gives into +0.0: the group-by keeps the two as separate groups, the
    # device orders -0.0 before +0.0 and the expectation calls them a tie; that order has its own test in
    # test_gpu_sort_columns.py)
    dk = np.round(rng.normal(size=n) * 20, 0) + 0.0
    st = ArrowStorage()
    st.import_numpy("t", {"k": k, "k32": k32, "v": v, "w": w, "f": f, "dk": dk}, fragment_size=25_000)
    return st


# (every order ends in the unique group key or runs on a perfect-hash layout: the unsorted and the sorted execution are two
# runs, and only a total order makes them comparable row by row whatever the entry order of an open-addressing table is)
_QUERIES = {
    "perfect_count_desc_limit": QueryUnit(
        "t", groupby=[ColRef("k")],
        targets=[KeyRef(0, "k"), Agg("count", name="n"), Agg("sum", ColRef("v"), "s"), Agg("avg", ColRef("w"), "a")],
        order_by=[OrderEntry("n", desc=True), OrderEntry("k")], limit=10),
    "baseline_nullable_k32_nulls_first": QueryUnit(
        "t", groupby=[ColRef("k32")], force_baseline=True,
        targets=[KeyRef(0, "k32"), Agg("count", name="n"), Agg("max", ColRef("w"), "m")],
        order_by=[OrderEntry("k32", nulls_first=True)]),
    "float_min_desc": QueryUnit(
        "t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("min", ColRef("f"), "fm")],
        order_by=[OrderEntry("fm", desc=True), OrderEntry(0)], limit=100, offset=5),
    "double_key": QueryUnit(
        "t", groupby=[ColRef("dk")], targets=[KeyRef(0, "dk"), Agg("sum", ColRef("v"), "s")],
        order_by=[OrderEntry("dk", desc=True)], offset=3),
    "avg_nulls_last_then_key": QueryUnit(
        "t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("avg", ColRef("w"), "a")],
        order_by=[OrderEntry("a"), OrderEntry("k", desc=True)]),
    "limit_only": QueryUnit(
        "t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("count", name="n")], limit=17, offset=4),
}


@pytest.fixture(scope="module")
def storage():
    return _storage()


@pytest.mark.parametrize("name", sorted(_QUERIES))
def test_execute_applies_the_sort_info(gpu_executor_factory, storage, name):
    q = _QUERIES[name]
    ex = gpu_executor_factory(storage)
    cp = compile_query(storage, q)
    plain = dataclasses.replace(q, order_by=[], limit=None, offset=0)
    unsorted = ex.execute(plain, result="columns")
    got = ex.execute(q, result="columns")
    try:
        want, perm = _expected(cp, unsorted, q.limit, q.offset)
        assert got.num_rows == len(perm) == got.capacity and len(perm) > 0
        assert got.to_columns() == want
        if name == "perfect_count_desc_limit":
            assert want["n"] == sorted(want["n"], reverse=True) and len(want["n"]) == 10
    finally:
        unsorted.free()
        got.free()


def test_engine_run_gives_the_sorted_arrow_table(storage):
    from hdk_amd.engine import Engine
    eng = Engine()
    eng.storage = storage
    q = _QUERIES["perfect_count_desc_limit"]
    plain = dataclasses.replace(q, order_by=[], limit=None, offset=0)
    cp = compile_query(storage, q)
    unsorted = eng.execute(plain, result="columns")
    try:
        _, perm = _expected(cp, unsorted, q.limit, q.offset)
        want = unsorted.to_arrow().take(perm.astype(np.int64))
    finally:
        unsorted.free()
    got = eng.run(q, result="columns")
    assert got.equals(want) and got.num_rows == 10
    with pytest.raises(ValueError):
        eng.run(q)  # result="buffer": a hash table has no row order


def test_sort_twice_and_after_free_of_the_source(gpu_executor_factory, storage):
    q = _QUERIES["avg_nulls_last_then_key"]
    ex = gpu_executor_factory(storage)
    cp = compile_query(storage, q)
    unsorted = ex.execute(dataclasses.replace(q, order_by=[], limit=None, offset=0), result="columns")
    want, _ = _expected(cp, unsorted, None, 0)
    once = unsorted.sort(q.order_by)
    assert unsorted.to_columns() != want and unsorted.num_rows == once.num_rows  # the source stays as it was
    unsorted.free()
    assert once.to_columns() == want
    twice = once.sort(cp.order_by, no_select=True)  # sorting a sorted result changes nothing
    once.free()
    assert twice.to_columns() == want
    top = twice.sort([OrderEntry("k")], limit=5)
    twice.free()
    assert top.to_columns()["k"] == sorted(want["k"])[:5] and top.capacity == 5
    none = top.sort([OrderEntry("k")], offset=5)
    assert none.num_rows == 0 and none.to_columns() == {"k": [], "a": []}
    top.free()


FUZZ_SEED, FUZZ_QUERIES = 5013, 20


def fuzz_cases(storage_of, seed=FUZZ_SEED, count=FUZZ_QUERIES):
    """[(query with a random 1-3-entry order_by / limit / offset, compiled plan)] of the seeded wide generator's group-bys;
    plans that must run on the CPU (dictionary keys in the order included) are left out."""
    rng = np.random.default_rng(seed)
    st = storage_of(rng)
    cases = []
    for _ in range(count):
        q = random_query_wide(rng)
        nt = len(q.targets)
        order = [OrderEntry(int(t), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
                 for t in rng.permutation(nt)[:int(rng.integers(1, 4))]]
        limit = [None, 1, 10, 1000][int(rng.integers(0, 4))]
        offset = [0, 0, 3][int(rng.integers(0, 3))]
        if not q.groupby:
            continue
        q = dataclasses.replace(q, order_by=order, limit=limit, offset=offset)
        try:
            cp = compile_query(st, q)
        except QueryMustRunOnCpu:
            continue
        if cp.plan.query_kind in (A.Q_PERFECT_HASH, A.Q_BASELINE_HASH):
            cases.append((q, cp))
    return st, cases


def test_fuzz_group_bys_with_random_orders(gpu_executor_factory):
    st, cases = fuzz_cases(lambda rng: make_tables_wide(rng, 20_000, 700))
    ex = gpu_executor_factory(st)
    ran = 0
    for q, cp in cases:
        step = ex.prepare(cp)
        try:
            step.enqueue()
            unsorted = step.fetch_columns()  # (one block, sorted in place of a second run: ties keep ITS row order)
        finally:
            step.free()
        try:
            want, perm = _expected(cp, unsorted, q.limit, q.offset)
            for no_select in (False, True):
                got = unsorted.sort(cp.order_by, q.limit, q.offset, no_select=no_select)
                try:
                    assert got.num_rows == len(perm), q
                    assert got.to_columns() == want, q
                finally:
                    got.free()
        finally:
            unsorted.free()
        ran += 1
    assert ran >= 10
