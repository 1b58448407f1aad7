"""HAVING through the query path: Executor.execute(QueryUnit(having=...), result="columns"), DeviceColumns.filter and
Engine.run.  The exact check filters the SAME DeviceColumns object and compares with having_expect applied to its
to_host(); the execute() path runs the group-by again and is compared after an order that ends in the unique key, or as
row sets (the entry order of an open-addressing table is not fixed between runs)."""
import dataclasses

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd.ir import FP64, Agg, And, Cast, Cmp, ColRef, KeyRef, Lit, Not, Or, OrderEntry, QueryMustRunOnCpu, QueryUnit, TargetRef
from hdk_amd.plan import compile_query, resolve_having
from hdk_amd.storage import ArrowStorage

from fuzz_queries import make_tables_wide, random_query_wide
from having_expect import expected_rows
from sort_expect import expected_perm

pytestmark = pytest.mark.gpu


def _storage():
    rng = np.random.default_rng(2027)
    n = 60_000
    k = rng.integers(0, 3000, n).astype(np.int64)
    k32 = rng.integers(-2000, 2000, n).astype(np.int32)
    k32[rng.random(n) < 0.01] = A.NULL_INT
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    w = rng.integers(-50, 50, n).astype(np.int64)
    w[rng.random(n) < 0.9] = A.NULL_BIGINT  # (sparse enough for groups whose AVG / MAX is NULL)
    f = (rng.normal(size=n) * 10).astype(np.float32)
    st = ArrowStorage()
    st.import_numpy("t", {"k": k, "k32": k32, "v": v, "w": w, "f": f}, fragment_size=25_000)
    return st


def T(x):
    return TargetRef(x)


_PERFECT = dict(groupby=[ColRef("k")],
                targets=[KeyRef(0, "k"), Agg("count", name="n"), Agg("sum", ColRef("v"), "s"), Agg("avg", ColRef("w"), "a")])
_QUERIES = {
    "perfect_count_and_nullable_avg": QueryUnit("t", **_PERFECT, having=[Cmp(T("n"), ">", Lit(18)), Cmp(T("a"), "<", Lit(5))]),
    "baseline_nullable_k32_key_and_max": QueryUnit(
        "t", groupby=[ColRef("k32")], force_baseline=True,
        targets=[KeyRef(0, "k32"), Agg("count", name="n"), Agg("max", ColRef("w"), "m")],
        having=[Cmp(T("k32"), ">=", Lit(0)), Cmp(T("m"), ">", Lit(10))]),
    "float_min_against_a_float_literal": QueryUnit(
        "t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("min", ColRef("f"), "fm")],
        having=[Cmp(T("fm"), "<", Lit(-15.5))]),
    "target_against_target": QueryUnit("t", **_PERFECT, having=[Cmp(T("s"), ">", T("n"))]),
    "literal_on_the_left_or_not": QueryUnit(
        "t", **_PERFECT, having=[Or(Cmp(Lit(25), "<", T(1)), Not(Cmp(T("a"), ">=", Lit(0.0)))), Cmp(T("k"), "<>", Lit(7))]),
    "having_order_limit_offset": QueryUnit(
        "t", **_PERFECT, having=[Cmp(T("n"), ">", Lit(18)), Cmp(T("a"), "<", Lit(5))],
        order_by=[OrderEntry("n", desc=True), OrderEntry("k")], limit=10, offset=2),
    "baseline_having_then_order_by_key": QueryUnit(
        "t", groupby=[ColRef("k32")], force_baseline=True,
        targets=[KeyRef(0, "k32"), Agg("count", name="n"), Agg("max", ColRef("w"), "m")],
        having=[And(Cmp(T("k32"), ">=", Lit(0)), Cmp(T("n"), ">=", Lit(15)))], order_by=[OrderEntry("k32", desc=True)], offset=1),
    "nothing_passes": QueryUnit("t", **_PERFECT, having=[Cmp(T("n"), ">", Lit(10**6))]),
    "everything_passes": QueryUnit("t", **_PERFECT, having=[Cmp(T("n"), ">=", Lit(1))]),
}


@pytest.fixture(scope="module")
def storage():
    return _storage()


def _rows(columns):
    names = list(columns)
    return sorted(zip(*[columns[c] for c in names]), key=repr)


def _take(columns, idx):
    return {name: [vals[i] for i in idx.tolist()] for name, vals in columns.items()}


def _plain(q):
    return dataclasses.replace(q, having=[], order_by=[], limit=None, offset=0)


def _check_filter_of(cols, cp, conds):
    """cols.filter(conds) and cols.filter(resolved) against having_expect on cols.to_host() -> the expected row indices"""
    hv = resolve_having(cp, conds)
    words = [c.view(np.int64) for c in cols.to_host()]
    want = expected_rows(words, hv.leaves, hv.prog)
    for arg in (conds, hv):
        kept = cols.filter(arg)
        try:
            assert kept.num_rows == len(want)
            assert kept.block is not None or len(want) == 0
            for t, c in enumerate(kept.to_host()):
                assert np.array_equal(c.view(np.int64), words[t][want]), t
        finally:
            kept.free()
    assert all(np.array_equal(c.view(np.int64), w) for c, w in zip(cols.to_host(), words))  # the source stays valid
    return want


@pytest.mark.parametrize("name", sorted(_QUERIES))
def test_execute_applies_having(gpu_executor_factory, storage, name):
    q = _QUERIES[name]
    ex = gpu_executor_factory(storage)
    cp = compile_query(storage, q)
    unfiltered = got = None
    try:
        unfiltered = ex.execute(_plain(q), result="columns")
        got = ex.execute(q, result="columns")
        want = _check_filter_of(unfiltered, cp, q.having)
        if name == "nothing_passes":
            assert len(want) == 0 and got.num_rows == 0 and got.block is None
        elif name == "everything_passes":
            assert len(want) == unfiltered.num_rows > 0
        else:
            assert 0 < len(want) < unfiltered.num_rows
        words = [c.view(np.int64)[want] for c in unfiltered.to_host()]
        kept_cols = _take(unfiltered.to_columns(), want)
        if q.order_by:  # (ends in the unique key: comparable row by row)
            entries = [(t, d, nf) + rs.dense_column_null(cp, t) for t, d, nf in cp.order_by]
            perm = expected_perm(words, entries)[q.offset:]
            if q.limit is not None:
                perm = perm[:q.limit]
            assert got.num_rows == len(perm) > 0
            assert got.to_columns() == _take(kept_cols, perm)
        else:
            assert got.num_rows == len(want)
            assert _rows(got.to_columns()) == _rows(kept_cols)
    finally:
        for c in (unfiltered, got):
            if c is not None:
                c.free()


def test_null_groups_do_not_pass(gpu_executor_factory, storage):
    """`a < 5` drops the groups whose AVG is NULL, and so does NOT (a < 5): NULL is not TRUE either way."""
    ex = gpu_executor_factory(storage)
    q = QueryUnit("t", **_PERFECT)
    cp = compile_query(storage, q)
    cols = ex.execute(q, result="columns")
    try:
        a = cols.to_columns()["a"]
        nulls = sum(x is None for x in a)
        assert 0 < nulls < len(a)
        lt = _check_filter_of(cols, cp, [Cmp(T("a"), "<", Lit(5))])
        ge = _check_filter_of(cols, cp, [Not(Cmp(T("a"), "<", Lit(5)))])
        assert len(lt) + len(ge) == len(a) - nulls and len(lt) and len(ge)
    finally:
        cols.free()


def test_engine_run_gives_the_filtered_arrow_table(storage):
    from hdk_amd.engine import Engine
    eng = Engine()
    eng.storage = storage
    q = _QUERIES["having_order_limit_offset"]
    got = eng.run(q, result="columns")
    assert got.num_rows == 10
    n, a = got.column("n").to_pylist(), got.column("a").to_pylist()
    assert all(x > 18 for x in n) and all(x is not None and x < 5 for x in a) and n == sorted(n, reverse=True)
    with pytest.raises(ValueError, match="columns"):
        eng.run(dataclasses.replace(q, order_by=[], limit=None, offset=0))  # result="buffer"


def test_the_large_result_path_counts_first(gpu_executor_factory, storage):
    """Above FILTER_ONE_CALL_BYTES of worst-case output the passing rows are counted first and the block is exact."""
    from hdk_amd.executor import DeviceColumns
    ex = gpu_executor_factory(storage)
    q = _QUERIES["perfect_count_and_nullable_avg"]
    cp = compile_query(storage, q)
    cols = ex.execute(_plain(q), result="columns")
    old = DeviceColumns.FILTER_ONE_CALL_BYTES
    try:
        one_call = cols.filter(q.having)
        assert one_call.capacity == cols.num_rows
        DeviceColumns.FILTER_ONE_CALL_BYTES = 1024
        want = _check_filter_of(cols, cp, q.having)
        exact = cols.filter(q.having)
        assert exact.capacity == exact.num_rows == len(want) == one_call.num_rows
        assert all(np.array_equal(x, y) for x, y in zip(exact.to_host(), one_call.to_host()))
        exact.free()
        one_call.free()
    finally:
        DeviceColumns.FILTER_ONE_CALL_BYTES = old
        cols.free()


def test_having_survives_the_out_of_slots_retry(gpu_executor_factory):
    """A planner-sized open-addressing table that is too small (statistics narrower than the data): execute() re-runs with
    a doubled guess and still applies the HAVING to the result of the run that fitted."""
    from hdk_amd import plan as P
    from hdk_amd.storage import ChunkStats
    rng = np.random.default_rng(43)
    n = 60_000
    st = ArrowStorage()
    st.import_numpy("t", {"x": rng.integers(1, 5_001, n).astype(np.int32), "v": rng.integers(-100, 100, n, dtype=np.int64)},
                    fragment_size=20_000)
    having = [Cmp(T("c"), ">", Lit(12)), Cmp(T("k"), "<", Lit(4000.5))]
    q = QueryUnit("t", groupby=[Cast(ColRef("x"), FP64)], targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s"), Agg("count", None, "c")],
                  having=having)
    ex = gpu_executor_factory(st)
    pinned = dataclasses.replace(q, having=[], baseline_entry_count=16_384)
    whole = ex.execute(pinned, result="columns")
    try:
        want = _check_filter_of(whole, compile_query(st, pinned), having)
        want_rows = _rows(_take(whole.to_columns(), want))
    finally:
        whole.free()
    col = st.get("t").columns["x"]
    col.stats = [ChunkStats(1, 5, False) for _ in col.stats]
    ex = gpu_executor_factory(st)
    old = P.BIG_GROUP_THRESHOLD
    P.BIG_GROUP_THRESHOLD = 1_000  # (so that 60 K rows count as a big input and the NDV bound is what sizes the table)
    try:
        assert ex.compile(q).entry_count < 100
        got = ex.execute(q, result="columns")
    finally:
        P.BIG_GROUP_THRESHOLD = old
    try:
        assert got.compiled.entry_count == 16_384
        assert 0 < got.num_rows == len(want_rows) < 5000
        assert _rows(got.to_columns()) == want_rows
    finally:
        got.free()


def _random_having(rng, cp, host):
    """1-3 leaves over the plan's eligible targets, literals taken from the result itself, under a random connective"""
    ok = [oc.target_idx for oc in cp.out_cols if oc.dictionary is None and oc.type.kind not in ("dict", "decimal") and not oc.scale]
    if not ok:
        return None
    ops = ["=", "<>", "<", ">", "<=", ">="]
    leaves = []
    for _ in range(int(rng.integers(1, 4))):
        t = int(rng.choice(ok))
        op = ops[int(rng.integers(0, 6))]
        if rng.random() < 0.3:
            leaves.append(Cmp(T(t), op, T(int(rng.choice(ok)))))
            continue
        x = host[t][int(rng.integers(0, len(host[t])))]
        lit = Lit(float(x)) if host[t].dtype == np.float64 else Lit(int(x))
        leaves.append(Cmp(lit, op, T(t)) if rng.random() < 0.2 else Cmp(T(t), op, lit))
    cond = leaves[0]
    for lf in leaves[1:]:
        cond = (And, Or)[int(rng.integers(0, 2))](cond, lf)
        if rng.random() < 0.3:
            cond = Not(cond)
    return [cond] if rng.random() < 0.7 else leaves


def test_fuzz_group_bys_with_random_havings(gpu_executor_factory):
    rng = np.random.default_rng(5017)
    st = make_tables_wide(rng, 20_000, 700)
    ex = gpu_executor_factory(st)
    ran = 0
    for _ in range(24):
        q = random_query_wide(rng)
        if not q.groupby:
            continue
        try:
            cp = compile_query(st, q)
        except QueryMustRunOnCpu:
            continue
        if cp.plan.query_kind not in (A.Q_PERFECT_HASH, A.Q_BASELINE_HASH):
            continue
        step = ex.prepare(cp)
        try:
            step.enqueue()
            cols = step.fetch_columns()
        finally:
            step.free()
        try:
            if cols.num_rows == 0:
                continue
            conds = _random_having(rng, cp, cols.to_host())
            if conds is None:
                continue  # (every target is dictionary-encoded or decimal)
            want = _check_filter_of(cols, cp, conds)
            kept = cols.filter(conds)
            try:
                assert repr(kept.to_columns()) == repr(_take(cols.to_columns(), want)), q  # (repr: a NaN equals itself)
            finally:
                kept.free()
        finally:
            cols.free()
        ran += 1
    assert ran >= 12
