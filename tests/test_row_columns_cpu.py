"""Dense device columns for projections and non-grouped results, host side: the schema (plan.describe_columns), the numpy
statement of hdk_hip_columnarize_rows (result_set.rows_to_dense) and the executor's split of such a unit into what
compile_query takes and the stages that follow on its columns.  The reference is the host reader (result_set.to_columns /
to_arrow) on buffers that the oracle wrote."""
import dataclasses

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd.ir import (Agg, BinOp, Cmp, ColRef, KeyRef, Lit, OrderEntry, Proj, QueryMustRunOnCpu, QueryUnit, ResultJoin, TargetRef,
                        Type, Window)
from hdk_amd.plan import ColumnDesc, compile_query, describe_columns, is_row_unit, split_row_unit
from hdk_amd.storage import ArrowStorage

from test_projection import run_projection_oracle
from util import run_oracle

WORDS = ["ash", "birch", "cedar", "elm", "fir"]
N = 3000


def _types(nullable):
    return {"i8": Type("int", 1, nullable), "i16": Type("int", 2, nullable), "i32": Type("int", 4, nullable),
            "i64": Type("int", 8, nullable), "d": Type("fp", 8, nullable), "b": Type("bool", 1, nullable),
            "dt": Type("date", 4, nullable, unit="d"), "ts": Type("timestamp", 8, nullable),
            "dec": Type("decimal", 8, nullable, scale=2), "w": Type("dict", 4, nullable), "rid": Type("int", 8, False)}


def _storage(nullable, n=N):
    """NULLs (when the columns may hold them) and negative values in every column"""
    rng = np.random.default_rng(5)
    ty = _types(nullable)
    cols = {"i8": rng.integers(-100, 100, n).astype(np.int8), "i16": rng.integers(-30000, 30000, n).astype(np.int16),
            "i32": rng.integers(-10**9, 10**9, n).astype(np.int32), "i64": rng.integers(-2**60, 2**60, n),
            "d": rng.normal(size=n), "b": rng.integers(0, 2, n).astype(np.int8), "dt": rng.integers(-5000, 20000, n).astype(np.int32),
            "ts": rng.integers(-10**9, 2 * 10**9, n), "dec": rng.integers(-10**6, 10**6, n), "w": rng.integers(0, len(WORDS), n).astype(np.int32),
            "rid": np.arange(n, dtype=np.int64)}
    if nullable:
        for name, a in cols.items():
            if name == "rid":
                continue
            hit = rng.random(n) < 0.1
            if name == "d":
                a.view(np.int64)[hit] = A.NULL_DOUBLE_BITS
            else:
                a[hit] = ty[name].null_value()
    st = ArrowStorage()
    t = st.import_numpy("t", cols, fragment_size=1111, types=ty)
    t.columns["w"].dictionary = list(WORDS)
    return st


PLANS = {
    "ints": [Proj(ColRef("i8"), "i8"), Proj(ColRef("i16"), "i16"), Proj(ColRef("i32"), "i32"), Proj(ColRef("i64"), "i64"),
             Proj(ColRef("d"), "d"), Proj(ColRef("rid"), "rid")],
    "typed": [Proj(ColRef("b"), "b"), Proj(ColRef("dt"), "dt"), Proj(ColRef("ts"), "ts"), Proj(ColRef("dec"), "dec"),
              Proj(ColRef("w"), "w"), Proj(ColRef("rid"), "rid")],
    "computed": [Proj(ColRef("i32") * 2 + ColRef("i8"), "e"), Proj(ColRef("d") * ColRef("d"), "dd"), Proj(ColRef("i16") - ColRef("i8")),
                 Proj(ColRef("i32") - ColRef("i16"), "sq"), Proj(ColRef("i64"), "i64")],
}
QUAL = [Cmp(ColRef("rid"), ">=", Lit(700))]


@pytest.fixture(scope="module", params=[True, False], ids=["nullable", "not_null"])
def table(request):
    return request.param, _storage(request.param)


def _plan(st, which, columnar, **kw):
    return compile_query(st, QueryUnit("t", quals=QUAL, targets=PLANS[which], output_columnar=columnar, **kw))


@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
@pytest.mark.parametrize("which", list(PLANS))
def test_describe_columns_of_a_projection(table, which, columnar):
    nullable, st = table
    cp = _plan(st, which, columnar)
    assert cp.plan.query_kind == A.Q_PROJECTION and bool(cp.plan.output_columnar) == columnar
    schema = describe_columns(cp)
    assert len(schema) == len(PLANS[which]) and all(isinstance(d, ColumnDesc) and d.kind == "proj" and d.agg == "" for d in schema)
    ty = _types(nullable)
    for t, (d, oc, tgt) in enumerate(zip(schema, cp.out_cols, PLANS[which])):
        tg = cp.plan.targets[t]
        assert (d.name, d.target_idx, d.type, d.dictionary, d.scale) == (oc.name, t, oc.type, oc.dictionary, oc.scale)
        assert d.is_fp == bool(tg.arg_is_fp) and d.nullable == bool(tg.arg.nullable)
        w = cp.slot_widths[t]
        assert w == (8 if not columnar else w)
        if isinstance(tgt.expr, ColRef):
            ct = ty[tgt.expr.name]
            # a column read as it is: its own nullability, and its own sentinel sign-extended from whatever the slot holds
            assert d.nullable == ct.nullable
            if ct.is_date_in_days:  # (the scan reads a day count as epoch seconds: an int64 with BIGINT's NULL)
                assert d.null_bits == A.NULL_BIGINT and w == 8
                continue
            assert d.null_bits == (A.NULL_DOUBLE_BITS if ct.is_fp else ct.null_value())
            if columnar:
                assert w == ct.size
        else:
            nv = int(tg.arg.null_val)
            if not tg.arg_is_fp and w < 8:
                nv = int(np.int64(nv).astype({4: np.int32, 2: np.int16, 1: np.int8}[w]))
            assert d.null_bits == A.to_i64(nv)
    by_name = {d.name: d for d in schema}
    if which == "typed":
        assert by_name["w"].dictionary == WORDS and by_name["dec"].scale == 2 and by_name["dec"].type.kind == "decimal"
    if which == "computed":
        assert by_name["dd"].is_fp and not by_name["e"].is_fp and not by_name["sq"].is_fp
    # the positions: one trailing column, NOT NULL, int64
    with_pos = describe_columns(cp, positions=True)
    assert with_pos[:-1] == schema
    pos = with_pos[-1]
    assert (pos.name, pos.is_fp, pos.nullable, pos.target_idx, pos.type.size) == ("__pos", False, False, len(schema), 8)


def test_a_target_called_like_the_positions_column_is_refused(table):
    _, st = table
    cp = compile_query(st, QueryUnit("t", targets=[Proj(ColRef("i64"), "__pos")]))
    assert [d.name for d in describe_columns(cp)] == ["__pos"]
    with pytest.raises(ValueError, match="__pos"):
        describe_columns(cp, positions=True)
    grouped = compile_query(st, QueryUnit("t", groupby=[ColRef("i8")], targets=[KeyRef(0, "k")]))
    with pytest.raises(ValueError, match="positions"):
        describe_columns(grouped, positions=True)


@pytest.mark.parametrize("columnar", [False, True], ids=["rowwise", "columnar"])
@pytest.mark.parametrize("which", list(PLANS))
def test_projection_columns_read_like_the_fetched_buffer(oracle, table, which, columnar):
    """described_to_columns / described_to_arrow over rows_to_dense == to_columns / to_arrow over the buffer; again with a
    scan limit that the matches overrun (total_matched > entry_count)"""
    _, st = table
    for kw in ({}, {"scan_limit": 500}):
        q = QueryUnit("t", quals=QUAL, targets=PLANS[which], output_columnar=columnar, **kw)
        cp, buf, err, total = run_projection_oracle(oracle, st, q)
        n = int(cp.entry_count)
        assert total == N - 700 and (total > n) == bool(kw) and (err < 0 if kw else err == 0)
        schema = describe_columns(cp)
        dense = rs.rows_to_dense(cp, buf, total)
        assert all(c.dtype == np.int64 and len(c) == min(total, n) for c in dense)
        want = rs.to_columns(cp, buf, n, total)
        got = rs.described_to_columns(schema, dense)
        assert list(got) == list(want)
        for name in want:
            assert got[name] == want[name], name
        assert rs.described_to_arrow(schema, got).equals(rs.to_arrow(cp, buf, n, total))
        if which != "computed":
            assert any(v is None for v in want[PLANS[which][1].name]) == table[0]
        # the positions are word 0 of every row / the positions column
        with_pos = rs.rows_to_dense(cp, buf, total, positions=True)
        pos, _ = rs.projection_arrays(cp, buf, total)
        assert len(with_pos) == len(dense) + 1 and np.array_equal(with_pos[-1], pos)
        # no row, and a count below zero
        assert all(len(c) == 0 for c in rs.rows_to_dense(cp, buf, 0)) and all(len(c) == 0 for c in rs.rows_to_dense(cp, buf, -3))


def _agg_storage(n):
    rng = np.random.default_rng(17)
    v = rng.integers(-1000, 1000, n)
    v[rng.random(n) < 0.2] = A.NULL_BIGINT
    f = rng.normal(size=n).astype(np.float32)
    f.view(np.int32)[rng.random(n) < 0.2] = A.NULL_FLOAT_BITS
    d = rng.normal(size=n)
    nul = np.full(n, A.NULL_BIGINT, dtype=np.int64)
    fnul = np.full(n, A.NULL_FLOAT_BITS, dtype=np.int32).view(np.float32)
    st = ArrowStorage()
    st.import_numpy("t", {"v": v, "f": f, "d": d, "nul": nul, "fnul": fnul, "dec": rng.integers(-10**5, 10**5, n),
                          "rid": np.arange(n, dtype=np.int64)}, fragment_size=999,
                    types={"dec": Type("decimal", 8, True, scale=3), "rid": Type("int", 8, False)})
    return st


NON_GROUPED = {
    "ints": [Agg("count", None, "n"), Agg("count", ColRef("v"), "nv"), Agg("sum", ColRef("v"), "s"), Agg("min", ColRef("v"), "lo"),
             Agg("max", ColRef("v"), "hi"), Agg("avg", ColRef("v"), "m")],
    "floats": [Agg("sum", ColRef("f"), "s"), Agg("min", ColRef("f"), "lo"), Agg("max", ColRef("f"), "hi"), Agg("avg", ColRef("f"), "m"),
               Agg("count", ColRef("f"), "n")],
    "doubles": [Agg("sum", ColRef("d"), "s"), Agg("min", ColRef("d"), "lo"), Agg("avg", ColRef("d"), "m"), Agg("max", ColRef("d"), "hi")],
    # (with rows only: result_set.columns_to_arrow types a decimal aggregate that is NULL in every row by its integer type,
    # described_to_arrow as the double it would show -- as they do for a group-by result)
    "decimals": [Agg("avg", ColRef("dec"), "mdec"), Agg("sum", ColRef("dec"), "sdec"), Agg("min", ColRef("dec"), "lodec")],
    "all_null": [Agg("sum", ColRef("nul"), "s"), Agg("min", ColRef("nul"), "lo"), Agg("avg", ColRef("nul"), "m"),
                 Agg("count", ColRef("nul"), "n"), Agg("avg", ColRef("fnul"), "fm"), Agg("max", ColRef("fnul"), "fhi"),
                 Agg("sum", ColRef("fnul"), "fs")],
    "single": [Agg("single_value", ColRef("v"), "one"), Agg("single_value", ColRef("rid"), "rid")],
}


@pytest.mark.parametrize("which,rows", [(w, r) for w in NON_GROUPED for r in (2500, 0) if (w, r) != ("decimals", 0)])
def test_non_grouped_columns_read_like_the_fetched_buffer(oracle, which, rows):
    st = _agg_storage(rows)
    quals = [Cmp(ColRef("rid"), "=", Lit(7))] if which == "single" else []
    cp, buf, err = run_oracle(oracle, st, QueryUnit("t", quals=quals, targets=NON_GROUPED[which]))
    assert err == 0 and cp.plan.query_kind == A.Q_NON_GROUPED and set(cp.slot_widths) == {8}
    schema = describe_columns(cp)
    dense = rs.rows_to_dense(cp, buf)
    assert len(dense) == len(NON_GROUPED[which]) and all(c.dtype == np.int64 and len(c) == 1 for c in dense)
    want = rs.to_columns(cp, buf)
    got = rs.described_to_columns(schema, dense)
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], name
    assert rs.described_to_arrow(schema, got).equals(rs.to_arrow(cp, buf))
    if which == "all_null" or (rows == 0 and which != "single"):
        assert all(v == [None] for name, v in want.items() if not name.startswith("n"))  # AVG at count 0 included
    with pytest.raises(ValueError, match="positions"):
        rs.rows_to_dense(cp, buf, positions=True)


def test_non_grouped_avg_is_one_double_division():
    """AVG word == bits of float64(sum) / float64(count), also for a sum beyond 2^53, where the integer quotient rounds
    differently; the float accumulator's low word is widened first"""
    st = _agg_storage(10)
    cp = compile_query(st, QueryUnit("t", targets=[Agg("avg", ColRef("v"), "m"), Agg("avg", ColRef("d"), "md"), Agg("avg", ColRef("f"), "mf"),
                                                   Agg("sum", ColRef("f"), "sf")]))
    s = 2**62 + 12345
    f32 = np.array([1.7], dtype=np.float32)
    buf = np.array([s, 3, np.float64(2.5).view(np.int64), 7, int(f32.view(np.int32)[0]) | (0x7777 << 32), 3,
                    int(f32.view(np.int32)[0]) | (0x1234 << 32)], dtype=np.int64)
    dense = rs.rows_to_dense(cp, buf)
    want = [np.float64(s) / np.float64(3), np.float64(2.5) / np.float64(7), np.float64(f32[0]) / np.float64(3), np.float64(f32[0])]
    assert [int(c[0]) for c in dense] == [int(np.float64(x).view(np.int64)) for x in want]
    assert float(dense[0].view(np.float64)[0]) != s // 3
    buf[1] = buf[3] = buf[5] = 0
    assert [int(c[0]) for c in rs.rows_to_dense(cp, buf)[:3]] == [A.NULL_DOUBLE_BITS] * 3


# ---- the executor's split -------------------------------------------------------------------------------------------------
PROJ_Q = QueryUnit("t", quals=QUAL, targets=[Proj(ColRef("rid"), "rid"), Proj(ColRef("i32"), "v")])
AGG_Q = QueryUnit("t", targets=[Agg("sum", ColRef("i32"), "s"), Agg("count", None, "n")])
STAGES = {"windows": [Window("row_number", partition_by=["v"], order_by=[OrderEntry("rid")], name="rn")],
          "select": [Proj(TargetRef("rid"), "rid")], "order_by": [OrderEntry("v", desc=True)], "limit": 10, "offset": 3}


def test_which_units_are_row_units():
    assert is_row_unit(PROJ_Q) and is_row_unit(AGG_Q)
    assert not is_row_unit(QueryUnit("t", groupby=[ColRef("i8")], targets=[KeyRef(0), Agg("count", None)]))
    assert not is_row_unit(QueryUnit("t", groupby=[ColRef("i8")], targets=[Agg("count", None)]))
    assert not is_row_unit(QueryUnit("t", targets=[Proj(ColRef("i8")), Agg("count", None)]))
    assert not is_row_unit(QueryUnit("t"))


def test_the_inner_unit_carries_none_of_the_stripped_fields():
    right = object()
    for base in (PROJ_Q, AGG_Q):
        q = dataclasses.replace(base, result_joins=[ResultJoin(right, ["rid"])], having=[Cmp(TargetRef(0), ">", Lit(1))], **STAGES)
        inner = split_row_unit(q)
        assert (inner.result_joins, inner.windows, inner.select, inner.order_by, inner.limit, inner.offset) == ([], [], [], [], None, 0)
        assert inner.having == q.having and inner.scan_limit is None
        assert (inner.table, inner.quals, inner.targets) == (q.table, q.quals, q.targets)
        assert q.limit == 10 and q.windows  # the unit itself is not touched


def test_scan_limit_is_set_exactly_when_nothing_looks_across_the_rows():
    lim = dataclasses.replace(PROJ_Q, limit=10, offset=3)
    assert split_row_unit(lim).scan_limit == 13
    assert split_row_unit(dataclasses.replace(lim, select=STAGES["select"])).scan_limit == 13  # a select keeps rows and order
    assert split_row_unit(dataclasses.replace(lim, offset=0)).scan_limit == 10
    assert split_row_unit(dataclasses.replace(lim, scan_limit=5)).scan_limit == 5  # its own
    for kw in ({"order_by": STAGES["order_by"]}, {"windows": STAGES["windows"]}, {"result_joins": [ResultJoin(object(), ["rid"])]},
               {"limit": None}, {"limit": None, "offset": 0}, {"limit": 0, "offset": 0}):
        assert split_row_unit(dataclasses.replace(lim, **kw)).scan_limit is None, kw
    assert split_row_unit(dataclasses.replace(AGG_Q, limit=10)).scan_limit is None  # not a projection


class _Stop(Exception):
    pass


def _executor(st, seen):
    """an Executor that compiles what it is asked to prepare and stops there: nothing touches a device"""
    from hdk_amd.executor import Executor
    ex = Executor.__new__(Executor)
    ex.storage = st

    def prepare(q, frag_ids=None, **kw):
        seen.append(q)
        compile_query(st, q)
        raise _Stop()
    ex.prepare = prepare
    return ex


def test_execute_hands_the_inner_unit_to_the_step(table):
    _, st = table
    for base in (PROJ_Q, AGG_Q):
        for field in STAGES:
            seen = []
            q = dataclasses.replace(base, **{field: STAGES[field]})
            with pytest.raises(_Stop):
                _executor(st, seen).execute(q, result="columns")
            assert seen == [split_row_unit(q)] and is_row_unit(seen[0])
            if not (base is PROJ_Q and field == "windows"):  # (which compile_query does not look at on a projection)
                with pytest.raises(QueryMustRunOnCpu, match="no dense device columns"):
                    compile_query(st, q)  # compile_query itself still refuses the unit
    seen = []
    with pytest.raises(_Stop):
        _executor(st, seen).execute(dataclasses.replace(PROJ_Q, limit=10, offset=3), result="columns")
    assert seen[0].scan_limit == 13
    seen = []
    with pytest.raises(_Stop):  # nothing to strip: the unit as it is
        _executor(st, seen).execute(PROJ_Q, result="columns")
    assert seen == [PROJ_Q]
    with pytest.raises(ValueError, match="negative"):
        _executor(st, []).execute(dataclasses.replace(PROJ_Q, limit=-1), result="columns")


def test_having_on_a_row_unit_still_must_run_on_cpu(table):
    _, st = table
    having = [Cmp(TargetRef(0), ">", Lit(1))]
    for base in (PROJ_Q, AGG_Q):
        for kw in ({}, {"order_by": [OrderEntry(0)]}, {"limit": 5}):
            with pytest.raises(QueryMustRunOnCpu, match="HAVING"):
                _executor(st, []).execute(dataclasses.replace(base, having=having, **kw), result="columns")


def test_result_buffer_keeps_raising(table):
    _, st = table
    from hdk_amd.executor import Executor
    ex = Executor.__new__(Executor)
    for base in (PROJ_Q, AGG_Q):
        for field in STAGES:
            with pytest.raises(ValueError, match="columns"):
                ex.execute(dataclasses.replace(base, **{field: STAGES[field]}), result="buffer")
        with pytest.raises(ValueError, match="columns"):
            ex.execute(dataclasses.replace(base, result_joins=[ResultJoin(object(), ["rid"])]))
        with pytest.raises(ValueError, match="columns"):
            ex.execute(dataclasses.replace(base, having=[Cmp(TargetRef(0), ">", Lit(1))]))


def test_fetch_columns_positions_needs_a_projection(table):
    _, st = table
    from hdk_amd.executor import PreparedStep
    step = PreparedStep.__new__(PreparedStep)
    step.cp = compile_query(st, AGG_Q)
    with pytest.raises(ValueError, match="positions"):
        step.fetch_columns(positions=True)
    step.cp = compile_query(st, QueryUnit("t", groupby=[ColRef("i8")], targets=[KeyRef(0, "k")]))
    with pytest.raises(ValueError, match="positions"):
        step.fetch_columns(positions=True)


# ---- group-by schemas are what they were ------------------------------------------------------------------------------------
def _parent_dense_column_null(cp, t):
    """dense_column_null as it stood before projections had a schema, restated"""
    tg = cp.plan.targets[t]
    if tg.agg == A.AGG_ID:
        kt = cp.key_types[tg.key_idx]
        return bool(kt.is_fp), bool(kt.nullable), A.to_i64(kt.null_as_int64_or_double_bits() if kt.is_fp else kt.null_value())
    if tg.agg == A.AGG_COUNT:
        return False, False, 0
    if tg.agg == A.AGG_AVG or tg.arg_is_fp == A.FP_SLOT_FLOAT:
        return True, bool(tg.agg == A.AGG_AVG or tg.skip_null), A.NULL_DOUBLE_BITS
    first = sum(2 if cp.plan.targets[i].agg == A.AGG_AVG else 1 for i in range(t))
    nullv = int(tg.null_val)
    if cp.slot_widths[first] == 4:
        nullv = int(np.int64(nullv).astype(np.int32))
    return bool(tg.arg_is_fp), bool(tg.skip_null), nullv


def test_group_by_schemas_are_unchanged():
    from fuzz_queries import make_tables_wide, random_query_wide
    rng = np.random.default_rng(2024)
    st = make_tables_wide(rng, 4000, 300)
    seen = 0
    for _ in range(60):
        q = random_query_wide(rng)
        try:
            cp = compile_query(st, q)
        except QueryMustRunOnCpu:
            continue
        if cp.plan.query_kind not in (A.Q_PERFECT_HASH, A.Q_BASELINE_HASH):
            continue
        seen += 1
        schema = describe_columns(cp)
        assert [d.target_idx for d in schema] == list(range(cp.plan.num_targets))
        for d, oc in zip(schema, sorted(cp.out_cols, key=lambda c: c.target_idx)):
            is_fp, nullable, null_bits = _parent_dense_column_null(cp, oc.target_idx)
            assert rs.dense_column_null(cp, oc.target_idx) == (is_fp, nullable, null_bits)
            scaled = oc.kind == "agg" and oc.agg in ("sum", "min", "max", "avg")
            assert d == ColumnDesc(oc.name, is_fp, nullable, A.to_i64(null_bits), oc.type, oc.target_idx, oc.kind, oc.agg, oc.dictionary,
                                   oc.scale if scaled else 0)
    assert seen >= 8
