"""Joining against a device result: a registered result (Executor.register_columns) and a QueryUnit as the INNER table of
a join, end to end on the device.  The inner tables are real GROUP BY results; every unit over the registered table is held
to the same unit over a host table imported from the result's host copy, and each test names the join table kind it ran on."""
import dataclasses
import math

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import storage as S
from hdk_amd._lib import HdkHipError
from hdk_amd.ir import Agg, BinOp, Cmp, ColRef, JoinSpec, KeyRef, Lit, Proj, QueryMustRunOnCpu, QueryUnit, Type

import chunk_expect as E

pytestmark = pytest.mark.gpu

NB, NF, NG, FRAG = 6_000, 5_000, 300, 128
DAY = 86400
DATE_S = Type("date", 8, True, unit="s")


@pytest.fixture(scope="module")
def base():
    """the table the inner results aggregate: g with NULLs, a second component h, a third w, a day in seconds"""
    rng = np.random.default_rng(1017)
    g = rng.integers(0, NG, NB).astype(np.int32)
    g[rng.random(NB) < 0.03] = A.NULL_INT
    h = rng.integers(0, 4, NB).astype(np.int32)
    w = rng.integers(0, 3, NB).astype(np.int32)
    v = rng.integers(-500, 500, NB).astype(np.int32)
    v[rng.random(NB) < 0.1] = A.NULL_INT
    ts = (rng.integers(-20, 30, NB) * DAY).astype(np.int64)
    return {"g": g, "h": h, "w": w, "v": v, "ts": ts}


@pytest.fixture(scope="module")
def fact():
    """the outer table: keys that hit, miss and are NULL"""
    rng = np.random.default_rng(1018)
    fk = rng.integers(-20, NG + 40, NF).astype(np.int32)
    fk[rng.random(NF) < 0.05] = A.NULL_INT
    fh = rng.integers(0, 5, NF).astype(np.int32)
    val = rng.integers(-100, 100, NF).astype(np.int64)
    fd = (rng.integers(-25, 35, NF) * DAY).astype(np.int64)
    fd[rng.random(NF) < 0.05] = A.NULL_BIGINT
    return {"fk": fk, "fh": fh, "val": val, "fd": fd, "grp": rng.integers(0, 7, NF).astype(np.int32)}


@pytest.fixture()
def ex(gpu_executor_factory, base, fact):
    st = S.ArrowStorage()
    st.import_numpy("t", base, fragment_size=2_500, types={"ts": DATE_S})
    st.import_numpy("f", fact, fragment_size=2_000, types={"fd": DATE_S})  # three fragments
    ex = gpu_executor_factory(st)
    yield ex
    for name, tb in list(st.tables.items()):
        if isinstance(tb, S.DeviceTable):
            ex.drop_registered(name)
    for cache in (ex._join_cache, ex._fused_cache):
        for b in cache.values():
            b.free()
        cache.clear()
    ex.cache.clear()


G, H, W, V = ColRef("g"), ColRef("h"), ColRef("w"), ColRef("v")
BY_G = QueryUnit("t", groupby=[G], targets=[KeyRef(0, "k"), Agg("sum", V, "s"), Agg("count", None, "c")])
BY_GH = QueryUnit("t", groupby=[G, H], targets=[KeyRef(0, "k"), KeyRef(1, "h"), Agg("sum", V, "s"), Agg("count", None, "c")])
BY_GHW = QueryUnit("t", groupby=[G, H, W], targets=[KeyRef(0, "k"), KeyRef(1, "h"), KeyRef(2, "w"), Agg("sum", V, "s"),
                                                    Agg("count", None, "c")])
BY_DAY = QueryUnit("t", groupby=[ColRef("ts")], targets=[KeyRef(0, "d"), Agg("sum", V, "s"), Agg("count", None, "c")])
FK, FH, VAL = ColRef("fk"), ColRef("fh"), ColRef("val")


def rows_of(columns):
    rows = list(zip(*columns.values()))
    return sorted(rows, key=lambda r: tuple((v is not None, v if v is not None else 0) for v in r))


def same_rows(got, want):
    """exact for integers, 1e-6 relative for doubles (the project's rule)"""
    if len(got) != len(want):
        return False
    for a, b in zip(got, want):
        for p, q in zip(a, b):
            if isinstance(p, float) or isinstance(q, float):
                if p is None or q is None or not math.isclose(p, q, rel_tol=1e-6, abs_tol=1e-12):
                    return False
            elif p != q:
                return False
    return True


def run_rows(ex, q):
    return rows_of(ex.execute(q).to_columns())


def host_twin(ex, cols, reg, name, fragment_size):
    """the registered table's values imported from the host copy of the columns (the sentinel rewrite stated by chunk_expect)"""
    sel = [(j, d.is_fp, d.nullable, d.null_bits, reg.columns[d.name].type.null_value()) for j, d in enumerate(cols.schema)]
    words = E.copy([w.view(np.int64) for w in cols.to_host()], cols.num_rows, sel)
    types = {d.name: reg.columns[d.name].type for d in cols.schema}
    arrays = {d.name: (w.view(np.float64) if types[d.name].is_fp else w) for d, w in zip(cols.schema, words)}
    return ex.storage.import_numpy(name, arrays, fragment_size=fragment_size, types=types), dict(zip(types, words))


def register(ex, inner, name="r", twin="h", frag=FRAG):
    """-> (the DeviceTable made of the inner unit's result, its host twin, the twin's words by column)"""
    cols = ex.execute(inner, result="columns")
    try:
        assert 40 <= cols.num_rows <= 5_000
        reg = ex.register_columns(name, cols, fragment_size=frag, joinable=True)
        h, words = host_twin(ex, cols, reg, twin, frag)
    finally:
        cols.free()
    assert reg.num_fragments >= 2
    return reg, h, words


def both(ex, unit_of, kind):
    """run unit_of(table) over the registered table "r" and its host twin "h": the same plan, the kind named, the same rows"""
    q_dev, q_host = unit_of("r"), unit_of("h")
    cp, cph = ex.compile(q_dev), ex.compile(q_host)
    assert cp.join_infos[0]["kind"] == kind
    strip = [{k: v for k, v in i.items() if k != "inner_table"} for i in cp.join_infos]
    assert strip == [{k: v for k, v in i.items() if k != "inner_table"} for i in cph.join_infos]
    assert bytes(cp.plan) == bytes(cph.plan) and cp.entry_count == cph.entry_count and cp.buffer_bytes == cph.buffer_bytes
    got, want = run_rows(ex, q_dev), run_rows(ex, q_host)
    assert same_rows(got, want), (got[:3], want[:3])
    assert got, "an empty answer compares nothing"
    return got


def agg_unit(jtype="inner", null_safe=False, key="k"):
    def make(table):
        j = JoinSpec(table, FK, key, type=jtype, null_safe=null_safe)
        tn = table if isinstance(table, str) else None  # (a subquery's private name cannot be spelled: its columns by name alone)
        if jtype in ("semi", "anti"):
            targets = [KeyRef(0, "grp"), Agg("sum", VAL, "sv"), Agg("count", None, "n")]
        else:
            targets = [KeyRef(0, "grp"), Agg("sum", BinOp("+", VAL, ColRef("s", tn)), "sv"), Agg("count", None, "n"),
                       Agg("count", ColRef("c", tn), "nc")]
        return QueryUnit("f", joins=[j], groupby=[ColRef("grp")], targets=targets)
    return make


# ---- one-to-one ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jtype", ["inner", "left", "semi", "anti"])
def test_one_to_one(ex, jtype):
    reg, _, _ = register(ex, BY_G)
    both(ex, agg_unit(jtype), A.JOIN_ONE_TO_ONE)
    if jtype in ("semi", "anti"):
        assert reg.key_multiplicity == {}  # (the first row of a key wins the fill: nothing to measure)
    else:
        assert reg.key_multiplicity == {(("k",), False, 1): (1, NG)}


def test_one_to_one_against_an_independent_numpy_join(ex, fact):
    _, _, words = register(ex, BY_G)
    got = both(ex, agg_unit("inner"), A.JOIN_ONE_TO_ONE)
    k, s, c = words["k"], words["s"], words["c"]
    s_of = {int(a): (int(b), int(n)) for a, b, n in zip(k, s, c) if a != A.NULL_BIGINT}
    want = {}
    for fk, grp, val in zip(fact["fk"].tolist(), fact["grp"].tolist(), fact["val"].tolist()):
        if fk == A.NULL_INT or fk not in s_of:
            continue
        sv, n, nc = want.get(grp, (None, 0, 0))
        sk = s_of[fk][0]
        if sk != A.NULL_BIGINT:
            sv = (sv or 0) + val + sk
        want[grp] = (sv, n + 1, nc + 1)
    assert got == sorted((g,) + t for g, t in want.items())


@pytest.mark.parametrize("fuse", [True, False])
def test_one_to_one_fused_and_not_fused(ex, fuse):
    register(ex, BY_G)
    ex.fuse_join_tables = fuse
    try:
        steps = [ex.prepare(agg_unit("inner")(t)) for t in ("r", "h")]
        try:
            assert steps[0].cp.join_infos[0]["kind"] == A.JOIN_ONE_TO_ONE
            assert steps[0].kernel_names() == steps[1].kernel_names()
            kinds = [int(s.plan.joins[0].kind) for s in steps]
            assert kinds == [A.JOIN_ONE_TO_ONE_FUSED if fuse else A.JOIN_ONE_TO_ONE] * 2
            got, want = (rows_of(s.run().to_columns()) for s in steps)
            assert got and same_rows(got, want)
        finally:
            for s in steps:
                s.free()
    finally:
        ex.fuse_join_tables = True


def test_null_safe_with_null_keys_on_both_sides(ex, fact):
    reg, _, words = register(ex, BY_G)
    assert (words["k"] == A.NULL_BIGINT).sum() == 1 and (fact["fk"] == A.NULL_INT).sum() > 0
    safe = both(ex, agg_unit("inner", null_safe=True), A.JOIN_ONE_TO_ONE)
    plain = both(ex, agg_unit("inner"), A.JOIN_ONE_TO_ONE)
    assert sum(r[2] for r in safe) == sum(r[2] for r in plain) + int((fact["fk"] == A.NULL_INT).sum())
    assert reg.key_multiplicity[(("k",), True, 1)] == (1, NG + 1)


def test_group_by_over_a_joined_column_and_a_filter_on_one(ex):
    register(ex, BY_G)

    def grouped(table):
        return QueryUnit("f", joins=[JoinSpec(table, FK, "k")], groupby=[ColRef("c", table)],
                         targets=[KeyRef(0, "c"), Agg("sum", VAL, "sv"), Agg("count", None, "n")])

    def filtered(table):
        return QueryUnit("f", joins=[JoinSpec(table, FK, "k")], quals=[Cmp(ColRef("s", table), ">", Lit(0))],
                         targets=[Agg("sum", VAL, "sv"), Agg("count", None, "n"), Agg("min", ColRef("s", table), "lo")])

    assert len(both(ex, grouped, A.JOIN_ONE_TO_ONE)) > 5
    got = both(ex, filtered, A.JOIN_ONE_TO_ONE)
    assert got[0][2] > 0


# ---- one-to-many, keyed ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jtype", ["inner", "left"])
def test_one_to_many(ex, jtype):
    reg, _, words = register(ex, BY_GH)
    both(ex, agg_unit(jtype), A.JOIN_ONE_TO_MANY)
    k = words["k"][words["k"] != A.NULL_BIGINT]
    assert reg.key_multiplicity == {(("k",), False, 1): (int(np.unique(k, return_counts=True)[1].max()), NG)}


def keyed_unit(jtype="inner"):
    def make(table):
        return QueryUnit("f", joins=[JoinSpec(table, [FK, FH], ["k", "h"], type=jtype)], groupby=[ColRef("grp")],
                         targets=[KeyRef(0, "grp"), Agg("sum", BinOp("+", VAL, ColRef("s", table)), "sv"), Agg("count", None, "n")])
    return make


@pytest.mark.parametrize("jtype", ["inner", "left"])
def test_keyed_one_to_one(ex, jtype):
    reg, _, _ = register(ex, BY_GH)
    both(ex, keyed_unit(jtype), A.JOIN_KEYED_ONE_TO_ONE)
    assert reg.key_multiplicity[(("k", "h"), False, 1)][0] == 1


def test_keyed_one_to_many(ex):
    reg, _, _ = register(ex, BY_GHW)
    both(ex, keyed_unit(), A.JOIN_KEYED_ONE_TO_MANY)
    assert reg.key_multiplicity[(("k", "h"), False, 1)][0] == 3


def test_a_projection_with_fan_out(ex, fact):
    reg, _, words = register(ex, BY_GH)

    def unit(table):
        return QueryUnit("f", joins=[JoinSpec(table, FK, "k")], targets=[Proj(FK, "fk"), Proj(VAL, "val"), Proj(ColRef("h", table), "h"),
                                                                          Proj(ColRef("s", table), "s")])

    got = both(ex, unit, A.JOIN_ONE_TO_MANY)
    per_key = dict(zip(*np.unique(words["k"][words["k"] != A.NULL_BIGINT], return_counts=True)))
    assert max(per_key.values()) > 1
    assert len(got) == sum(int(per_key.get(int(x), 0)) for x in fact["fk"].tolist() if x != A.NULL_INT)
    one = ex.compile(QueryUnit("f", targets=[Proj(FK, "fk")]))
    assert ex.compile(unit("r")).entry_count == one.entry_count * reg.key_multiplicity[(("k",), False, 1)][0]  # the fan-out


def test_a_date_in_seconds_key(ex):
    reg, _, _ = register(ex, BY_DAY, frag=32)
    assert reg.columns["d"].type == DATE_S

    def unit(table):
        return QueryUnit("f", joins=[JoinSpec(table, ColRef("fd"), "d")], groupby=[ColRef("grp")],
                         targets=[KeyRef(0, "grp"), Agg("sum", BinOp("+", VAL, ColRef("c", table)), "sv"), Agg("count", None, "n")])

    both(ex, unit, A.JOIN_ONE_TO_ONE)
    assert reg.key_multiplicity == {(("d",), False, DAY): (1, 50)}


# ---- the inner table as a unit; both tables results ------------------------------------------------------------------------
def test_the_inner_table_as_a_unit(ex):
    register(ex, BY_G)
    want = run_rows(ex, agg_unit("left")("h"))
    got = run_rows(ex, agg_unit("left")(BY_G))
    assert got and same_rows(got, want)
    assert sorted(ex.storage.tables) == ["f", "h", "r", "t"]
    with pytest.raises(ValueError, match="execute"):
        ex.compile(agg_unit("left")(BY_G))
    # an outer subquery and an inner one in one unit
    outer = QueryUnit("f", quals=[Cmp(VAL, ">=", Lit(0))], targets=[Proj(FK, "fk"), Proj(VAL, "val"), Proj(ColRef("grp"), "grp")])
    q = dataclasses.replace(agg_unit("inner")(BY_G), table=outer)
    ref = dataclasses.replace(agg_unit("inner")("h"), quals=[Cmp(VAL, ">=", Lit(0))])
    assert same_rows(run_rows(ex, q), run_rows(ex, ref))
    assert sorted(ex.storage.tables) == ["f", "h", "r", "t"]


def test_a_raising_outer_unit_leaves_no_subquery_behind(ex):
    inner = dataclasses.replace(BY_G, targets=BY_G.targets + [Agg("sum", BinOp("-", V, V), "z")])  # z: 0, or NULL
    bad = QueryUnit("f", joins=[JoinSpec(inner, FK, "k")], targets=[Agg("sum", BinOp("/", VAL, ColRef("z")), "q")])
    with pytest.raises(HdkHipError) as e:
        ex.execute(bad)
    assert e.value.code == A.ERR_DIV_BY_ZERO
    assert sorted(ex.storage.tables) == ["f", "t"]
    assert not [k for k in list(ex._join_cache) + list(ex._fused_cache) if str(k[0]).startswith("__subquery_")]
    ok = QueryUnit("f", joins=[JoinSpec(inner, FK, "k")], targets=[Agg("sum", BinOp("+", VAL, ColRef("c")), "q")])
    assert run_rows(ex, ok)[0][0] is not None and sorted(ex.storage.tables) == ["f", "t"]


def test_both_tables_registered_results(ex):
    register(ex, BY_G)
    outer = QueryUnit("f", groupby=[FK], targets=[KeyRef(0, "fk"), Agg("sum", VAL, "val"), Agg("count", None, "n")])
    cols = ex.execute(outer, result="columns")
    try:
        ex.register_columns("o", cols, fragment_size=FRAG)
    finally:
        cols.free()

    def unit(table):
        return QueryUnit("o", joins=[JoinSpec(table, FK, "k", type="left")],
                         targets=[Agg("sum", BinOp("+", VAL, ColRef("s", table)), "sv"), Agg("count", None, "rows"),
                                  Agg("count", ColRef("c", table), "hits"), Agg("sum", ColRef("n"), "n")])

    got = both(ex, unit, A.JOIN_ONE_TO_ONE)
    assert got[0][3] == NF and 0 < got[0][2] < got[0][1]


# ---- the caches follow the table, and stale statistics are found before a build ---------------------------------------------
def test_a_name_registered_again_is_joined_by_its_new_rows(ex):
    q = QueryUnit("f", joins=[JoinSpec("r", FK, "k")], targets=[Agg("sum", ColRef("c", "r"), "c"), Agg("count", None, "n")])
    first = ex.execute(BY_G, result="columns")
    second = ex.execute(dataclasses.replace(BY_G, quals=[Cmp(G, "<", Lit(100))]), result="columns")
    try:
        ex.register_columns("r", first, joinable=True)
        a = run_rows(ex, q)
        assert [k[0] for k in ex._join_cache] == ["r"]
        ex.drop_registered("r")
        assert not ex._join_cache and not ex._fused_cache
        ex.register_columns("r", second, joinable=True)
        b = run_rows(ex, q)
        h, _ = host_twin(ex, second, ex.storage.get("r"), "h", FRAG)
        want = run_rows(ex, dataclasses.replace(q, joins=[JoinSpec("h", FK, "k")], targets=[Agg("sum", ColRef("c", "h"), "c"),
                                                                                          Agg("count", None, "n")]))
        assert b == want and 0 < b[0][1] < a[0][1]
    finally:
        first.free()
        second.free()


def test_stale_statistics_are_found_before_any_build(ex):
    reg, _, _ = register(ex, BY_G)
    st = reg.columns["k"].stats
    assert st[0].max is not None and st[0].max > 100
    for i, s in enumerate(st):  # narrow the range by hand: the rows above 100 now lie outside it
        if s.max is not None:
            st[i] = S.ChunkStats(min(s.min, 100), min(s.max, 100), s.has_nulls)
    with pytest.raises(QueryMustRunOnCpu, match="stale statistics"):
        ex.execute(agg_unit("inner")("r"))
    assert not ex._join_cache and not ex._fused_cache and reg.key_multiplicity == {}


def test_a_default_registration_stays_the_outer_table_only(ex):
    cols = ex.execute(BY_G, result="columns")
    try:
        reg = ex.register_columns("r", cols)
        assert reg.joinable is False
        for jtype in ("inner", "semi"):
            with pytest.raises(QueryMustRunOnCpu, match="outer table"):
                ex.execute(agg_unit(jtype)("r"))
        assert reg.key_multiplicity == {} and not ex._join_cache
        assert run_rows(ex, QueryUnit("r", targets=[Agg("count", None, "n")])) == [(NG + 1,)]
        ex.drop_registered("r")
        assert ex.register_columns("r", cols, joinable=True).joinable
        assert run_rows(ex, agg_unit("inner")("r"))
    finally:
        cols.free()
