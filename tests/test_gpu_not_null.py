"""Columns declared NOT NULL through every kernel family, on the device.

Every case of not_null_cases.py runs declared NOT NULL, with and without the types' in-band NULL patterns planted as values,
against the oracle (which test_not_null_cpu.py checks against plain numpy): the launch must take the route recorded on the
CPU, and its buffer must be the oracle's -- keys, integers, counts and the init patterns of empty entries bit for bit, fp SUM
and AVG within assert_buffers_equal's tolerances.  An open-addressing table places its groups in insertion order, so those
are compared row by row by key and as a multiset of raw entries.  Then the same plan on the interpreters and on global
atomics, and under a pinned small grid where slabs are folded.  Beyond the scan kernels: the device reduction of per-fragment
partials against the oracle's, and the result stages (dense columns, sort, filter, regroup) on a NOT NULL plan.
"""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd._lib import check, lib
from hdk_amd.ir import Agg, Cmp, ColRef, KeyRef, Lit, OrderEntry, QueryUnit, TargetRef
from hdk_amd.plan import compile_query

import not_null_cases as N
from test_gpu_baseline import _check_rows
from test_gpu_projection import _sorted_rows
from test_not_null_cpu import CASES, TWIN_ROUTES, record_routes
from test_projection import run_projection_oracle
from util import assert_buffers_equal, oracle_init_buffer, run_oracle

pytestmark = pytest.mark.gpu

# the nullable declaration over the same data: only the shapes this file adds to the suite's (a sentinel under OR / NOT, one
# nullable and one NOT NULL operand, a LEFT join's payload, the narrow keys at their type's minimum)
TWINS = ("direct_sum_or", "direct_sum_eq", "vec_expr_mixed", "ng_mixed_expr", "vec_join_left", "pr_expr", "keys_values_k8", "key_k16s")


@pytest.fixture(scope="module")
def tables():
    return {(d, s): N.make_tables(d, s) for d in ("nullable", "not_null") for s in (False, True)}


@pytest.fixture(scope="module")
def routes(tables):
    return record_routes(tables)


@pytest.fixture(scope="module")
def executors(gpu_executor_factory, tables):
    made = {}

    def get(declared, sentinel):
        if (declared, sentinel) not in made:
            made[(declared, sentinel)] = gpu_executor_factory(tables[(declared, sentinel)])
        return made[(declared, sentinel)]

    return get


def _raw_entries(cp, buf):
    """the entries of a row-wise table as sorted rows of quads: the groups AND the empty entries with their init patterns"""
    m = np.ascontiguousarray(buf[:cp.buffer_quads]).reshape(cp.entry_count, int(cp.plan.row_size_quad))
    return m[np.lexsort(m.T[::-1])]


def _has_fp_sum(cp):
    return any(cp.plan.targets[t].arg_is_fp and cp.plan.targets[t].agg in (A.AGG_SUM, A.AGG_AVG) for t in range(cp.plan.num_targets))


def _assert_same(cp, got, want):
    if cp.plan.query_kind != A.Q_BASELINE_HASH:
        assert_buffers_equal(cp, got, want)
        return
    _check_rows(cp, got, want)
    if not cp.plan.output_columnar and not _has_fp_sum(cp):
        assert np.array_equal(_raw_entries(cp, got), _raw_entries(cp, want))


def _run_case(oracle, ex, st, case, expect_names):
    name, q, env, flags = case
    with N.switches(env):
        if N.is_projection(q):
            cp, want, err, nrows = run_projection_oracle(oracle, st, q)
            assert err == 0 and (nrows > 0 or name == "pr_fast_columnar")  # (`c = INT32_MIN` finds no row in the plain table)
            want_rows = _sorted_rows(cp, want, nrows)
            for f in dict.fromkeys((flags, A.LAUNCH_FORCE_GENERIC, A.LAUNCH_FORCE_SCALAR)):
                step = ex.prepare(cp, flags=f)
                if f == flags:
                    assert step.kernel_names() == expect_names
                res = step.run()
                step.free()
                assert res.total_matched == nrows, (name, f)
                assert np.array_equal(_sorted_rows(cp, res.buffer, nrows), want_rows), (name, f)
            return
        cp, want, err = run_oracle(oracle, st, q)
        assert err == 0
        step = ex.prepare(cp, flags=flags)
        names = step.kernel_names()
        assert names == expect_names
        got = step.run().buffer
        step.free()
        _assert_same(cp, got, want)
        others = [A.LAUNCH_FORCE_GENERIC, A.LAUNCH_FORCE_SCALAR]
        if cp.plan.query_kind != A.Q_NON_GROUPED:
            others.append(A.LAUNCH_FORCE_GLOBAL_ATOMICS)
        for f in others:
            if f != flags:
                _assert_same(cp, ex.execute(cp, flags=f).buffer, want)
        if names.endswith(",hdk_finalize"):  # the LDS families: per-block slabs, folded -- seven blocks walk every tile
            _assert_same(cp, ex.execute(cp, flags=flags, grid=7).buffer, want)


@pytest.mark.parametrize("sentinel", [False, True], ids=["plain", "sentinel"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_not_null_columns(oracle, executors, tables, routes, case, sentinel):
    _run_case(oracle, executors("not_null", sentinel), tables[("not_null", sentinel)], case, routes[(case[0], sentinel)])


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in TWINS], ids=lambda c: c[0])
def test_nullable_twins_of_the_new_shapes(oracle, executors, tables, routes, case):
    """The same data declared nullable: the planted patterns are NULLs."""
    _run_case(oracle, executors("nullable", True), tables[("nullable", True)], case, TWIN_ROUTES[(case[0], True)])


# ---- reduction of partials ---------------------------------------------------------------------------------------------------
def _reduce_targets():
    V, C_, M16, M8, D, F = (ColRef(c) for c in ("val", "c", "m16", "m8", "d", "f"))
    return [Agg("sum", V, "sv"), Agg("min", V, "mnv"), Agg("max", C_, "mxc"), Agg("avg", M16, "a16"), Agg("min", F, "mnf"),
            Agg("sum", F, "sf"), Agg("max", D, "mxd")]


@pytest.mark.parametrize("layout", ["perfect", "columnar", "non_grouped", "baseline"])
def test_device_reduce_of_not_null_partials(oracle, executors, tables, layout):
    """hdk_hip_reduce_buffers over the per-fragment partials of a NOT NULL plan with planted sentinels == the oracle's
    ResultSetReduction restatement over the same partials in the same order, bit for bit (fp included: the order is the same).
    The slots start at 0 / INT64_MAX / INT64_MIN / +-DBL_MAX / +-FLT_MAX, not at the sentinel, and a sentinel in a partial is a
    value.  A baseline partial is re-inserted into a fresh table of twice the entries, whose groups land in insertion order:
    compared as rows by key and by the number of entries left empty."""
    st, ex = tables[("not_null", True)], executors("not_null", True)
    mgr = ex.mgr
    K = ColRef("key")
    q = {"perfect": QueryUnit("t", groupby=[K], targets=[KeyRef(0, "k")] + _reduce_targets()),
         "columnar": QueryUnit("t", groupby=[K], output_columnar=True, targets=[KeyRef(0, "k")] + _reduce_targets()),
         "non_grouped": QueryUnit("t", targets=_reduce_targets() + [Agg("count", ColRef("val"), "cv")]),
         "baseline": QueryUnit("t", groupby=[K], force_baseline=True, baseline_entry_count=211, output_columnar=True,
                               targets=[KeyRef(0, "k")] + _reduce_targets())}[layout]
    cp = compile_query(st, q)
    p = cp.plan
    nfrag = st.get("t").num_fragments
    assert nfrag == 4 and all(p.targets[t].skip_null == (1 if layout == "non_grouped" else 0) for t in range(p.num_targets) if p.targets[t].agg != A.AGG_ID)
    partials = [ex.execute(cp, frag_ids=[fr]).buffer.copy() for fr in range(nfrag)]
    n_this = cp.entry_count
    if layout == "baseline":
        n_this = 2 * cp.entry_count
        this, that = oracle_init_buffer(oracle, cp, entry_count=n_this), partials
    else:
        this, that = partials[0].copy(), partials[1:]
    want = this.copy()
    for pbuf in that:
        assert oracle.reduce(p, want, n_this, pbuf, cp.entry_count, cp.init_vals) == 0
    d_this = mgr.to_device(this, 0)
    d_that = [mgr.to_device(pb, 0) for pb in that]
    d_err = mgr.to_device(np.zeros(1, dtype=np.int32), 0)
    ptrs = (C.c_void_p * len(that))(*[d.ptr for d in d_that])
    counts = (C.c_uint32 * len(that))(*([cp.entry_count] * len(that)))
    iv = np.ascontiguousarray(cp.init_vals, dtype=np.int64)
    check(lib().hdk_hip_reduce_buffers(C.byref(p), d_this.ptr, n_this, ptrs, counts, len(that), iv.ctypes.data, d_err.ptr, 0, None))
    mgr.synchronizeStream(0)
    assert int(mgr.to_host(d_err.ptr, 4, 0, np.int32)[0]) == 0
    got = mgr.to_host(d_this.ptr, this.nbytes, 0, np.int64)
    for d in [d_this, d_err] + d_that:
        d.free()
    if layout == "baseline":
        g, w = rs.to_columns(cp, got, n_this), rs.to_columns(cp, want, n_this)
        assert sorted(zip(*g.values())) == sorted(zip(*w.values())) and len(g["k"]) == 64
        assert int(rs.non_empty_mask(cp, got, n_this).sum()) == 64
    else:
        assert np.array_equal(got, want)
        _cp, full, err = run_oracle(oracle, st, cp)  # and the merged partials are the single-pass result
        assert err == 0
        assert_buffers_equal(cp, got, full)
    cols = rs.to_columns(cp, got, n_this)
    assert None not in cols["mnf"] and None not in cols["mxd"]
    if layout != "non_grouped":  # grouped: the planted INT64_MIN of a key's group (every key but 0 has one) is its MIN
        assert sorted(cols["k"]) == list(range(64))
        assert all((mn == A.NULL_BIGINT and s < 0) if k else (mn >= 0 and s > 0) for k, mn, s in zip(cols["k"], cols["mnv"], cols["sv"]))
    else:  # non-grouped: skipped although not nullable
        assert cols["mnv"][0] >= 0 and cols["sv"][0] > 0 and cols["cv"][0] == N.T_ROWS - 63


# ---- the result stages ---------------------------------------------------------------------------------------------------------
def test_result_stages_keep_sentinels_as_values(executors, columns_of_t):
    """execute(result="columns") of a NOT NULL group-by whose key and MIN columns hold their types' sentinels: the column
    descriptors are not nullable, and to_host / sort / filter / group_by / to_columns treat the patterns as the values they are.
    Expectations: numpy over the fetched columns and over the table."""
    t = columns_of_t
    ex = executors("not_null", True)
    C_, V, M16 = ColRef("c"), ColRef("val"), ColRef("m16")
    q = QueryUnit("t", groupby=[C_], targets=[KeyRef(0, "k"), Agg("count", None, "n"), Agg("min", V, "mnv"), Agg("max", V, "mxv"),
                                              Agg("min", M16, "mn16"), Agg("sum", M16, "s16")])
    cols = ex.execute(q, result="columns")
    made = [cols]
    try:
        desc = {d.name: d for d in cols.columns()}
        assert [desc[n].nullable for n in ("k", "n", "mnv", "mxv", "mn16", "s16")] == [False] * 6
        k, n, mnv, mxv, mn16, s16 = cols.to_host()
        c = t["c"].astype(np.int64)
        order = np.argsort(k, kind="stable")
        assert np.array_equal(k[order], np.unique(c)) and k.min() == A.NULL_INT  # the planted INT32_MIN is a group
        for i in order:
            rows = c == k[i]
            assert (n[i], mnv[i], mxv[i], mn16[i], s16[i]) == (rows.sum(), t["val"][rows].min(), t["val"][rows].max(),
                                                              t["m16"][rows].min(), t["m16"][rows].astype(np.int64).sum())
        has_min = mnv == A.NULL_BIGINT
        assert 10 < has_min.sum() < len(k) and (mn16 == A.NULL_SMALLINT).all()
        # to_columns: ints, never None
        pc = cols.to_columns()
        assert pc["k"] == k.tolist() and pc["mnv"] == mnv.tolist() and pc["mn16"] == mn16.tolist()
        assert all(type(v) is int for name in ("k", "mnv", "mn16") for v in pc[name])
        # sort: NULLS FIRST has no NULL to move -- descending, INT64_MIN / INT32_MIN come last; ascending NULLS LAST, first
        for name, col in (("mnv", mnv), ("k", k)):
            down = cols.sort([OrderEntry(name, desc=True, nulls_first=True)])
            up = cols.sort([OrderEntry(name, desc=False, nulls_first=False)])
            made += [down, up]
            ti = list(desc).index(name)
            assert np.array_equal(down.to_host()[ti], np.sort(col)[::-1]) and down.to_host()[ti][-1] == col.min() < -2**30
            assert np.array_equal(up.to_host()[ti], np.sort(col)) and up.to_host()[ti][0] == col.min()
        # filter: mnv < 0 is TRUE for INT64_MIN, k = INT32_MIN for the planted key
        kept = cols.filter([Cmp(TargetRef("mnv"), "<", Lit(0))])
        made.append(kept)
        assert np.array_equal(kept.to_host()[0], k[has_min]) and (kept.to_host()[2] == A.NULL_BIGINT).all()
        one = cols.filter([Cmp(TargetRef("k"), "=", Lit(A.NULL_INT))])
        made.append(one)
        assert one.num_rows == 1 and one.to_host()[1][0] == (c == A.NULL_INT).sum()
        # regroup: MIN over the columns returns the sentinels, and a key holding one is a group like any other
        by16 = cols.group_by(["mn16"], [("id", "mn16", None), ("min", "mnv", "lo"), ("min", "k", "lok"), ("max", "mxv", "hi"), ("count", None, "g")])
        made.append(by16)
        assert [d.nullable for d in by16.columns()] == [False] * 5
        assert [a.tolist() for a in by16.to_host()] == [[A.NULL_SMALLINT], [A.NULL_BIGINT], [A.NULL_INT], [int(mxv.max())], [len(k)]]
        assert by16.to_columns() == {"mn16": [A.NULL_SMALLINT], "lo": [A.NULL_BIGINT], "lok": [A.NULL_INT], "hi": [int(mxv.max())], "g": [len(k)]}
        byn = cols.group_by(["n"], [("id", "n", None), ("min", "mnv", "lo"), ("min", "k", "lok")])
        made.append(byn)
        gn, glo, glok = byn.to_host()
        assert np.array_equal(gn, np.unique(n))
        for i, v in enumerate(gn):
            assert (glo[i], glok[i]) == (mnv[n == v].min(), k[n == v].min())
        assert (glo == A.NULL_BIGINT).any() and (glok == A.NULL_INT).any()
    finally:
        for d in made:
            d.free()


@pytest.fixture(scope="module")
def columns_of_t():
    return N.make_columns(True)["t"]
