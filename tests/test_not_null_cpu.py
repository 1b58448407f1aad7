"""NOT NULL columns on the CPU: the oracle against an independent numpy model, the reference's non-grouped rule by hand, the
facts of a NOT NULL plan, and the route every case of not_null_cases.py takes on an assumed MI355X.

The oracle serves the GPU suite (test_gpu_not_null.py) as the reference; here it is itself checked, for the grouped cases and
the projections, against plain SQL semantics evaluated in numpy over the same arrays -- with no NULL anywhere but in the
column that stays nullable (`nv`) and behind a LEFT join.  The routes are recorded in ROUTES, which the GPU suite asserts
against the kernel names of the launch it runs.
"""
import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd.ir import Agg, And, BinOp, Cast, Cmp, ColRef, ExtractYear, KeyRef, Lit, Not, Or
from hdk_amd.plan import compile_query

import not_null_cases as N
from test_projection import run_projection_oracle
from util import run_oracle

CASES = N.cases()
CASE_IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def tables():
    return {(d, s): N.make_tables(d, s) for d in ("nullable", "not_null") for s in (False, True)}


@pytest.fixture(scope="module")
def columns():
    return {s: N.make_columns(s) for s in (False, True)}


# ---------------------------------------------------------------------------------------------------------------------------
# the independent model: SQL over numpy arrays, declared NOT NULL
# ---------------------------------------------------------------------------------------------------------------------------
def _is_sentinel(arr):
    if arr.dtype == np.float64:
        return arr.view(np.int64) == A.NULL_DOUBLE_BITS
    if arr.dtype == np.float32:
        return arr.view(np.int32) == A.NULL_FLOAT_BITS
    return arr == np.iinfo(arr.dtype).min


class _Rows:
    """The joined rows of a query: one row-index array per table slot (-1: a LEFT join's missing partner)."""

    def __init__(self, cols, q):
        self.cols, self.q = cols, q
        n = len(next(iter(cols[q.table].values())))
        self.idx = [np.arange(n)]
        for j in q.joins:
            inner = cols[j.inner_table]
            by_key = {}
            for r, k in enumerate(zip(*[inner[c].tolist() for c in j.inner_cols])):
                by_key.setdefault(k, []).append(r)
            probe = [self.value(k) for k in j.outer_keys]
            assert not any(m.any() for _v, m, _f in probe)
            rows, partner = [], []
            for r, k in enumerate(zip(*[v.tolist() for v, _m, _f in probe])):
                hits = by_key.get(k, [-1] if j.type == "left" else [])
                rows += [r] * len(hits)
                partner += hits
            rows = np.array(rows, dtype=np.int64)
            self.idx = [i[rows] for i in self.idx] + [np.array(partner, dtype=np.int64)]

    def _resolve(self, c):
        q = self.q
        if c.table in (None, q.table) and c.name in self.cols[q.table]:
            return 0, q.table
        for ji, j in enumerate(q.joins):
            if c.table in (None, j.inner_table) and c.name in self.cols[j.inner_table]:
                return ji + 1, j.inner_table
        raise KeyError(c)

    def value(self, e):
        """-> (values as int64 or float64, NULL mask, float32 accumulator?)"""
        if isinstance(e, ColRef):
            slot, table = self._resolve(e)
            idx = self.idx[slot]
            arr = self.cols[table][e.name][np.maximum(idx, 0)]
            left = slot > 0 and self.q.joins[slot - 1].type == "left"
            null = idx < 0
            if left or (table, e.name) in N.ALWAYS_NULLABLE:
                null = null | _is_sentinel(arr)  # (the sentinel of a matched row too: NULL is in band)
            return arr.astype(np.float64 if arr.dtype.kind == "f" else np.int64), null, arr.dtype == np.float32
        if isinstance(e, Lit):
            n = len(self.idx[0])
            return np.full(n, e.value, dtype=np.float64 if isinstance(e.value, float) else np.int64), np.zeros(n, dtype=bool), False
        if isinstance(e, BinOp):
            (a, am, _), (b, bm, _) = self.value(e.lhs), self.value(e.rhs)
            op = {"+": np.add, "-": np.subtract, "*": np.multiply, "%": np.fmod}[e.op]
            return op(a, b), am | bm, False
        if isinstance(e, ExtractYear):
            v, m, _ = self.value(e.arg)
            return v.astype("datetime64[s]").astype("datetime64[Y]").astype(np.int64) + 1970, m, False
        if isinstance(e, Cast):
            v, m, _ = self.value(e.arg)
            if e.to.is_fp:
                return v.astype(np.float64), m, False
            assert (v >= 0).all()  # decimal(…, 2) -> integer, rounded half up
            return (v + 50) // 100, m, False
        raise TypeError(e)

    def cond(self, c):
        """three-valued: -> (TRUE where not NULL, NULL)"""
        if isinstance(c, Cmp):
            (a, am, _), (b, bm, _) = self.value(c.lhs), self.value(c.rhs)
            op = {"=": np.equal, "<>": np.not_equal, "<": np.less, ">": np.greater, "<=": np.less_equal, ">=": np.greater_equal}[c.op]
            return op(a, b), am | bm
        if isinstance(c, Not):
            t, n = self.cond(c.arg)
            return ~t, n
        (t1, n1), (t2, n2) = self.cond(c.lhs), self.cond(c.rhs)
        if isinstance(c, And):
            false = (~t1 & ~n1) | (~t2 & ~n2)
            return ~false & ~(n1 | n2), ~false & (n1 | n2)
        assert isinstance(c, Or)
        true = (t1 & ~n1) | (t2 & ~n2)
        return true, ~true & (n1 | n2)

    def keep(self):
        keep = np.ones(len(self.idx[0]), dtype=bool)
        for c in self.q.quals:
            t, n = self.cond(c)
            keep &= t & ~n
        return keep


def _aggregate(kind, v, f32, scale):
    """one aggregate over the non-NULL values `v` of a group, in row order"""
    if kind == "count":
        return len(v)
    if len(v) == 0:
        return None
    if kind in ("min", "max"):
        r = v.min() if kind == "min" else v.max()
        return (float(r) if v.dtype.kind == "f" else int(r) / scale if scale > 1 else int(r))
    if v.dtype.kind == "f":  # the reference adds row by row, in float for a FLOAT argument
        s = float(np.cumsum(v.astype(np.float32), dtype=np.float32)[-1]) if f32 else float(np.cumsum(v)[-1])
    else:
        s = sum(v.tolist())
    if kind == "avg":
        s = s / len(v)
    return s / scale if scale > 1 else s


def model_rows(cols, q):
    """The rows of `q` by SQL's rules, sorted: keys and aggregates of a group-by, or the projected rows."""
    rows = _Rows(cols, q)
    keep = rows.keep()
    if N.is_projection(q):
        out = []
        for t in q.targets:
            v, m, _ = rows.value(t.expr)
            out.append([None if nul else x for x, nul in zip(v[keep].tolist(), m[keep].tolist())])
        return sorted(zip(*out), key=_sort_key)
    keys = [rows.value(k)[0][keep] for k in q.groupby]
    stacked = np.stack(keys, axis=1)
    uniq, inverse = np.unique(stacked, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(inverse, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(uniq)))])
    args = []
    for t in q.targets:
        if isinstance(t, Agg) and t.arg is not None:
            v, m, f32 = rows.value(t.arg)
            scale = 100 if isinstance(t.arg, ColRef) and t.arg.name == "dec" else 1
            args.append((v[keep], m[keep], f32, scale))
        else:
            args.append(None)
    out = []
    for g in range(len(uniq)):
        members = order[bounds[g]:bounds[g + 1]]
        row = []
        for t, a in zip(q.targets, args):
            if isinstance(t, KeyRef):
                k = uniq[g, t.idx]
                row.append(float(k) if keys[t.idx].dtype.kind == "f" else int(k))
            elif a is None:
                row.append(len(members))
            else:
                v, m, f32, scale = a
                row.append(_aggregate(t.kind, v[members][~m[members]], f32, scale))
        out.append(tuple(row))
    return sorted(out, key=_sort_key)


def _sort_key(r):
    return tuple((x is None, x) for x in r)


def _oracle_rows(oracle, st, q, env):
    with N.switches(env):
        if N.is_projection(q):
            cp, buf, err, n = run_projection_oracle(oracle, st, q)
            cols = rs.to_columns(cp, buf, nrows=n)
        else:
            cp, buf, err = run_oracle(oracle, st, q)
            cols = rs.to_columns(cp, buf)
    assert err == 0
    return cp, sorted(zip(*[cols[oc.name] for oc in cp.out_cols]), key=_sort_key)


@pytest.mark.parametrize("sentinel", [False, True], ids=["plain", "sentinel"])
@pytest.mark.parametrize("case", [c for c in CASES if not c[0].startswith("ng_")], ids=lambda c: c[0])
def test_oracle_agrees_with_numpy_on_not_null_columns(oracle, tables, columns, case, sentinel):
    """Grouped cases and projections, declared NOT NULL: the planted sentinels are values to SQL and must be to the oracle.
    Integers, counts, keys, MIN and MAX exactly; fp SUM and AVG within 1e-9 relative (test_oracle_sql.py's bound)."""
    name, q, env, _flags = case
    cp, got = _oracle_rows(oracle, tables[("not_null", sentinel)], q, env)
    want = model_rows(columns[sentinel], q)
    assert len(got) == len(want) and (len(got) > 0 or not sentinel)  # (`c = INT32_MIN` finds no row in the plain table)
    fp_sum = [isinstance(t, Agg) and t.kind in ("sum", "avg") for t in q.targets]
    for g, w in zip(got, want):
        for x, y, loose in zip(g, w, fp_sum):
            if loose and isinstance(y, float):
                assert x is not None and abs(x - y) <= 1e-9 * max(1, abs(y)), (name, g, w)
            else:
                assert x == y and type(x) is type(y), (name, g, w)


# ---------------------------------------------------------------------------------------------------------------------------
# non-grouped: the reference's rule
# ---------------------------------------------------------------------------------------------------------------------------
def test_non_grouped_aggregates_skip_the_slot_sentinel_although_not_null(oracle, tables, columns):
    """Without GROUP BY every aggregate with an argument is a *_skip_val call whatever the argument's nullability
    (TargetExprBuilder.cpp:546-551: `need_skip_null = !arg_type->isNullable()` is overridden for non-grouped queries; the slots
    start at the NULL sentinel, OutputBufferInitialization.cpp:57-60).  The skip value is the SLOT's sentinel: for COUNT, MIN
    and MAX the argument type's NULL, for an integer SUM NULL_BIGINT, for an fp SUM NULL_DOUBLE.  So over NOT NULL columns
    holding their sentinel: COUNT, MIN and MAX skip the planted rows, SUM of a narrow column adds them, SUM of an int64
    column skips INT64_MIN."""
    t = columns[True]["t"]
    st = tables[("not_null", True)]
    by_name = {c[0]: c for c in CASES}
    _, got = _oracle_rows(oracle, st, by_name["ng_cols"][1], {})
    got = dict(zip([tg.name for tg in by_name["ng_cols"][1].targets], got[0]))
    n = len(t["val"])
    val, c, m16, m8 = (t[k].astype(np.int64) for k in ("val", "c", "m16", "m8"))
    planted = {"val": val == A.NULL_BIGINT, "c": c == A.NULL_INT, "m16": m16 == A.NULL_SMALLINT, "m8": m8 == A.NULL_TINYINT}
    assert all(p.sum() > 30 for p in planted.values())
    assert got == {
        "n": n,
        "cv": n - int(planted["val"].sum()), "mnv": int(val[~planted["val"]].min()), "mxv": int(val.max()),
        "sv": int(val[~planted["val"]].sum()),                      # the SUM slot's sentinel is the argument's own: skipped
        "cc": n - int(planted["c"].sum()), "mnc": int(c[~planted["c"]].min()), "mxc": int(c.max()),
    }
    q = by_name["ng_cols_sums"][1]
    _, sums = _oracle_rows(oracle, st, q, {})
    sums = dict(zip([tg.name for tg in q.targets], sums[0]))
    assert sums == {"sc": int(c.sum()), "ac": int(c.sum()) / n,  # INT32_MIN is not NULL_BIGINT: added, and counted by AVG
                    "s16": int(m16.sum()), "s8": int(m8.sum())}
    got["sc"] = sums["sc"]
    q = by_name["ng_cols_narrow"][1]
    _, narrow = _oracle_rows(oracle, st, q, {})
    assert dict(zip([tg.name for tg in q.targets], narrow[0])) == {
        "c16": n - int(planted["m16"].sum()), "mn16": int(m16[~planted["m16"]].min()), "mx16": int(m16.max()), "s16": int(m16.sum()),
        "c8": n - int(planted["m8"].sum()), "mn8": int(m8[~planted["m8"]].min()), "s8": int(m8.sum()),
        "a8": int(m8.sum()) / n,                                     # (AVG's sum adds them and its count counts them)
    }
    assert got["mnc"] > A.NULL_INT and got["sc"] < A.NULL_INT and got["sv"] > 0
    # fp: COUNT / MIN / MAX compare with the argument's sentinel (FLOAT's widened to double); SUM and AVG too -- their slot
    # holds a double (a float for a FLOAT argument) whose sentinel is the same bit pattern
    q = by_name["ng_cols_fp"][1]
    _, got = _oracle_rows(oracle, st, q, {})
    got = dict(zip([tg.name for tg in q.targets], got[0]))
    d, f = t["d"], t["f"]
    pd, pf = d.view(np.int64) == A.NULL_DOUBLE_BITS, f.view(np.int32) == A.NULL_FLOAT_BITS
    assert pd.sum() > 30 and pf.sum() > 30
    assert (got["cd"], got["mnd"], got["mxd"]) == (n - int(pd.sum()), float(d[~pd].min()), float(d[~pd].max()))
    assert got["sd"] == float(np.cumsum(d[~pd])[-1]) and got["ad"] == got["sd"] / got["cd"]
    assert (got["cf"], got["mnf"]) == (n - int(pf.sum()), float(f[~pf].min()))
    assert got["sf"] == float(np.cumsum(f[~pf], dtype=np.float32)[-1])
    # the same table declared nullable gives the same non-grouped answers: the rule makes the declaration irrelevant here
    _, twin = _oracle_rows(oracle, tables[("nullable", True)], q, {})
    assert dict(zip([tg.name for tg in q.targets], twin[0])) == got


# ---------------------------------------------------------------------------------------------------------------------------
# plan facts
# ---------------------------------------------------------------------------------------------------------------------------
def _dbits(x):
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def _fbits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


def _leaves(x):
    yield x.leaf0
    for i in range(x.nsteps):
        if x.steps[i].op in (A.OP_ADD, A.OP_SUB, A.OP_MUL, A.OP_DIV, A.OP_MOD):
            yield x.steps[i].rhs


def test_plan_facts_of_a_not_null_group_by(tables):
    st = tables[("not_null", True)]
    by_name = {c[0]: c for c in CASES}
    cp = compile_query(st, by_name["vec_all_widths"][1])
    p = cp.plan
    assert p.query_kind == A.Q_PERFECT_HASH and p.key_has_nulls[0] == 0 and p.keys[0].nullable == 0
    want = {"count": 0, "sum": 0, "avg": 0, "min": 2**63 - 1, "max": -2**63}
    s = 0
    for ti, t in enumerate(cp.query.targets):
        tg = p.targets[ti]
        if isinstance(t, Agg):
            assert tg.skip_null == 0 and tg.arg.nullable == 0 and all(lf.nullable == 0 for lf in _leaves(tg.arg)), t
            assert int(cp.init_vals[s]) == want[t.kind], t
        s += 2 if tg.agg == A.AGG_AVG else 1
    assert all(p.quals[i].lhs.leaf0.nullable == 0 for i in range(p.num_quals))
    # fp and float slots: 0.0, +-DBL_MAX, and +-FLT_MAX in the low four bytes of a float accumulator
    cp = compile_query(st, by_name["vec_fp"][1])
    dmax, fmax = float(np.finfo(np.float64).max), float(np.finfo(np.float32).max)
    want = {"d_count": 0, "d_sum": 0, "d_min": _dbits(dmax), "d_max": _dbits(-dmax), "d_avg": 0,
            "f_count": 0, "f_sum": 0, "f_min": _fbits(fmax), "f_max": _fbits(-fmax), "f_avg": 0}
    s = 0
    for ti, t in enumerate(cp.query.targets):
        tg = cp.plan.targets[ti]
        if isinstance(t, Agg):
            assert tg.skip_null == 0 and int(cp.init_vals[s]) == want[t.name], t
        s += 2 if tg.agg == A.AGG_AVG else 1
    # a 4-byte layout: COUNT(*) by a narrow key
    q4 = by_name["keys_count"][1]
    import dataclasses
    cp = compile_query(st, dataclasses.replace(q4, groupby=q4.groupby[1:], targets=[KeyRef(0, "k2"), Agg("count", None, "n")]))
    assert cp.slot_widths == [4, 4] and cp.plan.key_has_nulls[0] == 0
    # filters and joins: no leaf nullable, the probe without a NULL check
    cp = compile_query(st, by_name["direct_sum_or"][1])
    assert cp.plan.num_filter_ops > 0 and all(cp.plan.quals[i].lhs.leaf0.nullable == 0 for i in range(cp.plan.num_quals))
    cp = compile_query(st, by_name["vec_join_group"][1])
    assert cp.plan.joins[0].null_mode == A.JOIN_NULL_NONE and cp.plan.joins[0].outer_key.nullable == 0
    assert all(cp.plan.targets[ti].skip_null == 0 for ti in range(1, cp.plan.num_targets))
    # a LEFT join makes the inner table's columns nullable again, the outer table's stay as declared
    cp = compile_query(st, by_name["vec_join_left"][1])
    skip = {t.name: cp.plan.targets[ti].skip_null for ti, t in enumerate(cp.query.targets)}
    assert skip == {"k": 0, "n": 0, "cd": 1, "mnd": 1, "mxa": 1, "sa": 1}
    # one nullable operand makes the expression nullable; the NOT NULL leaf stays non-nullable
    cp = compile_query(st, by_name["vec_expr_mixed"][1])
    tg = cp.plan.targets[1]
    assert tg.skip_null == 1 and tg.arg.nullable == 1 and [lf.nullable for lf in _leaves(tg.arg)] == [0, 1]
    # non-grouped: skip although not nullable, slots start at the sentinel
    cp = compile_query(st, by_name["ng_cols"][1])
    for ti, t in enumerate(cp.query.targets):
        tg = cp.plan.targets[ti]
        assert tg.skip_null == (0 if t.arg is None else 1) and (t.arg is None or tg.arg.nullable == 0)
    assert int(cp.init_vals[2]) == A.NULL_BIGINT and int(cp.init_vals[4]) == A.NULL_BIGINT and int(cp.init_vals[6]) == A.NULL_INT
    # and the nullable twin differs in exactly these facts
    cp = compile_query(tables[("nullable", True)], by_name["vec_all_widths"][1])
    assert cp.plan.key_has_nulls[0] == 0 and cp.plan.targets[1].skip_null == 1 and int(cp.init_vals[3]) == A.NULL_BIGINT


# ---------------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------------
# the routes of csrc/route.h a NOT NULL plan must reach (first kernel of the route -> a case that reaches it is found below)
ROUTES_WANTED = {
    "STREAM_DIRECT": "hdk_scan_agg_direct,hdk_finalize",
    "COLS": "hdk_scan_agg_cols,hdk_finalize",
    "KEYS": "hdk_scan_agg_keys,hdk_finalize",
    "KEYS_VALUES": "hdk_scan_agg_keys_values,hdk_finalize",
    "VEC": "hdk_scan_agg_vec,hdk_finalize",
    "VEC_JOIN": "hdk_scan_agg_vec_join,hdk_finalize",
    "VEC_KEYED": "hdk_scan_agg_vec_keyed,hdk_finalize",
    "VEC_MANY": "hdk_scan_agg_vec_many,hdk_finalize",
    "GENERIC": "hdk_scan_agg_generic,hdk_finalize",
    "JOIN_DIRECT": "hdk_join_agg_direct,hdk_finalize",
    "JOIN_SLICED": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced,hdk_join_agg_direct,hdk_finalize",
    "SLICED2": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "BH_PACKED": "hdk_scan_agg_bh_packed,hdk_bh_fold_slabs",
    "BH_PACKED_PLAIN": "hdk_scan_agg_bh_packed_plain,hdk_bh_fold_slabs",
    "BH_DENSE": "hdk_scan_agg_bh_dense,hdk_bh_fold_slabs",
    "BH_DENSE_PLAIN": "hdk_scan_agg_bh_dense_plain,hdk_bh_fold_slabs",
    "BHM": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "BHM_PERFECT": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize",
    "BHM_PART": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "BHM_PART_PERFECT": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_finalize",
    "BH_DENSE_PART": "hdk_bh_dscatter,hdk_bh_daggregate",
    "BH_PARTITIONED": "hdk_bh_scatter,hdk_bh_aggregate",
    "BH_DIRECT": "hdk_scan_agg_bh_direct",
    "BH_VEC": "hdk_scan_agg_bh_vec",
    "BH_VEC_JOIN": "hdk_scan_agg_bh_vec_join",
    "RADIX_PARTITIONED": "hdk_part_scatter,hdk_part_scatter,hdk_part_aggregate,hdk_part_overflow,hdk_scan_agg_baseline_direct",
    "PERFECT_PARTITIONED": "hdk_pp_scatter,hdk_pp_scatter2,hdk_pp_aggregate,hdk_scan_agg_global",
    "BASELINE_DIRECT": "hdk_scan_agg_baseline_direct",
    "GLOBAL": "hdk_scan_agg_global",
    "PROJECT_FAST": "hdk_scan_project_count,hdk_scan_project_offsets,hdk_scan_project_dense,hdk_scan_project_direct",
    "PROJECT_SCALAR": "hdk_scan_project_scalar",
    "PROJECT_JOIN": "hdk_scan_project_join",
}

# case -> why its sentinel-free NOT NULL plan takes another route than its nullable twin (the matcher's refusing condition),
# or route -> why no NOT NULL plan reaches it
_KEYS_OPS = ("match_keys_values (scan_agg.hip) takes at most kKeysMaxOps = 8 word operations: a nullable argument costs its value "
             "word AND a NULL-count word (FOP_ADD_ONE_IF_NULL), so the nullable twin is refused (`nops > kKeysMaxOps`) and goes to "
             "the next route, while the NOT NULL plan has no NULL-count words and fits")
ROUTE_EXCEPTIONS = {
    "keys_values_k8": _KEYS_OPS,        # nullable: VEC
    "vec_all_widths": _KEYS_OPS,        # nullable: VEC
    "vec_narrow": _KEYS_OPS,            # nullable: VEC
    "vec_fp": _KEYS_OPS,                # nullable: VEC
    "vec_fp32": _KEYS_OPS,              # nullable: VEC
    "vec_fp_columnar": _KEYS_OPS,       # nullable: VEC
    "bhm_perfect_two_keys": _KEYS_OPS,  # nullable: BHM_PERFECT (the LDS family's matchers come first for the NOT NULL plan)
    # nullable: COLS
    "ng_cols_narrow": "match_cols (scan_agg.hip) reads a column under ONE skip rule (`ca->col[ci].nullable != nullable`): non-grouped "
                      "COUNT / MIN / MAX of a NOT NULL narrow column skip the type's minimum, the slot's sentinel, while SUM / AVG of it "
                      "skip nothing (target_skip_value, host_match.h) -- the list is refused and the batched interpreter runs it",
}

# (case name, sentinel) -> the kernels of the NOT NULL plan's launch; filled by record_routes()
ROUTES = {}
TWIN_ROUTES = {}  # the same for the nullable declaration


def record_routes(tables=None):
    """ROUTES and TWIN_ROUTES, from hdk_hip_describe_launch on an assumed MI355X (no device is touched)."""
    if not ROUTES:
        tables = tables or {(d, s): N.make_tables(d, s) for d in ("nullable", "not_null") for s in (False, True)}
        for name, q, env, flags in CASES:
            for (declared, sentinel), st in tables.items():
                with N.switches(env):
                    names = N.describe(st, compile_query(st, q), flags)
                (ROUTES if declared == "not_null" else TWIN_ROUTES)[(name, sentinel)] = names
    return ROUTES


def test_not_null_plans_take_their_nullable_twins_routes(tables):
    record_routes(tables)
    differ = {name for name in CASE_IDS if ROUTES[(name, False)] != TWIN_ROUTES[(name, False)]}
    assert differ == {k for k in ROUTE_EXCEPTIONS if k in CASE_IDS}, {n: (ROUTES[(n, False)], TWIN_ROUTES[(n, False)]) for n in differ}


def test_not_null_plans_reach_every_route(tables):
    record_routes(tables)
    reached = set(ROUTES.values())
    missing = {r for r, kernels in ROUTES_WANTED.items() if kernels not in reached}
    assert missing == {k for k in ROUTE_EXCEPTIONS if k in ROUTES_WANTED}, missing
    # the planted variants of the packed shapes route wherever their values let them; the sentinel-free ones stay packed
    assert ROUTES[("bh_dense_plain", True)] == ROUTES_WANTED["BH_DENSE_PLAIN"]
    assert ROUTES[("keys_values_k8", True)] == ROUTES_WANTED["KEYS_VALUES"]  # (an int8 key holding -128)
