"""The cases of tests/error_cases.py, checked without a device: every case takes the route it names under every placement, the
cases cover every aggregate route that a corpus plan with an arithmetic step reaches, each placement's data has the property its
name promises, and an independent statement of the expected code -- which rows pass the filters, find a partner and have
non-NULL operands, and whether the exact integer result leaves the type -- equals what the oracle returns.
tests/test_gpu_error_cases.py launches them."""
import json
import os

import numpy as np
import pytest

import error_cases as E
import relaunch_cases as RL
import routing_corpus as RC
import test_kernel_routing_cpu as R
from hdk_amd import _abi as A
from hdk_amd._lib import sync_switches

CASES = E.cases()
IDS = [c.id for c in CASES]


def _describe(case, placement):
    """the route as PreparedStep asks for it: the plan over the placement's storage, all its rows, the variant applied as
    routing_corpus.describe_all applies one (test_relaunch_cases_cpu._describe_halves' way)"""
    cp = E.compiled(case, placement)
    flags, switches = RL.variant_flags(case.variant), RL.variant_switches(case.variant)
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("HDK_HIP_") and k != "HDK_HIP_LIB"}
    try:
        os.environ.update(switches)
        sync_switches()
        return RC.describe(RL.launch_plan(cp, flags, E.N), E.N, flags, R.ASSUMED_MI355X)
    finally:
        for k in switches:
            os.environ.pop(k, None)
        os.environ.update(saved)
        sync_switches()


def test_fragments_are_unequal_and_off_every_tile():
    assert len(E.FRAGS) == 9 and len(set(E.FRAGS)) == 9 and sorted(E.FRAGS)[0] == 1 and 110_000 <= E.N <= 130_000
    assert all(n % 64 and n % 1024 and n % 4096 for n in E.FRAGS)
    ends = np.cumsum(E.FRAGS)
    assert E.ROWS["first"] == 0 and E.ROWS["last"] == E.N - 1 and E.ROWS["last"] % 64 != 63
    assert E.ROWS["seam"] + 1 in ends[1:-2] and E.FRAGS[list(ends).index(E.ROWS["alone"] + 1)] == 1
    for case in CASES:
        assert tuple(case.build().get(case.query.table).frag_rows) == E.FRAGS, case.id


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_each_case_takes_the_expected_route(case):
    got = {p: _describe(case, p) for p in E.placements(case)}
    assert got == {p: E.expected_route(case, p) for p in got}
    if not isinstance(case.expected_route, str):  # the statistics of the planted data decide: both routes are pinned
        assert case.expected_route["clean"] != case.expected_route["*"]


def _arithmetic_steps(p):
    exprs = [p.targets[t].arg for t in range(p.num_targets) if p.targets[t].has_arg or p.query_kind == A.Q_PROJECTION] + [p.keys[k] for k in range(p.key_count)] + \
        [p.quals[q].lhs for q in range(p.num_quals)]
    return [e.steps[s] for e in exprs for s in range(e.nsteps) if e.steps[s].op <= A.OP_MOD]


def _routes_of_corpus_plans_with_arithmetic():
    with open(RC.GOLDEN) as f:
        golden = json.load(f)
    table = RC.unpack(golden)
    small = [ri for ri, rows in enumerate(golden["rows"]) if rows in (100_000, 1_000_000)]
    assert len(small) == 2
    plans = [pid for pid, cp in RC.corpus() if _arithmetic_steps(cp.plan)]
    assert len(plans) >= 40
    want = {names for pid in plans for ri in small for names in table[pid][ri].values()
            if not names.startswith("error")}
    return golden, want


def test_the_cases_cover_every_aggregate_route_that_evaluates_arithmetic():
    golden, want = _routes_of_corpus_plans_with_arithmetic()
    assert len(want) >= 21 and sum(r.startswith("hdk_scan_project") for r in want) >= 3
    have = {r for c in CASES for r in ([c.expected_route] if isinstance(c.expected_route, str) else c.expected_route.values())}
    assert not (set(E.EXCLUDED) & have), "an excluded route has a case"
    missing = want - have - set(E.EXCLUDED)
    assert not missing, sorted(missing)
    # the two routes with a second scatter level show in the corpus at 10^9 rows only: reached as test_gpu_cluster.py does
    level2 = {n for n in golden["names"] if "hdk_join_scatter_level2" in n}
    assert len(level2) == 2 and level2 <= have
    # the routes the cases must reach whatever the corpus holds
    first = {r.split(",")[0] for r in have}
    assert {"hdk_scan_agg_direct", "hdk_scan_agg_vec", "hdk_scan_agg_vec_join", "hdk_scan_agg_vec_many", "hdk_scan_agg_vec_keyed", "hdk_scan_agg_bh_vec",
            "hdk_scan_agg_bh_vec_join", "hdk_scan_agg_generic", "hdk_scan_agg_global", "hdk_pp_scatter", "hdk_join_agg_direct", "hdk_cluster_by_key",
            "hdk_join_order_probe", "hdk_scan_project", "hdk_scan_project_scalar", "hdk_scan_project_join", "hdk_scan_project_keyed"} <= first
    assert any("hdk_join_agg_sliced," in r for r in have) and any("hdk_join_agg_sliced2," in r for r in have)
    # every overflow route takes every placement: a case with a filter and one with a join where the route has them
    for route in have:
        if not any(k in route for k in ("hdk_scan_agg_bhm", "hdk_bhm_scatter", "hdk_join_agg_sliced2", "hdk_scan_agg_bh_dense")):
            on = [c for c in CASES if route in (c.expected_route if isinstance(c.expected_route, str) else c.expected_route["*"])
                  and c.spec.op in "+-*" and c.spec.only is None]
            assert on, route
            assert any(set(E.RAISING) | {"null_operand"} <= set(E.placements(c)) for c in on), route


def test_no_plan_with_arithmetic_reaches_the_kernels_that_evaluate_none():
    """error_cases.NO_ARITHMETIC: three routes whose matchers admit plain columns only have nothing to test here"""
    _golden, want = _routes_of_corpus_plans_with_arithmetic()
    for kernel, where in E.NO_ARITHMETIC.items():
        assert not any(r.split(",")[0] == kernel for r in want), kernel
        assert len(where.split()) >= 6
    by_id = {c.id: c for c in CASES}
    for cid in ("baseline_mul8", "baseline_partitioned_mul8"):  # the baseline-hash shape with an expression: the general kernel
        assert by_id[cid].expected_route == "hdk_scan_agg_global"
    assert by_id["bh_mul4"].expected_route == "hdk_scan_agg_bh_vec"


def test_exclusions_are_few_and_explained():
    assert len(E.EXCLUDED) <= 3
    for route, reason in E.EXCLUDED.items():
        assert route.startswith("hdk_") and len(reason.split()) >= 8, (route, reason)


def test_the_planner_emits_the_width_each_case_names():
    """check_width of a column-column and a column-literal step: the wider operand's SQL type, an integer literal INTEGER
    (plan.py: make_expr); every width the planner can emit has a case"""
    seen = set()
    for case in CASES:
        steps = _arithmetic_steps(E.compiled(case).plan)
        assert steps, case.id
        ops = {"+": A.OP_ADD, "-": A.OP_SUB, "*": A.OP_MUL, "/": A.OP_DIV, "%": A.OP_MOD, "f/": A.OP_DIV}
        mine = [s for s in steps if s.op == ops[case.spec.op]]
        assert mine and all(s.check_width == case.spec.width for s in mine), (case.id, [s.check_width for s in mine])
        assert all((s.rhs.kind == A.LEAF_INT) == (case.spec.b[0] == "lit") for s in mine), case.id
        seen.add((case.spec.op, case.spec.width, case.spec.b[0] == "lit"))
    for width in (1, 2, 4, 8):
        assert {op for op, w, lit in seen if w == width and not lit} >= ({"+", "-", "*"} if width >= 4 else {"*"}), width
    assert {(op, w) for op, w, lit in seen if lit} >= {("+", 4), ("-", 4), ("+", 8), ("-", 8)}  # (a literal is 4 bytes wide at least)
    assert {op for op, _w, _l in seen} >= {"/", "%", "f/"}


# ---- the independent statement ----------------------------------------------------------------------------------------------------
def _is_null(arr, nullable):
    if not nullable:
        return np.zeros(len(arr), dtype=bool)
    if arr.dtype.kind == "f":
        return arr.view(np.int64) == np.int64(A.NULL_DOUBLE_BITS)
    return arr == np.iinfo(arr.dtype).min


def _combined(storage, table, cols):
    """one int64 per row for a (composite) key of small components"""
    out = np.zeros(storage.get(table).num_rows, dtype=np.int64)
    for c in cols:
        v = E.column(storage, table, c).astype(np.int64)
        assert len(cols) == 1 or (0 <= v.min() and v.max() < 1000)
        out = out * 1000 + v
    return out


def evaluate(case, storage):
    """Every (outer row, inner row) the plan's row function evaluates the case's step for, stated from the data alone:
    -> (outer row per pair, evaluated, offends, exact results of the evaluated pairs as Python ints where they matter).
    A pair is evaluated when its outer row passes the filters, has a partner (a LEFT join keeps the row and reads the inner
    operand as NULL) and neither operand is NULL."""
    s = case.spec
    outer = case.query.table
    t = storage.get(outer)
    cols = {c: E.column(storage, outer, c) for c in t.column_order}
    n = t.num_rows
    live = s.live(cols) if s.live is not None else np.ones(n, dtype=bool)
    orow, irow = np.arange(n), None
    if s.join is not None:
        fkey, dkey = _combined(storage, outer, s.join.fk), _combined(storage, s.join.dim, s.join.dkey)
        order = np.argsort(dkey, kind="stable")
        lo, hi = np.searchsorted(dkey[order], fkey, "left"), np.searchsorted(dkey[order], fkey, "right")
        cnt = hi - lo
        if len(s.join.fk) == 1:
            cnt[fkey == np.iinfo(np.int64).min] = 0  # a NULL key has no partner
        orow = np.repeat(np.arange(n), cnt)
        irow = order[np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
        if s.join.kind == "left":
            alone = np.flatnonzero(cnt == 0)
            orow, irow = np.concatenate([orow, alone]), np.concatenate([irow, np.full(len(alone), -1)])

    def operand(ref):
        if ref[0] == "lit":
            return np.full(len(orow), ref[1], dtype=np.int64), np.zeros(len(orow), dtype=bool)
        col = storage.get(ref[0]).columns[ref[1]]
        arr = E.column(storage, ref[0], ref[1])
        null = _is_null(arr, col.type.nullable)
        if ref[0] == outer:
            return arr[orow], null[orow]
        return arr[irow], null[irow] | (irow < 0)

    (a, a_null), (b, b_null) = operand(s.a), operand(s.b)
    evaluated = live[orow] & ~a_null & ~b_null
    if s.op in ("/", "%", "f/"):
        return orow, evaluated, b == 0, None
    a, b = a.astype(np.int64), b.astype(np.int64)
    m = E.type_max(s.width)
    estimate = {"+": np.abs(a.astype(np.float64)) + np.abs(b.astype(np.float64)), "-": np.abs(a.astype(np.float64)) + np.abs(b.astype(np.float64)),
                "*": np.abs(a.astype(np.float64)) * np.abs(b.astype(np.float64))}[s.op]
    big = estimate >= 2.0**62  # (below it the int64 result is the exact one)
    with np.errstate(over="ignore"):
        r = {"+": a + b, "-": a - b, "*": a * b}[s.op]
    offends = (r > m) | (r < -m - 1)
    exact = {}
    for i in np.flatnonzero(big):
        x, y = int(a[i]), int(b[i])
        exact[int(i)] = {"+": x + y, "-": x - y, "*": x * y}[s.op]
        offends[i] = not (-m - 1 <= exact[int(i)] <= m)
    results = {int(i): exact.get(int(i), int(r[i])) for i in np.flatnonzero(evaluated & (big | (np.abs(r) >= m - 1)))}
    return orow, evaluated, offends, results


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_each_placement_has_its_property_and_the_oracle_agrees_with_the_independent_statement(oracle, case):
    s = case.spec
    code = A.ERR_DIV_BY_ZERO if s.op in ("/", "%", "f/") else A.ERR_OVERFLOW_OR_UNDERFLOW
    m = E.type_max(s.width) if s.width else 0
    for placement in E.placements(case):
        storage = E.storage_for(case, placement)
        orow, evaluated, offends, results = evaluate(case, storage)
        raising = evaluated & offends
        if placement in E.RAISING or placement == "stale":
            where = E.ROWS["last" if placement == "stale" else placement]
            # (exactly one ROW; a one-to-many join may evaluate it once per partner)
            assert raising.any() and set(orow[raising]) == {where}, (placement, int(raising.sum()))
        else:
            assert raising.sum() == 0, (placement, orow[raising][:5])
        for dead_row in E.DEAD_ROWS if placement in ("filtered", "null_operand", "no_partner") else ():
            # the planted operands are there, in a row that is not evaluated
            at = orow == dead_row
            # (null_operand under a one-to-many join: the pair with the NULL partner; the row's other partners are evaluated)
            assert (not evaluated[at].all()) if placement == "null_operand" else (not evaluated[at].any()), placement
            planted = E.placement_edits(case, placement)
            assert planted and any(r == dead_row for rows in planted.values() for r in rows)
            if placement != "null_operand":
                assert (offends & ~evaluated).sum() >= 1, placement
        if placement == "edge":
            ends = set(results.values()) & {m, -m}
            assert ends == ({m, -m} if s.b[0] != "lit" else ({m} if s.op == "+" else {-m})), (placement, ends)
        if placement == "edge_min":
            assert -m - 1 in set(results.values())
        stated = code if raising.any() else 0
        assert stated == E.expected_code(case, placement), placement
        _cp, _buf, err = E.oracle_result(oracle, case, placement)
        assert err == stated, (placement, err, stated)


def _sliced_body(case):
    """scan_join.hip, match_join_sliced: the FAST probe body for ONE target SUM(x + payload) into an ADD word unless SLICE_GENERAL
    is set; jd_eval otherwise"""
    targets = case.query.targets
    one_sum = len(targets) == 1 and targets[0].kind == "sum" and case.spec.op == "+"
    return "fast" if one_sum and "SLICE_GENERAL" not in case.variant else "jd_eval"


def test_both_bodies_of_the_sliced_join_have_a_case_with_every_placement():
    sliced = [c for c in CASES if "hdk_join_agg_sliced," in E.expected_route(c, "last")]
    bodies = {}
    for c in sliced:
        assert set(E.RAISING) | {"null_operand", "no_partner", "edge", "edge_min"} <= set(E.placements(c)), c.id
        bodies.setdefault(_sliced_body(c), []).append(c.id)
    assert bodies == {"fast": ["join_sliced_add8"], "jd_eval": ["join_sliced_jd_eval_add8", "join_sliced_general_add8"]}, bodies


def test_the_sliced2_bound_pair_sits_on_the_bounds(oracle):
    """the statistics of fact.val and dim.dval at the bound are exactly the last values scan_join.hip admits (x_fits_narrow,
    payload_fits_32_bits); each `past` table moves ONE of the four ends by one, and nothing else"""
    def ends(kind):
        st = E.star_bound_storage(kind)
        x, p = st.get("fact").columns["val"].table_stats(), st.get("dim").columns["dval"].table_stats()
        return {"x_min": x.min, "x_max": x.max, "p_min": p.min, "p_max": p.max}
    at = ends("at")
    assert at == {"x_min": -2**31 + 1, "x_max": 2**31 - 1, "p_min": -2**31 + 2, "p_max": 2**31 - 1}
    assert E.star_bound_storage("at").get("fact").columns["val"].table_stats().has_nulls
    for kind in ("x_max", "x_min", "p_max", "p_min"):
        got = ends(kind)
        assert {k for k in at if got[k] != at[k]} == {kind} and abs(got[kind] - at[kind]) == 1, (kind, got)
    by_id = {c.id: c for c in CASES}
    assert "hdk_join_agg_sliced2" in by_id["s2_at_bound"].expected_route
    for kind in ("x_max", "x_min", "p_max", "p_min"):
        assert "sliced2" not in by_id[f"s2_past_{kind}"].expected_route


def test_divisions_that_raise_nothing_give_the_reference_values(oracle):
    """INT64_MIN / -1 and x % -1 in NOT NULL columns (error_cases.VALUE_ROW, the group of key 9).  What the oracle gives, written
    down: the quotient wraps to INT64_MIN and is aggregated as a value (MIN takes it), the remainder is 0, no error"""
    imin = -2**63
    for case in CASES:
        if not case.id.endswith("_values"):
            continue
        st = case.build()
        m, qm, key = (E.column(st, "t", c) for c in ("m", "qm", "key"))
        assert m[E.VALUE_ROW] == imin and qm[E.VALUE_ROW] == -1 and key[E.VALUE_ROW] == 9 and (qm != 0).all()
        cp, buf, err = E.oracle_result(oracle, case, "clean")
        assert err == 0
        row = RL.result_rows(cp, buf)[(9,)]
        rest = [(int(a), int(b)) for a, b, k, i in zip(m, qm, key, range(len(m))) if k == 9 and i != E.VALUE_ROW]
        trunc = lambda a, b: abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1)  # noqa: E731
        assert row["qmin"] == imin and row["qmax"] == max(trunc(a, b) for a, b in rest)
        assert row["r"] == sum(a - trunc(a, b) * b for a, b in rest)  # (the special row adds 0; so does every x % -1)
        assert any(b == -1 for _a, b in rest)


def test_stale_statistics_are_stale():
    """a `stale` placement's planted value lies outside the bounds its column records; every other placement's statistics hold"""
    n = 0
    for case in CASES:
        for placement in E.placements(case):
            st = E.storage_for(case, placement)
            col = st.get(case.spec.a[0]).columns[case.spec.a[1]]
            arr = E.column(st, *case.spec.a)
            valid = arr[~_is_null(arr, col.type.nullable)]
            inside = col.table_stats().min <= valid.min() and valid.max() <= col.table_stats().max
            assert inside == (placement != "stale"), (case.id, placement)
            n += placement == "stale"
    assert n >= 6
