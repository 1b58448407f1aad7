"""The cases of tests/relaunch_cases.py, checked without a device: every case takes the route it names (for each half it is
launched with), the cases cover every aggregate route of the routing corpus, their data has the properties that make a second
launch tell a merge from a store, and the oracle runs them.  tests/test_gpu_relaunch.py launches them."""
import json
import os

import pytest

import relaunch_cases as RL
import routing_corpus as RC
import test_kernel_routing_cpu as R
from hdk_amd._lib import sync_switches

CASES = RL.cases()


def _describe_halves(case):
    """the route of each half as PreparedStep asks for it: total_rows = the HALF's rows, the variant applied as
    routing_corpus.describe_all applies one"""
    cp = RL.compiled(case)
    flags, switches = RL.variant_flags(case.variant), RL.variant_switches(case.variant)
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("HDK_HIP_") and k != "HDK_HIP_LIB"}
    try:
        os.environ.update(switches)
        sync_switches()
        rows = case.storage.get(case.query.table).frag_rows
        out = {}
        for split, halves in RL.SPLITS.items():
            for half, frags in zip("AB", halves):
                n = sum(rows[f] for f in frags)
                out[(split, half)] = RC.describe(RL.launch_plan(cp, flags, n), n, flags, R.ASSUMED_MI355X)
        return out
    finally:
        for k in switches:
            os.environ.pop(k, None)
        os.environ.update(saved)
        sync_switches()


def test_fragments_are_unequal_and_off_every_tile():
    assert len(RL.FRAG_ROWS) == 8 and len(set(RL.FRAG_ROWS)) == 8 and 110_000 <= RL.N <= 130_000
    sizes = list(RL.FRAG_ROWS) + [sum(RL.FRAG_ROWS[f] for f in half) for halves in RL.SPLITS.values() for half in halves]
    assert all(n % 64 and n % 1024 and n % 4096 for n in sizes)
    for case in CASES:
        assert tuple(case.storage.get(case.query.table).frag_rows) == RL.FRAG_ROWS, case.id


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_each_half_takes_the_expected_route(case):
    got = _describe_halves(case)
    assert set(got.values()) == {case.expected_route}, got


def test_the_cases_cover_every_aggregate_route_of_the_corpus():
    with open(RC.GOLDEN) as f:
        golden = json.load(f)
    table = RC.unpack(golden)
    small = [ri for ri, rows in enumerate(golden["rows"]) if rows in (100_000, 1_000_000)]
    assert len(small) == 2
    want = {names for rows in table.values() for ri in small for names in rows[ri].values()
            if not names.startswith("error") and not names.split(",")[0].startswith("hdk_scan_project")}
    assert len(want) >= 32
    have = {c.expected_route for c in CASES}
    assert not (set(RL.EXCLUDED) & have), "an excluded route has a case"
    missing = want - have - set(RL.EXCLUDED)
    assert not missing, sorted(missing)
    # the two routes with a second scatter level show in the corpus at 10^9 rows only: reached here as test_gpu_cluster.py does
    level2 = {n for n in golden["names"] if "hdk_join_scatter_level2" in n}
    assert len(level2) == 2 and level2 <= have | set(RL.EXCLUDED)


def test_exclusions_are_few_and_explained():
    assert len(RL.EXCLUDED) <= 3
    for route, reason in RL.EXCLUDED.items():
        assert route.startswith("hdk_") and len(reason.split()) >= 8, (route, reason)


def test_the_targets_cover_every_aggregate_type_and_layout():
    seen, layouts = set(), set()
    for case in CASES:
        cp = RL.compiled(case)
        p = cp.plan
        layouts.add((int(p.query_kind), int(p.key_count), bool(p.keyless), bool(p.output_columnar)))
        for oc, t in zip(cp.out_cols, case.query.targets):
            if oc.kind == "agg":
                tg = p.targets[oc.target_idx]
                arg = "*" if t.arg is None else ("float" if tg.arg_is_fp == RL.A.FP_SLOT_FLOAT else ("double" if tg.arg_is_fp else "int"))
                if isinstance(t.arg, RL.ColRef) and t.arg.table is None:  # (COUNT's slot does not say what it counts: the column does)
                    ctype = case.storage.get(case.query.table).columns[t.arg.name].type
                    arg = ("float" if ctype.size == 4 else "double") if ctype.is_fp else f"int{8 * ctype.size}"
                seen.add((oc.agg, arg))
    for arg in ("int32", "int64", "double", "float"):
        for agg in ("count", "sum", "min", "max", "avg"):
            assert (agg, arg) in seen, (agg, arg)
    assert ("count", "*") in seen
    A = RL.A
    kinds = {(k, nk >= 2) for k, nk, _kl, _c in layouts}
    assert {(A.Q_NON_GROUPED, False), (A.Q_PERFECT_HASH, False), (A.Q_PERFECT_HASH, True), (A.Q_BASELINE_HASH, False),
            (A.Q_BASELINE_HASH, True)} <= kinds
    assert any(kl for k, _nk, kl, _c in layouts if k == A.Q_PERFECT_HASH) and any(not kl for k, _nk, kl, _c in layouts if k == A.Q_PERFECT_HASH)
    assert {k for k, _nk, _kl, c in layouts if c} >= {A.Q_PERFECT_HASH, A.Q_BASELINE_HASH}
    widths = {(a.dtype.kind, a.dtype.itemsize) for case in CASES for c in case.storage.get(case.query.table).columns.values() for a in c.fragments[:1]}
    assert {("i", 4), ("i", 8), ("f", 4), ("f", 8)} <= widths


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_the_oracle_runs_the_case_and_its_data_has_the_properties(oracle, case):
    """each property in at least three groups where the result has 24 groups or more (three of every class of eight keys), in at
    least one otherwise (the plans without GROUP BY have one group, the small domains one key of a class)"""
    cp, want, err = RL.oracle_result(oracle, case)
    assert err == 0
    groups = len(RL.result_rows(cp, want))
    at_least = 3 if groups >= 24 else 1
    for split in RL.SPLITS:
        got = RL.data_properties(oracle, case, split)
        short = {name: got.get(name, 0) for name in RL.expected_properties(case) if got.get(name, 0) < at_least}
        assert not short, (split, groups, short)
        if case.query.groupby:
            assert (got.get("null_key", 0) > 0) == (case.id not in RL.NO_NULL_KEY), (split, got.get("null_key", 0))
    _cp, _want3, err3 = RL.oracle_result(oracle, case, storage=RL.storage_with_half_b_twice(case))
    assert err3 == 0


def test_only_the_hand_edited_plans_have_narrow_slots():
    """compile_query gives every slot 4 or 8 bytes (0: a projected key of a baseline table), so a QueryUnit alone cannot ask for
    the 1- and 2-byte MIN / MAX slots the library accepts in a columnar buffer: relaunch_cases.compiled edits them into the
    NARROW_SLOTS cases.  The day the planner emits such slots itself, this fails and those shapes belong among the cases."""
    for case in CASES:
        widths = set(RL.compiled(case).slot_widths)
        if case.id in RL.NARROW_SLOTS:
            assert {1, 2} <= widths, (case.id, widths)
        else:
            assert widths <= {0, 4, 8}, (case.id, widths)
    assert len(RL.NARROW_SLOTS) >= 1 and set(RL.NARROW_SLOTS) <= {c.id for c in CASES}


def test_most_cases_have_every_property():
    """the exceptions of relaunch_cases.LACKS stay exceptions: most grouped cases show groups in one half only, NULLs in one half
    only and (with a MIN / MAX target) extremes split across the halves"""
    assert set(RL.LACKS) | set(RL.NO_NULL_KEY) <= {c.id for c in CASES}
    grouped = [c for c in CASES if c.query.groupby]
    full = [c for c in grouped if {"only_a", "only_b", "both", "null_a", "null_b", "null_both"} <= RL.expected_properties(c)]
    assert len(full) >= 0.8 * len(grouped), (len(full), len(grouped))
    assert sum("min_in_a" in RL.expected_properties(c) for c in CASES) >= 10 and sum("max_in_b" in RL.expected_properties(c) for c in CASES) >= 10
