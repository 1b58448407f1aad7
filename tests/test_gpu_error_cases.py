"""The device reports the reference's arithmetic error codes -- 1, division by zero; 7, overflow or underflow of a checked + - *
-- on every route that evaluates such a step, and only for rows the reference evaluates.

Each case of tests/error_cases.py is launched once per placement over all its fragments, under its own variant; every launch
first asserts the route.  A raising placement (exactly one live offending row: the first row, the last row of the last fragment
inside a partial tile, the last row of a middle fragment, the row of a one-row fragment) must end in HdkHipError with the oracle's
code; a silent one (the same operands in a row that a filter rejects, beside a NULL operand, without a join partner; results
exactly at the ends of the type) must leave error word 0 and the oracle's buffer, bit for bit (a projection: the oracle's rows).
Where FORCE_SCALAR names another kernel, every placement is launched under it as well.
tests/test_error_cases_cpu.py checks routes, coverage, the data's properties and the expected codes without a device."""
import numpy as np
import pytest

import error_cases as E
import relaunch_cases as RL
import routing_corpus as RC
import test_kernel_routing_cpu as R
from hdk_amd import _abi as A
from hdk_amd._lib import HdkHipError
from hdk_amd.plan import compile_query

from test_gpu_projection import _sorted_rows
from test_gpu_relaunch import _assert_is_the_oracles
from util import run_oracle

pytestmark = pytest.mark.gpu

CASES = {c.id: c for c in E.cases()}


def _scalar_route(case, placement):
    """what FORCE_SCALAR names for the placement's plan (with the plain join table, no switches: the flag overrides both), or
    None where that is the launch's own route"""
    names = RC.describe(E.compiled(case, placement), E.N, A.LAUNCH_FORCE_SCALAR, R.ASSUMED_MI355X)
    return None if names == E.expected_route(case, placement) else names


SCALAR = {(cid, p): _scalar_route(c, p) for cid, c in CASES.items() for p in E.placements(c)}
PARAMS = [(cid, p, "own") for cid, c in CASES.items() for p in E.placements(c)] + [(cid, p, "scalar") for (cid, p), r in SCALAR.items() if r]

@pytest.fixture
def executor_of(gpu_executor_factory):
    """an executor over a placement's storage for one test; its device columns and join tables are released with the test (every
    placement has a storage of its own: none would be used again)"""
    made = []

    def make(storage):
        made.append(gpu_executor_factory(storage))
        return made[-1]

    yield make
    for ex in made:
        ex.cache.clear()


def _assert_projection_is_the_oracles(cp, res, want, nrows):
    """the same rows, in any order: row position and every projected value, bit for bit"""
    assert res.total_matched == nrows
    assert np.array_equal(_sorted_rows(cp, res.buffer, nrows), _sorted_rows(cp, want, nrows))


def _flags(case, mode, monkeypatch):
    if mode == "scalar":
        return A.LAUNCH_FORCE_SCALAR
    for name, value in RL.variant_switches(case.variant).items():
        monkeypatch.setenv(name, value)
    return RL.variant_flags(case.variant)


@pytest.mark.parametrize("cid,placement,mode", PARAMS, ids=["-".join(p) for p in PARAMS])
def test_the_launch_reports_the_reference_code(oracle, executor_of, monkeypatch, cid, placement, mode):
    case = CASES[cid]
    cp, want, err = E.oracle_result(oracle, case, placement)
    assert err == E.expected_code(case, placement)
    step = executor_of(E.storage_for(case, placement)).prepare(cp, flags=_flags(case, mode, monkeypatch))
    try:
        assert step.kernel_names() == (E.expected_route(case, placement) if mode == "own" else SCALAR[cid, placement])
        if err:
            with pytest.raises(HdkHipError) as ei:
                step.run()
            assert ei.value.code == err
        else:
            res = step.run()
            assert res.error_code == 0
            if E.is_projection(case):
                _assert_projection_is_the_oracles(cp, res, want, E.oracle_matched(case, placement))
            else:
                _assert_is_the_oracles(oracle, cp, res.buffer, want)
    finally:
        step.free()


@pytest.mark.parametrize("variant", E.BOTH_CODES_VARIANTS)
def test_the_larger_code_is_reported_when_two_are_raised(oracle, executor_of, variant):
    """include/hdk_hip.h, hdk_hip_launch: of several codes the numerically largest.  (The oracle walks the rows in order and
    reports the first one -- this case alone is held to the documented rule, not to the oracle.)"""
    st, q = E.both_codes()
    cp, _want, err = run_oracle(oracle, st, compile_query(st, q))
    assert err == A.ERR_DIV_BY_ZERO
    step = executor_of(st).prepare(cp, flags=RL.variant_flags(variant))
    try:
        assert step.kernel_names().split(",")[0] == {"generic": "hdk_scan_agg_vec", "scalar": "hdk_scan_agg_generic", "global": "hdk_scan_agg_global"}[variant]
        with pytest.raises(HdkHipError) as ei:
            step.run()
        assert ei.value.code == max(A.ERR_DIV_BY_ZERO, A.ERR_OVERFLOW_OR_UNDERFLOW)
    finally:
        step.free()


@pytest.mark.parametrize("cid,placement", E.NOTHING_STICKS, ids=[c for c, _p in E.NOTHING_STICKS])
def test_a_launch_that_raised_leaves_nothing_behind(oracle, executor_of, monkeypatch, cid, placement):
    """one executor, two prepared steps: `clean` over the fragments without the planted row, `bad` over all of them.  clean, bad,
    clean: both clean runs give the oracle's buffer and `bad` raises -- no fallback flag, watch word or workspace cursor of the
    launch that ended in an error reaches the next one"""
    case = CASES[cid]
    row = E.ROWS["last" if placement == "stale" else placement]
    without = [f for f in range(len(E.FRAGS)) if f != E.fragment_of(row)]
    cp, want, err = E.oracle_result(oracle, case, placement, frag_ids=without)
    _cp, _all, err_all = E.oracle_result(oracle, case, placement)
    assert err == 0 and err_all == E.expected_code(case, placement) != 0
    flags = _flags(case, "own", monkeypatch)
    ex = executor_of(E.storage_for(case, placement))
    steps = []
    try:
        clean = ex.prepare(cp, frag_ids=without, flags=flags)
        steps.append(clean)
        bad = ex.prepare(cp, flags=flags)
        steps.append(bad)
        assert bad.kernel_names() == E.expected_route(case, placement)
        for _ in range(2):
            res = clean.run()
            assert res.error_code == 0
            _assert_is_the_oracles(oracle, cp, res.buffer, want)
            with pytest.raises(HdkHipError) as ei:
                bad.run()
            assert ei.value.code == err_all
        res = clean.run()
        assert res.error_code == 0
        _assert_is_the_oracles(oracle, cp, res.buffer, want)
    finally:
        for step in steps:
            step.free()


def test_the_parametrisation_is_what_it_should_be():
    """FORCE_SCALAR names another kernel for every case but those that run the row-at-a-time interpreter or the general
    open-addressing kernel anyway"""
    own = {cid for (cid, _p), r in SCALAR.items() if r is None}
    assert own >= {cid for cid, c in CASES.items() if c.variant == "scalar"}
    for (cid, p), r in SCALAR.items():
        if r is None:
            own_route = E.expected_route(CASES[cid], p)
            assert own_route in ("hdk_scan_agg_generic,hdk_finalize", "hdk_scan_agg_global", "hdk_scan_project_scalar") or \
                own_route.endswith(",hdk_scan_agg_global"), (cid, p)
        else:
            assert r.split(",")[0] in ("hdk_scan_agg_generic", "hdk_scan_agg_global", "hdk_scan_project_scalar"), (cid, p, r)
    assert 800 <= len(PARAMS) <= 1400
