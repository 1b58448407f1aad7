"""A launch merges into what its output buffer holds (include/hdk_hip.h: hdk_hip_launch) -- on every aggregate route.

Each case of tests/relaunch_cases.py is launched as two halves with DIFFERENT rows into one buffer: half A into a freshly
initialised buffer, half B into what A left, with no initialisation in between.  The halves are the interleaved fragments
(0, 2, 4, 6 | 1, 3, 5, 7) or the contiguous ones (0-3 | 4-7); the two launches take the case's route X both times, or X and then
another kernel (FORCE_GLOBAL_ATOMICS; FORCE_SCALAR where that is no different kernel or the plan is not grouped), or the other
kernel first.  The buffer must equal the oracle's over all eight fragments, bit for bit: the data (see relaunch_cases) has
groups that only one half sees, arguments that are NULL in one half only, minima in A and maxima in B, and sums that are exact
in any order.  Once per case a third launch of half B must give the oracle's result over A + B + B (the same fragments imported
twice), which a fold that is right only on a fresh or once-touched table misses.
tests/test_relaunch_cases_cpu.py checks routes, coverage and the data's properties without a device."""
import numpy as np
import pytest

import relaunch_cases as RL
import routing_corpus as RC
import test_kernel_routing_cpu as R
from hdk_amd import _abi as A

from test_gpu_baseline import _assert_reference_placement, _check_rows, _rows
from util import assert_buffers_equal

pytestmark = pytest.mark.gpu

# (built at import, as the parametrisation needs them: collecting this module generates the cases' tables -- under a second, shared
# with test_relaunch_cases_cpu.py through relaunch_cases' caches -- and asks the library for routes, so it needs the built library)
CASES = {c.id: c for c in RL.cases()}


def _other_flag(case):
    """the launch flag of the OTHER kernel of a case: FORCE_GLOBAL_ATOMICS, FORCE_SCALAR for a non-grouped plan or where the
    global flag names the case's own route, None where neither is a different kernel.  (Asked of the plan with the plain join
    table and without the case's switches: both flags keep the executor from fusing the table and override every switch; the
    test asserts that the step so prepared does not name the case's route.)  1- and 2-byte slots are refused by the global
    kernel (scan_agg.hip: only the LDS strategy writes them): those cases alternate the two interpreters."""
    if case.id in RL.NARROW_SLOTS:
        return A.LAUNCH_FORCE_GENERIC if RL.variant_flags(case.variant) & A.LAUNCH_FORCE_SCALAR else A.LAUNCH_FORCE_SCALAR
    cp = RL.compiled(case)
    candidates = (A.LAUNCH_FORCE_SCALAR,) if cp.plan.query_kind == A.Q_NON_GROUPED else (A.LAUNCH_FORCE_GLOBAL_ATOMICS, A.LAUNCH_FORCE_SCALAR)
    for flag in candidates:
        if RC.describe(cp, RL.N // 2, flag, R.ASSUMED_MI355X) != case.expected_route:
            return flag
    return None


OTHER = {cid: _other_flag(c) for cid, c in CASES.items()}
PARAMS = [(cid, split, order) for cid in CASES for split in RL.SPLITS
          for order in (("x_x", "x_other", "other_x") if OTHER[cid] is not None else ("x_x",))]

_executors = {}


def _executor(factory, storage):
    """one executor per storage: the columns and join tables go to the device once"""
    if id(storage) not in _executors:
        _executors[id(storage)] = factory(storage)
    return _executors[id(storage)]


def _assert_is_the_oracles(oracle, cp, got, want):
    p = cp.plan
    if p.query_kind != A.Q_BASELINE_HASH:
        # entries, stored keys and untouched slots; sums are exact (multiples of 1/8), so no tolerance
        assert_buffers_equal(cp, got, want, fp_rtol=0.0, float32_rtol=0.0)
        assert np.array_equal(np.asarray(got[:cp.buffer_quads]), np.asarray(want[:cp.buffer_quads]))
        return
    # open addressing: the entry a group takes depends on the insertion order -- rows by key, every value exact
    _check_rows(cp, got, want, rtol=0.0, float32_rtol=0.0)
    rows = _rows(cp, got)
    nk = int(p.key_count)
    assert len({r[:nk] for r in rows}) == len(rows) == len(_rows(cp, want))  # no group twice
    if not p.output_columnar:
        _assert_reference_placement(oracle, cp, got)


@pytest.mark.parametrize("cid,split,order", PARAMS, ids=["-".join(p) for p in PARAMS])
def test_a_second_launch_merges_into_the_first(oracle, gpu_executor_factory, monkeypatch, cid, split, order):
    case = CASES[cid]
    cp, want, err = RL.oracle_result(oracle, case)
    assert err == 0
    for name, value in RL.variant_switches(case.variant).items():
        monkeypatch.setenv(name, value)
    ex = _executor(gpu_executor_factory, case.storage)
    x = RL.variant_flags(case.variant)
    first, second = {"x_x": (x, x), "x_other": (x, OTHER[cid]), "other_x": (OTHER[cid], x)}[order]
    a_ids, b_ids = RL.SPLITS[split]
    steps = []
    try:
        s1 = ex.prepare(cp, frag_ids=a_ids, flags=first)
        steps.append(s1)
        s2 = ex.prepare(cp, frag_ids=b_ids, flags=second, out_ptr=s1.out_ptr)
        steps.append(s2)
        for step, is_x in ((s1, order != "other_x"), (s2, order != "x_other")):
            if is_x:
                assert step.kernel_names() == case.expected_route
            else:
                assert step.kernel_names() != case.expected_route
        s1.init_output()
        s1.launch()
        s2.launch()  # (no init_output, no INIT_OUTPUT: into what s1 left)
        ex.mgr.synchronizeStream(0)

        def read():
            assert int(ex.mgr.to_host(s1.d_err.ptr, 4, 0, np.int32)[0]) == 0
            assert int(ex.mgr.to_host(s2.d_err.ptr, 4, 0, np.int32)[0]) == 0
            return ex.mgr.to_host(s1.out_ptr, max(cp.buffer_bytes, 8), 0, np.int64)[:cp.buffer_bytes // 8]

        _assert_is_the_oracles(oracle, cp, read(), want)
        if split == "interleaved" and order == "x_x":
            # a third launch, half B again: the oracle over the table with B's fragments imported twice
            _cp, want3, err3 = RL.oracle_result(oracle, case, storage=RL.storage_with_half_b_twice(case, split))
            assert err3 == 0
            s2.launch()
            ex.mgr.synchronizeStream(0)
            _assert_is_the_oracles(oracle, cp, read(), want3)
    finally:
        for step in steps:
            step.free()


def test_only_the_general_baseline_kernel_has_no_other_kernel_to_alternate_with():
    """the parametrisation above is computed: pin what it came to.  FORCE_GLOBAL_ATOMICS or FORCE_SCALAR names a different kernel
    for every case but the open-addressing plans that hdk_scan_agg_global runs anyway (both flags name it again): those run X
    then X only, every other case under both splits in all three orders"""
    alone = {cid for cid, flag in OTHER.items() if flag is None}
    assert alone == {cid for cid, c in CASES.items() if c.expected_route == "hdk_scan_agg_global" and c.query.force_baseline}
    assert 0 < len(alone) <= 2 and len(PARAMS) == 6 * (len(CASES) - len(alone)) + 2 * len(alone)
