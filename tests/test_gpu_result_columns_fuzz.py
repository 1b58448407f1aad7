"""Differential fuzz of the device-side columnar results: for every grouped plan the seeded generators draw (perfect and
baseline hash, row-wise and columnar, keyless, 4-byte keys, zero-width slots, AVG, float accumulators),
step.fetch_columns() must give the rows step.fetch() gives, and its per-target arrays the host reader's values bit for
bit."""
import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd.ir import QueryMustRunOnCpu

from fuzz_queries import make_tables, make_tables_wide, random_query, random_query_wide
from test_gpu_result_columns import expected_columns
from util import run_oracle

pytestmark = pytest.mark.gpu

_ROWS, _ND, _QUERIES = 20_000, 700, 40


def _features(cp):
    p = cp.plan
    f = {("perfect" if p.query_kind == A.Q_PERFECT_HASH else "baseline") + ("_columnar" if p.output_columnar else "_rowwise")}
    if p.keyless:
        f.add("keyless_columnar" if p.output_columnar else "keyless_rowwise")
    if p.key_width == 4:
        f.add("k4")
    for t in range(p.num_targets):
        tg = p.targets[t]
        if tg.slot_width == 0:
            f.add("w0")
        if tg.agg == A.AGG_AVG:
            f.add("avg")
        if tg.arg_is_fp == A.FP_SLOT_FLOAT:
            f.add("float_slot")
    return f


def _grouped_plans(oracle, seed):
    """(storage, [(query index, query, compiled plan)]) of the grouped plans of a seed that the oracle runs without error."""
    wide = seed >= 5000
    rng = np.random.default_rng(seed)
    st = (make_tables_wide if wide else make_tables)(rng, _ROWS, _ND)
    plans = []
    for i in range(_QUERIES):
        q = (random_query_wide if wide else random_query)(rng)
        try:
            cp, _, err = run_oracle(oracle, st, q)
        except QueryMustRunOnCpu:
            continue
        if err == 0 and cp.plan.query_kind in (A.Q_PERFECT_HASH, A.Q_BASELINE_HASH):
            plans.append((i, q, cp))
    return st, plans


_SEEDS = [1, 2, 3, 5011, 5012]


@pytest.mark.parametrize("seed", _SEEDS)
def test_fetch_columns_equals_fetch(oracle, gpu_executor_factory, seed):
    st, plans = _grouped_plans(oracle, seed)
    ex = gpu_executor_factory(st)
    compared = 0
    for i, q, cp in plans:
        step = ex.prepare(cp)
        try:
            step.enqueue()
            res = step.fetch()
            cols = step.fetch_columns()
            try:
                host = cols.to_host()
                want_rows, want = expected_columns(cp, res.buffer, res.entry_count)
                assert cols.num_rows == want_rows == res.row_count(), (seed, i, q)
                for t, (g, w) in enumerate(zip(host, want)):
                    assert np.array_equal(g.view(np.int64), w), (seed, i, t, q)
                assert cols.to_columns() == res.to_columns(), (seed, i, q)
            finally:
                cols.free()
        finally:
            step.free()
        compared += 1
    assert compared >= 25, compared


def test_the_seeds_cover_every_layout(oracle):
    """The plans compared above (the same generator, on the host alone) include every form the call accepts."""
    seen = set()
    for seed in _SEEDS:
        for _, _, cp in _grouped_plans(oracle, seed)[1]:
            seen |= _features(cp)
    want = {"perfect_rowwise", "perfect_columnar", "baseline_rowwise", "baseline_columnar", "keyless_rowwise",
            "keyless_columnar", "k4", "w0", "avg", "float_slot"}
    assert want <= seen, sorted(want - seen)
