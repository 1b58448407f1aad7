"""bench.py --dump-outputs, checked without a GPU: the oracle fills the same output buffer the timed path's kernels fill, and
dump_outputs must write what ExecutionResult.to_columns reads from it (float64, NULL as NaN, rows sorted) -- and, above the
size limit, a seeded sample of the rows that does not depend on where an open-addressing table put them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402
from hdk_amd import _abi as A  # noqa: E402
from hdk_amd.executor import ExecutionResult  # noqa: E402
from hdk_amd.ir import Agg, ColRef, KeyRef, QueryUnit  # noqa: E402
from hdk_amd.storage import ArrowStorage  # noqa: E402
from oracle import oracle as O  # noqa: E402
from util import run_oracle  # noqa: E402

Q = QueryUnit("t", groupby=[ColRef("key")], targets=[KeyRef(0, "key"), Agg("sum", ColRef("val"), "s"), Agg("count", None, "n")])


def _result(key_high, seed):
    rng = np.random.default_rng(seed)
    n = 20_000
    key = rng.integers(0, key_high, n, dtype=np.int64)
    val = rng.integers(-2**31, 2**31, n, dtype=np.int64)
    val[key % 7 == 3] = A.NULL_BIGINT  # whole groups of NULLs: SUM is NULL there
    st = ArrowStorage()
    st.import_numpy("t", {"key": key, "val": val}, fragment_size=5_000)
    cp, buf, err = run_oracle(O, st, Q)
    assert err == 0
    return cp, buf


def _sorted_rows(cp, buf):
    cols = ExecutionResult(cp, buf, cp.entry_count).to_columns()
    return sorted(zip(cols["key"], cols["s"], cols["n"]))


def _load(d):
    return [np.load(os.path.join(d, f"{c}.npy")) for c in ("key", "s", "n")]


def _same(got, want_rows):
    want = [np.array([np.nan if v is None else v for v in col], dtype=np.float64) for col in zip(*want_rows)]
    for g, w in zip(got, want):
        assert g.dtype == np.float64 and g.shape == w.shape
        assert np.array_equal(g, w, equal_nan=True)


def test_the_whole_result_sorted_with_nulls_as_nan(tmp_path):
    cp, buf = _result(64, 1)
    assert cp.plan.query_kind == A.Q_PERFECT_HASH
    bench.dump_outputs(str(tmp_path), cp, buf, cp.entry_count)
    got = _load(str(tmp_path))
    _same(got, _sorted_rows(cp, buf))
    assert len(got[0]) == 64 and np.isnan(got[1]).sum() > 0


@pytest.mark.parametrize("key_high", [64, 1 << 40])
def test_a_large_result_is_a_seeded_sample_of_the_sorted_rows(tmp_path, monkeypatch, key_high):
    cp, buf = _result(key_high, 2)
    if key_high > 64:
        assert cp.plan.query_kind == A.Q_BASELINE_HASH  # (thinned out by key before it is decoded)
    rows = _sorted_rows(cp, buf)
    keep = 40 if key_high == 64 else 500
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", keep * 3 * 8)
    bench.dump_outputs(str(tmp_path), cp, buf.copy(), cp.entry_count)
    pick = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(len(rows), keep, replace=False))
    _same(_load(str(tmp_path)), [rows[i] for i in pick])
