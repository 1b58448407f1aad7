"""Host-only parts of the device-side columnar results: the workspace arithmetic and the argument checks that come back
before any device is touched."""
import ctypes as C

import numpy as np

from hdk_amd import _abi as A
from hdk_amd._lib import lib
from hdk_amd.ir import Agg, ColRef, KeyRef, QueryUnit
from hdk_amd.plan import compile_query
from hdk_amd.storage import ArrowStorage


def test_workspace_bytes_is_host_arithmetic():
    f = lib().hdk_hip_result_columns_workspace_bytes
    assert f(1) > 0
    sizes = [f(n) for n in (0, 1, 4095, 4096, 4097, 10**6, 200_000_000, 2**31, 2**32 - 1)]
    assert sizes == sorted(sizes)
    assert f(200_000_000) >= 4 * (200_000_000 // 4096)   # one uint32 per tile of a few thousand entries
    assert f(2**32 - 1) <= 8 << 20                       # within a few MB even for the largest table


def _plan():
    st = ArrowStorage()
    st.import_numpy("t", {"k": np.arange(100, dtype=np.int64) % 10, "v": np.arange(100, dtype=np.int64)})
    return compile_query(st, QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0), Agg("sum", ColRef("v"))]))


def test_columnarize_checks_the_plan_before_any_device():
    L = lib()
    rows = C.c_uint64(0)
    iv = np.zeros(4, dtype=np.int64)
    # (the pointers are never dereferenced: the plan check comes first)
    assert L.hdk_hip_columnarize_result(None, 8, 10, iv.ctypes.data, None, 0, C.addressof(rows), None, 0, 0, None) == A.ERR_INVALID_ARG
    cp = _plan()
    bad = type(cp.plan).from_buffer_copy(cp.plan)
    bad.abi_version = 1
    st = L.hdk_hip_columnarize_result(C.byref(bad), 8, 10, iv.ctypes.data, None, 0, C.addressof(rows), None, 0, 0, None)
    assert st == A.ERR_INVALID_ARG and b"ABI" in L.hdk_hip_last_error()


def test_version_says_the_abi_grew():
    assert lib().hdk_hip_version() >= 1001


def test_dense_tail_gives_the_host_reader_rows(oracle):
    """result_set.dense_to_columns over the values the device writes (restated in numpy) equals to_columns on the buffer:
    names, order, None for NULL, AVG, decimal scale -- the host half of DeviceColumns.to_columns()."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from hdk_amd import result_set as rs
    from fuzz_queries import make_tables_wide, random_query_wide
    from hdk_amd.ir import QueryMustRunOnCpu
    from util import run_oracle
    rng = np.random.default_rng(5011)
    st = make_tables_wide(rng, 5000, 300)
    done = 0
    for _ in range(30):
        q = random_query_wide(rng)
        try:
            cp, buf, err = run_oracle(oracle, st, q)
        except QueryMustRunOnCpu:
            continue
        if err or cp.plan.query_kind not in (A.Q_PERFECT_HASH, A.Q_BASELINE_HASH):
            continue
        dense = _device_values(cp, buf)
        assert rs.dense_to_columns(cp, dense) == rs.to_columns(cp, buf), q
        done += 1
    assert done >= 15


def _device_values(cp, buf):
    """The 8-byte value per target and non-empty entry, by the table of include/hdk_hip.h."""
    from hdk_amd import result_set as rs
    p = cp.plan
    n = int(p.entry_count)
    mask = rs.non_empty_mask(cp, buf, n)
    slots, keys = rs._slot_arrays(cp, buf, n), rs._key_arrays(cp, buf, n)
    out, s = [], 0
    for t in range(p.num_targets):
        tg = p.targets[t]
        a = (slots[s] if slots[s] is not None else keys[tg.key_idx])[mask].astype(np.int64)
        lo = (a & 0xFFFFFFFF).astype(np.uint32)
        if tg.agg == A.AGG_AVG:
            cnt = slots[s + 1][mask].astype(np.int64)
            dividend = lo.view(np.float32).astype(np.float64) if tg.arg_is_fp == A.FP_SLOT_FLOAT else \
                a.view(np.float64) if tg.arg_is_fp else a.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                bits = (dividend / cnt.astype(np.float64)).view(np.int64).copy()
            bits[cnt == 0] = A.NULL_DOUBLE_BITS
        elif tg.arg_is_fp == A.FP_SLOT_FLOAT and tg.agg not in (A.AGG_COUNT, A.AGG_ID):
            bits = lo.view(np.float32).astype(np.float64).view(np.int64).copy()
            if tg.skip_null:
                bits[lo == np.uint32(A.NULL_FLOAT_BITS)] = A.NULL_DOUBLE_BITS
        else:
            bits = a
        out.append(bits)
        s += 2 if tg.agg == A.AGG_AVG else 1
    return out
