"""What hdk_hip_group_columns must give: a numpy evaluator of its contract (include/hdk_hip.h), written apart from the
kernels and checked against SQLite in test_group_columns_cpu.py.

Columns are arrays of int64 WORDS (a double column is its bit patterns).  A run is a maximal stretch of adjacent rows whose
words in every key column are equal; each run gives one output row, in input order.  An out is anything with the fields
of hdk_hip_group_out (the `Out` below): kind "id" | "count" | "sum" | "min" | "max", col (< 0: COUNT(*)), is_fp, nullable,
null_bits."""
from collections import namedtuple

import numpy as np

Out = namedtuple("Out", "kind col is_fp nullable null_bits", defaults=(False, False, 0))

NULL_I64 = -(1 << 63)
NULL_F64_BITS = int(np.array([np.finfo(np.float64).tiny]).view(np.int64)[0])  # DBL_MIN, the in-band NULL of a double


def bits(x):
    """doubles -> their int64 words"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def run_starts(cols, key_cols, n):
    """first row of every run, ascending"""
    if n == 0:
        return np.empty(0, dtype=np.int64)
    head = np.zeros(n, dtype=bool)
    head[0] = True
    for k in key_cols:
        w = np.asarray(cols[k][:n]).view(np.int64)
        head[1:] |= w[1:] != w[:-1]
    return np.flatnonzero(head)


def group(cols, n, key_cols, outs):
    """-> (list of int64 word arrays, one per out; number of runs)"""
    cols = [np.ascontiguousarray(c).view(np.int64) for c in cols]
    starts = run_starts(cols, key_cols, n)
    runs = len(starts)
    ends = np.append(starts[1:], n) if runs else starts
    res = []
    for o in outs:
        if o.kind == "count" and o.col < 0:
            res.append((ends - starts).astype(np.int64))
            continue
        w = cols[o.col][:n]
        if o.kind == "id":
            assert o.col in key_cols
            res.append(w[starts].copy())
            continue
        valid = w != np.int64(o.null_bits) if o.nullable else np.ones(n, dtype=bool)
        # (the non-NULL words of a run, counted through a prefix sum: reduceat misreads empty stretches)
        cum = np.concatenate([[0], np.cumsum(valid)])
        cnt = (cum[ends] - cum[starts]).astype(np.int64)
        if o.kind == "count":
            res.append(cnt)
            continue
        out = np.full(runs, np.int64(o.null_bits), dtype=np.int64)
        if runs:
            if o.kind == "sum":
                if o.is_fp:
                    x = np.where(valid, w.view(np.float64), 0.0)
                    r = np.add.reduceat(x, starts)
                    val = r.view(np.int64)
                else:
                    x = np.where(valid, w, 0).astype(np.uint64)  # wraps
                    val = np.add.reduceat(x, starts).astype(np.uint64).view(np.int64)
            else:
                red = np.minimum if o.kind == "min" else np.maximum
                if o.is_fp:
                    x = np.where(valid, w.view(np.float64), np.inf if o.kind == "min" else -np.inf)
                    val = red.reduceat(x, starts).view(np.int64)
                else:
                    ident = np.iinfo(np.int64).max if o.kind == "min" else np.iinfo(np.int64).min
                    val = red.reduceat(np.where(valid, w, ident), starts)
            out = np.where(cnt > 0, val, out)
        res.append(out.astype(np.int64))
    return res, runs
