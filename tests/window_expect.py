"""What hdk_hip_window_columns must give: a numpy evaluator of its contract (include/hdk_hip.h), written apart from the
kernels and checked against SQLite in test_window_columns_cpu.py.

Columns are arrays of int64 WORDS (a double column is its bit patterns).  A partition is a maximal stretch of adjacent
rows whose words in every partition column are equal, a peer group a maximal stretch inside it whose words in every order
column are equal too.  Every row gives one word per out, in input order.  An out is anything with the fields of
hdk_hip_window_out (the `WOut` below): kind one of KINDS, col (< 0: COUNT(*)), frame "rows" | "range" | "partition",
is_fp, nullable, null_bits, param (NTILE's n, LAG / LEAD's k)."""
from collections import namedtuple

import numpy as np

from group_expect import NULL_F64_BITS, NULL_I64, bits  # noqa: F401  (re-exported for the tests)

WOut = namedtuple("WOut", "kind col frame is_fp nullable null_bits param", defaults=(-1, "rows", False, False, 0, 0))

KINDS = ["row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile", "lag", "lead", "first_value", "last_value",
         "avg", "min", "max", "sum", "count"]  # the order of hdk_hip_window_kind
FRAMES = ["rows", "range", "partition"]  # the order of hdk_hip_window_frame
AGGREGATES = ("avg", "min", "max", "sum", "count")


def _stretches(cols, key_cols, n, head):
    """-> (first row, last row) of every row's stretch; `head` marks rows that begin one whatever the keys say"""
    head = head.copy()
    head[0] = True
    for k in key_cols:
        w = cols[k][:n]
        head[1:] |= w[1:] != w[:-1]
    firsts = np.flatnonzero(head)
    lasts = np.append(firsts[1:] - 1, n - 1)
    sid = np.cumsum(head) - 1
    return firsts[sid], lasts[sid], sid, head


def _running(x, start, red):
    """x[start[r]] red ... red x[r] for an associative `red`: every row's window, clipped at its stretch's first row, is
    doubled (all rows at once) until it covers the longest stretch"""
    y = x.copy()
    r = np.arange(len(x))
    longest = int((r - start).max()) + 1
    d = 1
    while d < longest:
        src = r - d
        ok = src >= start
        y[ok] = red(y[ok], y[src[ok]])
        d *= 2
    return y


def window(cols, n, part_cols, order_cols, outs):
    """-> list of int64 word arrays of n rows, one per out"""
    cols = [np.ascontiguousarray(c).view(np.int64) for c in cols]
    if n == 0:
        return [np.empty(0, dtype=np.int64) for _ in outs]
    start, end, pid, phead = _stretches(cols, part_cols, n, np.zeros(n, dtype=bool))
    pstart, pend, qid, _ = _stretches(cols, order_cols, n, phead)
    r = np.arange(n, dtype=np.int64)
    size = end - start + 1
    res = []
    for o in outs:
        if o.kind == "row_number":
            res.append(r - start + 1)
        elif o.kind == "rank":
            res.append(pstart - start + 1)
        elif o.kind == "dense_rank":
            res.append(qid - qid[start] + 1)
        elif o.kind == "percent_rank":
            rank = pstart - start + 1
            res.append(bits(np.where(size == 1, 0.0, (rank - 1).astype(np.float64) / np.maximum(size - 1, 1).astype(np.float64))))
        elif o.kind == "cume_dist":
            res.append(bits((pend - start + 1).astype(np.float64) / size.astype(np.float64)))
        elif o.kind == "ntile":
            assert o.param >= 1
            per = -(-size // o.param)  # ceil(size / n), the reference's tile size
            res.append((r - start) // per + 1)
        elif o.kind in ("lag", "lead"):
            assert o.param >= 0
            src = r - o.param if o.kind == "lag" else r + o.param
            inside = (src >= start) & (src <= end)
            res.append(np.where(inside, cols[o.col][np.clip(src, 0, n - 1)], np.int64(o.null_bits)))
        elif o.kind == "first_value":
            res.append(cols[o.col][start])
        elif o.kind == "last_value":
            res.append(cols[o.col][{"rows": r, "range": pend, "partition": end}[o.frame]])
        else:
            res.append(_aggregate(cols, n, o, start, {"rows": r, "range": pend, "partition": end}[o.frame]))
    return [np.ascontiguousarray(x).astype(np.int64) for x in res]


def _aggregate(cols, n, o, start, last):
    """the aggregate over rows start[r] .. last[r] of every row r"""
    assert o.kind in AGGREGATES
    if o.kind == "count" and o.col < 0:
        return last - start + 1
    w = cols[o.col][:n]
    valid = w != np.int64(o.null_bits) if o.nullable else np.ones(n, dtype=bool)
    cum = np.concatenate([[0], np.cumsum(valid)]).astype(np.int64)
    cnt = cum[last + 1] - cum[start]
    if o.kind == "count":
        return cnt
    if o.kind in ("sum", "avg"):
        if o.is_fp:
            # (a running sum that never leaves its partition: the difference of two prefix sums would lose a tiny value)
            total = _running(np.where(valid, w.view(np.float64), 0.0), start, np.add)[last]
        else:
            ps = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(np.where(valid, w, 0).astype(np.uint64))])  # wraps
            total = (ps[last + 1] - ps[start]).view(np.int64)
        if o.kind == "avg":
            avg = total.astype(np.float64) / np.maximum(cnt, 1).astype(np.float64)
            return np.where(cnt > 0, bits(avg), np.int64(NULL_F64_BITS))
        val = bits(total) if o.is_fp else total
    else:
        red = np.minimum if o.kind == "min" else np.maximum
        if o.is_fp:
            x = np.where(valid, w.view(np.float64), np.inf if o.kind == "min" else -np.inf)
            val = bits(_running(x, start, red)[last])
        else:
            ident = np.iinfo(np.int64).max if o.kind == "min" else np.iinfo(np.int64).min
            val = _running(np.where(valid, w, ident), start, red)[last]
    return np.where(cnt > 0, val, np.int64(o.null_bits))
