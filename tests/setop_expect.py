"""The contracts of hdk_hip_concat_columns and hdk_hip_setop_columns, in code that is not under test.  Not a test file.

`cols` is a list of int64 numpy arrays, the 8-byte words of dense columns (doubles as their bits).  A pair is the tuple
(lcol, rcol, lnullable, rnullable, lnull_bits, rnull_bits, out_null_bits): the fields of hdk_hip_setop_col."""
import collections

import numpy as np

import sort_expect as S

UNION, INTERSECT, INTERSECT_ALL, EXCEPT, EXCEPT_ALL = range(5)
OPS = {("union", False): UNION, ("intersect", False): INTERSECT, ("intersect", True): INTERSECT_ALL,
       ("except", False): EXCEPT, ("except", True): EXCEPT_ALL}
NULL_I64 = np.int64(-2**63)
NULL_I32 = np.int64(-2**31)
NULL_F64_BITS = np.int64(0x0010000000000000)


def concat(lcols, ln, rcols, rn, pairs, side_col=-1, tag_first=False):
    """hdk_hip_concat_columns -> the output columns (num_cols, or num_cols + 1 with a side column), ln + rn rows each"""
    out = []
    for lc, rc, lnullable, rnullable, lnull, rnull, onull in pairs:
        a = np.asarray(lcols[lc][:ln], dtype=np.int64).copy() if ln else np.empty(0, dtype=np.int64)
        b = np.asarray(rcols[rc][:rn], dtype=np.int64).copy() if rn else np.empty(0, dtype=np.int64)
        if lnullable:
            a[a == np.int64(lnull)] = np.int64(onull)
        if rnullable:
            b[b == np.int64(rnull)] = np.int64(onull)
        out.append(np.concatenate([a, b]))
    if side_col >= 0:
        first, second = (1, 0) if tag_first else (0, 1)
        out.insert(side_col, np.concatenate([np.full(ln, first, dtype=np.int64), np.full(rn, second, dtype=np.int64)]))
    return out


def counters(cols, n, key_cols, tag_col):
    """-> (is_left, rb, lb) per row: rb / lb = the rows with a non-zero / zero tag BEFORE the row in its run of adjacent
    rows that are bit-equal on every key column"""
    tag = np.asarray(cols[tag_col][:n], dtype=np.int64)
    head = np.zeros(n, dtype=bool)  # the first row of a run
    if n:
        head[0] = True
    for k in key_cols:
        w = np.asarray(cols[k][:n], dtype=np.int64)
        head[1:] |= w[1:] != w[:-1]
    right = (tag != 0).astype(np.int64)
    left = (tag == 0).astype(np.int64)
    start = np.maximum.accumulate(np.where(head, np.arange(n), 0)) if n else np.empty(0, dtype=np.int64)
    cr = np.cumsum(right) - right  # exclusive
    cl = np.cumsum(left) - left
    return tag == 0, cr - cr[start], cl - cl[start]


def keep(cols, n, key_cols, tag_col, op):
    """the rows hdk_hip_setop_columns keeps, as a mask"""
    return keep_of(*counters(cols, n, key_cols, tag_col), op)


def keep_of(is_left, rb, lb, op):
    """the table of the header, literally, over what counters() gives"""
    if op == UNION:
        return rb + lb == 0
    if op == INTERSECT:
        return is_left & (lb == 0) & (rb > 0)
    if op == INTERSECT_ALL:
        return is_left & (lb < rb)
    if op == EXCEPT:
        return is_left & (lb == 0) & (rb == 0)
    if op == EXCEPT_ALL:
        return is_left & (lb >= rb)
    raise ValueError(op)


def setop(cols, n, key_cols, tag_col, op, out_idx):
    """hdk_hip_setop_columns -> (the output columns, row_count)"""
    m = keep(cols, n, key_cols, tag_col, op)
    return [np.asarray(cols[t][:n], dtype=np.int64)[m] for t in out_idx], int(m.sum())


def method(lcols, ln, rcols, rn, pairs, fp, op, all=False):
    """The end-to-end meaning of DeviceColumns.union / intersect / except_: -> the output columns.  UNION ALL is the
    concatenation, left first.  Everything else: the right rows in front with tag 1, the stable sort on all columns
    ascending with NULLs last (sort_expect.expected_perm), the keep rule.  `fp[j]`: column j holds doubles."""
    nc = len(pairs)
    if op == "union" and all:
        return concat(lcols, ln, rcols, rn, pairs)
    swapped = [(rc, lc, rnl, lnl, rnull, lnull, onull) for lc, rc, lnl, rnl, lnull, rnull, onull in pairs]
    block = concat(rcols, rn, lcols, ln, swapped, nc, True)
    order = [(j, False, False, bool(fp[j]), bool(pairs[j][2] or pairs[j][3]), int(pairs[j][6])) for j in range(nc)]
    perm = S.expected_perm(block, order)
    block = [c[perm] for c in block]
    return setop(block, ln + rn, list(range(nc)), nc, OPS[(op, bool(all))], list(range(nc)))[0]


def multiset(cols, nulls=None):
    """the rows as a Counter of tuples; nulls[j] (or None): the word of column j that reads as None"""
    n = len(cols[0]) if cols else 0
    lists = []
    for j, c in enumerate(cols):
        vals = [int(x) for x in np.asarray(c, dtype=np.int64).tolist()]
        if nulls is not None and nulls[j] is not None:
            vals = [None if v == int(nulls[j]) else v for v in vals]
        lists.append(vals)
    return collections.Counter(tuple(l[i] for l in lists) for i in range(n))


def counter_setop(left: collections.Counter, right: collections.Counter, op, all):
    """multiset arithmetic: the meaning the keep rule must have"""
    if op == "union":
        return left + right if all else collections.Counter(set(left) | set(right))
    if op == "intersect":
        return left & right if all else collections.Counter(set(left) & set(right))
    return left - right if all else collections.Counter(set(left) - set(right))
