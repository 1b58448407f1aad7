"""The expected order of hdk_hip_sort_columns, in code that is not under test.  Not a test file.

An order entry here is a tuple (col, desc, nulls_first, is_fp, nullable, null_bits): the fields of hdk_hip_order_entry.
`cols` is a list of int64 numpy arrays, the 8-byte words of the dense columns (doubles as their bits).
-0.0 and NaN stay out of the generic generators: the documented order differs from operator< there (they have one test
of their own)."""
import functools

import numpy as np

INT64_MAX, INT64_MIN = 2**63 - 1, -(2**63)
NULL_DOUBLE_BITS = 0x0010000000000000


def expected_perm(cols, order):
    """Stable numpy: per order entry, most significant first, a NULL rank (0 / 1 / 2 by nulls_first) and a value (~v for
    descending integers, -v for descending doubles, 0 in place of a NULL), fed to np.lexsort."""
    keys = []
    n = len(cols[0])
    for col, desc, nulls_first, is_fp, nullable, null_bits in reversed(order):
        w = np.ascontiguousarray(cols[col], dtype=np.int64)
        is_null = (w == np.int64(null_bits)) if nullable else np.zeros(n, dtype=bool)
        if is_fp:
            v = w.view(np.float64).copy()
            v[is_null] = 0.0
            v = -v if desc else v
            v[is_null] = 0.0
        else:
            v = w.copy()
            v[is_null] = 0
            v = ~v if desc else v
            v[is_null] = 0
        rank = np.where(is_null, 0 if nulls_first else 2, 1).astype(np.int8)
        keys.append(v)
        keys.append(rank)
    return np.lexsort(keys).astype(np.uint32) if keys else np.arange(n, dtype=np.uint32)


def comparator_perm(cols, order):
    """ResultSetComparator (QueryEngine/ResultSetSort.cpp:329-480) restated, for sorted(..., key=cmp_to_key); ties keep
    the row order (sorted is stable)."""
    rows = [[int(x) for x in np.asarray(c, dtype=np.int64).tolist()] for c in cols]
    fvals = [np.asarray(c, dtype=np.int64).view(np.float64).tolist() for c in cols]

    def less(a, b):
        for col, desc, nulls_first, is_fp, nullable, null_bits in order:
            l, r = rows[col][a], rows[col][b]
            ln, rn = nullable and l == null_bits, nullable and r == null_bits
            if ln and rn:
                continue
            if ln != rn:
                return ln == bool(nulls_first)
            if l == r:
                continue
            if is_fp:
                return (fvals[col][a] < fvals[col][b]) != bool(desc)
            return (l < r) != bool(desc)
        return False

    def cmp(a, b):
        return -1 if less(a, b) else (1 if less(b, a) else 0)

    return np.array(sorted(range(len(rows[0])), key=functools.cmp_to_key(cmp)), dtype=np.uint32)


def out_rows_of(n, limit, offset):
    after = n - offset if n > offset else 0
    return min(limit, after) if limit else after


def dbits(x):
    return int(np.float64(x).view(np.int64))


def random_case(rng, n, num_entries):
    """Three columns (int64 with the extreme values, int64 with heavy ties, double with inf / denormal / DBL_MIN) and
    `num_entries` order entries over them with random directions; DBL_MIN is NULL or a value by the entry's nullable."""
    a = rng.integers(INT64_MIN + 1, INT64_MAX, n, dtype=np.int64, endpoint=True)
    a[rng.random(n) < 0.05] = INT64_MAX
    a[rng.random(n) < 0.05] = INT64_MIN + 1
    a[rng.random(n) < 0.05] = INT64_MIN
    b = rng.integers(-3, 4, n, dtype=np.int64)
    b[rng.random(n) < 0.1] = INT64_MIN
    d = rng.normal(size=n) * 1e3
    d[rng.random(n) < 0.03] = np.inf
    d[rng.random(n) < 0.03] = -np.inf
    d[rng.random(n) < 0.03] = 5e-324
    d[rng.random(n) < 0.05] = 2.2250738585072014e-308
    d[d == 0] = 1.0
    cols = [a, b, d.view(np.int64).copy()]
    nulls = [INT64_MIN, INT64_MIN, NULL_DOUBLE_BITS]
    order = []
    for c in rng.permutation(3)[:num_entries].tolist():
        order.append((c, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), c == 2, bool(rng.random() < 0.8), nulls[c]))
    return cols, order
