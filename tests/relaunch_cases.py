"""Cases for launching into a buffer that already holds groups (tests/test_relaunch_cases_cpu.py, tests/test_gpu_relaunch.py).

`hdk_hip_launch` merges into what the output buffer holds (include/hdk_hip.h).  Every aggregate route of the routing corpus
(tests/golden/routing_corpus.json) gets a case here: a plan shape the suite already has, real data behind it, the launch variant
that reaches the route and the route `hdk_hip_describe_launch` names for it.  A case is
(id, storage, QueryUnit, variant, expected_route); `variant` is spelled like routing_corpus.VARIANTS, several parts joined by "+",
a valued switch as NAME=value.

Data (the same rules for every case): FRAG_ROWS outer rows in eight fragments of unequal sizes, launched as two halves
(SPLITS).  A key of a domain has an index j; j % 8 decides where the group lives and what its arguments look like:
  0  rows in fragments 0 and 2 only  -> the group is in half A only, under either split
  1  rows in fragments 5 and 7 only  -> in half B only
  2  everywhere; nullable arguments NULL except in fragments 5 and 7  -> NULL in every A row, a value in B
  3  everywhere; nullable arguments NULL except in fragments 0 and 2  -> a value in A, NULL in every B row
  4  everywhere; nullable arguments NULL in every row
  5, 6, 7  everywhere; arguments NULL in 5 % of the rows
Argument values grow with the fragment: the lower third of the range in fragments 0 and 2, the upper third in 5 and 7, the middle
elsewhere, so a shared group has its minimum in A and its maximum in B.  Which keys a fragment favours drifts with the row index.
A NULL key is present wherever the key column can hold one (NO_NULL_KEY lists the rest).  Floating-point arguments are multiples of 1/8 small enough that every sum (of doubles and of float accumulators) is exact in
any order: the GPU test compares bit for bit."""
import collections
import functools
import zlib

import numpy as np

from hdk_amd import _abi as A
from hdk_amd.ir import Agg, Cmp, ColRef, FP64, JoinSpec, KeyRef, Lit, QueryUnit, Type
from hdk_amd.plan import compile_query
from hdk_amd.storage import ArrowStorage, Column, Table, _stats

import join_variants_cases
import joins_cases
import routing_corpus as RC
import syn_queries as SQ
import test_kernel_routing_cpu as R

FRAG_ROWS = (13001, 17013, 14899, 16217, 13513, 16791, 14131, 14441)
N = sum(FRAG_ROWS)
SPLITS = {"interleaved": ([0, 2, 4, 6], [1, 3, 5, 7]), "contiguous": ([0, 1, 2, 3], [4, 5, 6, 7])}
ONLY_A, ONLY_B = (0, 2), (5, 7)  # fragments that are in half A (in half B) under either split
FRAG_OF_ROW = np.repeat(np.arange(len(FRAG_ROWS)), FRAG_ROWS)
_IN_A, _IN_B = np.isin(FRAG_OF_ROW, ONLY_A), np.isin(FRAG_OF_ROW, ONLY_B)

Case = collections.namedtuple("Case", "id storage query variant expected_route")

# routes of the corpus without a case: {route: what was tried}
EXCLUDED = {}

# what hdk_hip_describe_launch answers for each half of a case under its variant (test_relaunch_cases_cpu.py holds the library to it)
EXPECTED_ROUTE = {
    "r0": "hdk_scan_agg_direct,hdk_finalize",
    "r0_columnar": "hdk_scan_agg_direct,hdk_finalize",
    "r1": "hdk_scan_agg_direct,hdk_finalize",
    "r5": "hdk_scan_agg_keys,hdk_finalize",
    "r5_global": "hdk_scan_agg_global",
    "r6": "hdk_scan_agg_vec,hdk_finalize",
    "r7": "hdk_scan_agg_keys_values,hdk_finalize",
    "r7_scalar": "hdk_scan_agg_generic,hdk_finalize",
    "r8": "hdk_scan_agg_vec,hdk_finalize",
    "mixed_int": "hdk_scan_agg_vec,hdk_finalize",
    "mixed_fp": "hdk_scan_agg_vec,hdk_finalize",
    "mixed_fp2": "hdk_scan_agg_vec,hdk_finalize",
    "mixed_fp2_global": "hdk_scan_agg_global",
    "mixed_int_columnar": "hdk_scan_agg_vec,hdk_finalize",
    "mixed_fp_columnar": "hdk_scan_agg_vec,hdk_finalize",
    "narrow_minmax": "hdk_scan_agg_vec,hdk_finalize",
    "narrow_minmax_scalar": "hdk_scan_agg_generic,hdk_finalize",
    "mixed_nongrouped": "hdk_scan_agg_vec,hdk_finalize",
    "r22": "hdk_scan_agg_baseline_direct",
    "r22_partitioned": "hdk_part_scatter,hdk_part_scatter,hdk_part_aggregate,hdk_part_overflow,hdk_scan_agg_baseline_direct",
    "r22_columnar": "hdk_scan_agg_global",
    "two_keys": "hdk_scan_agg_global",
    "two_keys_int": "hdk_scan_agg_baseline_direct",
    "two_keys_partitioned": "hdk_part_scatter,hdk_part_scatter,hdk_part_aggregate,hdk_part_overflow,hdk_scan_agg_baseline_direct",
    "r20_bh_partitions": "hdk_bh_scatter,hdk_bh_aggregate",
    "r12": "hdk_scan_agg_bh_dense_plain,hdk_bh_fold_slabs",
    "r12_no_plain": "hdk_scan_agg_bh_dense,hdk_bh_fold_slabs",
    "r13_no_dense": "hdk_scan_agg_bh_packed_plain,hdk_bh_fold_slabs",
    "r16": "hdk_scan_agg_bh_dense,hdk_bh_fold_slabs",
    "r16_no_dense": "hdk_scan_agg_bh_packed,hdk_bh_fold_slabs",
    "r17": "hdk_scan_agg_bh_direct",
    "r17_no_direct": "hdk_scan_agg_bh_vec",
    "r12_packed": "hdk_scan_agg_bh_packed,hdk_bh_fold_slabs",
    "r10k_bhm_partitions": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "bh_sparse_dense_partitions": "hdk_bh_dscatter,hdk_bh_daggregate",
    "phs_x1k": "hdk_scan_agg_bh_dense_plain,hdk_bh_fold_slabs",
    "phs_x1k_columnar": "hdk_scan_agg_bh_dense_plain,hdk_bh_fold_slabs",
    "msbs1": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "msbs1_double_key": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "msbs2_partitions": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "msphs1": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize",
    "msphs1_columnar": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize",
    "msphs1_int64": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize",
    "msphs2_partitions": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_finalize",
    "phm1": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize",
    "phm3_bhm_partitions": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_finalize",
    "phm3_perfect_partitions": "hdk_pp_scatter,hdk_pp_scatter2,hdk_pp_aggregate,hdk_scan_agg_global",
    "nga1": "hdk_scan_agg_cols,hdk_finalize",
    "nga3": "hdk_scan_agg_cols,hdk_finalize",
    "nga4": "hdk_scan_agg_cols,hdk_finalize",
    "nga5": "hdk_scan_agg_cols,hdk_finalize",
    "nga5_no_cols": "hdk_scan_agg_vec,hdk_finalize",
    "c3": "hdk_join_agg_direct,hdk_finalize",
    "c3_cluster": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced,hdk_join_agg_direct,hdk_finalize",
    "c3w_cluster": "hdk_cluster_by_key,hdk_join_agg_direct,hdk_finalize",
    "c3m": "hdk_join_agg_direct,hdk_finalize",
    "c3d_cluster": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "c3m_two_levels": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_scatter_level2,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "c3g": "hdk_scan_agg_vec_join,hdk_finalize",
    "c3g_cluster": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "c3g_two_levels": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_scatter_level2,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "c3gm": "hdk_scan_agg_bh_vec_join",
    "c3gm_cluster": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_bh_vec_join,hdk_bh_fold_dense",
    "c3gm_two_levels": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_scatter_level2,hdk_join_agg_sliced2,hdk_scan_agg_bh_vec_join,hdk_bh_fold_dense",
    "c3f_cluster": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "c3x_cluster": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "j_otm_group_filter": "hdk_scan_agg_vec_many,hdk_finalize",
    "j_left_group": "hdk_scan_agg_vec_many,hdk_finalize",
    "j_keyed_composite": "hdk_scan_agg_vec_keyed,hdk_finalize",
    "j_keyed_wide": "hdk_scan_agg_vec_keyed,hdk_finalize",
    "jv_semi_dups_cluster": "hdk_cluster_by_key,hdk_cluster_params,hdk_scan_agg_vec_join,hdk_finalize",
    "jv_anti_dups": "hdk_scan_agg_vec_join,hdk_finalize",
}


# ---- data ---------------------------------------------------------------------------------------------------------------------
def add_table(st, name, columns, frag_rows=None, types=None):
    """ArrowStorage.import_numpy with fragments of the given (unequal) sizes"""
    n = len(next(iter(columns.values())))
    frag_rows = [int(r) for r in (frag_rows or [n])]
    bounds = np.concatenate([[0], np.cumsum(frag_rows)])
    cols = []
    for cname, arr in columns.items():
        t = (types or {}).get(cname) or (Type("fp", arr.dtype.itemsize) if arr.dtype.kind == "f" else Type("int", arr.dtype.itemsize))
        frags = [np.ascontiguousarray(arr[b:e]) for b, e in zip(bounds[:-1], bounds[1:])]
        cols.append(Column(cname, t, frags, [_stats(x, t) for x in frags]))
    return st.add_table(Table(name, cols, frag_rows))


def key_indices(rng, g):
    """One key index in [0, g) per outer row: half of a fragment's rows come from a window of the domain that moves with the
    row index, the rest from the whole domain; indices of class 0 / 1 outside their fragments move to a class that lives
    everywhere.  Index 0 and index g - 1 are present (the column's statistics span the domain)."""
    assert g >= 8
    pos = np.arange(N) * g // N
    j = np.where(rng.random(N) < 0.5, (pos + rng.integers(0, max(g // 4, 1), N)) % g, rng.integers(0, g, N))
    cls = j % 8
    stray = ((cls == 0) & ~_IN_A) | ((cls == 1) & ~_IN_B)
    moved = j - cls + 2 + rng.integers(0, 6, N)
    j = np.where(stray, np.where(moved < g, moved, 2 + rng.integers(0, 6, N)), j)
    j[0] = 0
    top = g - 1
    j[np.flatnonzero(_IN_B if top % 8 == 1 else _IN_A)[1]] = top
    return j


def null_mask(rng, j, rate=0.05):
    """which rows' nullable arguments are NULL, from the key index (see the module's docstring)"""
    cls = j % 8
    return ((cls == 2) & ~_IN_B) | ((cls == 3) & ~_IN_A) | (cls == 4) | ((cls >= 5) & (rng.random(len(j)) < rate))


def values(rng, lo, hi, dtype, nulls=None, eighths=False):
    """integers of [lo, hi] that grow with the fragment (lower third in fragments 0 and 2, upper third in 5 and 7); with
    `eighths` the column is floating point and holds value / 8; `nulls` rows get the type's NULL"""
    span = hi - lo + 1
    a, b = lo + span // 3, lo + 2 * span // 3
    v = np.where(_IN_A, rng.integers(lo, max(a, lo + 1), N), np.where(_IN_B, rng.integers(b, hi + 1, N), rng.integers(a, max(b, a + 1), N)))
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        out = (v / 8.0 if eighths else v.astype(np.float64)).astype(dtype)
        if nulls is not None:
            bits = out.view(np.int64 if dtype.itemsize == 8 else np.int32)
            bits[nulls] = A.NULL_DOUBLE_BITS if dtype.itemsize == 8 else A.NULL_FLOAT_BITS
        return out
    out = v.astype(dtype)
    if nulls is not None:
        out[nulls] = np.iinfo(dtype).min
    return out


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def syn_storage(keycol, int64=False, second_key=None):
    """The synthetic benchmark table (syn_queries.SYN_COLUMNS: INT columns uniform in [1, N]) grouped by `keycol`: the key
    column drifts, every other column is an argument with the NULL pattern of the row's key.  A double column d and a float
    column f (multiples of 1/8) ride along.  NULL keys in 1 % of the rows of every fragment.  `second_key` names a column that a
    plan groups by as well: it is uniform in every fragment and its NULLs (5 %) do not follow the first key's classes."""
    rng = _rng(f"syn {keycol} {int64} {second_key}")
    dt = np.int64 if int64 else np.int32
    j = key_indices(rng, SQ.SYN_COLUMNS[keycol])
    nulls = null_mask(rng, j)
    key = (j + 1).astype(dt)
    key[rng.random(N) < 0.01] = np.iinfo(dt).min
    cols = {keycol: key}
    for c in ("x10", "y10", "z10", "x100", "y100", "z100"):
        if c != keycol:
            cols[c] = values(rng, 1, SQ.SYN_COLUMNS[c], dt, nulls)
            if c == second_key:  # a key: uniform over its domain in every fragment
                cols[c] = np.where(rng.random(N) < 0.05, np.iinfo(dt).min, rng.integers(1, SQ.SYN_COLUMNS[c] + 1, N)).astype(dt)
    cols["d"] = values(rng, -400, 400, np.float64, nulls, eighths=True)
    cols["f"] = values(rng, -40, 40, np.float32, nulls, eighths=True)
    st = ArrowStorage()
    add_table(st, "syn", cols, FRAG_ROWS)
    return st


@functools.lru_cache(maxsize=None)
def sparse_storage():
    """syn(x100k, y10) with 4 000 keys spread over [1, 100 000]: the key range is far wider than a table sized for the groups"""
    rng = _rng("sparse")
    j = key_indices(rng, 4000)
    st = ArrowStorage()
    key = (j * 25 + 1).astype(np.int32)
    key[rng.random(N) < 0.01] = A.NULL_INT
    add_table(st, "syn", {"x100k": key, "y10": values(rng, 1, 10, np.int32, null_mask(rng, j))}, FRAG_ROWS)
    return st


@functools.lru_cache(maxsize=None)
def t_storage(by):
    """routing_corpus._routing_test_plans' t(key, val, c, k2, wide) and syn(sparse, y10), with a float column f and a second key
    wk2 and a SMALLINT and a TINYINT argument (s16, b8) beside them.  `key` has 64 values, `wide` and `sparse` 4 000, each with 1 % NULL keys (a baseline table that the placement check walks
    quickly); `by` ("key" or "wide") names the column whose classes the arguments follow."""
    rng = _rng(f"t {by}")
    j, jw = key_indices(rng, 64), key_indices(rng, 4000)
    nulls = null_mask(rng, j if by == "key" else jw)
    key = j.astype(np.int64)
    key[rng.random(N) < 0.01] = A.NULL_BIGINT
    wide, sparse = (jw * 274_877_906 + 5).astype(np.int64), ((jw * 22 + 3) * 7919).astype(np.int32)
    null_wide = rng.random(N) < 0.01
    wide[null_wide], sparse[null_wide] = A.NULL_BIGINT, A.NULL_INT
    st = ArrowStorage()
    add_table(st, "t", {"key": key, "val": values(rng, -2**31 + 1, 2**31 - 1, np.int64, nulls), "c": values(rng, -50, 49, np.int32, nulls),
                        "k2": (np.arange(N) * 7 // N + rng.integers(0, 2, N)).clip(0, 6).astype(np.int16),
                        "wide": wide, "f": values(rng, -40, 40, np.float32, nulls, eighths=True),
                        "d": values(rng, -400, 400, np.float64, nulls, eighths=True), "wk2": (jw % 5 - 2).astype(np.int32),
                        "s16": values(rng, -3000, 2999, np.int16, nulls), "b8": values(rng, -100, 99, np.int8, nulls)}, FRAG_ROWS)
    add_table(st, "syn", {"sparse": sparse, "y10": values(rng, 1, 10, np.int32, nulls)}, FRAG_ROWS)
    return st


@functools.lru_cache(maxsize=None)
def nga_storage():
    """The synthetic table for the non-grouped plans (one group: the NULL patterns go by COLUMN): x10 and dA are NULL outside
    fragments 5 and 7 (NULL in every A row, a value in B), y10 and dB outside 0 and 2 (the other way round), z10 everywhere; x100, y100,
    z100, d and f in 5 % of the rows."""
    rng = _rng("nga")
    some = lambda: rng.random(N) < 0.05  # noqa: E731
    st = ArrowStorage()
    add_table(st, "syn", {"x10": values(rng, 1, 10, np.int32, ~_IN_B), "y10": values(rng, 1, 10, np.int32, ~_IN_A),
                          "z10": values(rng, 1, 10, np.int32, np.ones(N, dtype=bool)), "x100": values(rng, 1, 100, np.int32, some()),
                          "y100": values(rng, 1, 100, np.int32, some()), "z100": values(rng, 1, 100, np.int32, some()),
                          "d": values(rng, -400, 400, np.float64, some(), eighths=True), "dA": values(rng, -400, 400, np.float64, ~_IN_B, eighths=True),
                          "dB": values(rng, -400, 400, np.float64, ~_IN_A, eighths=True),
                          "f": values(rng, -40, 40, np.float32, some(), eighths=True)}, FRAG_ROWS)
    return st


@functools.lru_cache(maxsize=None)
def joins_storage():
    """joins_cases' schema -- fact(fk, fa, fb, fwide, val) with dim(k, a, b, v, w, wide) -- for its grouped shapes: dim has three
    rows per key k (one-to-many) that share w, and (a, b) and wide are unique (keyed tables).  The plans group by dim.w (8 values):
    a fact row draws its class, then a key (and, independently, a composite key and a wide key) whose dimension rows have that w."""
    rng = _rng("joins")
    nd = 288
    r = np.arange(nd)
    w = (r // 3) % 8
    wide = (rng.permutation(nd).astype(np.int64) - nd // 2) * 30_000_000_000
    j = key_indices(rng, 8)
    pick = lambda: 3 * (j + 8 * rng.integers(0, 12, N)) + rng.integers(0, 3, N)  # noqa: E731  (a dimension row with w == j)
    r1, r2, r3 = pick(), pick(), pick()
    miss = rng.random(N)
    fk = np.where(miss < 0.03, A.NULL_BIGINT, np.where(miss < 0.06, 99, 100 + r1 // 3)).astype(np.int64)
    st = ArrowStorage()
    add_table(st, "dim", {"k": (100 + r // 3).astype(np.int64), "a": (r % 40).astype(np.int32), "b": (r // 40).astype(np.int32),
                          "v": rng.integers(-500, 500, nd).astype(np.int64), "w": w.astype(np.int16), "wide": wide}, [97, 97, 94])
    add_table(st, "fact", {"fk": fk, "fa": (r2 % 40).astype(np.int32), "fb": np.where(miss > 0.97, 8, r2 // 40).astype(np.int32),
                           "fwide": np.where(miss > 0.97, 7, wide[r3]).astype(np.int64),
                           "val": values(rng, -100, 99, np.int64, null_mask(rng, j))}, FRAG_ROWS)
    return st


@functools.lru_cache(maxsize=None)
def semi_storage():
    """join_variants_cases' fact(k, b, val) and dk(kd) for its semi join on a column with duplicates: every second key has
    partners (two or three of them); val's NULLs follow the classes of b, the key its anti-join shape groups by"""
    rng = _rng("semi")
    st = ArrowStorage()
    add_table(st, "dk", {"kd": np.repeat(np.arange(0, 4000, 2), 2 + np.arange(2000) % 2).astype(np.int64)}, [2503, 2497])
    k = rng.integers(-5, 4010, N).astype(np.int64)
    k[rng.random(N) < 0.03] = A.NULL_BIGINT
    jb = key_indices(rng, 8)
    b = jb.astype(np.int32)
    b[rng.random(N) < 0.01] = A.NULL_INT
    add_table(st, "fact", {"k": k, "b": b, "val": values(rng, -1000, 999, np.int64, null_mask(rng, jb))}, FRAG_ROWS)
    return st


@functools.lru_cache(maxsize=None)
def star_storage(group, nd=30_000):
    """fact(fk, val, g, g32) JOIN dim(key, dval, attr, dbig), the star shapes of routing_corpus._star_plans over a REAL dimension
    of `nd` unique keys.  `group` says which expression the plan groups by: the fact rows' key indices are drawn over ITS values
    and each row then picks a dimension row that has the value ("dval/15625", "dval%64", "attr": dimension side; "g32": fact side;
    "none": not grouped, and val is NULL outside fragments 5 and 7: the slots of SUM(val ...) / MIN(val) still hold their NULL after half A).
    3 % of the foreign keys are NULL, 3 % have no partner; 5 % of dval and dbig are NULL."""
    rng = _rng(f"star {group} {nd}")
    dkey = rng.permutation(nd).astype(np.int64)
    dval = rng.integers(0, 10**6, nd).astype(np.int64)
    attr = rng.integers(0, 64, nd).astype(np.int64)
    dbig = rng.integers(0, 2**40, nd).astype(np.int64)
    of_dim = {"dval/15625": dval // 15625, "dval%64": dval % 64, "attr": attr}.get(group)
    j = key_indices(rng, 64)
    if of_dim is not None:  # the fact row's group is its dimension row's
        order = np.argsort(of_dim, kind="stable")
        starts = np.searchsorted(of_dim[order], np.arange(64))
        counts = np.searchsorted(of_dim[order], np.arange(64), side="right") - starts
        assert counts.min() > 0
        fk = dkey[order[starts[j] + (rng.random(N) * counts[j]).astype(np.int64)]]
    else:
        fk = dkey[rng.integers(0, nd, N)]
    nulls = null_mask(rng, j) if group != "none" else ~_IN_B  # (not grouped: val is NULL in every A row, a value in B)
    dval[rng.random(nd) < 0.05] = A.NULL_BIGINT  # (after the groups were read: a NULL dval is a NULL group of few rows)
    dbig[rng.random(nd) < 0.05] = A.NULL_BIGINT
    miss = rng.random(N)
    fk = np.where(miss < 0.03, A.NULL_BIGINT, np.where(miss < 0.06, nd + 7, fk)).astype(np.int64)
    g = j.astype(np.int64)
    g[rng.random(N) < 0.01] = A.NULL_BIGINT  # (a NULL group key for the shape that groups by the fact column)
    st = ArrowStorage()
    add_table(st, "dim", {"key": dkey, "dval": dval, "attr": attr, "dbig": dbig})
    add_table(st, "fact", {"fk": fk, "val": values(rng, -2**31 + 1, 2**31 - 1, np.int64, nulls), "g": g, "g32": np.where(g == A.NULL_BIGINT, A.NULL_INT, g).astype(np.int32)}, FRAG_ROWS)
    return st


# ---- variants -----------------------------------------------------------------------------------------------------------------
def variant_flags(variant):
    return sum(RC.FLAGS[p] for p in variant.split("+") if p in RC.FLAGS)


def variant_switches(variant):
    """{HDK_HIP_* name: value} of a variant"""
    out = {}
    for p in variant.split("+"):
        if p != "none" and p not in RC.FLAGS:
            name, _, value = p.partition("=")
            assert name in RC.SWITCHES, p
            out["HDK_HIP_" + name] = value or "1"
    return out


def launch_plan(cp, flags, total_rows):
    """The plan as PreparedStep launches it for a step of `total_rows` rows (hdk_amd/executor.py, PreparedStep.__init__: `fuse`):
    a one-to-one join table takes its fused form when neither FORCE_SCALAR nor FORCE_GLOBAL_ATOMICS is set and the plan with
    the plain table would run one of the batched join kernels listed there.  (A copy of that rule for a box without a device;
    tests/test_gpu_relaunch.py asserts the executor's own answer, kernel_names(), against the same expected route.)"""
    if not cp.inner_tables or flags & (A.LAUNCH_FORCE_SCALAR | A.LAUNCH_FORCE_GLOBAL_ATOMICS):
        return cp
    batched = {"hdk_scan_agg_vec_join", "hdk_scan_project_join", "hdk_scan_agg_vec_keyed", "hdk_scan_project_keyed", "hdk_scan_agg_bh_vec_join"}
    plain = RC.describe(cp, total_rows, flags).split(",")
    if batched & set(plain) and len(cp.join_infos) == 1 and cp.join_infos[0]["kind"] == A.JOIN_ONE_TO_ONE:
        return R._fused(cp)
    return cp


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _star_queries():
    """routing_corpus._star_plans' shapes (that function hands out launch plans, not queries)"""
    j = [JoinSpec("dim", ColRef("fk"), "key")]
    V, D, At = ColRef("val"), ColRef("dval", "dim"), ColRef("attr", "dim")
    lt = [Cmp(D, "<", Lit(500_000))]
    return {"c3": ("none", QueryUnit("fact", joins=j, targets=[Agg("sum", V + D)])),
            "c3g": ("dval/15625", QueryUnit("fact", joins=j, groupby=[D / 15625], targets=[KeyRef(0), Agg("sum", V)])),
            "c3m": ("none", QueryUnit("fact", joins=j, targets=[Agg("sum", V), Agg("count", None), Agg("max", D)])),
            "c3gm": ("dval%64", QueryUnit("fact", joins=j, groupby=[D % 64], targets=[KeyRef(0), Agg("sum", V)])),
            "c3f": ("attr", QueryUnit("fact", joins=j, quals=lt, groupby=[At], targets=[KeyRef(0), Agg("sum", V), Agg("count", None)])),
            "c3x": ("g32", QueryUnit("fact", joins=j, quals=lt, groupby=[ColRef("g32")], targets=[KeyRef(0), Agg("sum", V)])),
            "c3d": ("none", QueryUnit("fact", joins=j, targets=[Agg("sum", D), Agg("min", V)])),
            "c3w": ("none", QueryUnit("fact", joins=j, targets=[Agg("sum", V + ColRef("dbig", "dim"))]))}


def _mixed_targets(kind, key_refs=1):
    """every aggregate over int32 / int64 arguments ("int"), over double / float arguments ("fp" and "fp2"), of one int64 column ("val"), or some of each ("both"):
    a plan holds eight targets at the most"""
    c, val, d, f = ColRef("c"), ColRef("val"), ColRef("d"), ColRef("f")
    aggs = {"int": [Agg("count", None), Agg("count", c), Agg("sum", c), Agg("min", c), Agg("max", val), Agg("avg", val)],
            "fp": [Agg("sum", d), Agg("min", d), Agg("avg", d), Agg("sum", f), Agg("max", f), Agg("avg", f)],
            "fp2": [Agg("count", d), Agg("max", d), Agg("count", f), Agg("min", f), Agg("sum", f), Agg("avg", d)],
            "val": [Agg("count", None), Agg("count", val), Agg("sum", val), Agg("min", val), Agg("max", val), Agg("avg", val)],
            "both": [Agg("count", None), Agg("sum", val), Agg("min", c), Agg("max", f), Agg("avg", d), Agg("sum", f)]}[kind]
    return [KeyRef(i) for i in range(key_refs)] + aggs


TWO_LEVELS = "cluster+SLICE_TWO_LEVELS+SLICE_FINE_KEYS=128"  # test_gpu_cluster.py::test_sliced2_two_scatter_levels' way to the second scatter level


@functools.lru_cache(maxsize=None)
def cases():
    """[Case]: the same list on every call"""
    import dataclasses
    rq = {pid: cp.query for pid, cp in RC._routing_test_plans()}
    jq = {c[0]: c[1] for c in joins_cases.make_case()[2]}
    vq = {c[0]: c[1] for c in join_variants_cases.make_variants()[2]}
    star = _star_queries()
    col = lambda q: dataclasses.replace(q, output_columnar=True)  # noqa: E731
    tk, tw = t_storage("key"), t_storage("wide")
    phs = lambda x: QueryUnit("syn", groupby=[ColRef(x)], targets=[KeyRef(0, "k")] + [  # noqa: E731  (test_gpu_bh_lds.py: _phs_query)
        Agg(k, ColRef("y10")) for k in ("count", "sum", "max", "min", "avg")])
    two_keys = lambda kind: QueryUnit("t", groupby=[ColRef("wide"), ColRef("wk2")], force_baseline=True, baseline_entry_count=16_384,  # noqa: E731
                                      targets=_mixed_targets(kind, 2))
    narrow = QueryUnit("t", groupby=[ColRef("key")], output_columnar=True, targets=[
        KeyRef(0), Agg("min", ColRef("s16")), Agg("max", ColRef("s16")), Agg("min", ColRef("b8")), Agg("max", ColRef("b8")), Agg("count", None),
        Agg("sum", ColRef("c"))])
    out = [
        # the headline's direct kernel and its neighbours on the 64-key table (routing_corpus r*)
        ("r0", tk, rq["r0"], "none"), ("r0_columnar", tk, col(rq["r0"]), "none"), ("r1", tk, rq["r1"], "none"),
        ("r5", tk, rq["r5"], "none"), ("r5_global", tk, rq["r5"], "global"),
        ("r6", tk, rq["r6"], "none"), ("r7", tk, rq["r7"], "none"), ("r7_scalar", tk, rq["r7"], "scalar"), ("r8", tk, rq["r8"], "none"),
        ("mixed_int", tk, QueryUnit("t", groupby=[ColRef("key")], targets=_mixed_targets("int")), "none"),
        ("mixed_fp", tk, QueryUnit("t", groupby=[ColRef("key")], targets=_mixed_targets("fp")), "none"),
        ("mixed_fp2", tk, QueryUnit("t", groupby=[ColRef("key")], targets=_mixed_targets("fp2")), "none"),
        ("mixed_fp2_global", tk, QueryUnit("t", groupby=[ColRef("key")], targets=_mixed_targets("fp2")), "global"),
        ("mixed_int_columnar", tk, QueryUnit("t", groupby=[ColRef("key")], targets=_mixed_targets("int"), output_columnar=True), "none"),
        ("mixed_fp_columnar", tk, QueryUnit("t", groupby=[ColRef("key")], targets=_mixed_targets("fp"), output_columnar=True), "none"),
        ("narrow_minmax", tk, narrow, "none"), ("narrow_minmax_scalar", tk, narrow, "scalar"),
        ("mixed_nongrouped", nga_storage(), QueryUnit("syn", targets=[Agg("sum", ColRef("d")), Agg("min", ColRef("d")), Agg("max", ColRef("f")), Agg("avg", ColRef("f")),
                                                                        Agg("sum", ColRef("dA")), Agg("max", ColRef("dB")), Agg("min", ColRef("z10"))]), "none"),
        # baseline hash: one and two keys, row-wise and columnar, one-pass and radix-partitioned
        ("r22", tw, rq["r22"], "none"), ("r22_partitioned", tw, rq["r22"], "partitioned"), ("r22_columnar", tw, col(rq["r22"]), "none"),
        ("two_keys", tw, two_keys("both"), "none"), ("two_keys_int", tw, two_keys("int"), "none"),
        ("two_keys_partitioned", tw, two_keys("val"), "partitioned"),
        ("r20_bh_partitions", tw, rq["r20"], "BH_PARTITIONS_ALWAYS"),
        # the open-addressing LDS kernels (bh / msbs) and the perfect-hash plans on the same kernels (msphs / phm / phs)
        ("r12", syn_storage("x10"), rq["r12"], "none"), ("r12_no_plain", syn_storage("x10"), rq["r12"], "NO_BH_PLAIN"),
        ("r13_no_dense", syn_storage("x1k"), rq["r13"], "NO_BH_DENSE"), ("r16", syn_storage("x10"), rq["r16"], "none"),
        ("r16_no_dense", syn_storage("x10"), rq["r16"], "NO_BH_DENSE"), ("r17", syn_storage("x10"), rq["r17"], "none"),
        ("r17_no_direct", syn_storage("x10"), rq["r17"], "NO_BH_DIRECT"), ("r12_packed", syn_storage("x10"), rq["r12"], "NO_BH_DENSE+NO_BH_PLAIN"),
        ("r10k_bhm_partitions", syn_storage("x10k"), R._bh("x10k"), "BH_PARTITIONS_ALWAYS"),
        ("bh_sparse_dense_partitions", sparse_storage(), dataclasses.replace(R._bh("x100k"), force_baseline=True, baseline_entry_count=8192),
         "BH_PARTITIONS_ALWAYS"),
        ("phs_x1k", syn_storage("x1k"), phs("x1k"), "none"), ("phs_x1k_columnar", syn_storage("x1k"), col(phs("x1k")), "none"),
        ("msbs1", syn_storage("x1k"), SQ.msbs(1), "none"), ("msbs1_double_key", syn_storage("x1k"), SQ.msbs(1, key_type=FP64), "none"),
        ("msbs2_partitions", syn_storage("x10k"), SQ.msbs(2), "BH_PARTITIONS_ALWAYS"),
        ("msphs1", syn_storage("x1k"), SQ.msphs(1), "none"), ("msphs1_columnar", syn_storage("x1k"), col(SQ.msphs(1)), "none"),
        ("msphs1_int64", syn_storage("x1k", True), SQ.msphs(1), "none"),
        ("msphs2_partitions", syn_storage("x10k"), SQ.msphs(2), "BH_PARTITIONS_ALWAYS"),
        ("phm1", syn_storage("x10", False, "y10"), SQ.phm(1), "none"),
        ("phm3_bhm_partitions", syn_storage("x1k", False, "y10"), SQ.phm(3), "BH_PARTITIONS_ALWAYS"),
        ("phm3_perfect_partitions", syn_storage("x1k", False, "y10"), SQ.phm(3), "PERFECT_PARTITIONS_ALWAYS"),
        # non-grouped aggregates over several columns
        ("nga1", nga_storage(), SQ.nga(1), "none"), ("nga3", nga_storage(), SQ.nga(3), "none"), ("nga4", nga_storage(), SQ.nga(4), "none"),
        ("nga5", nga_storage(), SQ.nga(5), "none"), ("nga5_no_cols", nga_storage(), SQ.nga(5), "NO_COLS_KERNEL"),
        # joins: the star shapes over a real dimension, one-to-many / keyed / semi tables
        ("c3", star_storage("none"), star["c3"][1], "none"), ("c3_cluster", star_storage("none"), star["c3"][1], "cluster"),
        ("c3w_cluster", star_storage("none"), star["c3w"][1], "cluster"), ("c3m", star_storage("none"), star["c3m"][1], "none"),
        ("c3d_cluster", star_storage("none"), star["c3d"][1], "cluster"), ("c3m_two_levels", star_storage("none"), star["c3m"][1], TWO_LEVELS),
        ("c3g", star_storage("dval/15625"), star["c3g"][1], "none"), ("c3g_cluster", star_storage("dval/15625"), star["c3g"][1], "cluster"),
        ("c3g_two_levels", star_storage("dval/15625"), star["c3g"][1], TWO_LEVELS),
        ("c3gm", star_storage("dval%64"), star["c3gm"][1], "none"), ("c3gm_cluster", star_storage("dval%64"), star["c3gm"][1], "cluster"),
        ("c3gm_two_levels", star_storage("dval%64"), star["c3gm"][1], TWO_LEVELS),
        ("c3f_cluster", star_storage("attr"), star["c3f"][1], "cluster"), ("c3x_cluster", star_storage("g32"), star["c3x"][1], "cluster"),
        ("j_otm_group_filter", joins_storage(), jq["otm_group_filter"], "none"), ("j_left_group", joins_storage(), jq["left_group"], "none"),
        ("j_keyed_composite", joins_storage(), jq["keyed_composite"], "none"), ("j_keyed_wide", joins_storage(), jq["keyed_wide"], "none"),
        ("jv_semi_dups_cluster", semi_storage(), vq["semi_dups"], "cluster"), ("jv_anti_dups", semi_storage(), vq["anti_dups"], "none"),
    ]
    assert len({c[0] for c in out}) == len(out)
    return [Case(cid, st, q, variant, EXPECTED_ROUTE[cid]) for cid, st, q, variant in out]


# ---- plans ---------------------------------------------------------------------------------------------------------------------
# compile_query gives every slot 4 or 8 bytes (0 for a projected key of a baseline table).  The library also takes the 1- and
# 2-byte MIN / MAX slots of a columnar buffer with logical-sized columns (include/hdk_hip.h: hdk_hip_target.slot_width; the LDS
# strategy only), which a caller that fills the plan itself can ask for: these cases get them, by the edit below.
NARROW_SLOTS = ("narrow_minmax", "narrow_minmax_scalar")
_compiled = {}


def compiled(case):
    """the case's CompiledPlan (one per case); for NARROW_SLOTS with every MIN / MAX over a SMALLINT / TINYINT column moved into a
    slot of the column's width, as RS/ColSlotContext.cpp lays out a columnar buffer with logical-sized columns"""
    if case.id not in _compiled:
        cp = compile_query(case.storage, case.query)
        if case.id in NARROW_SLOTS:
            p = cp.plan
            assert p.output_columnar and not any(t.kind == "avg" for t in case.query.targets if isinstance(t, Agg))
            for ti, t in enumerate(case.query.targets):  # (no AVG: target i owns slot i)
                if isinstance(t, Agg) and t.kind in ("min", "max"):
                    w = case.storage.get(case.query.table).columns[t.arg.name].type.size
                    if w < 4:
                        p.targets[ti].slot_width = p.targets[ti].slot2_width = w
                        cp.slot_widths[ti] = w
            total = 0 if p.keyless else p.key_count * ((p.entry_count * 8 + 7) // 8 * 8)
            for w in cp.slot_widths:
                total = (total + 7) // 8 * 8 + p.entry_count * w
            cp.buffer_bytes = (total + 7) // 8 * 8
        _compiled[case.id] = cp
    return _compiled[case.id]


# ---- what the tests share: oracle results, the halves' results, the table with half B twice --------------------------------------
_results = {}


def oracle_result(O, case, frag_ids=None, storage=None):
    """(compiled plan, the oracle's buffer, its error code) over the case's table, or over `frag_ids` of it, or over another
    storage with the SAME plan; computed once"""
    from util import run_oracle
    key = (case.id, None if frag_ids is None else tuple(frag_ids), id(storage) if storage is not None else None)
    if key not in _results:
        _results[key] = run_oracle(O, storage or case.storage, compiled(case), frag_ids)
    return _results[key]


_repeated = {}


def storage_with_half_b_twice(case, split="interleaved"):
    """The case's tables with the fragments of half B imported a second time behind the eight: what three launches A, B, B saw"""
    key = (id(case.storage), case.query.table, split)
    if key not in _repeated:
        again = SPLITS[split][1]
        st = ArrowStorage()
        for name, t in case.storage.tables.items():
            if name != case.query.table:
                st.add_table(t)
                continue
            cols = [Column(c.name, c.type, c.fragments + [c.fragments[f] for f in again], c.stats + [c.stats[f] for f in again], c.dictionary)
                    for c in t.columns.values()]
            st.add_table(Table(name, cols, list(t.frag_rows) + [t.frag_rows[f] for f in again]))
        _repeated[key] = st
    return _repeated[key]


def result_rows(cp, buf):
    """{key tuple: {target name: value}} of a result buffer (one row under the key () for a non-grouped plan)"""
    from hdk_amd import result_set as rs
    cols = rs.to_columns(cp, buf)
    names = list(cols)
    keys = [oc.name for oc in cp.out_cols if oc.kind == "key"]
    return {tuple(row[names.index(k)] for k in keys): dict(zip(names, row)) for row in zip(*[cols[n] for n in names])}


def data_properties(O, case, split):
    """Which of the module docstring's properties the case's data has under `split`, read off the oracle's results over each half
    (what the plan sees behind its filters and joins): {property: number of groups that show it}.  "only_a", "only_b", "both":
    groups in one half only, in both.  "null_a", "null_b", "null_both": shared groups with a SUM / MIN / MAX / AVG that is NULL over
    A and a value over B, the other way round, NULL over both.  "min_in_a", "max_in_b": shared groups whose MIN over A is below
    their MIN over B; whose MAX over B is above their MAX over A.  "null_key": groups with a NULL key, in all the table."""
    a_ids, b_ids = SPLITS[split]
    cp, bufa, erra = oracle_result(O, case, a_ids)
    _, bufb, errb = oracle_result(O, case, b_ids)
    assert erra == 0 and errb == 0
    ra, rb = result_rows(cp, bufa), result_rows(cp, bufb)
    out = collections.Counter()
    out["only_a"], out["only_b"] = len(set(ra) - set(rb)), len(set(rb) - set(ra))
    out["null_key"] = sum(any(v is None for v in k) for k in set(ra) | set(rb))
    aggs = [oc for oc in cp.out_cols if oc.kind == "agg" and oc.agg != "count"]
    for k in set(ra) & set(rb):
        shows = {"both"}
        for oc in aggs:
            x, y = ra[k][oc.name], rb[k][oc.name]
            if x is None or y is None:
                shows.add("null_both" if x is None and y is None else ("null_a" if x is None else "null_b"))
            elif oc.agg == "min" and x < y:
                shows.add("min_in_a")
            elif oc.agg == "max" and x < y:
                shows.add("max_in_b")
        out.update(shows)
    return {k: v for k, v in out.items() if v}


_NULLS = frozenset(("null_a", "null_b", "null_both"))
# Properties that a case does not show (everything else that its targets can show, its data must have): {id: (properties, why)}.
# The first group is ruled out by the plan's SHAPE; the second is a CHOICE of this file: a plan without GROUP BY has one group, the
# star and join shapes read one fact argument, and the tables are shared with the grouped cases whose classes they follow.
_ONE_GROUP = "a choice: one group over the table of the grouped cases, whose NULLs follow THEIR key's classes -- both halves hold values"
_NULL_IN_A = ("a choice: one group and one fact argument, NULL in every A row and a value in B (the slot still holds its NULL when "
              "half B arrives); MAX's argument is a dimension column")
LACKS = {
    "r8": (_NULLS, "the filter reads the argument: a row with a NULL argument fails it"),
    "r16": (_NULLS, "the filter reads the argument: a row with a NULL argument fails it"),
    "r16_no_dense": (_NULLS, "the filter reads the argument: a row with a NULL argument fails it"),
    "j_otm_group_filter": (_NULLS | {"min_in_a"}, "the filter reads SUM's argument; MIN's argument is a dimension column"),
    "j_left_group": (frozenset(("null_a", "null_b")), "AVG's argument is a dimension column: its NULLs come from the LEFT join's misses"),
    "r1": (_NULLS, _ONE_GROUP), "j_keyed_wide": (_NULLS, _ONE_GROUP), "jv_semi_dups_cluster": (_NULLS, _ONE_GROUP),
    "c3d_cluster": (frozenset(("null_b", "null_both", "min_in_a")), _NULL_IN_A),
}
for _cid in ("c3", "c3_cluster", "c3w_cluster", "c3m", "c3m_two_levels"):
    LACKS[_cid] = (frozenset(("null_b", "null_both", "max_in_b")), _NULL_IN_A)
# grouped cases without a NULL key: {id: why}
_DIM_KEY = "the key is a dimension column without NULLs, reached through an inner join"
NO_NULL_KEY = {"c3f_cluster": _DIM_KEY, "j_otm_group_filter": _DIM_KEY, "j_keyed_composite": _DIM_KEY}


def expected_properties(case):
    """what data_properties must find for the case under either split"""
    aggs = [t for t in case.query.targets if isinstance(t, Agg) and t.kind != "count"]
    out = {"both"} | ({"only_a", "only_b"} if case.query.groupby else set()) | (_NULLS if aggs else set())
    out |= {name for kind, name in (("min", "min_in_a"), ("max", "max_in_b")) if any(t.kind == kind for t in aggs)}
    return out - set(LACKS.get(case.id, ((), ""))[0])
