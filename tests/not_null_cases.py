"""Tables and queries over columns declared NOT NULL, one case per route of hdk_amd/csrc/route.h.

A NOT NULL column gets another plan than a nullable one (hdk_amd/plan.py: _make_leaf, _agg_init_val, eff_nullable): every leaf
has nullable = 0, so the type's in-band sentinel (-128, -32768, INT32_MIN, INT64_MIN, NULL_DOUBLE, NULL_FLOAT) is an ordinary
value; a grouped aggregate gets skip_null = 0 and the slot inits 0 / INT64_MAX / INT64_MIN / +-DBL_MAX; a non-grouped one keeps
skip_null = 1 (OutputBufferInitialization.cpp:57-60, TargetExprBuilder.cpp:546-551); no key NULL is translated and a join key
probes with HDK_JOIN_NULL_NONE.  Every matcher and kernel carries its own copy of these decisions.

make_tables(declared, sentinel, seed) builds the same data under either declaration; cases() lists (name, QueryUnit, env, flags).
Shared by the CPU suite (test_not_null_cpu.py: the oracle against numpy, the plan facts, the routes) and the GPU suite
(test_gpu_not_null.py: every kernel against the oracle).

What the data keeps to:
  * SUM overflow -- the reference's agg_sum is unchecked.  `val` (int64) is non-negative and holds INT64_MIN in at most one row
    per value of `key`; SUM(val) is only asked for under groupings that contain `key` (and non-grouped, where INT64_MIN is
    skipped as the SUM slot's sentinel).  The narrow measures sum into int64 without getting near its bounds.
  * key range -- the int8 key `k8` draws from -128..-121 (-127..-121 without sentinels); the int16 key comes as `k16` (never
    -32768) and `k16s` (with it: the perfect-hash range becomes 32 776 entries); `k32` is never planted.
  * packed routes -- the packed kernels refuse values beyond their bound, so the `syn` table has `y10` (never planted) beside
    `y10s` (planted), and the five-aggregate shape comes over either.
  * `nv` stays nullable under both declarations: the other side of `column op column` with mixed nullability.
`dec` and `ts` feed key expressions and stay sentinel-free so that the expressions keep a range.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from hdk_amd import _abi as A
from hdk_amd.ir import (Agg, Cast, Cmp, ColRef, ExtractYear, FP64, INT32, JoinSpec, KeyRef, Lit, Not, Or, Proj, QueryUnit,
                        Type)
from hdk_amd.storage import ArrowStorage

ASSUMED_MI355X = -355  # include/hdk_hip.h: HDK_HIP_DEVICE_ASSUMED_MI355X

NULL_DOUBLE = np.array([A.NULL_DOUBLE_BITS], dtype=np.int64).view(np.float64)[0]
NULL_FLOAT = np.array([A.NULL_FLOAT_BITS], dtype=np.int32).view(np.float32)[0]

# rows per fragment: three ragged fragments and one shorter than a 4 096-row tile
T_ROWS, T_FRAG = 40_003, 13_001
SYN_ROWS, SYN_FRAG = 60_000, 19_667
FACT_ROWS, FACT_FRAG, DIM_ROWS = 30_000, 9_667, 3_000

# columns that stay nullable whatever the declaration
ALWAYS_NULLABLE = {("t", "nv")}

_KINDS = {"dec": ("decimal", 2), "ts": ("timestamp", 0)}


def _types(table, cols, declared):
    out = {}
    for name, arr in cols.items():
        nullable = declared == "nullable" or (table, name) in ALWAYS_NULLABLE
        if name in _KINDS:
            out[name] = Type(_KINDS[name][0], 8, nullable, _KINDS[name][1])
        else:
            out[name] = Type("fp" if arr.dtype.kind == "f" else "int", arr.dtype.itemsize, nullable)
    return out


def make_columns(sentinel, seed=0):
    """{table: {column: array}}: the data of make_tables, the same for either declaration."""
    rng = np.random.default_rng(20_261_020 + seed)

    def plant(arr, value, frac=0.03):
        if sentinel:
            arr[rng.random(len(arr)) < frac] = value
        else:
            rng.random(len(arr))  # (the same draws follow either way)
        return arr

    n = T_ROWS
    key = rng.integers(0, 64, n, dtype=np.int64)
    val = rng.integers(0, 2**31, n, dtype=np.int64)
    if sentinel:  # one row per value of `key` but 0: an ODD number of them (an even one adds up to 0 mod 2^64, as if skipped)
        for g in range(1, 64):
            val[np.nonzero(key == g)[0][g % 5]] = A.NULL_BIGINT
    nv = rng.integers(-1000, 1000, n, dtype=np.int64)
    nv[rng.random(n) < 0.05] = A.NULL_BIGINT
    t = {
        "key": key,
        "k8": rng.integers(-128 if sentinel else -127, -120, n).astype(np.int8),
        "k16": rng.integers(0, 7, n).astype(np.int16),
        "k16s": plant(rng.integers(0, 7, n).astype(np.int16), A.NULL_SMALLINT),
        "k32": rng.integers(-3, 41, n).astype(np.int32),
        "val": val,
        "c": plant(rng.integers(-50, 50, n).astype(np.int32), A.NULL_INT),
        "m16": plant(rng.integers(-100, 101, n).astype(np.int16), A.NULL_SMALLINT),
        "m8": plant(rng.integers(-100, 101, n).astype(np.int8), A.NULL_TINYINT),
        # (a mean away from zero: no sum cancels, so the relative bounds on fp sums mean something)
        "d": plant(rng.normal(size=n) * 100 + 150, NULL_DOUBLE),
        "f": plant((rng.normal(size=n) * 100 + 150).astype(np.float32), NULL_FLOAT),
        "dec": rng.integers(0, 4_000, n, dtype=np.int64),  # 0.00 .. 39.99
        "ts": rng.integers(946_684_800, 1_577_836_800, n, dtype=np.int64),  # 2000 .. 2019
        "flt": plant(rng.integers(-20, 21, n).astype(np.int32), A.NULL_INT),
        "nv": nv,
    }
    n = SYN_ROWS
    syn = {c: rng.integers(1, hi + 1, n).astype(np.int32) for c, hi in (("x10", 10), ("x1k", 1000), ("x10k", 10_000),
                                                                         ("x100k", 100_000), ("y10", 10))}
    syn["y10s"] = plant(rng.integers(1, 11, n).astype(np.int32), A.NULL_INT)
    nd, nf = DIM_ROWS, FACT_ROWS
    dim = {"key": rng.permutation(nd).astype(np.int64) * 3 - 77,  # every third key only
           "dval": plant(rng.integers(0, 10**6, nd).astype(np.int64), A.NULL_BIGINT),
           "attr": plant(rng.integers(0, 48, nd).astype(np.int32), A.NULL_INT),
           "grp": rng.integers(0, 48, nd).astype(np.int32),  # a build-side key with duplicates, never planted
           "pay": rng.integers(0, 10**6, nd).astype(np.int64)}  # a payload that may be summed
    fact = {"fk": plant(rng.integers(-97, 3 * nd - 57, nf).astype(np.int64), A.NULL_BIGINT, 0.02),
            "fk0": rng.integers(-97, 3 * nd - 57, nf).astype(np.int64),  # the same key, never planted
            "x": rng.integers(0, 2**31, nf).astype(np.int64),
            "g": rng.integers(-3, 60, nf).astype(np.int64),
            "g32": plant(rng.integers(-3, 60, nf).astype(np.int32), A.NULL_INT)}
    return {"t": t, "syn": syn, "dim": dim, "fact": fact}


_FRAGS = {"t": T_FRAG, "syn": SYN_FRAG, "dim": None, "fact": FACT_FRAG}


def make_tables(declared, sentinel, seed=0):
    """An ArrowStorage with t, syn, dim and fact.  declared: "nullable" | "not_null" (every column but ALWAYS_NULLABLE's is
    imported NOT NULL); sentinel: a few percent of the rows of the planted columns hold the type's in-band NULL pattern --
    values under "not_null", NULLs under "nullable"."""
    assert declared in ("nullable", "not_null")
    st = ArrowStorage()
    for table, cols in make_columns(sentinel, seed).items():
        st.import_numpy(table, cols, fragment_size=_FRAGS[table], types=_types(table, cols, declared))
    return st


def _five(col, prefix=""):
    return [Agg(k, col, prefix + k) for k in ("count", "sum", "min", "max", "avg")]


def cases():
    """(name, QueryUnit, env, flags): env are HDK_HIP_* switches to set around compile / describe / launch, flags the launch
    flags.  Names starting "ng_" are non-grouped, "pr_" projections."""
    K, K8, K16, K16S, K32 = (ColRef(c) for c in ("key", "k8", "k16", "k16s", "k32"))
    V, C_, M16, M8, D, F, DEC, TS, FLT, NV = (ColRef(c) for c in ("val", "c", "m16", "m8", "d", "f", "dec", "ts", "flt", "nv"))
    X10, X1K, X10K, X100K, Y, YS = (ColRef(c) for c in ("x10", "x1k", "x10k", "x100k", "y10", "y10s"))
    FK, X, G, G32 = (ColRef(c) for c in ("fk", "x", "g", "g32"))
    DV, AT, PAY = ColRef("dval", "dim"), ColRef("attr", "dim"), ColRef("pay", "dim")
    j = [JoinSpec("dim", FK, "key")]
    j0 = [JoinSpec("dim", ColRef("fk0"), "key")]
    jl = [JoinSpec("dim", FK, "key", "left")]
    # TRUE for a planted INT32_MIN under NOT NULL, NULL under the nullable declaration -- inside OR / NOT, where the
    # three-valued combiner's NULL masks must stay empty
    sent_or = [Or(Cmp(FLT, "<", Lit(0)), Not(Cmp(C_, "<>", Lit(A.NULL_INT))))]
    sent_eq = [Or(Cmp(FLT, "=", Lit(A.NULL_INT)), Cmp(C_, ">", Lit(40)))]
    key1 = [KeyRef(0, "k")]

    def bh(x, y, **kw):
        return QueryUnit("syn", groupby=[Cast(x, FP64)], targets=key1 + _five(y), **kw)

    out = [
        # ---- the LDS family ------------------------------------------------------------------------------------------------
        ("direct_sum", QueryUnit("t", groupby=[K], targets=key1 + [Agg("sum", V, "s")]), {}, 0),
        ("direct_sum_filter", QueryUnit("t", quals=[Cmp(FLT, "<", Lit(0))], groupby=[K], targets=key1 + [Agg("sum", V, "s")]), {}, 0),
        ("direct_sum_or", QueryUnit("t", quals=sent_or, groupby=[K], targets=key1 + [Agg("sum", V, "s")]), {}, 0),
        ("direct_sum_eq", QueryUnit("t", quals=sent_eq, groupby=[K], targets=key1 + [Agg("sum", V, "s")]), {}, 0),
        ("ng_direct_sum", QueryUnit("t", targets=[Agg("sum", V, "s")]), {}, 0),
        ("ng_cols", QueryUnit("t", targets=[Agg("count", None, "n"), Agg("count", V, "cv"), Agg("min", V, "mnv"), Agg("max", V, "mxv"),
                                            Agg("sum", V, "sv"), Agg("count", C_, "cc"), Agg("min", C_, "mnc"), Agg("max", C_, "mxc")]), {}, 0),
        # (a narrow SUM cannot meet its slot's sentinel, NULL_BIGINT, and skips nothing; COUNT / MIN / MAX skip the type's minimum)
        ("ng_cols_sums", QueryUnit("t", targets=[Agg("sum", C_, "sc"), Agg("avg", C_, "ac"), Agg("sum", M16, "s16"), Agg("sum", M8, "s8")]), {}, 0),
        ("ng_cols_narrow", QueryUnit("t", targets=[Agg("count", M16, "c16"), Agg("min", M16, "mn16"), Agg("max", M16, "mx16"), Agg("sum", M16, "s16"),
                                                   Agg("count", M8, "c8"), Agg("min", M8, "mn8"), Agg("avg", M8, "a8"), Agg("sum", M8, "s8")]), {}, 0),
        ("ng_cols_fp", QueryUnit("t", targets=[Agg("count", D, "cd"), Agg("min", D, "mnd"), Agg("max", D, "mxd"), Agg("sum", D, "sd"),
                                               Agg("avg", D, "ad"), Agg("count", F, "cf"), Agg("min", F, "mnf"), Agg("sum", F, "sf")]), {}, 0),
        ("ng_vec_filter", QueryUnit("t", quals=sent_or, targets=[Agg("count", None, "n"), Agg("sum", C_, "sc"), Agg("min", C_, "mnc"),
                                                                 Agg("max", M16, "mx16"), Agg("avg", M8, "a8"), Agg("count", V, "cv")]), {}, 0),
        ("ng_mixed_expr", QueryUnit("t", targets=[Agg("sum", C_ + NV, "s"), Agg("min", NV - C_, "mn"), Agg("count", C_ * NV, "cn"),
                                                  Agg("sum", C_ + 1, "s1"), Agg("max", M16 * 2, "mx")]), {}, 0),
        ("keys_count", QueryUnit("t", groupby=[K, K16], targets=[KeyRef(0, "k"), KeyRef(1, "k2"), Agg("count", None, "n")]), {}, 0),
        ("vec_two_keys", QueryUnit("t", groupby=[K, K16], targets=[KeyRef(0, "k"), KeyRef(1, "k2"), Agg("count", None, "n"), Agg("sum", V, "sv"),
                                                                  Agg("min", V, "mnv"), Agg("max", C_, "mxc"), Agg("count", C_, "cc"),
                                                                  Agg("min", M8, "mn8")]), {}, 0),
        ("keys_values_k8", QueryUnit("t", groupby=[K8, K16], targets=[KeyRef(0, "k"), KeyRef(1, "k2"), Agg("count", None, "n"),
                                                                      Agg("min", V, "mnv"), Agg("max", V, "mxv"), Agg("sum", C_, "sc"),
                                                                      Agg("count", M8, "c8")]), {}, 0),
        ("vec_all_widths", QueryUnit("t", groupby=[K], targets=key1 + _five(V, "v_") + [Agg("min", C_, "mnc"), Agg("avg", C_, "ac")]), {}, 0),
        ("vec_narrow", QueryUnit("t", groupby=[K], targets=key1 + [Agg("min", M16, "mn16"), Agg("max", M16, "mx16"), Agg("sum", M16, "s16"),
                                                                  Agg("avg", M16, "a16"), Agg("sum", M8, "s8"), Agg("min", M8, "mn8"),
                                                                  Agg("count", M8, "c8")]), {}, 0),
        ("vec_fp", QueryUnit("t", groupby=[K], targets=key1 + _five(D, "d_") + _five(F, "f_")[1:3]), {}, 0),
        ("vec_fp32", QueryUnit("t", groupby=[K16], targets=key1 + _five(F, "f_") + [Agg("max", D, "mxd")]), {}, 0),
        ("vec_fp_columnar", QueryUnit("t", groupby=[K], output_columnar=True, targets=key1 + _five(D, "d_")[1:] + _five(F, "f_")[1:4]), {}, 0),
        ("vec_expr_lit", QueryUnit("t", groupby=[K16], targets=key1 + [Agg("sum", C_ + 7, "s"), Agg("min", C_ + 100, "mn"), Agg("max", M16 - 1, "mx"),
                                                                      Agg("avg", M8 + 1, "a"), Agg("count", V + 1, "cv")]), {}, 0),
        ("vec_expr_mixed", QueryUnit("t", groupby=[K], targets=key1 + [Agg("sum", C_ + NV, "s"), Agg("min", NV - C_, "mn"), Agg("max", NV + M16, "mx"),
                                                                      Agg("count", C_ * NV, "cn")]), {}, 0),
        ("direct_mixed_sum", QueryUnit("t", groupby=[K], targets=key1 + [Agg("sum", C_ + NV, "s")]), {}, 0),
        ("key_year", QueryUnit("t", groupby=[ExtractYear(TS)], targets=key1 + [Agg("count", None, "n"), Agg("min", C_, "mn"), Agg("sum", C_, "s")]), {}, 0),
        ("key_dec", QueryUnit("t", groupby=[Cast(DEC, INT32)], targets=key1 + [Agg("count", None, "n"), Agg("max", C_, "mx"), Agg("sum", DEC, "sd"),
                                                                             Agg("min", TS, "mts")]), {}, 0),
        ("key_k16s", QueryUnit("t", groupby=[K16S], targets=key1 + [Agg("count", None, "n"), Agg("min", V, "mnv"), Agg("sum", C_, "sc")]), {}, 0),
        ("key_c_planted", QueryUnit("t", groupby=[C_], targets=key1 + [Agg("count", None, "n"), Agg("min", V, "mnv"), Agg("max", M16, "mx")]), {}, 0),
        ("generic", QueryUnit("t", groupby=[K], targets=key1 + _five(C_)), {}, A.LAUNCH_FORCE_SCALAR),
        # ---- the open-addressing families ---------------------------------------------------------------------------------------
        ("bh_dense_plain", bh(X10, Y), {}, 0),
        ("bh_dense_plain_planted", bh(X10, YS), {}, 0),
        ("bh_dense_plain_1k", bh(X1K, Y), {}, 0),
        ("bh_dense_filter", bh(X10, Y, quals=[Cmp(Y, "<=", Lit(7))]), {}, 0),
        ("bh_dense_filter_planted", bh(X10, Y, quals=[Cmp(YS, "<=", Lit(7))]), {}, 0),
        ("bh_packed_plain", bh(X10, Y), {"HDK_HIP_NO_BH_DENSE": "1"}, 0),
        ("bh_packed_filter", bh(X10, Y, quals=[Cmp(Y, "<=", Lit(7))]), {"HDK_HIP_NO_BH_DENSE": "1"}, 0),
        ("bh_direct_fp", QueryUnit("t", groupby=[Cast(K32, FP64)], targets=key1 + [Agg("sum", D, "sd"), Agg("min", D, "mnd"), Agg("count", D, "cd")]), {}, 0),
        ("bh_vec_mod", QueryUnit("t", groupby=[K32 % 7], targets=key1 + [Agg("sum", D, "sd"), Agg("min", C_, "mnc"), Agg("count", C_, "cc")]), {}, 0),
        ("bh_k32_wide", QueryUnit("t", groupby=[Cast(K32, FP64)], targets=key1 + [Agg("min", V, "mnv"), Agg("max", V, "mxv"), Agg("count", V, "cv"),
                                                                                Agg("sum", C_, "sc")]), {}, 0),
        ("bhm", QueryUnit("syn", groupby=[Cast(X1K, FP64)], targets=key1 + [Agg("count", None, "n"), Agg("max", Y, "mxy"), Agg("max", X10, "mxx"),
                                                                           Agg("max", X10 + 1, "mxp"), Agg("sum", Y, "sy"), Agg("sum", X10 + 1, "sp")]), {}, 0),
        ("bhm_planted", QueryUnit("syn", groupby=[Cast(X1K, FP64)], targets=key1 + [Agg("count", None, "n"), Agg("max", YS, "mxy"), Agg("max", X10, "mxx"),
                                                                                   Agg("min", YS, "mny"), Agg("sum", YS, "sy"), Agg("count", YS, "cy")]), {}, 0),
        ("bhm_perfect", QueryUnit("syn", groupby=[X1K], targets=key1 + [Agg("count", None, "n"), Agg("max", Y, "mxy"), Agg("max", X10, "mxx"),
                                                                       Agg("max", X10 + 1, "mxp"), Agg("sum", Y, "sy"), Agg("sum", X10 + 1, "sp")]), {}, 0),
        ("bhm_perfect_two_keys", QueryUnit("syn", groupby=[X10, Y], targets=[KeyRef(0, "k"), KeyRef(1, "k2")] + _five(X1K)), {}, 0),
        ("bhm_part", QueryUnit("syn", groupby=[Cast(X10K, FP64)], targets=key1 + [Agg("count", None, "n"), Agg("max", Y, "mxy"), Agg("sum", Y, "sy"),
                                                                                 Agg("sum", X10 + 1, "sp")]), {"HDK_HIP_BH_PARTITIONS_ALWAYS": "1"}, 0),
        ("bhm_part_perfect", QueryUnit("syn", groupby=[X100K], targets=key1 + _five(Y)), {"HDK_HIP_BH_PARTITIONS_ALWAYS": "1"}, 0),
        ("bh_dense_part", bh(X100K, Y), {"HDK_HIP_NO_BHM": "1", "HDK_HIP_BH_PARTITIONS_ALWAYS": "1"}, 0),
        ("bh_partitioned", bh(X100K, Y), {"HDK_HIP_NO_BHM": "1", "HDK_HIP_NO_BH_DENSE_PARTITIONS": "1", "HDK_HIP_BH_PARTITIONS_ALWAYS": "1"}, 0),
        # ---- global memory ----------------------------------------------------------------------------------------------------------
        ("baseline_direct", QueryUnit("t", groupby=[K], force_baseline=True, baseline_entry_count=131_071,
                                      targets=key1 + [Agg("sum", V, "sv"), Agg("count", None, "n"), Agg("min", V, "mnv"), Agg("max", C_, "mxc")]), {}, 0),
        ("baseline_direct_k16s", QueryUnit("t", groupby=[K16S], force_baseline=True, baseline_entry_count=131_071,
                                           targets=key1 + [Agg("min", V, "mnv"), Agg("count", None, "n"), Agg("sum", C_, "sc")]), {}, 0),
        ("global", QueryUnit("t", groupby=[K], targets=key1 + [Agg("sum", V, "sv"), Agg("min", V, "mnv"), Agg("avg", V, "av"), Agg("min", C_, "mnc"),
                                                                  Agg("count", C_, "cc"), Agg("sum", D, "sd"), Agg("max", F, "mxf")]),
         {}, A.LAUNCH_FORCE_GLOBAL_ATOMICS),
        ("global_columnar", QueryUnit("t", groupby=[K], force_baseline=True, baseline_entry_count=131_071, output_columnar=True,
                                      targets=key1 + [Agg("sum", V, "sv"), Agg("min", V, "mnv"), Agg("max", C_, "mxc"), Agg("avg", M16, "a16"),
                                                      Agg("min", D, "mnd"), Agg("max", F, "mxf")]), {}, 0),
        ("perfect_partitioned", QueryUnit("syn", groupby=[X100K], targets=key1 + [Agg("sum", YS, "s"), Agg("min", YS, "mn"), Agg("count", YS, "cy")]),
         {"HDK_HIP_PERFECT_PARTITIONS_ALWAYS": "1", "HDK_HIP_PERFECT_SLICE_LOG2": "6", "HDK_HIP_NO_BHM": "1"}, 0),
        ("radix_partitioned", QueryUnit("syn", groupby=[X100K], force_baseline=True, baseline_entry_count=200_003,
                                        targets=key1 + [Agg("sum", YS, "s"), Agg("min", YS, "mn"), Agg("count", None, "n")]),
         {}, A.LAUNCH_FORCE_PARTITIONED),
        # ---- joins ----------------------------------------------------------------------------------------------------------------
        ("ng_join_direct", QueryUnit("fact", joins=j, targets=[Agg("sum", X + AT, "s"), Agg("count", None, "n")]), {}, 0),
        ("ng_join_direct_list", QueryUnit("fact", joins=j, targets=[Agg("sum", X, "sx"), Agg("min", DV, "mnd"), Agg("max", DV, "mxd"),
                                                                   Agg("count", DV, "cd"), Agg("min", AT, "mna")]), {}, 0),
        ("ng_join_sliced", QueryUnit("fact", joins=j0, targets=[Agg("sum", X + PAY, "s")]), {}, A.LAUNCH_CLUSTER_PROBES),
        ("ng_join_sliced_planted", QueryUnit("fact", joins=j, targets=[Agg("sum", X + PAY, "s")]), {}, A.LAUNCH_CLUSTER_PROBES),
        ("ng_join_sliced2", QueryUnit("fact", joins=j0, targets=[Agg("sum", X, "sx"), Agg("count", None, "n"), Agg("max", PAY, "mxp")]),
         {}, A.LAUNCH_CLUSTER_PROBES),
        ("ng_join_sliced2_planted", QueryUnit("fact", joins=j0, targets=[Agg("sum", X, "sx"), Agg("count", None, "n"), Agg("max", AT, "mxa"),
                                                                        Agg("min", AT, "mna")]), {}, A.LAUNCH_CLUSTER_PROBES),
        ("join_sliced2_group", QueryUnit("fact", joins=j0, groupby=[ColRef("grp", "dim")], targets=key1 + [Agg("sum", X, "sx"), Agg("count", None, "n"),
                                                                                                       Agg("max", AT, "mxa")]),
         {}, A.LAUNCH_CLUSTER_PROBES),
        ("vec_join_group", QueryUnit("fact", joins=j, groupby=[G], targets=key1 + [Agg("sum", X, "sx"), Agg("min", DV, "mnd"), Agg("max", AT, "mxa"),
                                                                                Agg("count", DV, "cd"), Agg("count", G32, "cg")]), {}, 0),
        ("vec_join_left", QueryUnit("fact", joins=jl, groupby=[G], targets=key1 + [Agg("count", None, "n"), Agg("count", DV, "cd"), Agg("min", DV, "mnd"),
                                                                                Agg("max", AT, "mxa"), Agg("sum", AT, "sa")]), {}, 0),
        ("ng_vec_join_left", QueryUnit("fact", joins=jl, targets=[Agg("count", None, "n"), Agg("count", DV, "cd"), Agg("min", DV, "mnd"),
                                                                 Agg("sum", AT, "sa")]), {}, 0),
        ("vec_keyed", QueryUnit("fact", joins=[JoinSpec("dim", [FK, G32], ["key", "grp"])], groupby=[G],
                                targets=key1 + [Agg("count", None, "n"), Agg("min", DV, "mnd")]), {}, 0),
        ("vec_many", QueryUnit("fact", joins=[JoinSpec("dim", G32, "grp")], groupby=[G], targets=key1 + [Agg("count", None, "n"), Agg("max", DV, "mxd")]), {}, 0),
        ("bh_vec_join", QueryUnit("fact", joins=j, groupby=[AT % 7], targets=key1 + [Agg("sum", X, "sx"), Agg("min", DV, "mnd")]), {}, 0),
        # ---- projections ------------------------------------------------------------------------------------------------------------
        ("pr_fast", QueryUnit("t", quals=[Cmp(FLT, "<", Lit(0))], targets=[Proj(V, "val"), Proj(C_, "c"), Proj(M16, "m16"), Proj(M8, "m8"),
                                                                         Proj(D, "d"), Proj(FLT, "flt")]), {}, 0),
        ("pr_fast_columnar", QueryUnit("t", quals=[Cmp(C_, "=", Lit(A.NULL_INT))], output_columnar=True,
                                       targets=[Proj(V, "val"), Proj(C_, "c"), Proj(M8, "m8")]), {}, 0),
        ("pr_expr", QueryUnit("t", quals=sent_or, targets=[Proj(V, "val"), Proj(C_ + NV, "e"), Proj(C_ + 100, "c2"), Proj(FLT, "flt")]), {}, 0),
        ("pr_scalar", QueryUnit("t", quals=[Cmp(FLT, "<", Lit(0))], targets=[Proj(V, "val"), Proj(C_, "c"), Proj(FLT, "flt")]), {}, A.LAUNCH_FORCE_SCALAR),
        ("pr_join", QueryUnit("fact", joins=j, quals=[Cmp(G32, "<", Lit(0))], targets=[Proj(X, "x"), Proj(DV, "dval"), Proj(AT, "attr"), Proj(G32, "g32")]), {}, 0),
        ("pr_join_left", QueryUnit("fact", joins=jl, quals=[Cmp(G32, "<", Lit(0))], targets=[Proj(X, "x"), Proj(DV, "dval"), Proj(AT, "attr")]), {}, 0),
    ]
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def is_projection(q):
    return bool(q.targets) and all(isinstance(t, Proj) for t in q.targets)


@contextlib.contextmanager
def switches(env):
    """HDK_HIP_* switches set for the duration (the library reads them when asked to: sync_switches)."""
    from hdk_amd._lib import sync_switches
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    sync_switches()
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        sync_switches()


def describe(st, cp, flags=0, grid=0, device=ASSUMED_MI355X):
    """The kernels the executor's launch of `cp` over the whole outer table takes, from hdk_hip_describe_launch on an assumed
    MI355X: the kernel options and the fused form of a one-to-one join table as PreparedStep makes them (executor.py)."""
    from hdk_amd._lib import lib, sync_switches
    sync_switches()
    rows = st.get(cp.query.table).num_rows
    ko = A.KernelOptions(grid, 0, 0, flags, rows, 0, 0)

    def names(plan):
        out = C.create_string_buffer(256)
        rc = lib().hdk_hip_describe_launch(C.byref(plan), C.byref(ko), device, out, 256)
        assert rc == 0, lib().hdk_hip_last_error()
        return out.value.decode()

    first = names(cp.plan)
    fused_readers = {"hdk_scan_agg_vec_join", "hdk_scan_project_join", "hdk_scan_agg_vec_keyed", "hdk_scan_project_keyed",
                     "hdk_scan_agg_bh_vec_join"}
    if not cp.inner_tables or flags & (A.LAUNCH_FORCE_SCALAR | A.LAUNCH_FORCE_GLOBAL_ATOMICS) or \
            not fused_readers & set(first.split(",")):
        return first
    plan = A.Plan.from_buffer_copy(cp.plan)
    for ji, info in enumerate(cp.join_infos):
        cols = [ci for ci, (_t, _c, slot) in enumerate(cp.input_cols) if slot == ji + 1]
        if info["kind"] != A.JOIN_ONE_TO_ONE or len(cols) > 7:
            continue
        for k, ci in enumerate(cols):
            plan.cols[ci].kind = A.COL_DOUBLE if plan.cols[ci].kind in (A.COL_FLOAT, A.COL_DOUBLE) else A.COL_INT
            plan.cols[ci].width = 8
            plan.cols[ci].table = -(ji + 1)
            plan.cols[ci].buf_idx = 1 + k
        plan.joins[ji].kind = A.JOIN_ONE_TO_ONE_FUSED
        plan.joins[ji].fused_stride = 1 + len(cols)
    return names(plan)
