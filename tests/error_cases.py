"""Cases for the arithmetic error codes (tests/test_error_cases_cpu.py, tests/test_gpu_error_cases.py): ERR_DIV_BY_ZERO (1) and
ERR_OVERFLOW_OR_UNDERFLOW (7, the checked + - * of QE/ArithmeticIR.cpp:277-520) on every route that evaluates one.

A case is (id, storage builder, QueryUnit, variant, expected_route, spec).  Its data is CLEAN: no row can raise.  A PLACEMENT edits
a copy of it (storage_for): the planted operands are one past the largest value of the operation's SQL type ("over"), exactly
that value ("top"), exactly minus it ("bottom") or the type's smallest value ("floor").

Raising placements -- exactly one live offending row, the launch must report the code:
  first   row 0 of fragment 0                         seam    the last row of a middle fragment
  last    the last row of the last fragment (a partial tile of every kernel: no fragment size is a multiple of 64)
  alone   the row of the one-row fragment
Silent placements -- the same operands in rows the reference never evaluates (planted twice: in the `last` row, a ragged tail, and
in the `first` row, inside a full tile of every kernel's unrolled body); error word 0 and the oracle's buffer bit for bit:
  filtered       a filter on another column rejects the row          null_operand   the other operand is NULL
  no_partner     join plans: the outer key is absent from the inner table (a LEFT join then reads the inner operand as NULL)
  edge           no row offends: one live row's result is "top", another's "bottom" (a column-literal step reaches one end only:
                 the column cannot hold a value beyond its own type)
  edge_min       one live row's result is "floor".  It is inside the type, so nothing is raised; at width 8 it equals the NULL
                 sentinel of the int64 the result is carried in, and the aggregate skips it like a NULL.  The oracle agrees on every
                 case (test_error_cases_cpu.py compares all of them).
  clean          the data as it is

Tables: FRAGS outer rows -- relaunch_cases.FRAG_ROWS with a fragment of ONE row in the middle -- about 120 000 rows."""
import collections
import functools

import numpy as np

from hdk_amd import _abi as A
from hdk_amd.ir import Agg, Cast, Cmp, ColRef, FP64, JoinSpec, KeyRef, Lit, Or, Proj, QueryUnit, Type
from hdk_amd.plan import compile_query
from hdk_amd.storage import ArrowStorage

import relaunch_cases as RL

FRAGS = RL.FRAG_ROWS[:4] + (1,) + RL.FRAG_ROWS[4:]
N = sum(FRAGS)
_ENDS = np.cumsum(FRAGS)
ROWS = {"first": 0, "last": N - 1, "seam": int(_ENDS[2]) - 1, "alone": int(_ENDS[3])}
EDGE_ROWS = (int(_ENDS[2]) - 1, int(_ENDS[6]) + 100)  # where `edge` puts "top" and "bottom"
DEAD_ROWS = (ROWS["last"], ROWS["first"])  # where the silent placements plant: a ragged tail and a full tile
RAISING = ("first", "last", "seam", "alone")
SILENT = ("filtered", "null_operand", "no_partner", "edge", "edge_min", "clean")

Case = collections.namedtuple("Case", "id build query variant expected_route spec")
# op: + - * / % (integer) or "f/" (fp division); width: the step's check_width (0 for the divisions); a: (table, column);
# b: (table, column) or ("lit", value); alive / dead: {outer column: value} that make the planted row pass / fail the plan's
# filters (dead None: the plan has no filter); live: the filters as numpy over the outer columns (None: every row passes);
# join: a Join or None; zero: the divisor a division case plants (0, 0.0 or -0.0)
# only: the placements the case takes (None: all that apply); stale: the planted columns keep the clean data's statistics
Spec = collections.namedtuple("Spec", "op width a b alive dead live join zero only stale", defaults=(None, None, None, None, 0, None, False))
# fk / dkey: the join's columns (outer, inner); kind: "inner" or "left"; present: two inner ROWS the planted outer rows point at;
# absent: an outer key without a partner
Join = collections.namedtuple("Join", "fk dim dkey kind present absent")


# ---- operands ------------------------------------------------------------------------------------------------------------------
def type_max(width):
    return (1 << (8 * width - 1)) - 1


_FACTORS = {1: (127, 1), 2: (217, 151), 4: (2**31 - 1, 1), 8: (49 * 73 * 127 * 337, 92737 * 649657)}  # a * b == type_max


def operand_pairs(op, width, lit=None):
    """{"over" | "top" | "bottom" | "floor": (a, b)} for a step a op b of the width; with `lit` b is that literal and only the
    pairs whose a the column can hold are there"""
    m = type_max(width)
    if lit is not None:
        want = {"over": m + 1, "top": m, "bottom": -m, "floor": -m - 1, "under": -m - 2}
        assert op in "+-" and lit > 0
        out = {k: ((v - lit) if op == "+" else (v + lit), lit) for k, v in want.items()}
        out = {k: ab for k, ab in out.items() if -m <= ab[0] <= m}
        if "over" not in out:  # a - literal leaves the type at the bottom
            out["over"] = out.pop("under")
        out.pop("under", None)
        return out
    if op == "+":
        return {"over": (m - 7, 8), "top": (m - 7, 7), "bottom": (-(m - 7), -7), "floor": (-(m - 7), -8)}
    if op == "-":
        return {"over": (m - 7, -8), "top": (m - 7, -7), "bottom": (-(m - 7), 7), "floor": (-(m - 7), 8)}
    assert op == "*"
    fa, fb = _FACTORS[width]
    assert fa * fb == m
    return {"over": (1 << (4 * width), 1 << (4 * width - 1)), "top": (fa, fb), "bottom": (-fa, fb),
            "floor": (-(1 << (4 * width)), 1 << (4 * width - 1))}


# scan_bhm.hip: kBhmMaxAbsVal, the largest |argument| and |result| its matcher takes.  Its own comparison with the largest value
# of the step's type (`rmax > tmax`) can never decide: a column-literal step is at least 4 bytes wide, and 2^31 - 1 is far
# beyond this bound, which is checked for the same result.  The bound pairs of that kernel are therefore at THIS value: the upper
# end under +, the lower end under -, and the last product inside it under *.
BHM_BOUND = (1 << 19) - 1


VALUE_ROW = 4321  # the row of m and qm that holds INT64_MIN and -1 (both NOT NULL columns: INT64_MIN is a value there)


# ---- data ----------------------------------------------------------------------------------------------------------------------
def _nullable(rng, v, dtype, rate=0.02):
    out = v.astype(dtype)
    out[rng.random(len(v)) < rate] = np.iinfo(dtype).min
    return out


def _fp_null(arr, mask):
    arr.view(np.int64)[mask] = A.NULL_DOUBLE_BITS
    return arr


@functools.lru_cache(maxsize=None)
def main_storage():
    """t: a 64-value key, a 4 000-value key (wide), a 10-value and a 1 000-value INT key (x, x1k) and a 10-value one (y10);
    operands a / b of every integer width in ranges whose sums, differences and products stay far inside the type, 2 % NULL;
    divisors q64 / q32 / z that are never zero; d holds multiples of 1/8 and z powers of two, so every quotient and every sum of
    quotients is exact in any order; c / c64 in [0, 99] for the filters; m and qm are NOT NULL columns for the value cases."""
    rng = RL._rng("error cases main")
    jw = rng.integers(0, 4000, N)
    cols = {"key": rng.integers(0, 64, N).astype(np.int64), "wide": (jw * 274_877_906 + 5).astype(np.int64),
            "x": rng.integers(1, 11, N).astype(np.int32), "x1k": rng.integers(1, 1001, N).astype(np.int32),
            "y10": rng.integers(1, 11, N).astype(np.int32)}
    for name, dtype, hi in (("", np.int64, 1000), ("32", np.int32, 1000), ("16", np.int16, 100), ("8", np.int8, 10)):
        cols["a" + name] = _nullable(rng, rng.integers(1, hi + 1, N), dtype)
        cols["b" + name] = _nullable(rng, rng.integers(1, hi + 1, N), dtype)
    cols["q64"] = _nullable(rng, rng.integers(1, 10, N), np.int64)
    cols["q32"] = _nullable(rng, rng.integers(1, 10, N), np.int32)
    c = rng.integers(0, 100, N)
    cols["c"], cols["c64"] = c.astype(np.int32), c.astype(np.int64)
    cols["d"] = _fp_null(rng.integers(-400, 401, N) / 8.0, rng.random(N) < 0.02)
    cols["z"] = _fp_null(np.array([1.0, 2.0, 4.0, 8.0, -1.0, -2.0])[rng.integers(0, 6, N)], rng.random(N) < 0.02)
    cols["m"] = rng.integers(-1000, 1000, N).astype(np.int64)
    cols["qm"] = np.array([1, 2, 3, -1, -2, -3])[rng.integers(0, 6, N)].astype(np.int64)
    cols["m"][VALUE_ROW], cols["qm"][VALUE_ROW], cols["key"][VALUE_ROW] = np.iinfo(np.int64).min, -1, 9  # INT64_MIN / -1, INT64_MIN % -1
    # p19 + 7 reaches BHM_BOUND exactly, p19x + 7 is one past it (the bound pair of the kernels that carry no check)
    for name, top in (("p19", BHM_BOUND - 7), ("p19x", BHM_BOUND - 6)):
        cols[name] = _nullable(rng, rng.integers(1, 1001, N), np.int32)
        cols[name][ROWS["seam"] - 5] = top
    cols["x10k"] = rng.integers(1, 10_001, N).astype(np.int32)
    # the lower end (n19 - 7 reaches -BHM_BOUND, n19x - 7 is one past it) and a product (m19 * 2 is the largest even value inside
    # the bound, m19x * 2 the first one outside: BHM_BOUND is odd)
    for name, end in (("n19", -BHM_BOUND + 7), ("n19x", -BHM_BOUND + 6), ("m19", BHM_BOUND // 2), ("m19x", BHM_BOUND // 2 + 1)):
        cols[name] = _nullable(rng, rng.integers(1, 1001, N), np.int32)
        cols[name][ROWS["seam"] - 5] = end
    st = ArrowStorage()
    not_null = {"m": Type("int", 8, False), "qm": Type("int", 8, False)}
    RL.add_table(st, "t", cols, FRAGS, types=not_null)
    return st


ND = 30_000


@functools.lru_cache(maxsize=None)
def star_storage():
    """fact(fk, val, g32, c) JOIN dim(key, dval, dbig, attr): relaunch_cases.star_storage's shapes over a dimension of ND unique
    keys.  3 % of the foreign keys are NULL, 3 % have no partner (ND + 7); 5 % of dval and dbig are NULL."""
    rng = RL._rng("error cases star")
    dkey = rng.permutation(ND).astype(np.int64)
    dval = rng.integers(0, 10**6, ND).astype(np.int64)
    dbig = rng.integers(0, 2**40, ND).astype(np.int64)
    dval[rng.random(ND) < 0.05] = A.NULL_BIGINT
    dbig[rng.random(ND) < 0.05] = A.NULL_BIGINT
    miss = rng.random(N)
    fk = np.where(miss < 0.03, A.NULL_BIGINT, np.where(miss < 0.06, ND + 7, dkey[rng.integers(0, ND, N)])).astype(np.int64)
    st = ArrowStorage()
    RL.add_table(st, "dim", {"key": dkey, "dval": dval, "dbig": dbig, "attr": rng.integers(0, 64, ND).astype(np.int64)})
    RL.add_table(st, "fact", {"fk": fk, "val": _nullable(rng, rng.integers(-2**31 + 1, 2**31, N), np.int64),
                              "g32": rng.integers(0, 64, N).astype(np.int32), "c": rng.integers(0, 100, N).astype(np.int32)}, FRAGS)
    return st


@functools.lru_cache(maxsize=None)
def joins_storage():
    """relaunch_cases.joins_storage's schema: dim has three rows per key k (one-to-many) that share w; (a, b) and wide are unique"""
    rng = RL._rng("error cases joins")
    nd = 288
    r = np.arange(nd)
    wide = (rng.permutation(nd).astype(np.int64) - nd // 2) * 30_000_000_000
    r1, r2, r3 = rng.integers(0, nd, N), rng.integers(0, nd, N), rng.integers(0, nd, N)
    miss = rng.random(N)
    st = ArrowStorage()
    RL.add_table(st, "dim", {"k": (100 + r // 3).astype(np.int64), "a": (r % 40).astype(np.int32), "b": (r // 40).astype(np.int32),
                             "v": rng.integers(-500, 500, nd).astype(np.int64), "w": ((r // 3) % 8).astype(np.int16), "wide": wide}, [97, 97, 94])
    RL.add_table(st, "fact", {"fk": np.where(miss < 0.03, A.NULL_BIGINT, np.where(miss < 0.06, 99, 100 + r1 // 3)).astype(np.int64),
                              "fa": (r2 % 40).astype(np.int32), "fb": np.where(miss > 0.97, 8, r2 // 40).astype(np.int32),
                              "fwide": np.where(miss > 0.97, 7, wide[r3]).astype(np.int64),
                              "val": _nullable(rng, rng.integers(-100, 100, N), np.int64), "c": rng.integers(0, 100, N).astype(np.int32)}, FRAGS)
    return st


def column(storage, table, name):
    """a column of the storage as one array (a copy)"""
    fr = storage.get(table).columns[name].fragments
    return np.concatenate(fr) if len(fr) > 1 else fr[0].copy()


def with_edits(storage, edits, stale=()):
    """A copy of `storage` with {(table, column): {row: value}} written (None: the type's NULL); fragments and types as they
    were, untouched columns shared.  The statistics are computed again -- except for the columns of `stale`, which keep the ones
    of the clean data (a chunk whose recorded bounds the data has left)."""
    from hdk_amd.storage import Column, Table, _stats
    out = ArrowStorage()
    for name, t in storage.tables.items():
        if not any(tn == name for (tn, _c) in edits):
            out.add_table(t)
            continue
        bounds = np.concatenate([[0], np.cumsum(t.frag_rows)])
        cols = []
        for cname in t.column_order:
            old = t.columns[cname]
            if (name, cname) not in edits:
                cols.append(old)
                continue
            arr = column(storage, name, cname)
            for row, value in edits[(name, cname)].items():
                if arr.dtype.kind == "f":
                    arr[row] = value if value is not None else np.frombuffer(np.int64(A.NULL_DOUBLE_BITS).tobytes(), dtype=np.float64)[0]
                else:
                    arr[row] = np.iinfo(arr.dtype).min if value is None else value
            frags = [np.ascontiguousarray(arr[b:e]) for b, e in zip(bounds[:-1], bounds[1:])]
            stats = list(old.stats) if (name, cname) in stale else [_stats(x, old.type) for x in frags]
            cols.append(Column(cname, old.type, frags, stats, old.dictionary))
        out.add_table(Table(name, cols, list(t.frag_rows)))
    return out


# ---- the bound pair of hdk_join_agg_sliced2 ----------------------------------------------------------------------------------------
# scan_join.hip: x_fits_narrow admits fact.val in [INT32_MIN + 1, INT32_MAX] (a column with NULLs gives up INT32_MIN),
# payload_fits_32_bits admits dim.dval in [INT32_MIN + 2, INT32_MAX] (two values to spare).  "at": both columns' statistics sit on
# all four ends; the others put ONE end one past.
I32_MAX, I32_MIN = 2**31 - 1, -2**31
S2_BOUNDS = {"at": {("fact", "val"): {100: I32_MAX, 200: I32_MIN + 1}, ("dim", "dval"): {50: I32_MAX, 60: I32_MIN + 2}},
             "x_max": {("fact", "val"): {100: I32_MAX + 1}}, "x_min": {("fact", "val"): {200: I32_MIN}},
             "p_max": {("dim", "dval"): {50: I32_MAX + 1}}, "p_min": {("dim", "dval"): {60: I32_MIN + 1}}}


@functools.lru_cache(maxsize=None)
def star_bound_storage(kind):
    edits = {k: dict(v) for k, v in S2_BOUNDS["at"].items()}
    for k, v in S2_BOUNDS[kind].items():
        edits[k].update(v)
    return with_edits(star_storage(), edits)


# ---- placements ----------------------------------------------------------------------------------------------------------------
def placements(case):
    """the placements a case takes"""
    s = case.spec
    if s.only is not None:
        return list(s.only)
    out = list(RAISING)
    if s.dead is not None:
        out.append("filtered")
    out.append("null_operand")
    if s.join is not None:
        out.append("no_partner")
    if s.op in "+-*":
        pairs = operand_pairs(s.op, s.width, s.b[1] if s.b[0] == "lit" else None)
        if "top" in pairs or "bottom" in pairs:
            out.append("edge")
        if "floor" in pairs:
            out.append("edge_min")
    return out + ["clean"]


def _plant(case, edits, row, a, b, alive=True, partner=0, has_partner=True):
    """operands a and b (None: NULL; b ignored for a literal) and what makes outer row `row` live or dead"""
    s = case.spec
    outer = case.query.table

    def put(table, col, r, v):
        edits.setdefault((table, col), {})[r] = v

    for col, v in ((s.alive if alive else s.dead) or {}).items():
        put(outer, col, row, v)
    if s.join is not None:
        inner_row = s.join.present[partner]
        keys = [column(case.build(), s.join.dim, k)[inner_row] for k in s.join.dkey] if has_partner else s.join.absent
        for col, v in zip(s.join.fk, keys):
            put(outer, col, row, int(v))
    put(s.a[0], s.a[1], row if s.a[0] == outer else s.join.present[partner], a)
    if s.b[0] != "lit":
        put(s.b[0], s.b[1], row if s.b[0] == outer else s.join.present[partner], b)


def placement_edits(case, placement):
    s = case.spec
    if placement == "clean":
        return {}
    division = s.op in ("/", "%", "f/")
    pairs = {"over": ((5.0 if s.op == "f/" else 5), s.zero)} if division else \
        operand_pairs(s.op, s.width, s.b[1] if s.b[0] == "lit" else None)
    over = pairs["over"]
    edits = {}
    if placement in RAISING:
        _plant(case, edits, ROWS[placement], *over)
    elif placement == "filtered":
        for row in DEAD_ROWS:
            _plant(case, edits, row, *over, alive=False)
    elif placement == "null_operand":
        for row in DEAD_ROWS:
            if s.b[0] == "lit" or division:
                _plant(case, edits, row, None, over[1])
            else:
                _plant(case, edits, row, over[0], None)
    elif placement == "no_partner":
        for row in DEAD_ROWS:
            _plant(case, edits, row, *over, has_partner=False)
    elif placement == "edge":
        for i, name in enumerate(("top", "bottom")):
            if name in pairs:
                _plant(case, edits, EDGE_ROWS[i], *pairs[name], partner=i)
    elif placement == "edge_min":
        _plant(case, edits, EDGE_ROWS[0], *pairs["floor"])
    elif placement == "stale":
        _plant(case, edits, ROWS["last"], *over)
    else:
        assert placement == "clean"
    return edits


_storages = {}


def storage_for(case, placement):
    edits = placement_edits(case, placement)
    stale = tuple(sorted(edits)) if placement == "stale" else ()
    key = (case.build, repr(sorted((k, sorted(v.items(), key=repr)) for k, v in edits.items())), stale)
    if key not in _storages:
        _storages[key] = with_edits(case.build(), edits, stale) if edits else case.build()
    return _storages[key]


def expected_code(case, placement):
    """what a launch over the placement must report, from the placement's name alone"""
    if placement in RAISING or placement == "stale":
        return A.ERR_DIV_BY_ZERO if case.spec.op in ("/", "%", "f/") else A.ERR_OVERFLOW_OR_UNDERFLOW
    return 0


def expected_route(case, placement):
    r = case.expected_route
    return r if isinstance(r, str) else r["clean" if placement == "clean" else "*"]


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# what hdk_hip_describe_launch answers for a case under its variant (test_error_cases_cpu.py holds the library to it).  A pair:
# the planted operands change the column's statistics, and with them the route -- "clean" names the route of the clean data, "*"
# the one of every other placement.
EXPECTED_ROUTE = {
    "x_mul8": "hdk_scan_agg_direct,hdk_finalize",
    "x_mul8_filtered": "hdk_scan_agg_direct,hdk_finalize",
    "x_addl8_colcol": "hdk_scan_agg_direct,hdk_finalize",
    "x_subl8_or": "hdk_scan_agg_direct,hdk_finalize",
    "x_sub8": "hdk_scan_agg_direct,hdk_finalize",
    "vec_mul8": "hdk_scan_agg_vec,hdk_finalize",
    "vec_add4": "hdk_scan_agg_vec,hdk_finalize",
    "generic_mul8": "hdk_scan_agg_generic,hdk_finalize",
    "generic_add4": "hdk_scan_agg_generic,hdk_finalize",
    "global_mul8": "hdk_scan_agg_global",
    "global_add4": "hdk_scan_agg_global",
    "vec_mul4": "hdk_scan_agg_vec,hdk_finalize",
    "vec_sub4": "hdk_scan_agg_vec,hdk_finalize",
    "vec_add8": "hdk_scan_agg_vec,hdk_finalize",
    "vec_sub8": "hdk_scan_agg_vec,hdk_finalize",
    "vec_add2": "hdk_scan_agg_vec,hdk_finalize",
    "vec_mul2": "hdk_scan_agg_vec,hdk_finalize",
    "vec_sub1": "hdk_scan_agg_vec,hdk_finalize",
    "vec_mul1": "hdk_scan_agg_vec,hdk_finalize",
    "vec_addl4": "hdk_scan_agg_vec,hdk_finalize",
    "vec_subl4": "hdk_scan_agg_vec,hdk_finalize",
    "vec_addl8": "hdk_scan_agg_vec,hdk_finalize",
    "global_key_add4": "hdk_scan_agg_global",
    "vec_qual_mul4": "hdk_scan_agg_vec,hdk_finalize",
    "vec_div8": "hdk_scan_agg_vec,hdk_finalize",
    "vec_mod4": "hdk_scan_agg_vec,hdk_finalize",
    "vec_fdiv": "hdk_scan_agg_vec,hdk_finalize",
    "vec_fdiv_negative_zero": "hdk_scan_agg_vec,hdk_finalize",
    "generic_div8": "hdk_scan_agg_generic,hdk_finalize",
    "generic_mod4": "hdk_scan_agg_generic,hdk_finalize",
    "generic_fdiv": "hdk_scan_agg_generic,hdk_finalize",
    "generic_fdiv_negative_zero": "hdk_scan_agg_generic,hdk_finalize",
    "global_div8": "hdk_scan_agg_global",
    "global_mod4": "hdk_scan_agg_global",
    "global_fdiv": "hdk_scan_agg_global",
    "global_fdiv_negative_zero": "hdk_scan_agg_global",
    "nongrouped_mul8": "hdk_scan_agg_vec,hdk_finalize",
    "baseline_mul8": "hdk_scan_agg_global",
    "baseline_partitioned_mul8": "hdk_scan_agg_global",
    "bh_mul4": "hdk_scan_agg_bh_vec",
    "bh_mod_key_mul4": "hdk_scan_agg_bh_vec",
    "bh_dense_mod_key": "hdk_scan_agg_bh_dense,hdk_bh_fold_slabs",
    "pp_mul4": "hdk_pp_scatter,hdk_pp_scatter2,hdk_pp_aggregate,hdk_scan_agg_global",
    "pp_addl4": "hdk_pp_scatter,hdk_pp_scatter2,hdk_pp_aggregate,hdk_scan_agg_global",
    "bhm_at_bound": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize",
    "bhm_past_bound": "hdk_scan_agg_vec,hdk_finalize",
    "bhm_stale": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize",
    "bhm_part_at_bound": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_finalize",
    "bhm_part_past_bound": "hdk_scan_agg_global",
    "bhm_part_stale": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_finalize",
    "bhm_cast_at_bound": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "bhm_cast_past_bound": "hdk_scan_agg_global",
    "bhm_cast_stale": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "bhm_cast_part_at_bound": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "bhm_cast_part_past_bound": "hdk_scan_agg_global",
    "bhm_cast_part_stale": "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_bhm_fold",
    "join_direct_add8": "hdk_join_agg_direct,hdk_finalize",
    "join_sliced_add8": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced,hdk_join_agg_direct,hdk_finalize",
    "join_clustered_add8": "hdk_cluster_by_key,hdk_join_agg_direct,hdk_finalize",
    "join_vec_add8": "hdk_scan_agg_vec_join,hdk_finalize",
    "join_vec_grouped_add8": "hdk_scan_agg_vec_join,hdk_finalize",
    "join_bh_vec_add8": "hdk_scan_agg_bh_vec_join",
    "join_generic_add8": "hdk_scan_agg_generic,hdk_finalize",
    "s2_vec_join": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "s2_vec_join_two_levels": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_scatter_level2,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "s2_vec_join_planted": {"clean": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
            "*": "hdk_cluster_by_key,hdk_cluster_params,hdk_scan_agg_vec_join,hdk_finalize"},
    "s2_bh_vec_join": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_bh_vec_join,hdk_bh_fold_dense",
    "s2_bh_vec_join_two_levels": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_scatter_level2,hdk_join_agg_sliced2,hdk_scan_agg_bh_vec_join,hdk_bh_fold_dense",
    "s2_bh_vec_join_planted": {"clean": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_bh_vec_join,hdk_bh_fold_dense",
            "*": "hdk_cluster_by_key,hdk_cluster_params,hdk_scan_agg_bh_vec_join"},
    "vec_values": "hdk_scan_agg_vec,hdk_finalize",
    "generic_values": "hdk_scan_agg_generic,hdk_finalize",
    "global_values": "hdk_scan_agg_global",
    "join_sliced_jd_eval_add8": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced,hdk_join_agg_direct,hdk_finalize",
    "join_sliced_general_add8": {"clean": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
            "*": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced,hdk_join_agg_direct,hdk_finalize"},
    "s2_at_bound": "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize",
    "s2_past_x_max": "hdk_scan_agg_vec_join,hdk_finalize",
    "s2_past_x_min": "hdk_scan_agg_vec_join,hdk_finalize",
    "s2_past_p_max": "hdk_scan_agg_vec_join,hdk_finalize",
    "s2_past_p_min": "hdk_scan_agg_vec_join,hdk_finalize",
    "proj_target_mul8": "hdk_scan_project",
    "proj_target_sub4": "hdk_scan_project",
    "proj_qual_add4": "hdk_scan_project",
    "proj_scalar_target_mul8": "hdk_scan_project_scalar",
    "proj_scalar_qual_add4": "hdk_scan_project_scalar",
    "proj_join_target_add8": "hdk_scan_project_join",
    "proj_join_qual_sub8": "hdk_scan_project_join",
    "proj_keyed_target_mul8": "hdk_scan_project_keyed",
    "proj_keyed_qual_sub8": "hdk_scan_project_keyed",
    "bhm_low_at_bound": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize",
    "bhm_low_past_bound": "hdk_scan_agg_vec,hdk_finalize",
    "bhm_mul_at_bound": "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize",
    "bhm_mul_past_bound": "hdk_scan_agg_vec,hdk_finalize",
    "join_many_mul8": "hdk_scan_agg_vec_many,hdk_finalize",
    "join_many_left_mul8": "hdk_scan_agg_vec_many,hdk_finalize",
    "join_keyed_mul8": "hdk_scan_agg_vec_keyed,hdk_finalize",
    "join_keyed_wide_sub8": "hdk_scan_agg_vec_keyed,hdk_finalize",
}

# Routes that evaluate NO arithmetic step: their matchers take plain outer columns as arguments and `column cmp literal` quals
# only, so no plan with a + - * / % reaches them and there is nothing of this file's to test on them.  The cases baseline_mul8 and
# baseline_partitioned_mul8 and bh_mul4 pin where such a plan goes instead.  {route's first kernel: where the matcher says so}
NO_ARITHMETIC = {
    "hdk_scan_project_count": "scan_project.hip, match_project_fast: plain_outer_col (or a plain joined column) for every target, plain quals",
    "hdk_scan_project_stream": "scan_project.hip, match_project_fast: the one-pass form of the same matcher (PROJECT_ONE_PASS)",
    "hdk_scan_agg_baseline_direct": "scan_baseline.hip, match_baseline_fast: plain_outer_col for every argument, match_plain_quals",
    "hdk_part_scatter": "scan_baseline.hip, part_tuple_shape: starts from match_baseline_fast (the radix-partitioned baseline route)",
    "hdk_scan_agg_bh_direct": "scan_bh.hip, match_bh_fast: plain_outer_col for every argument, match_plain_quals",
}

# routes of the coverage set (test_error_cases_cpu.py computes it) without a case: {route: why}
EXCLUDED = {}

_KEY = ColRef("key")
_LT90 = {"quals": [Cmp(ColRef("c"), "<", Lit(90))]}
_ALIVE, _DEAD = {"c": 5, "c64": 5}, {"c": 95, "c64": 95}


def _c_passes(cols):
    return cols["c"] < 90


def _grouped(expr, key=None, **kw):
    return QueryUnit("t", groupby=[key if key is not None else _KEY], targets=[KeyRef(0, "k"), Agg("sum", expr, "s"), Agg("count", None, "n")], **kw)


def _t(col):
    return ("t", col)


def _main_cases():
    a, b, a32, b32, a16, b16, a8, b8 = (ColRef(c) for c in ("a", "b", "a32", "b32", "a16", "b16", "a8", "b8"))
    c64 = ColRef("c64")
    filt = dict(alive=_ALIVE, dead=_DEAD, live=_c_passes)
    out = []
    # -- the streaming kernel's X mode (fast_x_value): column op column, column op literal; no filter, a plain `column cmp literal`
    #    qual, a column-column qual and an OR program (each one streamed beside the value column: X mode again)
    out += [
        ("x_mul8", _grouped(a * b), "none", Spec("*", 8, _t("a"), _t("b"))),
        ("x_mul8_filtered", _grouped(a * b, quals=[Cmp(c64, "<", Lit(90))]), "none", Spec("*", 8, _t("a"), _t("b"), **filt)),
        ("x_addl8_colcol", _grouped(a + 7, quals=[Cmp(c64, "<", ColRef("b"))]), "none",
         Spec("+", 8, _t("a"), ("lit", 7), alive={"c64": 5, "b": 50}, dead={"c64": 95, "b": 50},
              live=lambda c: (c["c64"] < c["b"]) & (c["b"] != A.NULL_BIGINT))),
        ("x_subl8_or", _grouped(a - 7, quals=[Or(Cmp(ColRef("a"), ">", Lit(-5000)), Cmp(_KEY, "=", Lit(70)))]), "none",
         Spec("-", 8, _t("a"), ("lit", 7), alive={"key": 70}, dead={"key": 3},
              live=lambda c: ((c["a"] > -5000) & (c["a"] != A.NULL_BIGINT)) | (c["key"] == 70))),
        ("x_sub8", _grouped(a - b), "none", Spec("-", 8, _t("a"), _t("b"))),
    ]
    # -- the interpreters: eval_expr_v (batched), eval_expr (row at a time), the global-atomics kernel; every width
    for tag, variant in (("vec", "generic"), ("generic", "scalar"), ("global", "global")):
        out += [
            (f"{tag}_mul8", _grouped(a * b, **_LT90), variant, Spec("*", 8, _t("a"), _t("b"), **filt)),
            (f"{tag}_add4", _grouped(a32 + b32, **_LT90), variant, Spec("+", 4, _t("a32"), _t("b32"), **filt)),
        ]
    out += [
        ("vec_mul4", _grouped(a32 * b32, **_LT90), "generic", Spec("*", 4, _t("a32"), _t("b32"), **filt)),
        ("vec_sub4", _grouped(a32 - b32, **_LT90), "generic", Spec("-", 4, _t("a32"), _t("b32"), **filt)),
        ("vec_add8", _grouped(a + b, **_LT90), "generic", Spec("+", 8, _t("a"), _t("b"), **filt)),
        ("vec_sub8", _grouped(a - b, **_LT90), "generic", Spec("-", 8, _t("a"), _t("b"), **filt)),
        ("vec_add2", _grouped(a16 + b16, **_LT90), "generic", Spec("+", 2, _t("a16"), _t("b16"), **filt)),
        ("vec_mul2", _grouped(a16 * b16, **_LT90), "generic", Spec("*", 2, _t("a16"), _t("b16"), **filt)),
        ("vec_sub1", _grouped(a8 - b8, **_LT90), "generic", Spec("-", 1, _t("a8"), _t("b8"), **filt)),
        ("vec_mul1", _grouped(a8 * b8, **_LT90), "generic", Spec("*", 1, _t("a8"), _t("b8"), **filt)),
        ("vec_addl4", _grouped(a32 + 7, **_LT90), "generic", Spec("+", 4, _t("a32"), ("lit", 7), **filt)),
        ("vec_subl4", _grouped(a32 - 7, **_LT90), "generic", Spec("-", 4, _t("a32"), ("lit", 7), **filt)),
        ("vec_addl8", _grouped(a + 7, **_LT90), "generic", Spec("+", 8, _t("a"), ("lit", 7), **filt)),
        # the expression in a group key and in a qual (no other filter: the qual IS the filter)
        ("global_key_add4", QueryUnit("t", groupby=[a32 + b32], targets=[KeyRef(0, "k"), Agg("count", None, "n")], **_LT90), "global",
         Spec("+", 4, _t("a32"), _t("b32"), **filt)),
        ("vec_qual_mul4", _grouped(ColRef("m"), quals=[Cmp(a32 * b32, ">", Lit(10))]), "none", Spec("*", 4, _t("a32"), _t("b32"))),
    ]
    # -- divisions: the interpreters only
    q64, q32, d, z = ColRef("q64"), ColRef("q32"), ColRef("d"), ColRef("z")
    for tag, variant in (("vec", "generic"), ("generic", "scalar"), ("global", "global")):
        out += [
            (f"{tag}_div8", _grouped(a / q64, **_LT90), variant, Spec("/", 0, _t("a"), _t("q64"), **filt)),
            (f"{tag}_mod4", _grouped(a32 % q32, **_LT90), variant, Spec("%", 0, _t("a32"), _t("q32"), **filt)),
            (f"{tag}_fdiv", _grouped(d / z, **_LT90), variant, Spec("f/", 0, _t("d"), _t("z"), zero=0.0, **filt)),
            (f"{tag}_fdiv_negative_zero", _grouped(d / z, **_LT90), variant, Spec("f/", 0, _t("d"), _t("z"), zero=-0.0, **filt)),
        ]
    # -- divisions that raise nothing: INT64_MIN / -1 and x % -1 (VALUE_ROW, in the group of key 9) and exact fp quotients.
    #    test_error_cases_cpu.py writes down what the oracle gives for that group
    m, qm = ColRef("m"), ColRef("qm")
    for tag, variant in (("vec", "generic"), ("generic", "scalar"), ("global", "global")):
        out.append((f"{tag}_values", QueryUnit("t", groupby=[_KEY], targets=[KeyRef(0, "k"), Agg("min", m / qm, "qmin"), Agg("max", m / qm, "qmax"),
                                                                            Agg("sum", m % qm, "r"), Agg("sum", d / z, "f")]), variant,
                    Spec("/", 0, _t("m"), _t("qm"), only=("clean",))))
    # -- the non-grouped shape and the other layouts
    out += [
        ("nongrouped_mul8", QueryUnit("t", targets=[Agg("sum", a * b, "s"), Agg("count", None, "n")], **_LT90), "none",
         Spec("*", 8, _t("a"), _t("b"), **filt)),
        ("baseline_mul8", _grouped(a * b, ColRef("wide"), force_baseline=True, baseline_entry_count=16_384, **_LT90), "none",
         Spec("*", 8, _t("a"), _t("b"), **filt)),
        ("baseline_partitioned_mul8", _grouped(a * b, ColRef("wide"), force_baseline=True, baseline_entry_count=16_384), "partitioned",
         Spec("*", 8, _t("a"), _t("b"))),
        ("bh_mul4", _grouped(a32 * b32, Cast(ColRef("x"), FP64), **_LT90), "none", Spec("*", 4, _t("a32"), _t("b32"), **filt)),
        ("bh_mod_key_mul4", _grouped(a32 * b32, ColRef("x1k") % 37, **_LT90), "none", Spec("*", 4, _t("a32"), _t("b32"), **filt)),
        # (a key of column % literal, plain arguments: the step cannot raise, the dense open-addressing kernel evaluates it)
        ("bh_dense_mod_key", QueryUnit("t", groupby=[ColRef("x1k") % 37], targets=[KeyRef(0, "k"), Agg("sum", ColRef("y10"), "s")]), "none",
         Spec("%", 0, _t("x1k"), ("lit", 37), only=("clean",))),
        ("pp_mul4", QueryUnit("t", groupby=[ColRef("x1k"), ColRef("y10")], targets=[KeyRef(0, "k0"), KeyRef(1, "k1"), Agg("sum", a32 * b32, "s"),
                                                                                      Agg("count", None, "n")]), "PERFECT_PARTITIONS_ALWAYS",
         Spec("*", 4, _t("a32"), _t("b32"))),
        ("pp_addl4", QueryUnit("t", groupby=[ColRef("x1k"), ColRef("y10")], targets=[KeyRef(0, "k0"), KeyRef(1, "k1"), Agg("sum", a32 + 7, "s"),
                                                                                       Agg("max", a32 + 7, "mx")]), "PERFECT_PARTITIONS_ALWAYS",
         Spec("+", 4, _t("a32"), ("lit", 7))),
    ]
    # -- the kernels that carry NO check (scan_bhm.hip and its partitioned form): the matcher proves from the statistics that
    #    column op literal stays inside the type.  At the bound: still on chip; one past it: a route with the check, which takes
    #    every placement; statistics that the data has left (stale): code 7 through the armed fallback, not a wrapped sum
    def ms(keyexpr, col):
        x = ColRef(col)
        return QueryUnit("t", groupby=[keyexpr], targets=[KeyRef(0, "k"), Agg("count", None, "c"), Agg("max", x, "mx"), Agg("max", x + 7, "mxp"),
                                                         Agg("sum", x + 7, "sp")])
    at, stale = dict(only=("clean",)), dict(only=("clean", "stale"), stale=True)
    for tag, keyexpr, variant in (("bhm", ColRef("x1k"), "none"), ("bhm_part", ColRef("x10k"), "BH_PARTITIONS_ALWAYS"),
                                  ("bhm_cast", Cast(ColRef("x1k"), FP64), "none"), ("bhm_cast_part", Cast(ColRef("x10k"), FP64), "BH_PARTITIONS_ALWAYS")):
        out += [
            (f"{tag}_at_bound", ms(keyexpr, "p19"), variant, Spec("+", 4, _t("p19"), ("lit", 7), **at)),
            (f"{tag}_past_bound", ms(keyexpr, "p19x"), variant, Spec("+", 4, _t("p19x"), ("lit", 7))),
            (f"{tag}_stale", ms(keyexpr, "a32"), variant, Spec("+", 4, _t("a32"), ("lit", 7), **stale)),
        ]
    def ms2(col, op):
        x = ColRef(col)
        e = x - 7 if op == "-" else x * 2
        return QueryUnit("t", groupby=[ColRef("x1k")], targets=[KeyRef(0, "k"), Agg("count", None, "c"), Agg("min", e, "mn"), Agg("sum", e, "sp")])
    out += [
        ("bhm_low_at_bound", ms2("n19", "-"), "none", Spec("-", 4, _t("n19"), ("lit", 7), **at)),
        ("bhm_low_past_bound", ms2("n19x", "-"), "none", Spec("-", 4, _t("n19x"), ("lit", 7))),
        ("bhm_mul_at_bound", ms2("m19", "*"), "none", Spec("*", 4, _t("m19"), ("lit", 2), **at)),
        ("bhm_mul_past_bound", ms2("m19x", "*"), "none", Spec("*", 4, _t("m19x"), ("lit", 2), **at)),
    ]
    return [(cid, main_storage, q, v, s) for cid, q, v, s in out]


def _join_cases():
    V, D, Dbig = ColRef("val"), ColRef("dval", "dim"), ColRef("dbig", "dim")
    j = [JoinSpec("dim", ColRef("fk"), "key")]
    star = Join(("fk",), "dim", ("key",), "inner", (11, 23), (ND + 7,))
    s_add = Spec("+", 8, ("fact", "val"), ("dim", "dval"), join=star)
    s_big = Spec("+", 8, ("fact", "val"), ("dim", "dbig"), join=star)
    c3 = QueryUnit("fact", joins=j, targets=[Agg("sum", V + D)])
    c3w = QueryUnit("fact", joins=j, targets=[Agg("sum", V + Dbig)])
    c3g = QueryUnit("fact", joins=j, groupby=[ColRef("g32")], targets=[KeyRef(0), Agg("sum", V + D)])
    c3gm = QueryUnit("fact", joins=j, groupby=[D % 64], targets=[KeyRef(0), Agg("sum", V + D)])
    out = [
        ("join_direct_add8", star_storage, c3, "none", s_add),
        ("join_sliced_add8", star_storage, c3, "cluster", s_add),
        ("join_clustered_add8", star_storage, c3w, "cluster", s_big),
        ("join_vec_add8", star_storage, c3, "generic", s_add),
        ("join_vec_grouped_add8", star_storage, c3g, "none", s_add),
        ("join_bh_vec_add8", star_storage, c3gm, "none", s_add),
        ("join_generic_add8", star_storage, c3, "scalar", s_add),
    ]
    # -- hdk_join_agg_sliced2 carries no check: fact.val and the payload fit 32 bits by their statistics, so x op payload cannot
    #    leave BIGINT
    s2 = dict(only=("clean", "stale"), stale=True)
    c3g15 = QueryUnit("fact", joins=j, groupby=[D / 15625], targets=[KeyRef(0), Agg("sum", V + D)])
    c3gm_add = QueryUnit("fact", joins=j, groupby=[D % 64], targets=[KeyRef(0), Agg("sum", V + D)])
    for tag, q in (("s2_vec_join", c3g15), ("s2_bh_vec_join", c3gm_add)):
        for vt, variant in (("", "cluster"), ("_two_levels", RL.TWO_LEVELS)):
            out.append((f"{tag}{vt}", star_storage, q, variant, s_add._replace(**s2)))
        # (planted operands leave 32 bits: the statistics send the launch to a route with the check)
        out.append((f"{tag}_planted", star_storage, q, "cluster", s_add))
    # -- hdk_join_agg_sliced's two bodies (scan_join.hip, match_join_sliced): FAST for ONE target SUM(x + payload) -- the case
    #    join_sliced_add8 above -- and jd_eval for everything else: a second target, and the FAST shape under SLICE_GENERAL.  Over
    #    the "x_max" table fact.val has left 32 bits, so the two-target plan is not hdk_join_agg_sliced2's either
    c3_2t = QueryUnit("fact", joins=j, targets=[Agg("sum", V + D), Agg("count", None)])
    out += [("join_sliced_jd_eval_add8", functools.partial(star_bound_storage, "x_max"), c3_2t, "cluster", s_add),
            ("join_sliced_general_add8", star_storage, c3, "cluster+SLICE_GENERAL", s_add)]
    # -- hdk_join_agg_sliced2's bound pair: statistics exactly on the last admitted values, and one past each of the four
    out.append(("s2_at_bound", functools.partial(star_bound_storage, "at"), c3g, "cluster", s_add._replace(only=("clean",))))
    for kind in ("x_max", "x_min", "p_max", "p_min"):
        out.append((f"s2_past_{kind}", functools.partial(star_bound_storage, kind), c3g, "cluster", s_add))
    Dv = ColRef("v", "dim")
    lt90 = [Cmp(ColRef("c"), "<", Lit(90))]
    filt = dict(alive={"c": 5}, dead={"c": 95}, live=_c_passes)
    otm = Join(("fk",), "dim", ("k",), "inner", (30, 90), (99,))
    left = otm._replace(kind="left")
    keyed = Join(("fa", "fb"), "dim", ("a", "b"), "inner", (30, 90), (39, 8))
    wide = Join(("fwide",), "dim", ("wide",), "inner", (30, 90), (7,))
    out += [
        ("join_many_mul8", joins_storage, QueryUnit("fact", joins=[JoinSpec("dim", ColRef("fk"), "k")], quals=lt90,
                                                     targets=[Agg("sum", V * Dv, "s"), Agg("count", None, "c")]), "none",
         Spec("*", 8, ("fact", "val"), ("dim", "v"), join=otm, **filt)),
        ("join_many_left_mul8", joins_storage, QueryUnit("fact", joins=[JoinSpec("dim", ColRef("fk"), "k", "left")], quals=lt90,
                                                          groupby=[ColRef("w", "dim")], targets=[KeyRef(0, "w"), Agg("sum", V * Dv, "s"), Agg("count", None, "c")]),
         "none", Spec("*", 8, ("fact", "val"), ("dim", "v"), join=left, **filt)),
        ("join_keyed_mul8", joins_storage, QueryUnit("fact", joins=[JoinSpec("dim", [ColRef("fa"), ColRef("fb")], ["a", "b"])], quals=lt90,
                                                      groupby=[ColRef("w", "dim")], targets=[KeyRef(0, "w"), Agg("sum", V * Dv, "s"), Agg("count", None, "c")]),
         "none", Spec("*", 8, ("fact", "val"), ("dim", "v"), join=keyed, **filt)),
        ("join_keyed_wide_sub8", joins_storage, QueryUnit("fact", joins=[JoinSpec("dim", ColRef("fwide"), "wide")],
                                                           targets=[Agg("count", None, "c"), Agg("sum", V - Dv, "s")]), "none",
         Spec("-", 8, ("fact", "val"), ("dim", "v"), join=wide)),
    ]
    return out


def _projection_cases():
    """the projection interpreters (scan_project.h): the expression in a projected target (under a filter on another column) and in
    a qual (then the qual is the filter); plain, row at a time, behind a one-to-one probe and behind a keyed probe"""
    a, b, a32, b32, key = (ColRef(c) for c in ("a", "b", "a32", "b32", "key"))
    filt = dict(alive=_ALIVE, dead=_DEAD, live=_c_passes)
    proj = lambda table, targets, **kw: QueryUnit(table, targets=[Proj(e, f"p{i}") for i, e in enumerate(targets)], output_columnar=True, **kw)  # noqa: E731
    out = [
        ("proj_target_mul8", main_storage, proj("t", [key, a * b], **_LT90), "none", Spec("*", 8, _t("a"), _t("b"), **filt)),
        ("proj_target_sub4", main_storage, proj("t", [key, a32 - b32], **_LT90), "none", Spec("-", 4, _t("a32"), _t("b32"), **filt)),
        ("proj_qual_add4", main_storage, proj("t", [key, a32], quals=[Cmp(a32 + b32, ">", Lit(100))]), "none", Spec("+", 4, _t("a32"), _t("b32"))),
        ("proj_scalar_target_mul8", main_storage, proj("t", [key, a * b], **_LT90), "scalar", Spec("*", 8, _t("a"), _t("b"), **filt)),
        ("proj_scalar_qual_add4", main_storage, proj("t", [key, a32], quals=[Cmp(a32 + b32, ">", Lit(100))]), "scalar", Spec("+", 4, _t("a32"), _t("b32"))),
    ]
    V, D, Dv, fk = ColRef("val"), ColRef("dval", "dim"), ColRef("v", "dim"), ColRef("fk")
    lt90 = [Cmp(ColRef("c"), "<", Lit(90))]
    jf = dict(alive={"c": 5}, dead={"c": 95}, live=_c_passes)
    star = Join(("fk",), "dim", ("key",), "inner", (11, 23), (ND + 7,))
    keyed = Join(("fa", "fb"), "dim", ("a", "b"), "inner", (30, 90), (39, 8))
    j, jk = [JoinSpec("dim", fk, "key")], [JoinSpec("dim", [ColRef("fa"), ColRef("fb")], ["a", "b"])]
    out += [
        ("proj_join_target_add8", star_storage, proj("fact", [fk, V + D], joins=j, quals=lt90), "none",
         Spec("+", 8, ("fact", "val"), ("dim", "dval"), join=star, **jf)),
        ("proj_join_qual_sub8", star_storage, proj("fact", [fk, V], joins=j, quals=[Cmp(V - D, ">", Lit(0))]), "none",
         Spec("-", 8, ("fact", "val"), ("dim", "dval"), join=star)),
        ("proj_keyed_target_mul8", joins_storage, proj("fact", [ColRef("fa"), V * Dv], joins=jk, quals=lt90), "none",
         Spec("*", 8, ("fact", "val"), ("dim", "v"), join=keyed, **jf)),
        ("proj_keyed_qual_sub8", joins_storage, proj("fact", [ColRef("fa"), V], joins=jk, quals=[Cmp(V - Dv, ">", Lit(0))]), "none",
         Spec("-", 8, ("fact", "val"), ("dim", "v"), join=keyed)),
    ]
    return out


def is_projection(case):
    return any(isinstance(t, Proj) for t in case.query.targets)


@functools.lru_cache(maxsize=None)
def cases():
    """[Case]: the same list on every call"""
    out = _main_cases() + _join_cases() + _projection_cases()
    assert len({c[0] for c in out}) == len(out)
    return [Case(cid, build, q, variant, EXPECTED_ROUTE.get(cid), spec) for cid, build, q, variant, spec in out]


_compiled = {}


def compiled(case, placement="clean"):
    """the case's plan over the placement's storage (the plan carries the columns' statistics)"""
    key = (case.id, placement)
    if key not in _compiled:
        _compiled[key] = compile_query(storage_for(case, placement), case.query)
    return _compiled[key]


_results = {}
_matched = {}  # projections: the rows the oracle wrote


def oracle_matched(case, placement):
    """the row count of a projection case's oracle_result (over all fragments)"""
    return _matched[(case.id, placement, None)]


def oracle_result(O, case, placement, frag_ids=None):
    """(compiled plan, the oracle's buffer, its error code), computed once"""
    from util import run_oracle
    key = (case.id, placement, None if frag_ids is None else tuple(frag_ids))
    if key not in _results and is_projection(case):
        from util import host_fragments, oracle_init_buffer, oracle_join_tables
        st, cp = storage_for(case, placement), compiled(case, placement)
        buf = oracle_init_buffer(O, cp)
        err, n = O.run_projection(cp.plan, host_fragments(O, st, cp, frag_ids), buf, cp.entry_count, oracle_join_tables(O, st, cp))
        _results[key], _matched[key] = (cp, buf, err), n
    if key not in _results:
        _results[key] = run_oracle(O, storage_for(case, placement), compiled(case, placement), frag_ids)
    return _results[key]


# ---- the two launch-level cases ---------------------------------------------------------------------------------------------------
BOTH_CODES_VARIANTS = ("generic", "scalar", "global")  # the three kernels that evaluate a division


@functools.lru_cache(maxsize=None)
def both_codes():
    """(storage, query): row 0 divides by zero, the last row overflows, both live.  The oracle reports the first error in row
    order (1); the device reports the numerically larger code (7: include/hdk_hip.h, hdk_hip_launch)."""
    pair = operand_pairs("*", 8)["over"]
    st = with_edits(main_storage(), {("t", "a32"): {0: 5}, ("t", "q32"): {0: 0}, ("t", "a"): {N - 1: pair[0]}, ("t", "b"): {N - 1: pair[1]},
                                     ("t", "c"): {0: 5, N - 1: 5}})
    q = QueryUnit("t", groupby=[_KEY], targets=[KeyRef(0, "k"), Agg("sum", ColRef("a") * ColRef("b"), "s"), Agg("sum", ColRef("a32") % ColRef("q32"), "r")], **_LT90)
    return st, q


# (case, placement) whose launch over all the fragments raises and whose launch without the planted row's fragment is clean: the
# streaming kernel, a join route of several passes with an armed fallback, the partitioned perfect-hash scatter, and a launch that
# ends in the fallback itself
NOTHING_STICKS = (("x_mul8", "alone"), ("join_sliced_add8", "alone"), ("join_sliced_jd_eval_add8", "alone"), ("pp_mul4", "alone"), ("bhm_stale", "stale"), ("vec_mul8", "seam"))


def fragment_of(row):
    return int(np.searchsorted(_ENDS, row, "right"))

