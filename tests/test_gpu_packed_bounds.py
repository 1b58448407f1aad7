"""The packed LDS accumulators [rows : 24 | sum : 40] at the bounds the host sizes them for.

The on-chip group-by kernels add COUNT and SUM of an argument with one 64-bit LDS add; the host bounds how many rows a block puts
into a word before it is decoded (scan_bhm.hip: max_rows_per_block, the generation of pass B; scan_bh_packed.hip: flush_rows) so
that the 40-bit sum field cannot run over.  These tests put a hot key's rows at those bounds with arguments as wide as the
matchers accept -- where a bound that is off gives a SUM that is off by 2^40 and a COUNT that is off by one, silently:

A  hdk_scan_agg_bhm under a caller's grid: a block's rows inside, just under and above what one word holds
B  the two-pass form at its natural generation (no HDK_HIP_BHM_PART_GENERATION): the first generation join at full size
C  `column * negative literal` next to a plain argument: signed words next to unsigned codes
D  the widest statistics the matchers accept, whatever kernel takes them
E  the one-argument packed kernels' fold-and-restart in the middle of a kernel

Every result is the oracle's bit for bit; the hot group is also checked against numpy's int64 COUNT / SUM / MIN / MAX over the
input columns."""
import functools

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd.ir import Agg, Cast, ColRef, FP64, KeyRef, QueryUnit
from hdk_amd.storage import ArrowStorage

from test_gpu_baseline import _assert_reference_placement, _check_rows
from test_gpu_bh_lds import _bh_query, _phs_query
from util import assert_buffers_equal, run_oracle

pytestmark = pytest.mark.gpu

BHM = "hdk_scan_agg_bhm"
PART = "hdk_bhm_scatter"
HOT = 7
SUM_LIMIT = 1 << 39           # a packed word's sum field is read back as a signed 40-bit number
WIDE = (1 << 19) - 1          # kBhmMaxAbsVal / kBhPackedMaxAbsVal: the widest |argument| the matchers take
FIVE = ("count", "sum", "max", "min", "avg")


def _five(arg, names=("c", "s", "mx", "mn", "a")):
    return [Agg(kd, arg, nm) for kd, nm in zip(FIVE, names)]


def _hot_expect(key, arg, mul=1, add=0, hot=HOT):
    """numpy's answer for the hot group: int64 arithmetic over the input columns, NULL arguments skipped"""
    v = arg[key == hot]
    v = v[v != A.NULL_INT].astype(np.int64) * mul + add
    return {"c": int(v.size), "s": int(v.sum()), "mx": int(v.max()), "mn": int(v.min()), "a": int(v.sum()) / int(v.size)}


def _check_hot(res, expect, key_name, hot=HOT, names=("c", "s", "mx", "mn", "a")):
    out = res.to_columns()
    i = [k is not None and int(k) == hot for k in out[key_name]].index(True)
    for want_name, nm in zip(("c", "s", "mx", "mn", "a"), names):
        if nm not in out:
            continue
        got, want = out[nm][i], expect[want_name]
        if want_name == "a":
            assert abs(got - want) <= 1e-6 * abs(want), (nm, got, want)  # (as _check_rows compares a double)
        else:
            assert got == want, (nm, got, want, got - want)


def _compare(oracle, cp, want, res):
    if cp.plan.query_kind == A.Q_BASELINE_HASH:
        _check_rows(cp, res.buffer, want)
        if not cp.plan.output_columnar:
            _assert_reference_placement(oracle, cp, res.buffer)
    else:
        assert_buffers_equal(cp, res.buffer, want)


def _run(oracle, make, st, plan, kernel, grid=0):
    """plan: (cp, want) of run_oracle, computed once per table and query and shared between the launches"""
    cp, want = plan
    step = make(st).prepare(cp, grid=grid)
    names = step.kernel_names()
    try:
        assert kernel is None or names.split(",")[0] == kernel, names
        res = step.run()
    finally:
        step.free()
    _compare(oracle, cp, want, res)
    return res


def _plan(oracle, st, q):
    cp, want, err = run_oracle(oracle, st, q)
    assert err == 0
    return cp, want


def _hot_table(n, groups, seed, hot_frac, lo, hi, hot_values, null_frac=0.0, fragment_size=None, hot=HOT):
    """key `x` in 1 .. groups with `hot` holding `hot_frac` of the rows; argument `y10` (the name _bh_query / _phs_query read)
    uniform in [lo, hi] with `hot_values(rng, count)` in the hot group.  The statistics come from the data: both extremes are
    planted, the low one outside the hot group."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, groups + 1, n).astype(np.int32)
    x[rng.random(n) < hot_frac] = hot
    y = rng.integers(lo, hi + 1, n).astype(np.int32)
    m = x == hot
    y[m] = hot_values(rng, int(m.sum()))
    cold = np.flatnonzero(~m)
    y[cold[0]], y[cold[-1]] = lo, hi
    y[np.flatnonzero(m)[0]] = hi
    if null_frac:
        nulls = rng.random(n) < null_frac
        nulls[[cold[0], cold[-1], np.flatnonzero(m)[0]]] = False
        y[nulls] = A.NULL_INT
    live = y[y != A.NULL_INT]
    assert live.min() == lo and live.max() == hi and y[m][0] == hi
    st = ArrowStorage()
    st.import_numpy("t", {"x": x, "y10": y}, fragment_size=fragment_size or n // 3 + 7)
    return st, x, y


def _near(top, spread=10):
    return lambda rng, count: rng.integers(top - spread, top + 1, count)


# ---- A: hdk_scan_agg_bhm, one pass, a caller's grid -----------------------------------------------------------------------------
# 8 000 groups of five aggregates: 16 bytes an entry (one packed word, MIN and MAX fields of 21 bits in a 64-bit word) = 128 KB,
# one 1024-thread block per CU, whose tiles are 1024 lanes x 8 rows; tile t of the launch (counted through the fragments, each
# rounded up to whole tiles) goes to block t % grid.
BHM_TILE = 8192
A_LO, A_HI = -500_000, 500_000
A_CODE_MAX = A_HI - A_LO + 1                     # the code of +500 000: value - raw_min + 1
A_B_OLD = (SUM_LIMIT - 1) // A_HI                # 1 099 511 rows: the bound sized from max |value|
A_B_TRUE = (SUM_LIMIT - 1) // A_CODE_MAX         # 549 755 rows: the bound sized from the largest code
Y = ColRef("y10")


def _a_queries():
    return {"perfect": _phs_query("x"), "open": _bh_query("x"),
            "plus": QueryUnit("t", groupby=[ColRef("x")], targets=[KeyRef(0, "k")] + _five(Y + 77))}


@functools.lru_cache(maxsize=None)
def _a_table(n, fragment_size):
    return _hot_table(n, 8_000, 61, 0.97, A_LO, A_HI, _near(A_HI), fragment_size=fragment_size)


_a_plans = {}


def _a_plan(oracle, n, fragment_size, which):
    key = (n, fragment_size, which)
    if key not in _a_plans:
        _a_plans[key] = _plan(oracle, _a_table(n, fragment_size)[0], _a_queries()[which])
    return _a_plans[key]


def _deal(frag_rows, grid, hot_mask):
    """(tiles, hot rows) of every block under the round-robin deal of the one-pass kernel"""
    tiles, hot = [0] * grid, [0] * grid
    csum = np.concatenate([[0], np.cumsum(hot_mask)])
    t, row_begin = 0, 0
    for n in frag_rows:
        for r0 in range(0, n, BHM_TILE):
            b = t % grid
            tiles[b] += 1
            hot[b] += int(csum[row_begin + min(r0 + BHM_TILE, n)] - csum[row_begin + r0])
            t += 1
        row_begin += n
    return tiles, hot


def _a_check(res, x, y, which):
    _check_hot(res, _hot_expect(x, y, add=77 if which == "plus" else 0), "key0" if which == "open" else "k")


A_N, A_FRAG = 3_200_000, 1_066_674


@pytest.mark.parametrize("which", ["perfect", "open", "plus"])
def test_bhm_one_pass_rows_per_block_between_the_code_bound_and_the_value_bound(oracle, gpu_executor_factory, which):
    """800 000 rows a block, 97 % of them in one group with values near +500 000: inside what max |value| allows (1 099 511
    rows), beyond what the codes allow (549 755) -- the sum field passed 2^39 and came back 2^40 short with one row too many.
    The result must be the oracle's; the flag and the armed fallback are a fine way to it."""
    st, x, y = _a_table(A_N, A_FRAG)
    grid = 4
    tiles, hot = _deal(st.get("t").frag_rows, grid, x == HOT)
    assert all(A_B_TRUE < t * BHM_TILE < A_B_OLD for t in tiles), tiles
    assert all(h * (A_CODE_MAX - 10) > SUM_LIMIT for h in hot), hot  # (the hot group alone runs a word over)
    res = _run(oracle, gpu_executor_factory, st, _a_plan(oracle, A_N, A_FRAG, which), BHM, grid=grid)
    _a_check(res, x, y, which)


@pytest.mark.parametrize("which", ["perfect", "plus"])
def test_bhm_one_pass_rows_per_block_above_the_value_bound(oracle, gpu_executor_factory, which):
    """1.6 M rows a block: beyond either bound -- the flag, the armed fallback, the oracle's result."""
    st, x, y = _a_table(A_N, A_FRAG)
    grid = 2
    tiles, _ = _deal(st.get("t").frag_rows, grid, x == HOT)
    assert all(t * BHM_TILE > A_B_OLD for t in tiles), tiles
    res = _run(oracle, gpu_executor_factory, st, _a_plan(oracle, A_N, A_FRAG, which), BHM, grid=grid)
    _a_check(res, x, y, which)


A_UNDER_N, A_UNDER_FRAG = 2_194_000, 1_097_000


@pytest.mark.parametrize("which", ["perfect", "open", "plus"])
def test_bhm_one_pass_just_under_the_code_bound_stays_on_chip(oracle, gpu_executor_factory, monkeypatch, which):
    """67 tiles a block (548 864 rows <= 549 755): the hot group's word ends above 0.9 x 2^39 and below 2^39.  No flag (the
    hook turns one into an error): the corrected bound is not a fallback in disguise."""
    monkeypatch.setenv("HDK_HIP_BHM_FLAG_IS_ERROR", "1")
    st, x, y = _a_table(A_UNDER_N, A_UNDER_FRAG)
    grid = 4
    tiles, hot = _deal(st.get("t").frag_rows, grid, x == HOT)
    assert all(t * BHM_TILE <= A_B_TRUE for t in tiles), tiles
    assert all(0.9 * SUM_LIMIT < h * A_CODE_MAX < SUM_LIMIT for h in hot), hot
    res = _run(oracle, gpu_executor_factory, st, _a_plan(oracle, A_UNDER_N, A_UNDER_FRAG, which), BHM, grid=grid)
    _a_check(res, x, y, which)


# ---- B: two passes, the natural generation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_frac", [0.0, 0.03])
def test_bhm_two_pass_natural_generation_holds_a_hot_key(oracle, gpu_executor_factory, monkeypatch, null_frac):
    """20 000 groups (beyond one block's LDS), 6 M rows (two passes without a switch), 95 % of them in one key with values near
    +500 000.  HDK_HIP_BHM_PART_TUPLES=256 keeps a sub-slab of up to 2 M tuples with ONE pass-B block, so each of the hot key's
    eight sub-slabs (about 0.7 M tuples) is one block's: fewer tuples than the generation sized from max |value| (1 097 728: never
    flushed, and the word ran over), more than the one sized from the codes (548 864: flushed once) -- the generation join of
    counts, sums, MIN, MAX and NULL counts at its natural size.  On chip: the hook turns a fallback into an error."""
    monkeypatch.delenv("HDK_HIP_BHM_PART_GENERATION", raising=False)
    monkeypatch.setenv("HDK_HIP_BHM_PART_TUPLES", "256")
    monkeypatch.setenv("HDK_HIP_BHM_FLAG_IS_ERROR", "1")
    n = 6_000_000
    st, x, y = _hot_table(n, 20_000, 62, 0.95, A_LO, A_HI, _near(A_HI), null_frac=null_frac)
    hot_live = y[(x == HOT) & (y != A.NULL_INT)]
    smallest_code = int(hot_live.min()) - A_LO + 1
    per_sub_slab = hot_live.size / 8  # (pass A deals its blocks' rows over eight regions: the margins below allow 10 % of unevenness)
    assert per_sub_slab * smallest_code >= 1.1 * SUM_LIMIT
    assert per_sub_slab * 1.1 < A_B_OLD
    for which, q in (("perfect", _phs_query("x")), ("open", _bh_query("x"))):
        res = _run(oracle, gpu_executor_factory, st, _plan(oracle, st, q), PART)
        _check_hot(res, _hot_expect(x, y), "key0" if which == "open" else "k")


# ---- C: signed words next to unsigned codes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["plus", "minus", "both"])
def test_bhm_signed_product_words_next_to_plain_codes(oracle, gpu_executor_factory, monkeypatch, pattern):
    """`y10 * -3` over statistics [-100 000, 100 000] adds signed values of up to +-300 000 to its word, the plain argument next
    to it codes of up to 200 001: the budget is the product's (1 832 519 rows).  223 tiles a block put 1.77 M hot rows into both
    words -- the product's sum ends near -2^39 (`plus`), near +2^39 (`minus`) or near 0 with both signs passing through the
    field (`both`); its decode must stay signed whatever is done for codes.  5 000 groups: 24 bytes an entry, still one block's
    LDS."""
    monkeypatch.setenv("HDK_HIP_BHM_FLAG_IS_ERROR", "1")
    top = 100_000
    budget = (SUM_LIMIT - 1) // (3 * top)
    grid, tiles_per_block = 2, budget // BHM_TILE
    n = grid * tiles_per_block * BHM_TILE - 4_321
    hot_values = {"plus": _near(top), "minus": lambda rng, c: -_near(top)(rng, c),
                  "both": lambda rng, c: _near(top)(rng, c) * np.where(np.arange(c) % 2 == 0, 1, -1)}[pattern]
    st, x, y = _hot_table(n, 5_000, 63, 0.97, -top, top, hot_values, fragment_size=(n // (2 * BHM_TILE) + 1) * BHM_TILE)
    tiles, hot = _deal(st.get("t").frag_rows, grid, x == HOT)
    assert all(t * BHM_TILE <= budget for t in tiles) and max(tiles) == tiles_per_block, tiles
    if pattern != "both":
        assert all(0.9 * SUM_LIMIT < h * 3 * (top - 10) and h * 3 * top < SUM_LIMIT for h in hot), hot
    prod = Y * -3
    q = QueryUnit("t", groupby=[ColRef("x")],
                  targets=[KeyRef(0, "k"), Agg("sum", prod, "s"), Agg("avg", prod, "a"), Agg("max", prod, "mx"), Agg("min", prod, "mn"),
                           Agg("count", prod, "c"), Agg("sum", Y, "sy"), Agg("avg", Y, "ay")])
    res = _run(oracle, gpu_executor_factory, st, _plan(oracle, st, q), BHM, grid=grid)
    _check_hot(res, _hot_expect(x, y, mul=-3), "k")
    _check_hot(res, _hot_expect(x, y), "k", names=("c", "sy", "-", "-", "ay"))


# ---- D: the widest statistics the matchers accept --------------------------------------------------------------------------------
@pytest.mark.parametrize("groups,extremes", [(40, "one_group"), (40, "two_groups"), (4_000, "one_group"), (4_000, "two_groups")])
def test_widest_argument_statistics_on_whatever_kernel_takes_them(oracle, gpu_executor_factory, groups, extremes):
    """Two argument columns with statistics [-(2^19 - 1), 2^19 - 1] and NULLs; both extremes in the hot group, or the low one in
    another.  Plain, `+ literal` and `* literal` arguments, MIN and MAX of both columns at once.  kernel=None: whichever kernel
    the matchers pick, the result is the oracle's."""
    rng = np.random.default_rng(64)
    n = 600_011
    x = rng.integers(1, groups + 1, n).astype(np.int32)
    x[rng.random(n) < 0.5] = HOT
    cols = {"x": x}
    for name in ("y10", "b"):
        v = rng.integers(-WIDE, WIDE + 1, n).astype(np.int32)
        v[rng.random(n) < 0.03] = A.NULL_INT
        hot, cold = np.flatnonzero(x == HOT), np.flatnonzero(x == HOT + 1)
        v[hot[1]] = WIDE
        v[(hot if extremes == "one_group" else cold)[2]] = -WIDE
        cols[name] = v
    st = ArrowStorage()
    st.import_numpy("t", cols, fragment_size=n // 3 + 7)
    B = ColRef("b")
    queries = (
        # the first kernel of step.kernel_names() with 40 / 4 000 groups:
        _phs_query("x"),                                       # hdk_scan_agg_bh_dense_plain / hdk_scan_agg_bh_dense_plain
        _bh_query("x"),                                        # hdk_scan_agg_bh_dense_plain / hdk_scan_agg_bh_dense_plain
        QueryUnit("t", groupby=[ColRef("x")],                  # hdk_scan_agg_keys_values / hdk_scan_agg_global (four 21-bit fields
                  targets=[KeyRef(0, "k"), Agg("min", Y, "mn"), Agg("max", Y, "mx"), Agg("min", B, "mnb"), Agg("max", B, "mxb"),  # are more than one 64-bit word)
                           Agg("count", None, "n")]),
        QueryUnit("t", groupby=[ColRef("x")],                  # hdk_scan_agg_keys_values / hdk_scan_agg_bhm
                  targets=[KeyRef(0, "k"), Agg("min", Y, "mn"), Agg("max", B, "mxb"), Agg("sum", Y, "s"), Agg("avg", B, "ab")]),
        QueryUnit("t", groupby=[ColRef("x")],                  # hdk_scan_agg_vec / hdk_scan_agg_global (y10 + 1 leaves the accepted range)
                  targets=[KeyRef(0, "k")] + _five(Y + 1)),
        QueryUnit("t", groupby=[ColRef("x")],                  # hdk_scan_agg_bhm / hdk_scan_agg_bhm (y10 * -1 stays inside it)
                  targets=[KeyRef(0, "k")] + _five(Y * -1) + [Agg("sum", B, "sb")]),
        QueryUnit("t", groupby=[Cast(ColRef("x"), FP64)],      # hdk_scan_agg_bh_vec / hdk_scan_agg_global (y10 * 3 leaves it)
                  targets=[KeyRef(0, "k")] + _five(Y * 3)),
    )
    for qi, q in enumerate(queries):
        res = _run(oracle, gpu_executor_factory, st, _plan(oracle, st, q), None)
        if qi in (0, 1, 4, 5, 6):
            mul, add = {0: (1, 0), 1: (1, 0), 4: (1, 1), 5: (-1, 0), 6: (3, 0)}[qi]
            _check_hot(res, _hot_expect(x, cols["y10"], mul=mul, add=add), "key0" if qi == 1 else "k")


# ---- E: the one-argument packed kernels fold their table and start over in mid-kernel -------------------------------------------
E_FLUSH = (SUM_LIMIT - 1) // WIDE  # flush_rows of scan_bh_packed.hip for statistics [-(2^19 - 1), 2^19 - 1]: 1 048 578 rows
E_PATTERNS = {
    "plus": (lambda rng, c: np.full(c, WIDE), 0.0),
    "minus": (lambda rng, c: np.full(c, -WIDE), 0.0),   # the sum goes towards -2^39 and borrows from the row field
    "both": (lambda rng, c: np.where(np.arange(c) % 2 == 0, WIDE, -WIDE), 0.0),
    "nulls": (lambda rng, c: rng.integers(WIDE - 5, WIDE + 1, c), 0.03),
}


def _e_table(n, groups, pattern, seed, hot=HOT):
    hot_values, null_frac = E_PATTERNS[pattern]
    # (the hot group also holds the ONE +max that _hot_table plants in it)
    return _hot_table(n, groups, seed, 0.9, -WIDE, WIDE, hot_values, null_frac=null_frac, hot=hot)


@pytest.mark.parametrize("pattern", list(E_PATTERNS))
@pytest.mark.parametrize("dense", [True, False])
def test_packed_one_pass_kernels_flush_in_mid_kernel(oracle, gpu_executor_factory, monkeypatch, dense, pattern):
    """ONE block (grid=1) walks 3 M rows, 90 % of them one key's, with flush_rows = 1 048 578: it folds its table into the output,
    re-initialises it and goes on -- twice -- and the last fold joins what is already there (bh_packed_kernel_body).  The dense
    form and the tag form, an open-addressing and a perfect-hash output table."""
    if not dense:
        monkeypatch.setenv("HDK_HIP_NO_BH_DENSE", "1")
    kernel = "hdk_scan_agg_bh_dense_plain" if dense else "hdk_scan_agg_bh_packed_plain"
    n = 3_000_000
    assert n >= 2.5 * E_FLUSH
    st, x, y = _e_table(n, 100, pattern, 65)
    for which, q in (("open", _bh_query("x")), ("perfect", _phs_query("x"))):
        res = _run(oracle, gpu_executor_factory, st, _plan(oracle, st, q), kernel, grid=1)
        _check_hot(res, _hot_expect(x, y), "key0" if which == "open" else "k")


@pytest.mark.parametrize("pattern", list(E_PATTERNS))
def test_packed_dense_partitions_flush_in_mid_kernel(oracle, gpu_executor_factory, monkeypatch, pattern):
    """Pass B of the range-bin form (hdk_bh_daggregate) has one block per bin and no grid to pin.  Three keys and the NULL key
    are four entries in two bins; pass A gives a bin eight sub-slabs of cap4 = (N / (2 x 8)) x 5 / 4 + 4 096 tuples and sends what
    does not fit -- a hot key's surplus -- through the exact path.  The hot bin's block therefore reads 8 x cap4 = 0.625 N + 32 768
    tuples: with N = 4.4 M (which is also beyond the 4 Mi rows at which the form is chosen) that is 2.78 M >= 2.5 x flush_rows,
    two folds in mid-kernel.  The route: an open-addressing table too large for tags in LDS (20 001 entries, forced), the dense
    one-pass forms switched off.

    The third kernel that reads flush_rows, hdk_bh_aggregate of the hash-bin form, has 256 bins whatever the table and sub-slabs
    of (N / 2 048) x 5 / 4 + 2 048 tuples: a block reads at most N / 205 + 16 384 tuples and needs N >= 211 M rows for its first
    fold in mid-kernel -- far beyond what a test of this suite may take; it is not covered here."""
    monkeypatch.setenv("HDK_HIP_NO_BH_DENSE", "1")
    n = 4_400_000
    cap4 = ((n // (2 * 8)) * 5 // 4 + 4096 + 3) & ~3
    hot = 1  # (entry 0 of bin 0)
    st, x, y = _e_table(n, 3, pattern, 66, hot=hot)
    assert (x == hot).sum() / 8 > 1.1 * cap4 and 8 * cap4 >= 2.5 * E_FLUSH
    q = _bh_query("x", force_baseline=True, baseline_entry_count=20_001)
    res = _run(oracle, gpu_executor_factory, st, _plan(oracle, st, q), "hdk_bh_dscatter")
    _check_hot(res, _hot_expect(x, y, hot=hot), "key0", hot=hot)
