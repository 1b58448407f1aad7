"""hdk_hip_project_columns on raw uploaded columns: computed columns over dense 8-byte columns in HBM.  The expectation
is tests/project_expect.py (numpy, checked against SQLite, the oracle and the truth tables in
test_project_columns_cpu.py).  Every case asserts every out word -- doubles bit for bit --, the error word, the poison
beyond num_rows and in a guard column, and an untouched input."""
import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import check, lib
from hdk_amd.plan import project_stack_depth

import project_expect as PE
from project_expect import bits, op
from test_project_columns_cpu import _Gen, _c_ops, _c_outs

pytestmark = pytest.mark.gpu

POISON64 = np.uint64(0x5A5A5A5A5A5A5A5A)
POISON_ERR = 0x5A5A5A5A
TILE = 1024  # rows per tile (hdk_amd/csrc/project_columns.hip: kPcTile)
N = 200_003
NULL_I, NULL_D = A.NULL_BIGINT, A.NULL_DOUBLE_BITS
NULL_I32 = -(1 << 31)  # INT32_MIN sign-extended: the NULL of a 4-byte slot in a dense column
I64_MAX, I64_MIN = 2**63 - 1, -2**63
D, O = A.ERR_DIV_BY_ZERO, A.ERR_OVERFLOW_OR_UNDERFLOW


@pytest.fixture(scope="module")
def mgr():
    from hdk_amd.hip_mgr import HipMgr
    return HipMgr()


def col(t, nullable=False, null=NULL_I, fp=False):
    return op(A.P_PUSH_COL, flags=(A.P_FLAG_NULLABLE if nullable else 0) | (A.P_FLAG_FP if fp else 0), col=t,
              imm=null if nullable else 0)


def lit(v):
    return op(A.P_PUSH_FP, imm=bits(v)) if isinstance(v, float) else op(A.P_PUSH_INT, imm=v)


def cmp_i(c):
    return op(A.P_CMP_I, flags=c)


def cmp_f(c):
    return op(A.P_CMP_F, flags=c)


def one_out(ops, fp=False):
    return [(0, len(ops), fp, True, NULL_D if fp else NULL_I)]


def run_project(mgr, cols, ops, outs, num_rows=None, with_error_word=True):
    """-> (out[(num_outs + 1), ocap] as uint64, the error word or None)"""
    L = lib()
    n, nc, no = (len(cols[0]) if num_rows is None else num_rows), len(cols), len(outs)
    cap, ocap = n + 3, n + 5
    host_in = np.full((nc, cap), 0x1111111111111111, dtype=np.int64)
    for t, c in enumerate(cols):
        host_in[t, :n] = c[:n]
    d_in = mgr.to_device(host_in.reshape(-1), 0)
    d_out = mgr.to_device(np.full((no + 1) * ocap, POISON64, dtype=np.uint64), 0)
    d_err = mgr.to_device(np.full(2, POISON_ERR, dtype=np.uint32), 0)  # a pre-poisoned error word and its neighbour
    try:
        check(L.hdk_hip_project_columns(d_in.ptr, cap, nc, n, _c_ops(ops), len(ops), _c_outs(outs), no, d_out.ptr, ocap,
                                        d_err.ptr if with_error_word else None, 0, None))
        mgr.synchronizeStream(0)
        out = mgr.to_host(d_out.ptr, (no + 1) * ocap * 8, 0, np.uint64).reshape(no + 1, ocap)
        err = mgr.to_host(d_err.ptr, 8, 0, np.uint32)
        back = mgr.to_host(d_in.ptr, nc * cap * 8, 0, np.int64).reshape(nc, cap)
    finally:
        for b in (d_in, d_out, d_err):
            b.free()
    assert np.array_equal(back, host_in), "the input was modified"
    assert int(err[1]) == POISON_ERR
    if not with_error_word:
        assert int(err[0]) == POISON_ERR
    return out, (int(err[0]) if with_error_word else None)


def check_case(mgr, cols, ops, outs, num_rows=None, with_error_word=True, want_err=None):
    cols = [np.ascontiguousarray(c).view(np.int64) for c in cols]
    n = len(cols[0]) if num_rows is None else num_rows
    words, nulls, code = PE.evaluate(cols, ops, outs, n)
    if want_err is not None:
        assert code == want_err, "the evaluator disagrees with the case"
    out, err = run_project(mgr, cols, ops, outs, n, with_error_word)
    if with_error_word:
        assert err == code
    for j, w in enumerate(words):
        if code == 0:  # (after an error the words are unspecified)
            bad = np.nonzero(out[j, :n].view(np.int64) != w)[0]
            assert bad.size == 0, (j, bad[:5], out[j, :n].view(np.int64)[bad[:5]], w[bad[:5]])
        assert (out[j, n:] == POISON64).all(), j
    assert (out[len(outs)] == POISON64).all(), "guard column"
    return words, nulls


# ---- row counts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, N])
def test_row_counts(mgr, n):
    rng = np.random.default_rng(n + 1)
    s = rng.integers(-10**6, 10**6, n).astype(np.int64)
    k = rng.integers(1, 100, n).astype(np.int64)
    s[rng.random(n) < 0.1] = NULL_I
    # s / k, cast(s as double) / k, and the guarded ratio x 100
    ops = [col(0, True), col(1), op(A.P_DIV_I)]
    ops2 = [col(0, True), op(A.P_CAST_I2F), col(1), op(A.P_CAST_I2F), op(A.P_DIV_F)]
    ops3 = [col(1), lit(50), cmp_i(A.CMP_EQ), op(A.P_PUSH_NULL_FP)] + ops2 + [op(A.P_SELECT), lit(100.0), op(A.P_MUL_F)]
    outs = [(0, 3, False, True, NULL_I), (3, 5, True, True, NULL_D), (8, len(ops3), True, True, NULL_D)]
    if n == 0:
        cols = [np.zeros(0, dtype=np.int64)] * 2
        out, err = run_project(mgr, cols, ops + ops2 + ops3, outs, 0)
        assert err == 0 and (out == POISON64).all()
        return
    check_case(mgr, [s, k], ops + ops2 + ops3, outs, want_err=0)


# ---- integer ops -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [0, 1, 2, 4, 8])
def test_integer_ops_at_the_bounds_of_each_check_width(mgr, width):
    w = width or 8
    top, bot = (1 << (8 * w - 1)) - 1, -(1 << (8 * w - 1))
    # (a, b, code): results exactly at the bounds pass, one beyond raises
    fits = {A.P_ADD_I: [(top - 1, 1), (bot + 1, -1), (top, 0), (bot, 0)],
            A.P_SUB_I: [(top - 1, -1), (bot + 1, 1), (-1, bot), (0, top)],
            A.P_MUL_I: [(top, 1), (bot, 1), (-(bot // 2), -2), (bot // 2, 2)]}
    over = {A.P_ADD_I: [(top, 1), (bot, -1)], A.P_SUB_I: [(top, -1), (bot, 1)],
            A.P_MUL_I: [(top // 2 + 1, 2), (bot, -1), (bot // 2 - 1, 2)]}
    for code in (A.P_ADD_I, A.P_SUB_I, A.P_MUL_I):
        prog = [col(0), col(1), op(code, width=width)]
        a = np.array([p[0] for p in fits[code]] * 50, dtype=np.int64)
        b = np.array([p[1] for p in fits[code]] * 50, dtype=np.int64)
        check_case(mgr, [a, b], prog, one_out(prog), want_err=0)
        for pa, pb in over[code]:
            a2, b2 = a.copy(), b.copy()
            a2[77], b2[77] = pa, pb
            check_case(mgr, [a2, b2], prog, one_out(prog), want_err=O if width else 0)
    # a NULL operand is not checked
    prog = [col(0, True), col(1), op(A.P_ADD_I, width=8)]
    check_case(mgr, [np.array([NULL_I, 5], dtype=np.int64), np.array([-1, 5], dtype=np.int64)], prog, one_out(prog), want_err=0)


def test_integer_division_and_modulo(mgr):
    a = np.array([I64_MIN, I64_MIN, I64_MIN, I64_MAX, 7, -7, 7, -7, 0, 5, I64_MIN + 1, 10**18], dtype=np.int64)
    b = np.array([-1, 1, 2, -1, 2, 2, -2, -2, 3, -1, -1, 7], dtype=np.int64)
    ops = [col(0), col(1), op(A.P_DIV_I), col(0), col(1), op(A.P_MOD_I)]
    words, _ = check_case(mgr, [a, b], ops, [(0, 3, False, False, 0), (3, 3, False, False, 0)], want_err=0)
    assert words[0][0] == I64_MIN and words[0][4:8].tolist() == [3, -3, -3, 3]
    assert words[1][0] == 0 and words[1][9] == 0 and words[1][4:8].tolist() == [1, -1, 1, -1]
    # NULL / 0 is NULL and raises nothing; a nullable 4-byte sentinel
    a = np.array([NULL_I32, 6, NULL_I32], dtype=np.int64)
    b = np.array([0, 3, 2], dtype=np.int64)
    prog = [col(0, True, NULL_I32), col(1), op(A.P_DIV_I)]
    words, nulls = check_case(mgr, [a, b], prog, one_out(prog), want_err=0)
    assert words[0].tolist() == [NULL_I, 2, NULL_I]
    check_case(mgr, [a, b], [col(0), col(1), op(A.P_MOD_I)], [(0, 3, False, False, 0)], want_err=D)


# ---- fp ops, casts and comparisons ---------------------------------------------------------------------------------------
def test_fp_ops_and_casts(mgr):
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999, -0.49999, -7.75, 1e15 + 0.5, -3.0, 0.0, -0.0, 123456.789, 1e-300, -2.25])
    y = np.array([3.0, -3.0, 0.1, 1e300, -1e-300, 7.0, 2.0, 0.3, -0.7, 1.0, 3.0, 5.0, 5.0, 1e10, 1e300, 1.5])
    ops = []
    outs = []
    for code in (A.P_ADD_F, A.P_SUB_F, A.P_MUL_F, A.P_DIV_F):
        outs.append((len(ops), 3, True, False, NULL_D))
        ops += [col(0, fp=True), col(1, fp=True), op(code)]
    outs.append((len(ops), 2, False, False, NULL_I))
    ops += [col(0, fp=True), op(A.P_CAST_F2I)]
    outs.append((len(ops), 3, True, False, NULL_D))
    ops += [col(0, fp=True), op(A.P_CAST_F2I), op(A.P_CAST_I2F)]
    words, _ = check_case(mgr, [x, y], ops, outs, want_err=0)
    assert words[4].tolist()[:9] == [1, -1, 2, -2, 3, -3, 0, 0, -8]
    # unfused: a * b + c rounds twice
    a = np.array([1.0 + 2.0**-30] * 8)
    c = np.array([-(1.0 + 2.0**-29)] * 8)
    prog = [col(0, fp=True), col(0, fp=True), op(A.P_MUL_F), col(1, fp=True), op(A.P_ADD_F)]
    words, _ = check_case(mgr, [a, c], prog, one_out(prog, True), want_err=0)
    assert words[0].view(np.float64)[0] == 0.0  # (an fma would leave 2^-60)
    # int64 -> double rounds to nearest even
    big = np.array([2**53 + 1, 2**53 + 3, -(2**53 + 1), I64_MAX, I64_MIN, 0], dtype=np.int64)
    prog = [col(0), op(A.P_CAST_I2F)]
    check_case(mgr, [big], prog, one_out(prog, True), want_err=0)
    # x / 0.0 and x / -0.0 raise; NULL / 0.0 does not
    z = np.array([1.0, 2.0, 0.0, 4.0])
    prog = [col(0, True, NULL_D, fp=True), col(1, fp=True), op(A.P_DIV_F)]
    check_case(mgr, [np.array([1.0, 2.0, 3.0, 4.0]), z], prog, one_out(prog, True), want_err=D)
    z[2] = -0.0
    check_case(mgr, [np.array([1.0, 2.0, 3.0, 4.0]), z], prog, one_out(prog, True), want_err=D)
    xs = np.array([1.0, 2.0, 3.0, 4.0]).view(np.int64).copy()
    xs[2] = NULL_D
    words, nulls = check_case(mgr, [xs, z], prog, one_out(prog, True), want_err=0)
    assert nulls[0].tolist() == [False, False, True, False] and words[0][2] == NULL_D


def test_comparisons_mixed_signed_zero_and_nan(mgr):
    nan = float("nan")
    x = np.array([0.0, -0.0, nan, 1.0, nan, 2.5, -1.0, 3.0])
    y = np.array([-0.0, 0.0, 1.0, nan, nan, 2.5, -2.0, 3.5])
    k = np.array([0, 0, 1, 1, 2, 2, -1, 3], dtype=np.int64)
    ops, outs = [], []
    for c in range(A.CMP_EQ, A.CMP_GE + 1):
        for prog in ([col(0, fp=True), col(1, fp=True), cmp_f(c)],                       # double with double
                     [col(2), op(A.P_CAST_I2F), col(0, fp=True), cmp_f(c)],              # int with double, through the cast
                     [col(2), lit(1), cmp_i(c)]):
            prog = prog + [lit(1), lit(0), op(A.P_SELECT)]
            outs.append((len(ops), len(prog), False, False, 0))
            ops += prog
        if len(outs) == 6:
            check_case(mgr, [x, y, k], ops, outs, want_err=0, with_error_word=False)
            ops, outs = [], []
    prog = [col(0, fp=True), col(1, fp=True), cmp_f(A.CMP_EQ), lit(1), lit(0), op(A.P_SELECT)]
    words, _ = check_case(mgr, [x, y, k], prog, [(0, 6, False, False, 0)], want_err=0)
    assert words[0].tolist() == [1, 1, 0, 0, 0, 1, 0, 0]  # -0.0 == +0.0; a NaN equals nothing
    prog[2] = cmp_f(A.CMP_NE)
    words, _ = check_case(mgr, [x, y, k], prog, [(0, 6, False, False, 0)], want_err=0)
    assert words[0].tolist() == [0, 0, 1, 1, 1, 0, 1, 1]


# ---- NULL sentinels ------------------------------------------------------------------------------------------------------
def test_null_sentinels_and_not_null_columns(mgr):
    a = np.array([NULL_I32, 1, NULL_I, 5, NULL_I32, 7] * 30, dtype=np.int64)
    f = np.array([1.5, 2.5, 3.5, 4.5, 5.5, 6.5] * 30).view(np.int64).copy()
    f[::4] = NULL_D
    ops, outs = [], []
    for prog, fp in (([col(0, True, NULL_I32), lit(1), op(A.P_ADD_I)], False),   # INT32_MIN sign-extended is NULL
                     ([col(0, True, NULL_I), lit(1), op(A.P_ADD_I)], False),     # INT64_MIN is NULL, INT32_MIN a value
                     ([col(0), lit(1), op(A.P_ADD_I)], False),                   # NOT NULL: both sentinels are values
                     ([col(1, True, NULL_D, fp=True), lit(2.0), op(A.P_MUL_F)], True),
                     ([col(1, fp=True), lit(2.0), op(A.P_MUL_F)], True),         # NOT NULL: DBL_MIN is a value
                     ([col(0, True, NULL_I32), op(A.P_IS_NULL), lit(1), lit(0), op(A.P_SELECT)], False),
                     ([col(0), op(A.P_IS_NULL), lit(1), lit(0), op(A.P_SELECT)], False),
                     ([col(1, True, NULL_D, fp=True), op(A.P_IS_NULL), op(A.P_NOT), col(0, True, NULL_I), op(A.P_PUSH_NULL_INT),
                       op(A.P_SELECT)], False)):
        outs.append((len(ops), len(prog), fp, True, NULL_D if fp else NULL_I))
        ops += prog
    words, nulls = check_case(mgr, [a, f], ops, outs, want_err=0)
    assert nulls[0][:6].tolist() == [True, False, False, False, True, False] and words[0][2] == I64_MIN + 1
    assert nulls[1][:6].tolist() == [False, False, True, False, False, False] and words[1][0] == NULL_I32 + 1
    assert not nulls[2].any() and words[2][2] == I64_MIN + 1 and words[2][0] == NULL_I32 + 1
    assert nulls[3][:5].tolist() == [True, False, False, False, True] and not nulls[4].any()
    assert words[4].view(np.float64)[0] == 2.0 * np.int64(NULL_D).view(np.float64)
    assert words[5][:6].tolist() == [1, 0, 0, 0, 1, 0] and not words[6].any()


# ---- CASE ----------------------------------------------------------------------------------------------------------------
def test_case_with_a_null_condition_and_nested_at_depth_six(mgr):
    rng = np.random.default_rng(4)
    n = 3000
    a = rng.integers(0, 4, n).astype(np.int64)
    b = rng.integers(-5, 6, n).astype(np.int64)
    a[rng.random(n) < 0.2] = NULL_I
    # CASE WHEN a = 1 THEN 10 ELSE 20 END: a NULL condition takes the ELSE
    prog = [col(0, True), lit(1), cmp_i(A.CMP_EQ), lit(10), lit(20), op(A.P_SELECT)]
    words, nulls = check_case(mgr, [a, b], prog, one_out(prog), want_err=0)
    assert (words[0][a == NULL_I] == 20).all() and not nulls[0].any()
    # CASE WHEN a = 0 THEN b WHEN a = 1 THEN NULL ELSE b * b END nests to the full stack: cond then cond then (b b MUL)
    nested = ([col(0, True), lit(0), cmp_i(A.CMP_EQ), col(1)] + [col(0, True), lit(1), cmp_i(A.CMP_EQ), op(A.P_PUSH_NULL_INT)]
              + [col(1), col(1), op(A.P_MUL_I, width=8)] + [op(A.P_SELECT), op(A.P_SELECT)])
    assert project_stack_depth(nested) == A.MAX_PROJECT_STACK
    words, nulls = check_case(mgr, [a, b], nested, one_out(nested), want_err=0)
    assert np.array_equal(nulls[0], a == 1) and (words[0][a == 0] == b[a == 0]).all()
    other = (a != 0) & (a != 1)  # 2, 3 and the NULLs
    assert (words[0][other] == b[other] ** 2).all()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_in_the_last_lane_of_the_last_partial_tile(mgr):
    rng = np.random.default_rng(8)
    s = rng.integers(-10**6, 10**6, N).astype(np.int64)
    k = rng.integers(1, 100, N).astype(np.int64)
    div = [col(0), col(1), op(A.P_DIV_I)]
    mul = [col(0), lit(1), op(A.P_MUL_I, width=4)]
    outs = [(0, 3, False, False, 0), (3, 3, False, False, 0)]
    assert (N - 1) // TILE == N // TILE and N % TILE != 0
    check_case(mgr, [s, k], div + mul, outs, want_err=0)  # a clean call: the pre-poisoned error word reads 0
    k0 = k.copy()
    k0[N - 1] = 0
    check_case(mgr, [s, k0], div + mul, outs, want_err=D)
    s7 = s.copy()
    s7[N - 1] = 2**31
    check_case(mgr, [s7, k], div + mul, outs, want_err=O)
    check_case(mgr, [s7, k0], div + mul, outs, want_err=O)  # both: the numerically largest
    s7[5], k0[N // 2] = -2**31 - 1, 0  # in other blocks too
    check_case(mgr, [s7, k0], div + mul, outs, want_err=O)
    # the same rows behind a CASE guard: no error, NULL outs
    gdiv = [col(1), lit(0), cmp_i(A.CMP_EQ), op(A.P_PUSH_NULL_INT)] + div + [op(A.P_SELECT)]
    gmul = ([col(0), lit(2**31 - 1), cmp_i(A.CMP_GT), col(0), lit(-2**31), cmp_i(A.CMP_LT), op(A.P_OR), op(A.P_PUSH_NULL_INT)] + mul
            + [op(A.P_SELECT)])
    outs = [(0, len(gdiv), False, True, NULL_I), (len(gdiv), len(gmul), False, True, NULL_I)]
    words, nulls = check_case(mgr, [s7, k0], gdiv + gmul, outs, want_err=0)
    assert np.nonzero(nulls[0])[0].tolist() == [N // 2, N - 1] and np.nonzero(nulls[1])[0].tolist() == [5, N - 1]
    assert words[0][N - 1] == NULL_I and words[1][N - 1] == NULL_I
    # an unmarked FALSE on the other side of an AND hides the error; a NULL does not
    hide = [col(1), lit(0), cmp_i(A.CMP_NE)] + div + [lit(0), cmp_i(A.CMP_GT), op(A.P_AND), lit(1), lit(0), op(A.P_SELECT)]
    check_case(mgr, [s, k0], hide, one_out(hide), want_err=0)
    nohide = [col(1, True, 0), lit(0), cmp_i(A.CMP_NE)] + hide[3:]  # (the zero reads as NULL on the guard's side only)
    check_case(mgr, [s, k0], nohide, one_out(nohide), want_err=D)


# ---- program shapes --------------------------------------------------------------------------------------------------------
def test_eight_outs_of_forty_eight_ops_over_one_column(mgr):
    rng = np.random.default_rng(9)
    v = rng.integers(-1000, 1000, 5000).astype(np.int64)
    ops, outs = [], []
    for j in range(8):
        prog = [col(0), lit(j + 1), op(A.P_MUL_I, width=8), col(0), op(A.P_ADD_I, width=8), op(A.P_CAST_I2F)]
        outs.append((len(ops), 6, True, False, NULL_D))
        ops += prog
    assert len(ops) == A.MAX_PROJECT_OPS
    check_case(mgr, [v], ops, outs, want_err=0)


def test_pass_through_literal_only_and_shared_op_ranges(mgr):
    rng = np.random.default_rng(10)
    n = 2500
    a = rng.integers(-9, 9, n).astype(np.int64)
    a[::7] = NULL_I32
    f = rng.normal(size=n).view(np.int64).copy()
    f[::5] = NULL_D
    # a pass-through copies the word unexamined: null_bits of the OUT differ from the column's sentinel on purpose
    ops = [col(0, True, NULL_I32), col(1, True, NULL_D, fp=True), lit(42), lit(2.5), op(A.P_PUSH_NULL_INT), col(0, True, NULL_I32),
           lit(0), op(A.P_ADD_I)]
    outs = [(0, 1, False, True, 777), (1, 1, True, True, 777), (2, 1, False, False, 0), (3, 1, True, False, 0),
            (4, 1, False, True, NULL_I), (5, 3, False, True, 777), (0, 1, False, False, 0)]
    words, nulls = check_case(mgr, [a, f], ops, outs, want_err=0, with_error_word=False)
    assert np.array_equal(words[0], a) and np.array_equal(words[1], f) and (words[2] == 42).all()
    assert (words[4] == NULL_I).all() and (words[5][::7] == 777).all() and np.array_equal(words[6], a)
    # eight distinct input columns in one call, the widest kernel
    cols = [rng.integers(-100, 100, n).astype(np.int64) for _ in range(9)]
    ops, outs = [], []
    for j in range(4):
        prog = [col(2 * j + 1), col(2 * j + 2), op(A.P_SUB_I, width=8)]
        outs.append((len(ops), 3, False, False, 0))
        ops += prog
    check_case(mgr, cols, ops, outs, want_err=0)


# ---- fuzz ------------------------------------------------------------------------------------------------------------------
def test_random_programs_against_the_evaluator(mgr):
    from test_project_columns_cpu import _sqlite_table
    cols, _ = _sqlite_table(20_000, seed=21)
    gen = _Gen(np.random.default_rng(22))
    ops, outs = [], []
    ran = 0
    for i in range(20):
        fp = i % 2 == 1
        prog, _ = (gen.fp_expr if fp else gen.int_expr)(3)
        assert project_stack_depth(prog) <= A.MAX_PROJECT_STACK
        if len(outs) == A.MAX_PROJECT_OUTS or len(ops) + len(prog) > A.MAX_PROJECT_OPS:
            check_case(mgr, cols, ops, outs, want_err=0)
            ran += len(outs)
            ops, outs = [], []
        outs.append((len(ops), len(prog), fp, True, NULL_D if fp else NULL_I))
        ops += prog
    check_case(mgr, cols, ops, outs, want_err=0)
    assert ran + len(outs) == 20
