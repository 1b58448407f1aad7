"""What hdk_hip_filter_columns must keep: a numpy three-valued evaluator over int64 words, written apart from the kernel
(values 1 / 0 / -1 for TRUE / FALSE / NULL instead of bit masks) and checked against SQLite in test_filter_columns_cpu.py.

A leaf is anything with the fields of hdk_hip_having_leaf (the `Leaf` below, or hdk_amd.plan.HavingLeaf); a program is
the postfix byte list of hdk_hip_plan::filter_ops, [] for the plain conjunction of all leaves."""
import operator
from collections import namedtuple

import numpy as np

from hdk_amd import _abi as A

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
NULL_DOUBLE_BITS = A.NULL_DOUBLE_BITS
TRUE, FALSE, NULL = 1, 0, -1

Leaf = namedtuple("Leaf", "lhs_col cmp rhs_is_col rhs_col rhs_lit cmp_fp lhs_is_fp lhs_nullable lhs_null_bits rhs_is_fp "
                          "rhs_nullable rhs_null_bits")
_OPS = {A.CMP_EQ: operator.eq, A.CMP_NE: operator.ne, A.CMP_LT: operator.lt, A.CMP_GT: operator.gt, A.CMP_LE: operator.le,
        A.CMP_GE: operator.ge}
SQL_OP = {A.CMP_EQ: "=", A.CMP_NE: "<>", A.CMP_LT: "<", A.CMP_GT: ">", A.CMP_LE: "<=", A.CMP_GE: ">="}


def dbits(x: float) -> int:
    return int(np.float64(x).view(np.int64))


def col_leaf(lhs, cmp, rhs, lhs_info=(False, False, 0), rhs_info=(False, False, 0)):
    """column lhs <cmp> column rhs; *_info = (is_fp, nullable, null_bits)"""
    return Leaf(lhs, cmp, True, rhs, 0, bool(lhs_info[0] or rhs_info[0]), bool(lhs_info[0]), bool(lhs_info[1]), lhs_info[2],
                bool(rhs_info[0]), bool(rhs_info[1]), rhs_info[2])


def lit_leaf(lhs, cmp, lit, lhs_info=(False, False, 0)):
    """column lhs <cmp> literal: a Python float compares as doubles, an int as int64 unless the column is fp"""
    fp = isinstance(lit, float) or lhs_info[0]
    return Leaf(lhs, cmp, False, 0, dbits(float(lit)) if fp else int(lit), bool(fp), bool(lhs_info[0]), bool(lhs_info[1]),
                lhs_info[2], bool(fp), False, 0)


def _side(words, is_fp, as_fp):
    if not as_fp:
        return words
    return words.view(np.float64) if is_fp else words.astype(np.float64)  # (double)int64, round to nearest even


def leaf_values(cols, lf) -> np.ndarray:
    """int8 per row: TRUE / FALSE / NULL"""
    a = np.ascontiguousarray(cols[lf.lhs_col], dtype=np.int64)
    null = (a == np.int64(lf.lhs_null_bits)) if lf.lhs_nullable else np.zeros(len(a), dtype=bool)
    if lf.rhs_is_col:
        b = np.ascontiguousarray(cols[lf.rhs_col], dtype=np.int64)
        if lf.rhs_nullable:
            null = null | (b == np.int64(lf.rhs_null_bits))
    else:
        b = np.full(len(a), lf.rhs_lit, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        t = _OPS[int(lf.cmp)](_side(a, lf.lhs_is_fp, lf.cmp_fp), _side(b, lf.rhs_is_fp, lf.cmp_fp))
    return np.where(null, NULL, np.where(t, TRUE, FALSE)).astype(np.int8)


def v_not(a):
    return np.where(a == NULL, NULL, 1 - a).astype(np.int8)


def v_and(a, b):
    return np.where((a == FALSE) | (b == FALSE), FALSE, np.where((a == NULL) | (b == NULL), NULL, TRUE)).astype(np.int8)


def v_or(a, b):
    return np.where((a == TRUE) | (b == TRUE), TRUE, np.where((a == NULL) | (b == NULL), NULL, FALSE)).astype(np.int8)


def evaluate(cols, leaves, prog) -> np.ndarray:
    vals = [leaf_values(cols, lf) for lf in leaves]
    if not len(prog):
        res = vals[0]
        for v in vals[1:]:
            res = v_and(res, v)
        return res
    stack = []
    for op in prog:
        if op < A.F_AND:
            stack.append(vals[op])
        elif op == A.F_NOT:
            stack.append(v_not(stack.pop()))
        else:
            b, a = stack.pop(), stack.pop()
            stack.append(v_and(a, b) if op == A.F_AND else v_or(a, b))
    assert len(stack) == 1
    return stack[0]


def expected_rows(cols, leaves, prog) -> np.ndarray:
    """indices of the rows on which the predicate is TRUE, ascending"""
    return np.flatnonzero(evaluate(cols, leaves, prog) == TRUE).astype(np.uint32)


# ---- trees: int = leaf index, ("and" | "or", a, b), ("not", a) ---------------------------------------------------
def postfix(tree) -> list:
    if isinstance(tree, int):
        return [tree]
    if tree[0] == "not":
        return postfix(tree[1]) + [A.F_NOT]
    return postfix(tree[1]) + postfix(tree[2]) + [A.F_AND if tree[0] == "and" else A.F_OR]


def random_tree(rng, num_leaves, depth):
    if depth == 0 or rng.random() < 0.25:
        return int(rng.integers(0, num_leaves))
    kind = ("and", "or", "not")[int(rng.integers(0, 3))]
    if kind == "not":
        return ("not", random_tree(rng, num_leaves, depth - 1))
    return (kind, random_tree(rng, num_leaves, depth - 1), random_tree(rng, num_leaves, depth - 1))


_INT_POOL = [INT64_MIN, INT64_MIN + 1, -1, 0, 1, 2, (1 << 53) + 1, INT64_MAX - 1, INT64_MAX]
_FP_POOL = [0.0, -0.0, 1.0, -1.0, 0.5, float("inf"), float("-inf"), float("nan"), 1e300, -2.5]


def random_case(rng, n, ncols=4, sql_safe=False):
    """-> (cols, infos, leaves, tree, prog).  cols: int64 words; infos[t] = (is_fp, nullable, null_bits).  Int and fp
    columns, nullable or not, literal and column-versus-column leaves, a random program of depth up to 3 (or, one time in
    five, the plain conjunction: prog == [], tree = the conjunction spelled out).  sql_safe: only int-versus-int and
    double-versus-double leaves over small exactly representable values (no NaN, infinities, signed zeros or sentinels as
    values), so that SQLite's numeric affinity cannot blur the comparison."""
    cols, infos = [], []
    for t in range(ncols):
        is_fp = bool(rng.integers(0, 2))
        nullable = bool(rng.integers(0, 2))
        null_bits = NULL_DOUBLE_BITS if is_fp else INT64_MIN
        if is_fp:
            v = rng.integers(-6, 7, n).astype(np.float64) / 2
            if not sql_safe:
                pool = np.array(_FP_POOL + [np.int64(NULL_DOUBLE_BITS).view(np.float64)])
                pick = rng.random(n) < 0.3
                v[pick] = pool[rng.integers(0, len(pool), int(pick.sum()))]
                if nullable:  # (a nullable column cannot hold its sentinel as a value)
                    v = np.where(v.view(np.int64) == NULL_DOUBLE_BITS, 0.25, v)
            w = v.view(np.int64).copy()
        else:
            w = rng.integers(-3, 4, n).astype(np.int64)
            if not sql_safe:
                pool = np.array(_INT_POOL, dtype=np.int64)
                pick = rng.random(n) < 0.3
                w[pick] = pool[rng.integers(0, len(pool), int(pick.sum()))]
                if nullable:
                    w[w == INT64_MIN] = 7
        if nullable:
            w[rng.random(n) < 0.2] = null_bits
        cols.append(w)
        infos.append((is_fp, nullable, null_bits))
    num_leaves = int(rng.integers(1, A.MAX_HAVING_LEAVES + 1))
    leaves = []
    for _ in range(num_leaves):
        lhs = int(rng.integers(0, ncols))
        cmp = int(rng.integers(A.CMP_EQ, A.CMP_GE + 1))
        same = [t for t in range(ncols) if infos[t][0] == infos[lhs][0]]
        if rng.random() < 0.4:
            rhs = int(rng.choice(same)) if sql_safe else int(rng.integers(0, ncols))
            leaves.append(col_leaf(lhs, cmp, rhs, infos[lhs], infos[rhs]))
            continue
        lit_fp = infos[lhs][0] if sql_safe else bool(rng.integers(0, 2))
        if lit_fp:
            lit = float(rng.integers(-6, 7)) / 2
            if not sql_safe and rng.random() < 0.3:
                lit = _FP_POOL[int(rng.integers(0, len(_FP_POOL)))]
        else:
            lit = int(rng.integers(-3, 4))
            if not sql_safe and rng.random() < 0.3:
                lit = _INT_POOL[int(rng.integers(0, len(_INT_POOL)))]
        leaves.append(lit_leaf(lhs, cmp, lit, infos[lhs]))
    if rng.random() < 0.2:
        tree = 0
        for k in range(1, num_leaves):
            tree = ("and", tree, k)
        return cols, infos, leaves, tree, []
    tree = random_tree(rng, num_leaves, 3)
    return cols, infos, leaves, tree, postfix(tree)
