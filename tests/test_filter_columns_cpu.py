"""hdk_hip_filter_columns without a device: the numpy expectation of the GPU tests against SQLite and the truth tables, the
host arithmetic and the argument checks of the C ABI, and the resolution of QueryUnit.having in compile_query."""
import ctypes as C
import dataclasses
import sqlite3

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd._lib import lib
from hdk_amd.ir import Agg, And, ColRef, Cmp, KeyRef, Lit, Not, Or, Proj, QueryMustRunOnCpu, QueryUnit, TargetRef
from hdk_amd.plan import Having, compile_query
from hdk_amd.storage import ArrowStorage

import having_expect as H


def _sql(tree, leaves):
    if isinstance(tree, int):
        lf = leaves[tree]
        if lf.rhs_is_col:
            rhs = f"c{lf.rhs_col}"
        else:
            rhs = repr(float(np.int64(lf.rhs_lit).view(np.float64))) if lf.rhs_is_fp else str(lf.rhs_lit)
        return f"(c{lf.lhs_col} {H.SQL_OP[lf.cmp]} {rhs})"
    if tree[0] == "not":
        return f"(NOT {_sql(tree[1], leaves)})"
    return f"({_sql(tree[1], leaves)} {tree[0].upper()} {_sql(tree[2], leaves)})"


@pytest.mark.parametrize("seed", range(8))
def test_evaluator_agrees_with_sqlite(seed):
    """SQLite's WHERE keeps the rows on which the predicate is TRUE and drops NULL and FALSE alike: the rule under test."""
    rng = np.random.default_rng(9100 + seed)
    n = 400
    for _ in range(6):
        cols, infos, leaves, tree, prog = H.random_case(rng, n, sql_safe=True)
        db = sqlite3.connect(":memory:")
        decl = ", ".join(f"c{t} {'REAL' if fp else 'INTEGER'}" for t, (fp, _, _) in enumerate(infos))
        db.execute(f"CREATE TABLE t (r INTEGER, {decl})")
        host = []
        for (fp, nullable, null_bits), w in zip(infos, cols):
            vals = w.view(np.float64).tolist() if fp else w.tolist()
            if nullable:
                vals = [None if b == null_bits else v for v, b in zip(vals, w.tolist())]
            host.append(vals)
        db.executemany(f"INSERT INTO t VALUES ({', '.join('?' * (len(cols) + 1))})", list(zip(range(n), *host)))
        want = [r for (r,) in db.execute(f"SELECT r FROM t WHERE {_sql(tree, leaves)} ORDER BY r")]
        db.close()
        assert H.expected_rows(cols, leaves, prog).tolist() == want, (seed, _sql(tree, leaves))


def test_truth_tables():
    T, F, N = H.TRUE, H.FALSE, H.NULL
    # nine rows: (a, b) over {TRUE, FALSE, NULL}^2, made by `c = 1` on nullable columns holding 1 / 0 / NULL
    word = {T: 1, F: 0, N: H.INT64_MIN}
    pairs = [(a, b) for a in (T, F, N) for b in (T, F, N)]
    cols = [np.array([word[a] for a, _ in pairs], dtype=np.int64), np.array([word[b] for _, b in pairs], dtype=np.int64)]
    info = (False, True, H.INT64_MIN)
    leaves = [H.lit_leaf(0, A.CMP_EQ, 1, info), H.lit_leaf(1, A.CMP_EQ, 1, info)]
    and_tab = {(T, T): T, (T, F): F, (T, N): N, (F, T): F, (F, F): F, (F, N): F, (N, T): N, (N, F): F, (N, N): N}
    or_tab = {(T, T): T, (T, F): T, (T, N): T, (F, T): T, (F, F): F, (F, N): N, (N, T): T, (N, F): N, (N, N): N}
    not_tab = {T: F, F: T, N: N}
    assert H.evaluate(cols, leaves, [0, 1, A.F_AND]).tolist() == [and_tab[p] for p in pairs]
    assert H.evaluate(cols, leaves, []).tolist() == [and_tab[p] for p in pairs]  # the plain conjunction
    assert H.evaluate(cols, leaves, [0, 1, A.F_OR]).tolist() == [or_tab[p] for p in pairs]
    assert H.evaluate(cols, leaves, [0, A.F_NOT]).tolist() == [not_tab[a] for a, _ in pairs]
    assert H.evaluate(cols, leaves, [0, 1, A.F_AND, A.F_NOT]).tolist() == [not_tab[and_tab[p]] for p in pairs]
    # only TRUE passes
    assert H.expected_rows(cols, leaves, [0, 1, A.F_OR, A.F_NOT]).tolist() == [i for i, p in enumerate(pairs) if or_tab[p] == F]


def test_double_comparisons_are_the_c_operators():
    nan, inf = float("nan"), float("inf")
    c = np.array([0.0, -0.0, nan, inf, -inf, 1.0], dtype=np.float64).view(np.int64)
    info = (True, False, 0)
    rows = lambda cmp, lit: H.expected_rows([c], [H.lit_leaf(0, cmp, lit, info)], []).tolist()
    assert rows(A.CMP_EQ, -0.0) == [0, 1]  # -0.0 == +0.0
    assert rows(A.CMP_NE, nan) == [0, 1, 2, 3, 4, 5] and rows(A.CMP_EQ, nan) == [] and rows(A.CMP_LE, nan) == []
    assert rows(A.CMP_NE, 1.0) == [0, 1, 2, 3, 4] and rows(A.CMP_LT, 1.0) == [0, 1, 4] and rows(A.CMP_GE, 1.0) == [3, 5]


# ---- the C ABI's host side -------------------------------------------------------------------------------------------
TILE = 4096
WS_BYTES_PER_ROW = 1 / 8 + 4 / TILE  # one pass bit a row, one 32-bit count a tile
WS_HEAD = TILE // 8 + 4 + 256  # a partly filled last tile, the total's counter, the counts rounded to 256 bytes


def test_workspace_is_monotone_and_bounded():
    L = lib()
    last = 0
    for n in [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 10 * TILE, 200_003, 1_100_003, 100_000_000, 2**32 - 1]:
        b = L.hdk_hip_filter_columns_workspace_bytes(n)
        assert b >= last and b % 8 == 0
        assert b <= n * WS_BYTES_PER_ROW + WS_HEAD, n
        assert b >= n / 8
        last = b


def _leaves(*specs):
    arr = (A.HavingLeaf * max(len(specs), 1))()
    for i, (lhs, cmp, rhs_is_col, rhs_col) in enumerate(specs):
        arr[i] = A.HavingLeaf(lhs, rhs_col, cmp, rhs_is_col, 0, 0, 0, 0, 0, 0, 0, 0, 5)
    return arr


def test_invalid_arguments_come_back_before_any_device():
    L = lib()
    one = _leaves((0, A.CMP_GT, 0, 0))
    two = _leaves((0, A.CMP_GT, 0, 0), (1, A.CMP_LT, 1, 0))
    ok_ptr = 4096  # (never dereferenced: every check comes first)

    def call(cols=ok_ptr, capacity=100, num_cols=2, num_rows=100, leaves=one, num_leaves=1, ops=(), out=1 << 30,
             out_capacity=100, row_count=8192, ws=None, ws_bytes=0):
        prog = (C.c_uint8 * max(len(ops), 1))(*ops)
        st = L.hdk_hip_filter_columns(cols, capacity, num_cols, num_rows, leaves, num_leaves, prog, len(ops), out, out_capacity,
                                      row_count, None, ws, ws_bytes, 0, None)
        return st, (L.hdk_hip_last_error() or b"").decode()

    for kw in ({"cols": None}, {"leaves": None}, {"row_count": None}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "NULL" in msg, kw
    for k in (0, 9, -1):
        st, msg = call(num_leaves=k)
        assert st == A.ERR_INVALID_ARG and "num_leaves" in msg
    for c in (-1, 2):
        st, msg = call(leaves=_leaves((c, A.CMP_GT, 0, 0)))
        assert st == A.ERR_INVALID_ARG and "column" in msg and "lhs" in msg
        st, msg = call(leaves=_leaves((0, A.CMP_GT, 1, c)))
        assert st == A.ERR_INVALID_ARG and "column" in msg and "rhs" in msg
    for cmp in (0, 7, 200):
        st, msg = call(leaves=_leaves((0, cmp, 0, 0)))
        assert st == A.ERR_INVALID_ARG and "cmp" in msg
    for ops, word in (((A.F_AND,), "underflow"), ((0, A.F_AND), "underflow"), ((A.F_NOT,), "underflow"), ((1,), "leaf index"),
                      ((0, 0), "depth"), ((0, 67), "unknown")):
        st, msg = call(ops=ops)
        assert st == A.ERR_INVALID_ARG and "program" in msg and word in msg, ops
    st, msg = call(leaves=two, num_leaves=2, ops=(0, 1, 2, A.F_AND, A.F_OR))
    assert st == A.ERR_INVALID_ARG and "leaf index" in msg
    st, msg = call(ops=(0,) + (A.F_NOT,) * 16)
    assert st == A.ERR_INVALID_ARG and "ops" in msg
    st, msg = call(num_rows=101)
    assert st == A.ERR_INVALID_ARG and "capacity" in msg
    st, msg = call(num_rows=2**32, capacity=2**33)
    assert st == A.ERR_INVALID_ARG and "32-bit" in msg
    st, msg = call(out=ok_ptr + 8)
    assert st == A.ERR_INVALID_ARG and "overlap" in msg
    st, msg = call(out=ok_ptr - 8, out_capacity=1)
    assert st == A.ERR_INVALID_ARG and "overlap" in msg
    need = L.hdk_hip_filter_columns_workspace_bytes(100)
    st, msg = call(ws=1 << 20, ws_bytes=need - 1)
    assert st == A.ERR_INVALID_ARG and "workspace" in msg
    st, msg = call(ws=(1 << 20) + 4, ws_bytes=need)
    assert st == A.ERR_INVALID_ARG and "aligned" in msg
    # every pair of blocks: cols [4096, 5696), out_cols 1600 bytes, row_count 8 bytes, the workspace `need` bytes
    for kw, names in (({"row_count": ok_ptr + 16}, ("row_count", "cols")), ({"row_count": (1 << 30) + 1592}, ("row_count", "out_cols")),
                      ({"ws": ok_ptr + 1024, "ws_bytes": need}, ("workspace", "cols")),
                      ({"ws": (1 << 30) - 8, "ws_bytes": need}, ("workspace", "out_cols")),
                      ({"ws": 8192 - need + 8, "ws_bytes": need}, ("workspace", "row_count"))):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "overlap" in msg and all(x in msg for x in names), (kw, msg)


def test_version_says_the_abi_grew():
    assert lib().hdk_hip_version() >= 1003
    assert A.MAX_HAVING_LEAVES == 8 and C.sizeof(A.HavingLeaf) == 40


# ---- plan level ------------------------------------------------------------------------------------------------------
def _storage():
    st = ArrowStorage()
    st.import_numpy("t", {"k": np.arange(100, dtype=np.int64) % 10, "v": np.arange(100, dtype=np.int64),
                          "f": np.arange(100, dtype=np.float64)})
    st.import_arrow(__import__("pyarrow").table({"s": ["a", "b", "a", "c"], "v": [1, 2, 3, 4]}), "d")
    return st


def _q(**kw):
    return QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s"), Agg("count", name="n"),
                                                          Agg("avg", ColRef("v"), "a"), Agg("min", ColRef("f"), "m")], **kw)


def test_defaults_leave_the_compiled_plan_alone():
    st = _storage()
    base = compile_query(st, _q())
    assert base.having is None and QueryUnit("t").having == []
    cp = compile_query(st, _q(having=[Cmp(TargetRef("n"), ">", Lit(3))]))
    assert bytes(base.plan) == bytes(cp.plan)  # nothing of the plan changes: HAVING happens on the result
    assert isinstance(cp.having, Having) and cp.having.prog == [] and len(cp.having.leaves) == 1


def test_names_indices_literals_and_programs_resolve():
    st = _storage()
    cp = compile_query(st, _q(having=[Cmp(TargetRef("n"), ">", Lit(3)), Cmp(TargetRef(3), "<", Lit(50)),
                                      Cmp(TargetRef("s"), ">=", TargetRef(2)), Cmp(TargetRef("s"), "<>", Lit(2.5))]))
    hv = cp.having
    assert hv.prog == []
    n_gt, a_lt, s_ge_n, s_ne = hv.leaves
    assert (n_gt.lhs_col, n_gt.cmp, n_gt.rhs_is_col, n_gt.rhs_lit, n_gt.cmp_fp, n_gt.lhs_nullable) == (2, A.CMP_GT, False, 3, False, False)
    # AVG is a nullable double column: an int literal is compared as a double
    assert (a_lt.lhs_col, a_lt.cmp_fp, a_lt.lhs_is_fp, a_lt.lhs_nullable, a_lt.lhs_null_bits) == (3, True, True, True, A.NULL_DOUBLE_BITS)
    assert a_lt.rhs_lit == H.dbits(50.0) and a_lt.rhs_is_fp and not a_lt.rhs_nullable
    assert (s_ge_n.lhs_col, s_ge_n.rhs_is_col, s_ge_n.rhs_col, s_ge_n.cmp, s_ge_n.cmp_fp) == (1, True, 2, A.CMP_GE, False)
    # a float literal against an int column: compared as doubles, the column converted
    assert (s_ne.cmp_fp, s_ne.lhs_is_fp, s_ne.rhs_is_fp, s_ne.rhs_lit) == (True, False, True, H.dbits(2.5))
    # literal on the left: swapped, the operator mirrored
    for op, mirrored in (("<", A.CMP_GT), (">", A.CMP_LT), ("<=", A.CMP_GE), (">=", A.CMP_LE), ("=", A.CMP_EQ), ("<>", A.CMP_NE)):
        lf = compile_query(st, _q(having=[Cmp(Lit(7), op, TargetRef("n"))])).having.leaves[0]
        assert (lf.lhs_col, lf.cmp, lf.rhs_is_col, lf.rhs_lit) == (2, mirrored, False, 7)
    # trees become a postfix program over the distinct leaves; the list is a conjunction
    a, b = Cmp(TargetRef("n"), ">", Lit(3)), Cmp(TargetRef("m"), "<", Lit(1.5))
    hv = compile_query(st, _q(having=[Or(Not(And(a, b)), a), b])).having
    assert len(hv.leaves) == 2 and hv.prog == [0, 1, A.F_AND, A.F_NOT, 0, A.F_OR, 1, A.F_AND]
    assert hv.leaves[1].lhs_is_fp and hv.leaves[1].cmp_fp


def test_compile_query_rejections():
    st = _storage()
    n_gt = Cmp(TargetRef("n"), ">", Lit(3))
    with pytest.raises(ValueError, match="nope"):
        compile_query(st, _q(having=[Cmp(TargetRef("nope"), ">", Lit(3))]))
    for idx in (5, -1):
        with pytest.raises(ValueError, match="index"):
            compile_query(st, _q(having=[Cmp(TargetRef(idx), ">", Lit(3))]))
    with pytest.raises(ValueError, match="index"):
        compile_query(st, _q(having=[Cmp(TargetRef("n"), ">", TargetRef(9))]))
    # not a group-by
    with pytest.raises(QueryMustRunOnCpu, match="group-by"):
        compile_query(st, QueryUnit("t", targets=[Agg("sum", ColRef("v"), "s")], having=[Cmp(TargetRef("s"), ">", Lit(3))]))
    with pytest.raises(QueryMustRunOnCpu, match="group-by"):
        compile_query(st, QueryUnit("t", targets=[Proj(ColRef("v"), "v")], having=[Cmp(TargetRef("v"), ">", Lit(3))]))
    # a dictionary-encoded target (its aggregate is fine)
    dq = lambda hv: QueryUnit("d", groupby=[ColRef("s")], targets=[KeyRef(0, "s"), Agg("count", name="n")], having=hv)
    with pytest.raises(QueryMustRunOnCpu, match="dictionary"):
        compile_query(st, dq([Cmp(TargetRef("s"), "=", Lit(1))]))
    with pytest.raises(QueryMustRunOnCpu, match="dictionary"):
        compile_query(st, dq([Cmp(TargetRef("n"), "=", TargetRef(0))]))
    compile_query(st, dq([n_gt]))
    # more than 8 leaves; a program that is too long
    with pytest.raises(QueryMustRunOnCpu, match="8"):
        compile_query(st, _q(having=[Cmp(TargetRef("n"), ">", Lit(i)) for i in range(9)]))
    deep = n_gt
    for _ in range(16):
        deep = Not(deep)
    with pytest.raises(QueryMustRunOnCpu, match="too long"):
        compile_query(st, _q(having=[deep]))
    # arithmetic, columns and constants inside a leaf
    for bad in (Cmp(TargetRef("n") + 1, ">", Lit(3)), Cmp(TargetRef("n"), ">", TargetRef("s") * 2), Cmp(ColRef("v"), ">", Lit(3)),
                Cmp(Lit(1), "<", Lit(3)), Cmp(TargetRef("n"), ">", ColRef("v"))):
        with pytest.raises(QueryMustRunOnCpu, match="arithmetic"):
            compile_query(st, _q(having=[bad]))


def test_target_refs_outside_having_are_told_so():
    st = _storage()
    for kw in ({"quals": [Cmp(TargetRef("n"), ">", Lit(3))]}, {"quals": [Not(Or(Cmp(ColRef("v"), ">", Lit(3)), Cmp(Lit(1), "<", TargetRef(0))))]},
               {"groupby": [TargetRef("k")]}, {"groupby": [ColRef("k") + TargetRef(1)]}):
        with pytest.raises(ValueError, match="only inside QueryUnit.having"):
            compile_query(st, dataclasses.replace(_q(), **kw))
    with pytest.raises(ValueError, match="only inside QueryUnit.having"):
        compile_query(st, QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", TargetRef("k"), "s")]))
    with pytest.raises(ValueError, match="only inside QueryUnit.having"):
        compile_query(st, QueryUnit("t", targets=[Proj(TargetRef(0), "v")]))


def test_decimal_targets_are_rejected():
    import decimal
    import pyarrow as pa
    st = ArrowStorage()
    st.import_arrow(pa.table({"k": pa.array([1, 2, 1], pa.int64()),
                              "d": pa.array([decimal.Decimal("1.50"), decimal.Decimal("2.25"), decimal.Decimal("3.00")],
                                            pa.decimal128(14, 2))}), "t")
    q = QueryUnit("t", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("d"), "s")],
                  having=[Cmp(TargetRef("s"), ">", Lit(2))])
    with pytest.raises(QueryMustRunOnCpu, match="decimal"):
        compile_query(st, q)
    # COUNT of a decimal is a plain count: its column has no scale (describe_columns), as after a regroup
    counted = dataclasses.replace(q, targets=[KeyRef(0, "k"), Agg("count", ColRef("d"), "n")], having=[Cmp(TargetRef("n"), ">", Lit(1))])
    assert compile_query(st, counted).having.leaves[0].lhs_col == 1


def test_buffer_result_with_having_is_an_error():
    from hdk_amd.executor import Executor
    ex = Executor.__new__(Executor)  # (the check comes before anything touches the device or the storage)
    q = _q(having=[Cmp(TargetRef("n"), ">", Lit(3))])
    with pytest.raises(ValueError, match="columns"):
        ex.execute(q, result="buffer")
    with pytest.raises(ValueError, match="columns"):
        ex.execute(q)


# (leaves as HavingLeaf's fields in order, program), written down from the resolver as it was when it read OutCols and
# result_set.dense_column_null: an fp target (fm, a), nullable ones (k32, m, a, s), a target on the right, a literal on the left
_RESOLVED = {
    "baseline_having_then_order_by_key": ([(0, 6, False, 0, 0, False, False, True, -2147483648, False, False, 0),
                                           (1, 6, False, 0, 15, False, False, False, 0, False, False, 0)], [0, 1, 64]),
    "baseline_nullable_k32_key_and_max": ([(0, 6, False, 0, 0, False, False, True, -2147483648, False, False, 0),
                                           (2, 4, False, 0, 10, False, False, True, -9223372036854775808, False, False, 0)], []),
    "everything_passes": ([(1, 6, False, 0, 1, False, False, False, 0, False, False, 0)], []),
    "float_min_against_a_float_literal": ([(1, 3, False, 0, -4598456694521987072, True, True, True, 4503599627370496, True, False, 0)], []),
    "having_order_limit_offset": ([(1, 4, False, 0, 18, False, False, False, 0, False, False, 0),
                                   (3, 3, False, 0, 4617315517961601024, True, True, True, 4503599627370496, True, False, 0)], []),
    "literal_on_the_left_or_not": ([(1, 4, False, 0, 25, False, False, False, 0, False, False, 0),
                                    (3, 6, False, 0, 0, True, True, True, 4503599627370496, True, False, 0),
                                    (0, 2, False, 0, 7, False, False, True, -9223372036854775808, False, False, 0)], [0, 1, 66, 65, 2, 64]),
    "nothing_passes": ([(1, 4, False, 0, 1000000, False, False, False, 0, False, False, 0)], []),
    "perfect_count_and_nullable_avg": ([(1, 4, False, 0, 18, False, False, False, 0, False, False, 0),
                                        (3, 3, False, 0, 4617315517961601024, True, True, True, 4503599627370496, True, False, 0)], []),
    "target_against_target": ([(2, 4, True, 1, 0, False, False, True, -9223372036854775808, False, False, 0)], []),
}


def test_resolve_having_gives_what_it_gave_from_out_cols():
    """resolve_having over describe_columns(cp) resolves the GPU suite's HAVINGs leaf for leaf and program for program as
    it did over cp.out_cols, and each leaf is the one having_expect builds from the column's (is_fp, nullable, null_bits)."""
    import test_gpu_having_queries as G
    from hdk_amd import result_set as rs
    from hdk_amd.plan import describe_columns, resolve_having, resolve_having_columns
    st = G._storage()
    assert sorted(G._QUERIES) == sorted(_RESOLVED)
    for name, q in G._QUERIES.items():
        cp = compile_query(st, q)
        hv = resolve_having(cp, q.having)
        assert ([dataclasses.astuple(lf) for lf in hv.leaves], hv.prog) == _RESOLVED[name], name
        assert hv == cp.having == resolve_having_columns(describe_columns(cp), q.having), name
        for lf in hv.leaves:
            info = rs.dense_column_null(cp, lf.lhs_col)
            if lf.rhs_is_col:
                want = H.col_leaf(lf.lhs_col, lf.cmp, lf.rhs_col, info, rs.dense_column_null(cp, lf.rhs_col))
            else:
                lit = float(np.int64(lf.rhs_lit).view(np.float64)) if lf.rhs_is_fp else lf.rhs_lit
                want = H.lit_leaf(lf.lhs_col, lf.cmp, lit, info)
            assert dataclasses.astuple(lf) == tuple(want), (name, lf)
