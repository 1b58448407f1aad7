"""What hdk_hip_project_columns must write, in numpy, from the contract in include/hdk_hip.h and nothing else.

    evaluate(cols, ops, outs) -> (words, nulls, error code)

cols: one int64 array per input column (doubles as their bits); ops: (code, check_width, flags, col, imm) tuples; outs:
(first_op, num_ops, is_fp, nullable, null_bits) tuples.  words[j] is out j's int64 words (null_bits where the result is
NULL), nulls[j] its NULL rows, and the code is the numerically largest one that reaches an out (0: none).  Words on rows
that raise are unspecified in the contract; here they are whatever the arithmetic left.
"""
import numpy as np

from hdk_amd import _abi as A

INT, FP, BOOL = 0, 1, 2
I64_MIN = -2**63


def bits(x) -> int:
    """the int64 that holds the double x"""
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def op(code, width=0, flags=0, col=0, imm=0):
    return (code, width, flags, col, imm)


class _Val:
    def __init__(self, cls, v, nul, err):
        self.cls, self.v, self.nul, self.err = cls, v, nul, err  # int64 words / bool / int32 pending code per row


def _wrap(x):
    """python ints (object array) -> int64, two's complement"""
    return np.array([((int(t) + 2**63) % 2**64) - 2**63 for t in x], dtype=np.int64)


def _int_arith(code, a, b, width):
    """-> (wrapped result, overflow rows)"""
    exact = {A.P_ADD_I: lambda x, y: x + y, A.P_SUB_I: lambda x, y: x - y, A.P_MUL_I: lambda x, y: x * y}[code](
        a.astype(object), b.astype(object))
    if width == 0:
        return _wrap(exact), np.zeros(a.size, dtype=bool)
    lim = 1 << (8 * width - 1)
    ovf = np.array([t > lim - 1 or t < -lim for t in exact], dtype=bool) if a.size else np.zeros(0, dtype=bool)
    return _wrap(exact), ovf


def _trunc_div(a, b):
    """C division and remainder of int64 arrays, b neither 0 nor -1"""
    q = a // b
    r = a - q * b
    fix = (r != 0) & ((a < 0) != (b < 0))
    q = np.where(fix, q + 1, q)
    return q, a - q * b


_CMP = {A.CMP_EQ: np.equal, A.CMP_NE: np.not_equal, A.CMP_LT: np.less, A.CMP_GT: np.greater, A.CMP_LE: np.less_equal,
        A.CMP_GE: np.greater_equal}


def _run(cols, n, prog):
    st = []
    zeros = lambda dt: np.zeros(n, dtype=dt)  # noqa: E731
    for code, width, flags, col, imm in prog:
        if code == A.P_PUSH_COL:
            w = np.asarray(cols[col], dtype=np.int64)[:n]
            nul = (w == np.int64(imm)) if flags & A.P_FLAG_NULLABLE else zeros(bool)
            st.append(_Val(FP if flags & A.P_FLAG_FP else INT, w.copy(), nul, zeros(np.int32)))
        elif code in (A.P_PUSH_INT, A.P_PUSH_FP):
            st.append(_Val(INT if code == A.P_PUSH_INT else FP, np.full(n, imm, dtype=np.int64), zeros(bool), zeros(np.int32)))
        elif code in (A.P_PUSH_NULL_INT, A.P_PUSH_NULL_FP):
            st.append(_Val(INT if code == A.P_PUSH_NULL_INT else FP, zeros(np.int64), np.ones(n, dtype=bool), zeros(np.int32)))
        elif code in (A.P_ADD_I, A.P_SUB_I, A.P_MUL_I, A.P_DIV_I, A.P_MOD_I):
            b, a = st.pop(), st.pop()
            assert a.cls == b.cls == INT
            nul = a.nul | b.nul
            err = np.maximum(a.err, b.err)
            if code in (A.P_DIV_I, A.P_MOD_I):
                zero, m1 = b.v == 0, b.v == -1
                q, r = _trunc_div(a.v, np.where(zero | m1, 1, b.v))
                with np.errstate(over="ignore"):
                    v = np.where(m1, -a.v, q) if code == A.P_DIV_I else np.where(m1, 0, r)
                raised, what = zero & ~nul, A.ERR_DIV_BY_ZERO
            else:
                v, ovf = _int_arith(code, a.v, b.v, width)
                raised, what = ovf & ~nul, A.ERR_OVERFLOW_OR_UNDERFLOW
            st.append(_Val(INT, v, nul, np.where(raised, np.maximum(err, what), err).astype(np.int32)))
        elif code in (A.P_ADD_F, A.P_SUB_F, A.P_MUL_F, A.P_DIV_F):
            b, a = st.pop(), st.pop()
            assert a.cls == b.cls == FP
            x, y = a.v.view(np.float64), b.v.view(np.float64)
            nul = a.nul | b.nul
            err = np.maximum(a.err, b.err)
            with np.errstate(all="ignore"):
                v = {A.P_ADD_F: np.add, A.P_SUB_F: np.subtract, A.P_MUL_F: np.multiply, A.P_DIV_F: np.divide}[code](x, y)
            if code == A.P_DIV_F:
                err = np.where((y == 0.0) & ~nul, np.maximum(err, A.ERR_DIV_BY_ZERO), err).astype(np.int32)
            st.append(_Val(FP, np.ascontiguousarray(v).view(np.int64), nul, err))
        elif code == A.P_CAST_I2F:
            a = st.pop()
            assert a.cls == INT
            st.append(_Val(FP, a.v.astype(np.float64).view(np.int64), a.nul, a.err))
        elif code == A.P_CAST_F2I:
            a = st.pop()
            assert a.cls == FP
            d = a.v.view(np.float64)
            with np.errstate(all="ignore"):
                v = np.trunc(d + np.where(d < 0.0, -0.5, 0.5)).astype(np.int64)
            st.append(_Val(INT, v, a.nul, a.err))
        elif code in (A.P_CMP_I, A.P_CMP_F):
            b, a = st.pop(), st.pop()
            assert a.cls == b.cls == (INT if code == A.P_CMP_I else FP)
            x, y = (a.v, b.v) if code == A.P_CMP_I else (a.v.view(np.float64), b.v.view(np.float64))
            st.append(_Val(BOOL, _CMP[flags](x, y).astype(np.int64), a.nul | b.nul, np.maximum(a.err, b.err)))
        elif code in (A.P_AND, A.P_OR):
            b, a = st.pop(), st.pop()
            assert a.cls == b.cls == BOOL
            ta, tb = (a.v != 0) & ~a.nul, (b.v != 0) & ~b.nul
            fa, fb = (a.v == 0) & ~a.nul, (b.v == 0) & ~b.nul
            if code == A.P_AND:
                t = ta & tb
                nul = ~(t | fa | fb)
                decided = (fa & (a.err == 0)) | (fb & (b.err == 0))  # an unmarked FALSE decides alone
            else:
                t = ta | tb
                nul = ~t & (a.nul | b.nul)
                decided = (ta & (a.err == 0)) | (tb & (b.err == 0))
            st.append(_Val(BOOL, t.astype(np.int64), nul, np.where(decided, 0, np.maximum(a.err, b.err)).astype(np.int32)))
        elif code == A.P_NOT:
            a = st.pop()
            assert a.cls == BOOL
            st.append(_Val(BOOL, (a.v == 0).astype(np.int64), a.nul, a.err))
        elif code == A.P_IS_NULL:
            a = st.pop()
            st.append(_Val(BOOL, a.nul.astype(np.int64), zeros(bool), a.err))
        elif code == A.P_SELECT:
            e, t, c = st.pop(), st.pop(), st.pop()
            assert c.cls == BOOL and t.cls == e.cls
            take = (c.v != 0) & ~c.nul
            st.append(_Val(t.cls, np.where(take, t.v, e.v), np.where(take, t.nul, e.nul),
                           np.maximum(c.err, np.where(take, t.err, e.err)).astype(np.int32)))
        else:
            raise AssertionError(f"unknown code {code}")
    assert len(st) == 1 and st[0].cls != BOOL
    return st[0]


def evaluate(cols, ops, outs, num_rows=None):
    n = len(cols[0]) if num_rows is None else int(num_rows)
    words, nulls, worst = [], [], 0
    for first, count, is_fp, nullable, null_bits in outs:
        prog = ops[first:first + count]
        r = _run(cols, n, prog)
        assert (r.cls == FP) == bool(is_fp)
        if len(prog) == 1 and prog[0][0] == A.P_PUSH_COL:  # a pass-through: the word unexamined
            words.append(r.v.copy())
        else:
            words.append(np.where(r.nul, np.int64(null_bits), r.v))
        nulls.append(r.nul.copy())
        if n:
            worst = max(worst, int(r.err.max()))
    return words, nulls, worst
