"""Host copy of an output buffer -> rows / Arrow.

The reader side of the layout contract (reference omniscidb/ResultSet/): which entries are real
groups (ResultSetStorage::isEmptyEntry, ResultSetStorage.cpp:439-521), how slots become values
(ResultSetIteration.cpp: AVG = sum/count with NULL for count 0 -- load_avg_*,
RuntimeFunctions.cpp:1615-1653; in-band NULLs -> Arrow nulls) and ArrowResultSetConverter's column
naming/typing (ResultSet/ArrowResultSetConverter.cpp:825).  Pure numpy: the buffer is already on
the host (copyGroupByBuffersFromGpu, QueryMemoryInitializer.cpp:1250-1283).
"""
from typing import Dict, List

import numpy as np

from . import _abi as A
from .plan import CompiledPlan, align8, columnar_slot_offsets, describe_columns


def _slot_arrays(cp: CompiledPlan, buf: np.ndarray, entry_count: int) -> List[np.ndarray]:
    """One numpy array (length entry_count) per slot, sign-extended to int64."""
    p = cp.plan
    raw = buf.view(np.uint8)
    out = []
    if p.query_kind == A.Q_NON_GROUPED:
        return [buf[i:i + 1].astype(np.int64) for i in range(len(cp.slot_widths))]
    if p.output_columnar:
        for off, w in zip(columnar_slot_offsets(cp, entry_count), cp.slot_widths):
            if not w:  # zero-width slot (projected key of a baseline table): read from the key column
                out.append(None)
                continue
            dt = {8: np.int64, 4: np.int32, 2: np.int16, 1: np.int8}[w]  # (1 / 2: logical-sized MIN / MAX slots)
            out.append(raw[off:off + entry_count * w].view(dt).astype(np.int64))
        return out
    rb = int(p.row_size_quad) * 8
    rows = raw[:entry_count * rb].reshape(entry_count, rb)
    s = 0
    for ti in range(p.num_targets):
        tg = p.targets[ti]
        for k in range(2 if tg.agg == A.AGG_AVG else 1):
            off = tg.slot_off if k == 0 else tg.slot2_off
            w = cp.slot_widths[s]
            s += 1
            if not w:
                out.append(None)
                continue
            dt = np.int64 if w == 8 else np.int32
            out.append(np.ascontiguousarray(rows[:, off:off + w]).view(dt).reshape(-1).astype(np.int64))
    return out


def _key_arrays(cp: CompiledPlan, buf: np.ndarray, entry_count: int) -> List[np.ndarray]:
    p = cp.plan
    if p.keyless or p.query_kind == A.Q_NON_GROUPED:
        return []
    raw = buf.view(np.uint8)
    keys = []
    if p.output_columnar:
        stride = align8(entry_count * 8)
        for k in range(p.key_count):
            keys.append(raw[k * stride:k * stride + entry_count * 8].view(np.int64).copy())
        return keys
    rb = int(p.row_size_quad) * 8
    rows = raw[:entry_count * rb].reshape(entry_count, rb)
    kw = int(p.key_width)
    dt = np.int64 if kw == 8 else np.int32
    for k in range(p.key_count):
        keys.append(np.ascontiguousarray(rows[:, k * kw:(k + 1) * kw]).view(dt).reshape(-1).astype(np.int64))
    return keys


def non_empty_mask(cp: CompiledPlan, buf: np.ndarray, entry_count: int) -> np.ndarray:
    """ResultSetStorage::isEmptyEntry[Columnar] negated."""
    p = cp.plan
    if p.query_kind == A.Q_NON_GROUPED:
        return np.ones(1, dtype=bool)
    if p.keyless:
        ks = int(p.idx_target_as_key)
        slot = _slot_arrays(cp, buf, entry_count)[ks]
        iv = int(cp.init_vals[ks])
        if cp.slot_widths[ks] == 4:
            iv = int(np.int64(iv).astype(np.int32))
        return slot != iv
    k0 = _key_arrays(cp, buf, entry_count)[0]
    empty = A.EMPTY_KEY_64 if (p.key_width == 8 or p.output_columnar) else A.EMPTY_KEY_32
    return k0 != empty


def projection_arrays(cp: CompiledPlan, buf: np.ndarray, nrows: int, capacity=None):
    """(row positions, [one int64/float64 numpy array per projected column]) of a Projection buffer
    holding `nrows` rows (TOTAL_MATCHED)."""
    p = cp.plan
    n = int(capacity if capacity is not None else p.entry_count)
    raw = np.ascontiguousarray(buf).view(np.uint8)
    nrows = min(int(nrows), n)
    cols = []
    if p.output_columnar:
        pos = raw[:n * 8].view(np.int64)[:nrows].copy()
        for off, w in zip(columnar_slot_offsets(cp, n), cp.slot_widths):
            dt = {8: np.int64, 4: np.int32, 2: np.int16, 1: np.int8}[w]
            cols.append(raw[off:off + n * w].view(dt)[:nrows].astype(np.int64))
    else:
        rb = int(p.row_size_quad) * 8
        rows = raw[:n * rb].reshape(n, rb)[:nrows]
        pos = np.ascontiguousarray(rows[:, :8]).view(np.int64).reshape(-1)
        for ti in range(p.num_targets):
            off = p.targets[ti].slot_off
            cols.append(np.ascontiguousarray(rows[:, off:off + 8]).view(np.int64).reshape(-1))
    return pos, cols


def _projection_columns(cp: CompiledPlan, buf: np.ndarray, nrows: int, capacity=None) -> Dict[str, list]:
    p = cp.plan
    _, cols = projection_arrays(cp, buf, nrows, capacity)
    res: Dict[str, list] = {}
    for oc, arr in zip(cp.out_cols, cols):
        tg = p.targets[oc.target_idx]
        if tg.arg_is_fp:
            nullv = tg.arg.null_val
            vals = [None if (tg.arg.nullable and v == nullv) else float(np.int64(v).view(np.float64))
                    for v in arr.tolist()]
        else:
            # a narrow columnar slot holds the value truncated to its width: compare with the truncated NULL
            w = cp.slot_widths[oc.target_idx]
            nullv = int(tg.arg.null_val)
            if w < 8:
                nullv = int(np.int64(nullv).astype({4: np.int32, 2: np.int16, 1: np.int8}[w]))
            vals = [None if (tg.arg.nullable and v == nullv) else v for v in arr.tolist()]
            if oc.dictionary is not None:
                vals = [None if v is None else oc.dictionary[v] for v in vals]
            elif oc.scale:
                vals = [None if v is None else v / 10 ** oc.scale for v in vals]
        res[oc.name] = vals
    return res


def to_columns(cp: CompiledPlan, buf: np.ndarray, entry_count=None, nrows=None) -> Dict[str, list]:
    """Materialise result rows as {column name: python list} in entry order (None = NULL)."""
    p = cp.plan
    n = int(entry_count if entry_count is not None else p.entry_count)
    buf = np.ascontiguousarray(buf)
    if p.query_kind == A.Q_PROJECTION:
        return _projection_columns(cp, buf, n if nrows is None else nrows, n)
    mask = non_empty_mask(cp, buf, n)
    slots = _slot_arrays(cp, buf, n)
    keys = _key_arrays(cp, buf, n)
    first_slot = []
    s = 0
    for ti in range(p.num_targets):
        first_slot.append(s)
        s += 2 if p.targets[ti].agg == A.AGG_AVG else 1
    res: Dict[str, list] = {}
    for oc in cp.out_cols:
        tg = p.targets[oc.target_idx]
        fs = first_slot[oc.target_idx]
        # a projected key without a slot of its own comes from the key columns (target_groupby_indices)
        vals = (slots[fs] if slots[fs] is not None else keys[oc.key_idx])[mask]
        cnt = slots[fs + 1][mask] if oc.agg == "avg" else None
        res[oc.name] = _column_values(cp, oc, vals, cnt, cp.slot_widths[fs])
    return res


def _column_values(cp: CompiledPlan, oc, vals: np.ndarray, cnt, w: int) -> list:
    """One output column as a python list (None = NULL) from the values of its non-empty entries, in entry order: `vals`
    are the slot (or key) words sign-extended to int64 and `cnt` AVG's count slot -- what the host reader takes out of a
    buffer.  `w`: the slot's width in the buffer."""
    p = cp.plan
    tg = p.targets[oc.target_idx]
    if oc.kind == "key":
        kt = cp.key_types[oc.key_idx]
        nullv = kt.null_value()
        col = []
        if kt.is_fp:  # the key word holds the double's bits (groupByColumnCodegen's bit-cast, QE/IRCodegen.cpp:1219-1221)
            fv = np.ascontiguousarray(vals, dtype=np.int64).view(np.float64)
            # (a FLOAT key sits in the word widened to double, its NULL the widened FLOAT sentinel: makeTargetValue's case 8)
            null_bits = kt.null_as_int64_or_double_bits()
            if kt.size == 4:
                fv = fv.astype(np.float32).astype(np.float64)
            for v, f in zip(vals.tolist(), fv.tolist()):
                col.append(None if (kt.nullable and v == null_bits) else f)
            return col
        for v in vals.tolist():
            if kt.nullable and v == nullv:
                col.append(None)
            elif oc.dictionary is not None:
                col.append(oc.dictionary[v])
            else:
                col.append(v)
        return col
    if oc.agg == "count":
        return [int(v) for v in vals.tolist()]
    nullv = int(tg.null_val)
    if w == 4:
        nullv = int(np.int64(nullv).astype(np.int32))
    nullable = bool(tg.skip_null)
    float_slot = tg.arg_is_fp == A.FP_SLOT_FLOAT
    if float_slot:
        # takes_float_argument: the value is the float in the slot's low 4 bytes (ResultSetIteration.cpp:50-60,
        # actual_compact_sz = sizeof(float)); NULL when those bits are the float sentinel
        vals = (vals.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
        fvals = vals.view(np.float32).astype(np.float64)
        is_null = vals == np.uint32(A.NULL_FLOAT_BITS)
    if oc.agg == "avg":
        col = []
        for i, (sv, c) in enumerate(zip(vals.tolist(), cnt.tolist())):
            if c == 0:
                col.append(None)  # load_avg_*: null when count == 0
            elif float_slot:
                col.append(float(fvals[i]) / c)
            elif tg.arg_is_fp:
                col.append(float(np.int64(sv).view(np.float64)) / c)
            else:
                col.append(sv / c)
        # decimal arguments: AVG(decimal) is scaled back (ResultSetIteration.cpp pair_to_double)
        if oc.scale:
            col = [None if v is None else v / 10 ** oc.scale for v in col]
        return col
    col = []
    for i, v in enumerate(vals.tolist()):
        if float_slot:
            col.append(None if (nullable and is_null[i]) else float(fvals[i]))
        elif nullable and v == nullv:
            col.append(None)
        elif tg.arg_is_fp:
            col.append(float(np.int64(v).view(np.float64)))
        else:
            col.append(v)
    if oc.scale and oc.agg in ("sum", "min", "max"):
        col = [None if v is None else v / 10 ** oc.scale for v in col]
    return col


def dense_column_null(cp: CompiledPlan, target_idx: int):
    """(is_fp, nullable, null_bits) of target `target_idx`'s dense device column: how its 8-byte words compare (as doubles or
    as int64) and which word, if any, is its in-band NULL, as hdk_hip_columnarize_result writes it: a float accumulator widened
    to double bits (NULL_FLOAT -> NULL_DOUBLE for a nullable argument), AVG divided (NULL_DOUBLE for count 0; an AVG that
    comes out as exactly DBL_MIN would read as NULL: sums of that size do not occur).  plan.describe_columns restates it."""
    tg = cp.plan.targets[target_idx]
    if tg.agg == A.AGG_ID:
        kt = cp.key_types[tg.key_idx]
        nullv = kt.null_as_int64_or_double_bits() if kt.is_fp else kt.null_value()
        return bool(kt.is_fp), bool(kt.nullable), A.to_i64(nullv)
    if tg.agg == A.AGG_COUNT:
        return False, False, 0
    float_slot = tg.arg_is_fp == A.FP_SLOT_FLOAT
    if tg.agg == A.AGG_AVG or float_slot:
        return True, bool(tg.agg == A.AGG_AVG or tg.skip_null), A.NULL_DOUBLE_BITS
    first_slot = sum(2 if cp.plan.targets[t].agg == A.AGG_AVG else 1 for t in range(target_idx))
    nullv = int(tg.null_val)
    if cp.slot_widths[first_slot] == 4:
        nullv = int(np.int64(nullv).astype(np.int32))
    return bool(tg.arg_is_fp), bool(tg.skip_null), nullv


def dense_to_columns(cp: CompiledPlan, dense: List[np.ndarray]) -> Dict[str, list]:
    """to_columns() from dense device columns: dense[t] holds target t's 8-byte values (int64 words), one per group in
    entry order, as hdk_hip_columnarize_result writes them.  The same names, order, NULLs, dictionary strings and
    decimal scaling as to_columns() on the buffer the columns were made from."""
    return described_to_columns(describe_columns(cp), dense)


def rows_to_dense(cp: CompiledPlan, buf: np.ndarray, total_matched=None, positions: bool = False) -> List[np.ndarray]:
    """hdk_hip_columnarize_rows stated in numpy over a host copy of the buffer: one array of int64 words per dense column
    (describe_columns(cp, positions) describes them).  A projection: rows [0, min(max(total_matched, 0), entry_count)) of
    the buffer in their order, every slot sign-extended from its width, the row positions last when asked for.  A
    non-grouped result: one row; a float accumulator widened to double (NULL_FLOAT -> NULL_DOUBLE under skip_null), AVG
    as double(sum) / double(count) with NULL_DOUBLE for count 0, everything else the slot as it is."""
    p = cp.plan
    buf = np.ascontiguousarray(buf)
    if p.query_kind == A.Q_PROJECTION:
        n = int(p.entry_count)
        rows = min(max(int(total_matched), 0), n)
        pos, cols = projection_arrays(cp, buf, rows, n)
        cols = [np.ascontiguousarray(c, dtype=np.int64) for c in cols]
        return cols + [np.ascontiguousarray(pos, dtype=np.int64)] if positions else cols
    if p.query_kind != A.Q_NON_GROUPED:
        raise ValueError("rows_to_dense takes projections and non-grouped results; a group-by buffer has empty entries")
    if positions:
        raise ValueError("positions: only a projection has row positions")
    slots = buf.view(np.int64)
    out, s = [], 0
    for ti in range(p.num_targets):
        tg = p.targets[ti]
        a = slots[s:s + 1].copy()
        float_slot = tg.arg_is_fp == A.FP_SLOT_FLOAT and tg.agg not in (A.AGG_COUNT, A.AGG_ID)
        f32 = (a & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
        if tg.agg == A.AGG_AVG:
            cnt = int(slots[s + 1])
            dividend = f32.astype(np.float64) if float_slot else a.view(np.float64) if tg.arg_is_fp else a.astype(np.float64)
            with np.errstate(all="ignore"):
                v = dividend / np.float64(cnt) if cnt else np.array([A.NULL_DOUBLE_BITS], dtype=np.int64).view(np.float64)
            a = v.view(np.int64)
            s += 2
        else:
            if float_slot:
                if tg.skip_null and int(f32.view(np.uint32)[0]) == (A.NULL_FLOAT_BITS & 0xFFFFFFFF):
                    a = np.array([A.NULL_DOUBLE_BITS], dtype=np.int64)
                else:
                    a = f32.astype(np.float64).view(np.int64)
            s += 1
        out.append(np.ascontiguousarray(a, dtype=np.int64))
    return out


def to_arrow(cp: CompiledPlan, buf: np.ndarray, entry_count=None, nrows=None):
    return columns_to_arrow(cp, to_columns(cp, buf, entry_count, nrows))


def columns_to_arrow(cp: CompiledPlan, cols: Dict[str, list]):
    """{column name: python list} (to_columns / dense_to_columns) -> pyarrow.Table with the targets' names and types."""
    import pyarrow as pa
    arrays, names = [], []
    for oc in cp.out_cols:
        v = cols[oc.name]
        if oc.kind in ("key", "proj") and oc.dictionary is not None:
            arr = pa.array(v, type=pa.string())
        elif oc.agg == "count":
            arr = pa.array(v, type=pa.int32() if oc.type.size == 4 else pa.int64())
        elif oc.type.is_fp or oc.agg == "avg" or any(isinstance(x, float) for x in v):
            arr = pa.array(v, type=pa.float64())
        else:
            width = {1: pa.int8(), 2: pa.int16(), 4: pa.int32(), 8: pa.int64()}[oc.type.size]
            arr = pa.array(v, type=pa.int64() if oc.agg == "sum" else width)
        arrays.append(arr)
        names.append(oc.name)
    return pa.table(arrays, names=names)


def described_to_columns(schema, dense: List[np.ndarray]) -> Dict[str, list]:
    """to_columns() for dense columns by their description (plan.ColumnDesc; DeviceColumns.schema): dense[t] holds
    column t's int64 words.  None for a NULL word, a dictionary's string for a string id, a double for an fp column, a
    scaled decimal divided by 10 ** scale."""
    res = {}
    for d, words in zip(schema, dense):
        w = np.ascontiguousarray(words).view(np.int64)
        null = (w == np.int64(d.null_bits)).tolist() if d.nullable else [False] * len(w)
        if d.is_fp:
            vals = w.view(np.float64).tolist()
        elif d.dictionary is not None and d.agg != "count":
            vals = [None if z else d.dictionary[v] for v, z in zip(w.tolist(), null)]
        else:
            vals = w.tolist()
        col = [None if z else v for v, z in zip(vals, null)]
        if d.scale and d.agg != "count":
            col = [None if v is None else v / 10 ** d.scale for v in col]
        res[d.name] = col
    return res


def described_to_arrow(schema, cols: Dict[str, list]):
    """{column name: python list} of described_to_columns -> pyarrow.Table with the columns' names and types."""
    import pyarrow as pa
    arrays = []
    for d in schema:
        v = cols[d.name]
        if d.dictionary is not None and d.agg != "count":
            ty = pa.string()
        elif d.kind == "proj":  # (columns_to_arrow's rule for a projected column: a decimal shows as the doubles it holds)
            ty = pa.float64() if d.is_fp or any(isinstance(x, float) for x in v) else \
                {1: pa.int8(), 2: pa.int16(), 4: pa.int32(), 8: pa.int64()}[d.type.size]
        elif d.is_fp or (d.scale and d.agg != "count"):
            ty = pa.float64()
        elif d.agg == "count":
            ty = pa.int32() if d.type.size == 4 else pa.int64()
        elif d.agg == "sum":
            ty = pa.int64()
        else:
            ty = {1: pa.int8(), 2: pa.int16(), 4: pa.int32(), 8: pa.int64()}.get(d.type.size, pa.int64())
        arrays.append(pa.array(v, type=ty))
    return pa.table(arrays, names=[d.name for d in schema])
