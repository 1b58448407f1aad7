"""Host side of the hot path: fragments -> device buffers -> kernel params -> launch -> result set.

Mirrors the reference's call chain for one execution step:
  Executor::fetchChunks            (QE/Execute.cpp:2965-3068)   -> `BufferCache.chunk`
  buildHashTableForQualifier       (QE/Execute.cpp:3692) + PerfectJoinHashTableBuilder::
      initHashTableOnGpu           (QE/JoinHashTable/Builders/PerfectHashTableBuilder.h:53-137)
                                                                -> `Executor._build_join_table`
  prepareKernelParams              (QE/QueryExecutionContext.cpp:788-964) -> `PreparedStep._params`
  createAndInitializeGroupByBufferGpu (QE/QueryMemoryInitializer.cpp:1054-1156) -> `init_output`
  DeviceKernel::launch             (QE/QueryExecutionContext.cpp:355)     -> `hdk_hip_launch`
  copyGroupByBuffersFromGpu        (:404-426) + aggregate_error_codes (:221-234) -> `fetch`
All compute goes through the C ABI; there is no CPU execution path in this package
(`device_type="CPU"` raises).
"""
import ctypes as C
import dataclasses
import itertools
from typing import Dict, List, Optional

import numpy as np

from . import _abi as A
from . import result_set
from ._lib import HdkHipError, check, lib, sync_switches
from .hip_mgr import DeviceBuffer, HipMgr
from .ir import QueryMustRunOnCpu, QueryUnit, Type
from .plan import (DEFAULT_MAX_GROUPS_BUFFER_ENTRY_GUESS, GROUP_KINDS, JOIN_TYPES, SETOP_CODES, SETOP_NAMES, ColumnDesc,
                   CompiledPlan, Having, columnar_init_vals, compact_init_vals, compile_query, describe_columns, eff_key_count, has_count_distinct, regroup_columns,
                   group_windows, is_row_unit, join_key_shape, resolve_having_columns, resolve_join_columns, resolve_order_by, resolve_select_columns,
                   resolve_setop_columns, resolve_window_columns, split_count_distinct, split_project_calls, split_row_unit)
from .storage import (DEFAULT_FRAGMENT_SIZE, ArrowStorage, Column, DeviceTable, registered_column_type,
                      stats_from_record)


class DeviceView:
    """A stretch of device memory that someone else owns: what BufferCache hands out for a storage.DeviceTable's chunks.
    Reads like a DeviceBuffer; free() does nothing."""

    def __init__(self, ptr: int, nbytes: int, device: int):
        self.ptr, self.nbytes, self.device = ptr, nbytes, device

    def free(self):
        pass


class BufferCache:
    """Device-resident chunks, keyed like DataMgr's GPU_LEVEL chunk cache (table, column, fragment).  The chunks of a
    storage.DeviceTable already are device-resident and belong to the table: chunk() / linearized() return a view of them
    computed from the table at hand and store nothing, so clear() never frees a table's block and a name that is
    registered again never serves the pointers of its predecessor."""

    def __init__(self, mgr: HipMgr, device_id: int):
        self.mgr, self.device_id = mgr, device_id
        self._chunks: Dict[tuple, DeviceBuffer] = {}

    def chunk(self, table, col_name, frag_idx) -> DeviceBuffer:
        if isinstance(table, DeviceTable):
            return DeviceView(table.device_chunk(col_name, frag_idx), table.frag_rows[frag_idx] * 8, table.device_id)
        key = (table.name, col_name, frag_idx)
        b = self._chunks.get(key)
        if b is None:
            b = self.mgr.to_device(table.columns[col_name].fragments[frag_idx], self.device_id)
            self._chunks[key] = b
        return b

    def linearized(self, table, col_name) -> DeviceBuffer:
        """All fragments of an inner-join column as one buffer (ColumnFetcher::linearizeColumnFragments)."""
        if isinstance(table, DeviceTable):  # (its columns are contiguous)
            return DeviceView(table.device_column(col_name), table.num_rows * 8, table.device_id)
        key = (table.name, col_name, "all")
        b = self._chunks.get(key)
        if b is None:
            frags = table.columns[col_name].fragments
            arr = frags[0] if len(frags) == 1 else np.concatenate(frags)
            b = self.mgr.to_device(arr, self.device_id)
            self._chunks[key] = b
        return b

    def put(self, key, buf: DeviceBuffer):
        self._chunks[key] = buf

    def clear(self):
        for b in self._chunks.values():
            b.free()
        self._chunks.clear()

    def nbytes(self):
        return sum(b.nbytes for b in self._chunks.values())


class ExecutionResult:
    """Host ResultSet + its layout; `to_arrow()` like pyhdk's ExecutionResult (_sql.pyx:76-83)."""

    def __init__(self, cp: CompiledPlan, buf: np.ndarray, entry_count: int, error_code: int = 0,
                 total_matched: Optional[int] = None):
        self.compiled = cp
        self.buffer = buf
        self.entry_count = entry_count
        self.error_code = error_code
        self.total_matched = total_matched  # projection: rows claimed (TOTAL_MATCHED)

    def to_arrow(self):
        return result_set.to_arrow(self.compiled, self.buffer, self.entry_count, self.total_matched)

    def to_columns(self):
        return result_set.to_columns(self.compiled, self.buffer, self.entry_count, self.total_matched)

    def row_count(self):
        if self.compiled.plan.query_kind == A.Q_PROJECTION:
            return min(int(self.total_matched or 0), self.entry_count)
        return int(result_set.non_empty_mask(self.compiled, self.buffer, self.entry_count).sum())


# below this many bytes of worst-case output (num_targets x rows x 8) dense columns are made in ONE call into a block of
# the worst-case row count; above it the rows are counted first and the block is sized exactly
ONE_CALL_BYTES = 64 << 20


def sized_columns(mgr, device_id, num_targets, worst_rows, call, one_call_bytes, drop_empty=False, max_rows=None):
    """Run a stage that writes dense columns and a row count -> (block, capacity, rows).
    `call(out_ptr, capacity, row_count_ptr)` enqueues the stage; out_ptr None with capacity 0 only counts.  The count is
    read back after one stream synchronisation per call.  `drop_empty`: no block when no row came back.  The floor of 8
    bytes on the worst-case block is fetch_columns' (a table of no entries); filter() never gets there with no rows.
    `max_rows`: a count above it raises HdkHipError(ERR_OUT_OF_GPU_MEM) before the exactly sized block is allocated (a
    join's output has no worst case to check beforehand)."""
    d_rows = mgr.alloc(8, device_id)
    block = None

    def run(out_ptr, capacity):
        call(out_ptr, capacity, d_rows.ptr)
        mgr.synchronizeStream(device_id)
        return int(mgr.to_host(d_rows.ptr, 8, device_id, np.uint64)[0])

    try:
        if num_targets * worst_rows * 8 <= one_call_bytes:
            block = mgr.alloc(max(num_targets * worst_rows * 8, 8), device_id)
            capacity = worst_rows
            rows = run(block.ptr, capacity)
        else:
            rows = capacity = run(None, 0)
            if max_rows is not None and rows > max_rows:
                raise HdkHipError(A.ERR_OUT_OF_GPU_MEM, f"the stage has {rows} output rows; at most {max_rows} are materialised")
            if rows:
                block = mgr.alloc(num_targets * rows * 8, device_id)
                run(block.ptr, capacity)
        if drop_empty and rows == 0 and block is not None:
            block.free()
            block, capacity = None, 0
    except Exception:
        if block is not None:
            block.free()
        raise
    finally:
        d_rows.free()
    return block, capacity, rows


def _device_error(err: int) -> HdkHipError:
    return HdkHipError(err, f"device error code {err} (QE/Execute.h:1019-1031)")


def _stage(cols, apply, keep=None):
    """One stage over dense columns: apply(cols) -> the next columns.  `cols` is handed back whether the stage returned or
    raised, unless it is `keep`."""
    try:
        return apply(cols)
    finally:
        if cols is not keep:
            cols.free()


def run_stages(cols, having=None, windows=(), select=(), order_by=(), limit=None, offset=0, joins=(), setops=()):
    """What a unit asks for above its GROUP BY, applied where the columns are: the joins with other results (ir.ResultJoin,
    in order; their right sides are not consumed), then HAVING (a plan.Having or conditions), which may read a joined
    column, the window functions, which may read what HAVING kept, the select list, which may read a window column, the
    set operations with other results (ir.ResultSetOp, in order; their right sides are not consumed), then the SortInfo,
    which names the columns it meets and orders the COMBINED rows.  Consumes `cols`: each stage reads the result of the
    one before, whose block is handed back, also when a stage raises.  -> the last result; `cols` itself when nothing
    applies."""
    for j in joins:
        cols = _stage(cols, lambda c: c.join(j.right, j.left_on, j.right_on, j.type, j.null_safe, j.right_cols))
    if having:
        cols = _stage(cols, lambda c: c.filter(having))
    if windows:
        cols = _stage(cols, lambda c: c.windows(windows))
    if select:
        cols = _stage(cols, lambda c: c.project(select))
    for so in setops:
        cols = _stage(cols, lambda c: c.setop(so.right, so.op, so.all))
    if order_by or limit is not None or offset:
        cols = _stage(cols, lambda c: c.sort(order_by, limit, offset))
    return cols


class DeviceColumns:
    """Dense result columns in device memory: what hdk_hip_columnarize_result made of a group-by buffer (the device form
    of the reference's ColumnarResults for a ResultSet that lives in HBM).  One 8-byte column per target, rows in entry
    order -- the order ExecutionResult.to_columns() gives.  Owns its device block until free().
    It always carries a schema, one plan.ColumnDesc per column: plan.describe_columns(cp) for a result made from a plan,
    and what group_by / window / project made of their input's otherwise.  `compiled` is the plan it descends from, kept
    for reference only."""

    def __init__(self, cp: CompiledPlan, mgr: HipMgr, device_id: int, block: Optional[DeviceBuffer], capacity: int,
                 num_rows: int, error_code: int = 0, schema: Optional[List[ColumnDesc]] = None):
        self.compiled, self.mgr, self.device_id = cp, mgr, device_id
        self.block, self.capacity, self.num_rows, self.error_code = block, int(capacity), int(num_rows), error_code
        self.schema = list(schema) if schema is not None else describe_columns(cp)

    @property
    def num_cols(self) -> int:
        return len(self.schema)

    def columns(self) -> List[ColumnDesc]:
        """One ColumnDesc per column."""
        return list(self.schema)

    def _like(self, block, capacity, num_rows, schema=None) -> "DeviceColumns":
        """A result of these columns: their schema unless the stage made a new one."""
        return DeviceColumns(self.compiled, self.mgr, self.device_id, block, capacity, num_rows, self.error_code,
                             self.schema if schema is None else schema)

    def _column_null(self, t: int):
        """(is_fp, nullable, null_bits) of column t; t < 0 is no column (COUNT(*)): nothing to compare"""
        if t < 0:
            return False, False, 0
        d = self.schema[t]
        return d.is_fp, d.nullable, d.null_bits

    def _block_ptr(self) -> int:
        if self.block is None or not self.block.ptr:
            raise ValueError("the columns have been freed")
        return self.block.ptr

    def device_ptr(self, target_idx: int) -> int:
        """Device address of target `target_idx`'s column: num_rows 8-byte values."""
        if not 0 <= target_idx < self.num_cols:
            raise IndexError(target_idx)
        return self._block_ptr() + target_idx * self.capacity * 8

    def _is_fp(self, target_idx: int) -> bool:
        return bool(self.schema[target_idx].is_fp)

    def _order_entries(self, entries):
        """(column, desc, nulls_first) triples as the library's array"""
        arr = (A.OrderEntry * len(entries))()
        for i, (t, desc, nulls_first) in enumerate(entries):
            is_fp, nullable, null_bits = self._column_null(t)
            arr[i] = A.OrderEntry(t, int(desc), int(nulls_first), int(is_fp), int(nullable), A.to_i64(null_bits))
        return arr

    def _copy_rows(self, block: DeviceBuffer, first: int, rows: int):
        """rows [first, first + rows) of every column into `block`, which holds `rows` rows per column"""
        for t in range(self.num_cols):
            self.mgr.copyDeviceToDevice(block.ptr + t * rows * 8, self.device_ptr(t) + first * 8, rows * 8, self.device_id,
                                        self.device_id)

    def to_host(self) -> List[np.ndarray]:
        """One numpy array of num_rows values per target: float64 for fp values (AVG, fp aggregates, fp keys), int64
        for everything else.  NULLs stay in band (the slot's sentinel sign-extended; NULL_DOUBLE for fp values)."""
        nt = self.num_cols
        n = self.num_rows
        if n == 0:
            return [np.empty(0, dtype=np.float64 if self._is_fp(t) else np.int64) for t in range(nt)]
        if self.capacity == n:  # exactly sized: one copy
            flat = self.mgr.to_host(self.device_ptr(0), nt * n * 8, self.device_id, np.int64)
            cols = [flat[t * n:(t + 1) * n] for t in range(nt)]
        else:
            cols = [self.mgr.to_host(self.device_ptr(t), n * 8, self.device_id, np.int64) for t in range(nt)]
        return [c.view(np.float64) if self._is_fp(t) else c for t, c in enumerate(cols)]

    def to_columns(self):
        return result_set.described_to_columns(self.schema, [c.view(np.int64) for c in self.to_host()])

    def to_arrow(self):
        return result_set.described_to_arrow(self.schema, self.to_columns())

    def row_count(self):
        return self.num_rows

    def sort(self, order_by, limit: Optional[int] = None, offset: int = 0, no_select: bool = False) -> "DeviceColumns":
        """ORDER BY `order_by` LIMIT `limit` OFFSET `offset` on the device (hdk_hip_sort_columns; the reference's
        ResultSet::sort, QE/ResultSetSort.cpp:64-188) -> a new DeviceColumns that owns a block of exactly the output
        rows; this object stays valid.  `order_by`: ir.OrderEntry items (target index or output name) or resolved
        (target index, desc, nulls_first) triples.  Ties keep their order in this object.  Without `order_by` the result
        is rows [offset, offset + limit) as they are: one copy per column, no sort.  no_select=True forces the full sort
        where a LIMIT would select the candidates first (HDK_HIP_SORT_NO_SELECT)."""
        if (limit is not None and limit < 0) or offset < 0:
            raise ValueError("limit and offset must not be negative")
        nt = self.num_cols
        entries = [e if isinstance(e, tuple) else None for e in order_by]
        if any(e is None for e in entries):
            entries = resolve_order_by(self.schema, nt, list(order_by))
        n = self.num_rows
        after = max(n - int(offset), 0)
        out_rows = after if not limit else min(int(limit), after)
        if limit == 0:  # (LIMIT 0 is no row; the C ABI's 0 means "no limit")
            out_rows = 0
        if out_rows == 0:
            return self._like(None, 0, 0)
        src = self._block_ptr()
        block = self.mgr.alloc(nt * out_rows * 8, self.device_id)
        try:
            if not entries:
                self._copy_rows(block, int(offset), out_rows)
            else:
                arr = self._order_entries(entries)
                check(lib().hdk_hip_sort_columns(src, self.capacity, nt, n, arr, len(entries), int(offset),
                                                 out_rows if limit else 0, A.SORT_NO_SELECT if no_select else 0, block.ptr,
                                                 out_rows, None, None, 0, self.device_id, None))
            self.mgr.synchronizeStream(self.device_id)
        except Exception:
            block.free()
            raise
        return self._like(block, out_rows, out_rows)

    FILTER_ONE_CALL_BYTES = ONE_CALL_BYTES

    def filter(self, having) -> "DeviceColumns":
        """HAVING on the device (hdk_hip_filter_columns; the reference's filter step over the previous step's result) ->
        a new DeviceColumns with the rows on which the predicate is TRUE, in this object's order; this object stays
        valid.  `having`: a Cond tree or a list of them (a conjunction) over ir.TargetRef / ir.Lit, or the resolved
        plan.Having.  Sizing as fetch_columns(): up to 64 MiB of worst-case output one call writes into a block of
        num_rows rows per column; above that the passing rows are counted first (out_cols = NULL) and the block holds
        exactly those.  One stream synchronisation per call, to read row_count back."""
        if not isinstance(having, Having):
            having = resolve_having_columns(self.schema, list(having) if isinstance(having, (list, tuple)) else [having])
        nt = self.num_cols
        n = self.num_rows
        if n == 0 or having is None:
            if having is None and n:
                return self.sort([])  # no predicate: every row, copied
            return self._like(None, 0, 0)
        src = self._block_ptr()
        leaves = (A.HavingLeaf * len(having.leaves))()
        for i, lf in enumerate(having.leaves):
            leaves[i] = A.HavingLeaf(lf.lhs_col, lf.rhs_col, lf.cmp, int(lf.rhs_is_col), int(lf.cmp_fp), int(lf.lhs_is_fp),
                                     int(lf.lhs_nullable), int(lf.rhs_is_fp), int(lf.rhs_nullable), 0,
                                     A.to_i64(lf.lhs_null_bits), A.to_i64(lf.rhs_null_bits), A.to_i64(lf.rhs_lit))
        ops = (C.c_uint8 * max(len(having.prog), 1))(*having.prog)

        def call(out_ptr, capacity, row_count_ptr):
            check(lib().hdk_hip_filter_columns(src, self.capacity, nt, n, leaves, len(having.leaves), ops,
                                               len(having.prog), out_ptr, capacity, row_count_ptr, None, None, 0,
                                               self.device_id, None))

        block, capacity, rows = sized_columns(self.mgr, self.device_id, nt, n, call, self.FILTER_ONE_CALL_BYTES,
                                              drop_empty=True)
        return self._like(block, capacity, rows)

    GROUP_ONE_CALL_BYTES = ONE_CALL_BYTES

    def group_by(self, keys, outs, presorted: bool = False) -> "DeviceColumns":
        """GROUP BY `keys` over these columns on the device (hdk_hip_group_columns; the device form of the reference's
        merge of partial results, QE/ResultSetReduction.cpp reduceOneSlot) -> a new DeviceColumns with one row per
        distinct key and one column per out, which carries its own schema; this object stays valid.  `keys`: columns by
        index or name.  `outs`: (kind, target, name) with kind in id / count / sum / min / max, target None for COUNT(*)
        and name None for a default (plan.regroup_columns has the rules for type and nullability).  The library groups
        ADJACENT rows: unless `presorted` says that rows with equal keys already are, a copy sorted by the keys is made
        first (hdk_hip_sort_columns, no limit) and freed afterwards.  Rows come out in that order: ascending by the
        keys, NULLs last.  Sizing as filter(): up to 64 MiB of worst-case output in one call, else count first."""
        key_cols, spec, descs = regroup_columns(self.schema, keys, outs)
        out = self._like(None, 0, 0, descs)
        n = self.num_rows
        if n == 0:
            return out
        self._block_ptr()
        src = self if presorted else self.sort([(k, False, False) for k in key_cols])
        try:
            nc = self.num_cols
            kc = (C.c_int32 * len(key_cols))(*key_cols)
            arr = (A.GroupOut * len(spec))()
            for j, (kind, t) in enumerate(spec):
                is_fp, nullable, null_bits = self._column_null(t)
                arr[j] = A.GroupOut(t, GROUP_KINDS[kind], int(is_fp), int(nullable), 0, A.to_i64(null_bits))

            def call(out_ptr, capacity, row_count_ptr):
                check(lib().hdk_hip_group_columns(src.block.ptr, src.capacity, nc, n, kc, len(key_cols), arr, len(spec), out_ptr,
                                                  capacity, row_count_ptr, None, 0, self.device_id, None))

            out.block, out.capacity, out.num_rows = sized_columns(self.mgr, self.device_id, len(spec), n, call,
                                                                  self.GROUP_ONE_CALL_BYTES, drop_empty=True)
        finally:
            if src is not self:
                src.free()
        return out

    def window(self, partition_by, order_by, outs, presorted: bool = False) -> "DeviceColumns":
        """Window functions OVER (PARTITION BY `partition_by` ORDER BY `order_by`) on the device (hdk_hip_window_columns;
        the reference's WindowFunctionContext, QE/WindowContext.cpp) -> a new DeviceColumns that carries a schema: these
        columns followed by one column per out, every input row once; this object stays valid.  `partition_by`: columns
        by index, name or ir.TargetRef; `order_by`: ir.OrderEntry items; `outs`: ir.Window items, of which kind, arg,
        frame, param and name are read (plan.resolve_window_columns has the rules for type and nullability).  The library
        reads ADJACENT rows: unless `presorted` says that the rows already are in that order, they are ordered by the
        partition keys ascending with NULLs last, then by `order_by` (hdk_hip_sort_columns, stable), straight into the
        first columns of the one block that also holds the window columns, which the library writes.  More outs than one
        call takes go through further calls over the same sorted columns."""
        part_cols, order, spec, descs = resolve_window_columns(self.schema, partition_by, order_by, outs)
        nc, nw, n = self.num_cols, len(spec), self.num_rows
        out = self._like(None, 0, 0, self.schema + descs)
        if n == 0:
            return out
        src = self._block_ptr()
        entries = [] if presorted else [(k, False, False) for k in part_cols] + order
        if len(entries) > A.MAX_ORDER_ENTRIES:
            raise QueryMustRunOnCpu("more than %d partition keys and order entries to sort by" % A.MAX_ORDER_ENTRIES)
        block = self.mgr.alloc((nc + nw) * n * 8, self.device_id)
        try:
            if not entries:
                self._copy_rows(block, 0, n)
            else:
                arr = self._order_entries(entries)
                check(lib().hdk_hip_sort_columns(src, self.capacity, nc, n, arr, len(entries), 0, 0, 0, block.ptr, n, None, None,
                                                 0, self.device_id, None))
            pc = (C.c_int32 * max(len(part_cols), 1))(*part_cols)
            oc = (C.c_int32 * max(len(order), 1))(*[t for t, _, _ in order])
            for j0 in range(0, nw, A.MAX_WINDOW_OUTS):
                part = spec[j0:j0 + A.MAX_WINDOW_OUTS]
                warr = (A.WindowOut * len(part))()
                for j, w in enumerate(part):
                    is_fp, nullable, null_bits = self._column_null(w.col)
                    warr[j] = A.WindowOut(w.col, w.kind, w.frame, int(is_fp), int(nullable), A.to_i64(null_bits), w.param)
                check(lib().hdk_hip_window_columns(block.ptr, n, nc, n, pc, len(part_cols), oc, len(order), warr, len(part),
                                                   block.ptr + (nc + j0) * n * 8, n, None, 0, self.device_id, None))
            self.mgr.synchronizeStream(self.device_id)
        except Exception:
            block.free()
            raise
        out.block, out.capacity, out.num_rows = block, n, n
        return out

    def windows(self, windows) -> "DeviceColumns":
        """A unit's window functions (QueryUnit.windows): one window() per distinct (partition_by, order_by) in order of
        first appearance, each over the result of the one before, whose block is handed back.  A window without a name is
        called <kind>_<number of columns + its index in `windows`>.  -> a new DeviceColumns; this object stays valid."""
        windows = [dataclasses.replace(w, name=w.name or f"{w.kind}_{self.num_cols + i}") for i, w in enumerate(windows)]
        if not windows:
            return self.sort([])  # nothing to add: every row, copied
        cols = self
        for partition_by, order_by, idx in group_windows(windows):
            cols = _stage(cols, lambda c: c.window(partition_by, order_by, [windows[i] for i in idx]), keep=self)
        return cols

    def project(self, outs) -> "DeviceColumns":
        """Computed columns on the device (hdk_hip_project_columns; the reference's project step over the previous step's
        result) -> a new DeviceColumns that carries the new schema and ONLY the listed columns, every input row once in
        this object's order; this object stays valid.  `outs`: ir.Proj items over ir.TargetRef (a column by index or name),
        Lit, BinOp, Cast, Case and the conditions Cmp / And / Or / Not / IsNull; a bare TargetRef copies its column
        (plan.resolve_select_columns has the rules for type, name and nullability).  One exactly sized block; a select list
        beyond one call's outs, ops or input columns goes through further calls that write into the same block.  One
        stream synchronisation, after which the error word is read: a division by zero or an overflow that a row raised
        frees the block and raises HdkHipError with the reference's code."""
        programs, descs = resolve_select_columns(self.schema, outs)
        out = self._like(None, 0, 0, descs)
        n = self.num_rows
        if n == 0:
            return out
        src = self._block_ptr()
        calls = split_project_calls(programs)
        block = self.mgr.alloc(len(programs) * n * 8, self.device_id)
        try:
            errors = self.mgr.alloc(4 * len(calls), self.device_id)  # one error word per call
            try:
                for c, (j0, count) in enumerate(calls):
                    part = programs[j0:j0 + count]
                    ops = (A.ProjectOp * sum(len(p.ops) for p in part))()
                    parr = (A.ProjectOut * count)()
                    at = 0
                    for j, p in enumerate(part):
                        parr[j] = A.ProjectOut(at, len(p.ops), int(p.is_fp), int(p.nullable), (C.c_uint8 * 6)(),
                                               A.to_i64(p.null_bits))
                        for code, width, flags, col, imm in p.ops:
                            ops[at] = A.ProjectOp(code, width, flags, 0, col, A.to_i64(imm))
                            at += 1
                    check(lib().hdk_hip_project_columns(src, self.capacity, self.num_cols, n, ops, at, parr, count,
                                                        block.ptr + j0 * n * 8, n, errors.ptr + 4 * c, self.device_id, None))
                self.mgr.synchronizeStream(self.device_id)
                err = int(self.mgr.to_host(errors.ptr, 4 * len(calls), self.device_id, np.int32).max())
            finally:
                errors.free()
            if err:
                raise _device_error(err)
        except Exception:
            block.free()
            raise
        out.block, out.capacity, out.num_rows = block, n, n
        return out

    def join(self, right: "DeviceColumns", left_on, right_on=None, how: str = "inner", null_safe: bool = False,
             right_cols=None, right_presorted: bool = False, sort_left: bool = False) -> "DeviceColumns":
        """Equi-join of these columns (the left side) with `right` on the device (hdk_hip_join_columns, a sort-merge join;
        the reference joins a previous step's result like any table, QE/ColumnFetcher.cpp:111) -> a new DeviceColumns that
        carries its own schema: every left column, then `right_cols` (default: every right column that is not a key; none
        for semi / anti); both inputs stay valid.  `left_on` / `right_on`: key columns by index or name (right_on None: the
        same on the right); `how`: inner, left, semi or anti; `null_safe`: a NULL key matches a NULL key (IS NOT DISTINCT
        FROM).  plan.resolve_join_columns has the rules for keys, names and nullability.  The library searches a SORTED
        right side: unless `right_presorted` says that `right` already ascends on its keys with NULLs last, a copy sorted
        by them is made first (hdk_hip_sort_columns) and freed afterwards.  Rows come out in this object's order, the
        matches of one row in the sorted right side's order; sort_left=True sorts a copy of this side by its keys as well,
        which shortens the searches: the rows then come out ascending by key, NULLs last.  Sizing: the number of output
        rows is not known in advance, so they are counted first and the block holds exactly those -- except that a semi
        or anti join whose worst case (every left row) stays within 64 MiB is made in one call.  2^32 or more output rows
        are counted exactly but not materialised: HdkHipError(ERR_OUT_OF_GPU_MEM) before anything is allocated."""
        if right.device_id != self.device_id:
            raise ValueError("the two sides of a join live on different devices")
        keys, outs, descs = resolve_join_columns(self.schema, right.schema, left_on, right_on, how, right_cols)
        out = self._like(None, 0, 0, descs)
        n, rn = self.num_rows, right.num_rows
        if n == 0:
            return out
        self._block_ptr()
        if rn:
            right._block_ptr()
        lsrc = self.sort([(lc, False, False) for lc, _ in keys]) if sort_left else self
        rsrc = right
        try:
            if rn and not right_presorted:
                rsrc = right.sort([(rc, False, False) for _, rc in keys])
            karr = (A.JoinKey * len(keys))()
            for i, (lc, rc) in enumerate(keys):
                a, b = self.schema[lc], right.schema[rc]
                karr[i] = A.JoinKey(lc, rc, int(a.nullable), int(b.nullable), (C.c_uint8 * 6)(), A.to_i64(a.null_bits),
                                    A.to_i64(b.null_bits))
            oarr = (A.JoinOut * len(outs))()
            for j, (side, col, null_bits) in enumerate(outs):
                oarr[j] = A.JoinOut(side, (C.c_uint8 * 3)(), col, null_bits)
            rptr = rsrc.block.ptr if rn else None
            flags = A.JOIN_NULL_SAFE if null_safe else 0

            def call(out_ptr, capacity, row_count_ptr):
                check(lib().hdk_hip_join_columns(lsrc.block.ptr, lsrc.capacity, self.num_cols, n, rptr, rsrc.capacity if rn else 0,
                                                 right.num_cols, rn, karr, len(keys), JOIN_TYPES[how], flags, oarr, len(outs),
                                                 out_ptr, capacity, row_count_ptr, None, None, None, 0, self.device_id, None))

            # only a semi / anti join has a worst case (every left row once); the others always count first
            one_call = ONE_CALL_BYTES if how in ("semi", "anti") else -1
            out.block, out.capacity, out.num_rows = sized_columns(self.mgr, self.device_id, len(outs), n, call, one_call,
                                                                  drop_empty=True, max_rows=(1 << 32) - 1)
        finally:
            if lsrc is not self:
                lsrc.free()
            if rsrc is not right:
                rsrc.free()
        return out

    SETOP_ONE_CALL_BYTES = ONE_CALL_BYTES

    def _concat(self, first: "DeviceColumns", second: "DeviceColumns", pairs, block: DeviceBuffer, capacity: int,
                side_col: int = -1, flags: int = 0):
        """hdk_hip_concat_columns: the rows of `first`, then those of `second`, into `block`; `pairs` as
        plan.resolve_setop_columns gives them for (first, second)"""
        arr = (A.SetopCol * len(pairs))()
        for j, (lc, rc, ln, rn, lbits, rbits, obits) in enumerate(pairs):
            arr[j] = A.SetopCol(lc, rc, int(ln), int(rn), (C.c_uint8 * 6)(), A.to_i64(lbits), A.to_i64(rbits), A.to_i64(obits))
        check(lib().hdk_hip_concat_columns(first.block.ptr if first.num_rows else None, first.capacity if first.num_rows else 0,
                                           first.num_cols, first.num_rows,
                                           second.block.ptr if second.num_rows else None,
                                           second.capacity if second.num_rows else 0, second.num_cols, second.num_rows, arr,
                                           len(pairs), side_col, flags, block.ptr, capacity, self.device_id, None))

    def _setop(self, other: "DeviceColumns", op: str, all: bool) -> "DeviceColumns":
        if other.device_id != self.device_id:
            raise ValueError("the two sides of a set operation live on different devices")
        pairs, descs = resolve_setop_columns(self.schema, other.schema)
        out = self._like(None, 0, 0, descs)
        nc, nl, nr = len(pairs), self.num_rows, other.num_rows
        if nl + nr >= 1 << 32:
            raise QueryMustRunOnCpu(f"a set operation over {nl} + {nr} rows: the library's row indices are 32 bits wide")
        if nl + nr == 0 or (nl == 0 and op != "union"):
            return out  # (without a left row INTERSECT and EXCEPT keep nothing)
        if nl:
            self._block_ptr()
        if nr:
            other._block_ptr()
        n = nl + nr
        if op == "union" and all:
            block = self.mgr.alloc(nc * n * 8, self.device_id)
            try:
                self._concat(self, other, pairs, block, n)
                self.mgr.synchronizeStream(self.device_id)
            except Exception:
                block.free()
                raise
            out.block, out.capacity, out.num_rows = block, n, n
            return out
        # the right rows FIRST and a tag that is 1 on them: the stable sort then leaves every run with its right rows in front
        swapped = [(rc, lc, rn, ln, rbits, lbits, obits) for lc, rc, ln, rn, lbits, rbits, obits in pairs]
        tag = ColumnDesc("__side", False, False, 0, Type("int", 8, False), nc, "proj")
        tagged = DeviceColumns(self.compiled, self.mgr, self.device_id, self.mgr.alloc((nc + 1) * n * 8, self.device_id), n, n,
                               schema=descs + [tag])
        ordered = None
        try:
            self._concat(other, self, swapped, tagged.block, n, nc, A.CONCAT_TAG_FIRST)
            ordered = tagged.sort([(t, False, False) for t in range(nc)])
            tagged.free()
            idx = (C.c_int32 * nc)(*range(nc))
            src = ordered.block.ptr

            def call(out_ptr, capacity, row_count_ptr):
                check(lib().hdk_hip_setop_columns(src, n, nc + 1, n, idx, nc, nc, SETOP_CODES[(op, bool(all))], idx, nc, out_ptr,
                                                  capacity, row_count_ptr, None, 0, self.device_id, None))

            out.block, out.capacity, out.num_rows = sized_columns(self.mgr, self.device_id, nc, n if op == "union" else nl, call,
                                                                  self.SETOP_ONE_CALL_BYTES, drop_empty=True)
        finally:
            tagged.free()
            if ordered is not None:
                ordered.free()
        return out

    def union(self, other: "DeviceColumns", all: bool = False) -> "DeviceColumns":
        """UNION [ALL] of these rows (the left operand) with `other`'s on the device -> a new DeviceColumns that carries its
        own schema (plan.resolve_setop_columns: columns pair by position, names and presentation from this side, NULLs of
        both sides rewritten to one sentinel per column); both inputs stay valid and the result owns an exactly sized block
        (up to 64 MiB of worst-case output one call writes a block of the worst-case row count, as filter() does).  Whole
        rows are compared word by word: NULL equals NULL, -0.0 differs from +0.0, doubles included.
        all=True is one hdk_hip_concat_columns call: this object's rows, then `other`'s, each in its order.
        Otherwise (and for intersect / except_) the right rows are concatenated in front of the left rows with a side
        column, sorted on all columns ascending with NULLs last (hdk_hip_sort_columns, stable), and hdk_hip_setop_columns
        keeps one row per distinct row; the side column never leaves.  The rows therefore come out ASCENDING in the device
        sort's order over all columns, NULLs last.  2^32 or more rows on both sides together must run on the CPU, which is
        found before anything is allocated; temporaries are handed back on every path."""
        return self._setop(other, "union", all)

    def intersect(self, other: "DeviceColumns", all: bool = False) -> "DeviceColumns":
        """INTERSECT [ALL] on the device: the rows of this object that `other` holds too -- once each, or with all=True
        min(l, r) copies of a row that is l times here and r times there.  Schema, comparison, method, output order and
        sizing as union() (the worst case is this object's rows)."""
        return self._setop(other, "intersect", all)

    def except_(self, other: "DeviceColumns", all: bool = False) -> "DeviceColumns":
        """EXCEPT [ALL] on the device: the rows of this object that `other` does not hold -- once each, or with all=True
        max(l - r, 0) copies of a row that is l times here and r times there.  Schema, comparison, method, output order and
        sizing as union() (the worst case is this object's rows)."""
        return self._setop(other, "except", all)

    def setop(self, other: "DeviceColumns", op: str, all: bool = False) -> "DeviceColumns":
        """union / intersect / except_ by name (ir.ResultSetOp.op)"""
        if op not in SETOP_NAMES:
            raise ValueError(f"set operation {op!r} (union, intersect or except)")
        return self._setop(other, op, all)

    def free(self):
        if self.block is not None:
            self.block.free()
            self.block = None


class PreparedStep:
    """Everything one (multi-fragment) kernel launch needs, resident on the device."""

    def __init__(self, ex: "Executor", cp: CompiledPlan, frag_ids: List[int], grid=0, flags=0,
                 out_ptr: Optional[int] = None, watchdog_ms: int = 0):
        self.ex, self.cp, self.frag_ids = ex, cp, list(frag_ids)
        self.mgr, self.dev = ex.mgr, ex.device_id
        self.L = lib()
        sync_switches()  # (a test or an A/B script may have changed HDK_HIP_* since the library read them)
        self.keep: List[DeviceBuffer] = []
        self._graph = None
        p = cp.plan
        storage = ex.storage
        outer = storage.get(cp.query.table)
        nfrag = len(self.frag_ids)
        self.rows_in_step = int(sum(outer.frag_rows[f] for f in self.frag_ids))
        self.ko = A.KernelOptions(grid, 0, 0, flags, self.rows_in_step, int(watchdog_ms), 0)
        ntab = 1 + len(cp.inner_tables)

        # ---- join hash tables (built once per device, cached) ----------------------------
        # the launch uses a private copy of the plan: fusing join tables rewrites column descriptors
        self.plan = A.Plan.from_buffer_copy(cp.plan)
        fuse = bool(cp.inner_tables) and ex.fuse_join_tables and \
            not (flags & (A.LAUNCH_FORCE_SCALAR | A.LAUNCH_FORCE_GLOBAL_ATOMICS)) and \
            bool({"hdk_scan_agg_vec_join", "hdk_scan_project_join", "hdk_scan_agg_vec_keyed", "hdk_scan_project_keyed",
                  "hdk_scan_agg_bh_vec_join"} &
                 set(self.kernel_names().split(",")))
        # (a table that will be fused is built together with its fused form: one sweep over the inner rows)
        self.join_tables = []
        for ji in range(len(cp.inner_tables)):
            spec = self._fuse_spec(ji) if fuse else None
            self.join_tables.append(ex._build_join_table(cp, ji, ((spec[0], self), spec[1], spec[2]) if spec else None))
        if fuse:
            self._fuse_join_tables()
        p = self.plan

        # ---- col_buffers[frag][buf_idx] ---------------------------------------------------
        ncols = len(cp.input_cols)
        flat = np.zeros(max(nfrag * ncols, 1), dtype=np.uint64)
        for fi, f in enumerate(self.frag_ids):
            for ci, (tn, cn, slot) in enumerate(cp.input_cols):
                if slot == 0:
                    flat[fi * ncols + ci] = ex.cache.chunk(outer, cn, f).ptr
                else:
                    flat[fi * ncols + ci] = ex.cache.linearized(storage.get(tn), cn).ptr
        d_flat = self._dev(flat)
        frag_ptrs = np.array([d_flat.ptr + fi * ncols * 8 for fi in range(nfrag)] or [0], dtype=np.uint64)
        d_frag_ptrs = self._dev(frag_ptrs)
        num_rows = np.zeros(max(nfrag * ntab, 1), dtype=np.int64)
        frag_offs = np.zeros(max(nfrag * ntab, 1), dtype=np.uint64)
        row_off = 0
        starts = np.concatenate([[0], np.cumsum(outer.frag_rows)]) if outer.frag_rows else [0]
        for fi, f in enumerate(self.frag_ids):
            num_rows[fi * ntab] = outer.frag_rows[f]
            frag_offs[fi * ntab] = starts[f]
            for ti, tn in enumerate(cp.inner_tables):
                num_rows[fi * ntab + 1 + ti] = storage.get(tn).num_rows
        self.rows_in_step = int(sum(outer.frag_rows[f] for f in self.frag_ids))
        d_num_rows = self._dev(num_rows)
        d_frag_offs = self._dev(frag_offs)
        d_nfrag = self._dev(np.array([nfrag], dtype=np.uint64))
        d_ntab = self._dev(np.array([ntab], dtype=np.uint32))
        self.init_vals_host = compact_init_vals(cp)
        d_init = self._dev(self.init_vals_host)
        self.d_init = d_init
        self.d_err = self._dev(np.zeros(1, dtype=np.int32))
        d_max_matched = self._dev(np.array([p.entry_count], dtype=np.int32))
        d_total_matched = self._dev(np.zeros(2, dtype=np.int32))  # int32 counter in an 8-byte cell
        self.d_total_matched = d_total_matched
        self.d_zero = self._dev(np.zeros(1, dtype=np.int64))
        if len(self.join_tables) == 1:
            jt_param = self.join_tables[0].ptr
        elif self.join_tables:
            jt_param = self._dev(np.array([t.ptr for t in self.join_tables], dtype=np.int64)).ptr
        else:
            jt_param = 0

        # ---- output buffer + GROUPBY_BUF ---------------------------------------------------
        self.buffer_bytes = cp.buffer_bytes
        if out_ptr is None:
            self.out = self.mgr.alloc(max(self.buffer_bytes, 8), self.dev)
            self.keep.append(self.out)
            self.out_ptr = self.out.ptr
        else:
            self.out_ptr = out_ptr
        if p.query_kind == A.Q_NON_GROUPED:
            nslots = len(cp.slot_widths)
            ptrs = np.array([self.out_ptr + 8 * i for i in range(nslots)], dtype=np.uint64)
        else:
            ptrs = np.array([self.out_ptr], dtype=np.uint64)
        d_gb = self._dev(ptrs)
        if p.output_columnar:
            self.d_col_sizes = self._dev(np.array(cp.slot_widths, dtype=np.int8))
            self.d_init_raw = self._dev(columnar_init_vals(cp))

        params = (C.c_void_p * A.KP_COUNT)()
        params[A.KP_COL_BUFFERS] = d_frag_ptrs.ptr
        params[A.KP_NUM_FRAGMENTS] = d_nfrag.ptr
        params[A.KP_LITERALS] = None
        params[A.KP_NUM_ROWS] = d_num_rows.ptr
        params[A.KP_FRAG_ROW_OFFSETS] = d_frag_offs.ptr
        params[A.KP_MAX_MATCHED] = d_max_matched.ptr
        params[A.KP_TOTAL_MATCHED] = d_total_matched.ptr
        params[A.KP_INIT_AGG_VALS] = d_init.ptr
        params[A.KP_GROUPBY_BUF] = d_gb.ptr
        params[A.KP_ERROR_CODE] = self.d_err.ptr
        params[A.KP_NUM_TABLES] = d_ntab.ptr
        params[A.KP_JOIN_HASH_TABLES] = jt_param or None
        self._params = params

        ws = C.c_size_t(0)
        check(self.L.hdk_hip_workspace_size(C.byref(p), C.byref(self.ko), self.dev, C.byref(ws)))
        self.workspace = self.mgr.alloc(max(ws.value, 16), self.dev)
        self.keep.append(self.workspace)
        self.workspace_bytes = ws.value

    def _dev(self, arr) -> DeviceBuffer:
        b = self.mgr.to_device(arr, self.dev)
        self.keep.append(b)
        return b

    def kernel_names(self) -> str:
        sync_switches()
        out = C.create_string_buffer(256)
        check(self.L.hdk_hip_describe_launch(C.byref(self.plan), C.byref(self.ko), self.dev, out, 256))
        return out.value.decode()

    def _fuse_spec(self, ji, max_bytes=2 << 30):
        """What the fused form of join ji's table holds: (cache key, plan columns read through the join, stride), or
        None when the table stays as it is (not one-to-one, more than seven columns, too large)."""
        cp = self.cp
        info = cp.join_infos[ji]
        if info["kind"] != A.JOIN_ONE_TO_ONE:
            return None
        cols = [ci for ci, (tn, cn, slot) in enumerate(cp.input_cols) if slot == ji + 1]
        stride = 1 + len(cols)
        if len(cols) > 7 or info["entry_count"] * stride * 8 > max_bytes:
            return None
        key = (info["inner_table"], info["inner_col"], tuple(cp.input_cols[ci][1] for ci in cols), info["uses_bw_eq"],
               info["for_semi_join"])
        return key, cols, stride

    def _payload_arrays(self, ji, cols):
        cp, p = self.cp, self.plan
        inner = self.ex.storage.get(cp.join_infos[ji]["inner_table"])
        ptrs = (C.c_void_p * max(len(cols), 1))()
        widths = (C.c_int32 * max(len(cols), 1))()
        kinds = (C.c_int32 * max(len(cols), 1))()
        for k, ci in enumerate(cols):
            ptrs[k] = self.ex.cache.linearized(inner, cp.input_cols[ci][1]).ptr
            widths[k] = cp.plan.cols[ci].width
            kinds[k] = cp.plan.cols[ci].kind
        return ptrs, widths, kinds

    def _fuse_join_tables(self):
        """Replace each one-to-one join table by the fused [row id | payload ...] form when the batched
        interpreter (or the projection kernel) will run the plan: one gather per probing row instead of
        slot -> row id -> inner column (HDK_JOIN_ONE_TO_ONE_FUSED, include/hdk_hip.h)."""
        cp, p = self.cp, self.plan
        for ji, info in enumerate(cp.join_infos):
            spec = self._fuse_spec(ji)
            if spec is None:
                continue
            key, cols, stride = spec
            entries = info["entry_count"]
            fused = self.ex._fused_cache.get(key)
            if fused is None:  # (the plain table came out of the cache: derive the fused form from it)
                ptrs, widths, kinds = self._payload_arrays(ji, cols)
                fused = self.mgr.alloc(entries * stride * 8, self.dev)
                check(self.L.hdk_hip_build_fused_join_table(self.join_tables[ji].ptr, entries, ptrs, widths, kinds,
                                                            len(cols), fused.ptr, self.dev, None))
                self.mgr.synchronizeStream(self.dev)
                self.ex._fused_cache[key] = fused
            for k, ci in enumerate(cols):
                # payload words are int64 (ints sign-extended, float widened to double by the decoder)
                p.cols[ci].kind = A.COL_DOUBLE if p.cols[ci].kind in (A.COL_FLOAT, A.COL_DOUBLE) else A.COL_INT
                p.cols[ci].width = 8
                p.cols[ci].table = -(ji + 1)
                p.cols[ci].buf_idx = 1 + k
            p.joins[ji].kind = A.JOIN_ONE_TO_ONE_FUSED
            p.joins[ji].fused_stride = stride
            self.join_tables[ji] = fused

    # ---- the three steps of launchGpuCode ------------------------------------------------------
    def init_output(self, stream=None):
        p = self.cp.plan
        props = self.mgr.getDeviceProperties(self.dev)
        if p.query_kind == A.Q_NON_GROUPED:
            # out_vec slots start at init_agg_vals (QueryExecutionContext.cpp:452-458); the keyless
            # row-wise fill with one "entry" of nslots quads is exactly that copy, on the stream
            check(self.L.hdk_hip_init_group_by_buffer(
                self.out_ptr, self.d_init.ptr, 1, 0, 8, len(self.cp.slot_widths), 1, 1,
                props.max_threads_per_block, props.grid_size, self.dev, stream))
        elif p.query_kind == A.Q_PROJECTION and not self.ex.init_projection_buffers:
            # The reference fills projection buffers like any other (QueryMemoryInitializer.cpp:1103-1153), but
            # every claimed output row is written completely (row position + each target) and nothing past
            # TOTAL_MATCHED is ever read: the fill (6 GB for a 256 M-row scan) is skipped unless asked for.
            pass
        elif p.output_columnar:
            check(self.L.hdk_hip_init_columnar_group_by_buffer(
                self.out_ptr, self.d_init_raw.ptr, p.entry_count, eff_key_count(p), len(self.cp.slot_widths),
                self.d_col_sizes.ptr, 1, p.keyless, 8, props.max_threads_per_block, props.grid_size,
                self.dev, stream))
        else:
            check(self.L.hdk_hip_init_group_by_buffer(
                self.out_ptr, self.d_init.ptr, p.entry_count, eff_key_count(p), p.key_width, p.row_size_quad,
                p.keyless, 1, props.max_threads_per_block, props.grid_size, self.dev, stream))
        if p.query_kind == A.Q_PROJECTION:
            # TOTAL_MATCHED restarts at 0 for every launch (prepareKernelParams,
            # QueryExecutionContext.cpp:941-950); reset on the launch stream with the fill kernel
            check(self.L.hdk_hip_init_group_by_buffer(
                self.d_total_matched.ptr, self.d_zero.ptr, 1, 0, 8, 1, 1, 1,
                props.max_threads_per_block, props.grid_size, self.dev, stream))

    def launch(self, stream=None, init_output=False):
        """hdk_hip_launch into the (initialised) output buffer; init_output=True hands the initialisation to the launch
        (HDK_HIP_LAUNCH_INIT_OUTPUT: row-wise group-by buffers only, and only for a buffer that holds nothing yet)."""
        ko = self.ko
        if init_output:
            ko = A.KernelOptions.from_buffer_copy(self.ko)
            ko.flags |= A.LAUNCH_INIT_OUTPUT
        check(self.L.hdk_hip_launch(C.byref(self.plan), self._params, C.byref(ko), self.dev, stream,
                                    self.workspace.ptr, self.workspace.nbytes))

    @property
    def launch_initialises(self) -> bool:
        """A fresh row-wise open-addressing table: the launch writes the empty image itself -- the radix-partitioned
        group-by builds it region by region in LDS, which saves a write and a read of the whole table."""
        p = self.cp.plan
        return p.query_kind == A.Q_BASELINE_HASH and not p.output_columnar

    def enqueue(self, stream=None):
        """One complete step on the stream: initialise the output buffer and launch (fused where the library can)."""
        if self.launch_initialises:
            self.launch(stream, init_output=True)
        else:
            self.init_output(stream)
            self.launch(stream)

    def _error_code(self, stream_synced: bool) -> int:
        """The step's error word once the stream has drained; a positive code raises."""
        if not stream_synced:
            self.mgr.synchronizeStream(self.dev)
        err = int(self.mgr.to_host(self.d_err.ptr, 4, self.dev, np.int32)[0])
        if err > 0:
            raise _device_error(err)
        return err

    def fetch(self, stream_synced=False) -> ExecutionResult:
        err = self._error_code(stream_synced)
        buf = self.mgr.to_host(self.out_ptr, max(self.buffer_bytes, 8), self.dev, np.int64)
        total = None
        if self.cp.plan.query_kind == A.Q_PROJECTION:
            total = int(self.mgr.to_host(self.d_total_matched.ptr, 4, self.dev, np.int32)[0])
        # err < 0: a projection ran out of output rows (benign under a LIMIT; aggregate_error_codes,
        # QueryExecutionContext.cpp:221-234, surfaces it only when nothing positive happened)
        return ExecutionResult(self.cp, buf[:self.buffer_bytes // 8], self.cp.entry_count, err, total)

    COLUMNS_ONE_CALL_BYTES = ONE_CALL_BYTES

    def fetch_columns(self, stream_synced=False, positions=False) -> DeviceColumns:
        """The step's result as dense device columns: the buffer stays in HBM, only what to_host() asks for crosses the
        link.  A group-by step goes through hdk_hip_columnarize_result, a projection or a non-grouped step through
        hdk_hip_columnarize_rows (_fetch_row_columns).  The device error code is checked as in fetch().
        Sizing: when num_targets x entry_count x 8 is at most COLUMNS_ONE_CALL_BYTES (64 MiB) one call writes into a block
        of entry_count rows per column -- over-allocating a few MB costs less than a second pass over the table.  Above
        that the groups are counted first (out_cols = NULL: one streaming pass) and the block holds exactly row_count
        rows per column: a half-empty 200 M-entry table then takes 1.6 GB, not 3.2 GB.
        `positions` (a projection only, else a ValueError): the row positions as a last column, "__pos"."""
        p = self.cp.plan
        if positions and p.query_kind != A.Q_PROJECTION:
            raise ValueError("positions=True: only a projection step has row positions")
        err = self._error_code(stream_synced)
        if p.query_kind in (A.Q_PROJECTION, A.Q_NON_GROUPED):
            return self._fetch_row_columns(err, positions)
        n, nt = int(self.cp.entry_count), int(p.num_targets)
        iv = np.ascontiguousarray(self.cp.init_vals, dtype=np.int64)

        def call(out_ptr, capacity, row_count_ptr):
            check(self.L.hdk_hip_columnarize_result(C.byref(p), self.out_ptr, n, iv.ctypes.data, out_ptr, capacity,
                                                    row_count_ptr, None, 0, self.dev, None))

        block, capacity, rows = sized_columns(self.mgr, self.dev, nt, n, call, self.COLUMNS_ONE_CALL_BYTES)
        return DeviceColumns(self.cp, self.mgr, self.dev, block, capacity, rows, err)

    def _fetch_row_columns(self, err: int, positions: bool) -> DeviceColumns:
        """fetch_columns() of a projection or a non-grouped step (hdk_hip_columnarize_rows; the device form of the
        reference's ColumnarResults::materializeAllColumnsProjection).  A projection's rows are the first
        min(TOTAL_MATCHED, entry_count) of its buffer, which the library reads on the device: the worst case is
        entry_count rows, and the one-call / count-first rule of fetch_columns applies (the count-only call reads one
        word).  A non-grouped step is one call into a block of one row.  `err` < 0 (the step ran out of output rows, benign
        under a LIMIT) travels in DeviceColumns.error_code."""
        p = self.cp.plan
        schema = describe_columns(self.cp, positions)
        nc = len(schema)
        projection = p.query_kind == A.Q_PROJECTION
        n = int(self.cp.entry_count) if projection else 1
        total = self.d_total_matched.ptr if projection else None

        def call(out_ptr, capacity, row_count_ptr):
            pos_ptr = out_ptr + (nc - 1) * capacity * 8 if (positions and out_ptr) else None
            check(self.L.hdk_hip_columnarize_rows(C.byref(p), self.out_ptr, n, total, out_ptr, capacity, pos_ptr,
                                                  row_count_ptr, self.dev, None))

        one_call = self.COLUMNS_ONE_CALL_BYTES if projection else max(self.COLUMNS_ONE_CALL_BYTES, nc * 8)
        block, capacity, rows = sized_columns(self.mgr, self.dev, nc, n, call, one_call)
        return DeviceColumns(self.cp, self.mgr, self.dev, block, capacity, rows, err, schema)

    def run(self, stream=None) -> ExecutionResult:
        self.enqueue(stream)
        return self.fetch()

    # ---- hipGraph: record init + launch once, replay per execution (small inputs are launch-bound) --------
    def capture_graph(self, stream=None):
        """Record `init_output(); launch()` as a hipGraph on `stream` (None = the manager's stream).  Only the
        LDS-strategy plans are captured (their launches are kernels only once the plan is resident in the
        workspace); for anything else this is a no-op and replay() falls back to the plain sequence."""
        if self._graph or not self.kernel_names().endswith("hdk_finalize"):
            return self
        self.init_output(stream)
        self.launch(stream)  # uploads the plan into the workspace head
        self.mgr.synchronizeStream(self.dev) if stream is None else None
        saved = self.ko.flags
        self.ko.flags = (saved | A.LAUNCH_PLAN_RESIDENT) & ~A.LAUNCH_RECORD_EVENTS
        try:
            check(self.L.hdk_hip_graph_begin_capture(self.dev, stream))
            self.init_output(stream)
            self.launch(stream)
            g = C.c_void_p()
            check(self.L.hdk_hip_graph_end_capture(self.dev, stream, C.byref(g)))
            self._graph = g
        finally:
            self.ko.flags = saved
        return self

    def replay(self, stream=None):
        """One execution: the recorded graph if there is one, else init_output() + launch()."""
        if self._graph:
            check(self.L.hdk_hip_graph_launch(self._graph, self.dev, stream))
        else:
            self.enqueue(stream)

    def free(self):
        if self._graph:
            self.L.hdk_hip_graph_destroy(self._graph)
            self._graph = None
        for b in self.keep:
            b.free()
        self.keep.clear()


class Executor:
    """One device's executor (cf. Executor + QueryExecutionContext for a MultifragmentKernel,
    QE/Execute.cpp:2084-2090: one kernel over all fragments assigned to the device)."""

    def __init__(self, storage: ArrowStorage, device_id: int = 0, mgr: Optional[HipMgr] = None):
        self.storage = storage
        self.mgr = mgr or HipMgr()
        self.device_id = device_id
        self.cache = BufferCache(self.mgr, device_id)
        self._join_cache: Dict[tuple, DeviceBuffer] = {}
        self._fused_cache: Dict[tuple, DeviceBuffer] = {}
        self.fuse_join_tables = True  # HDK_JOIN_ONE_TO_ONE_FUSED for the batched kernels
        self.init_projection_buffers = False  # see PreparedStep.init_output

    def compile(self, q: QueryUnit) -> CompiledPlan:
        """plan.compile_query, after the device has been asked what the planner cannot read from the host: the key
        multiplicity of every join whose inner table is a registered result (_measure_inner_tables)."""
        if isinstance(q.table, QueryUnit) or any(isinstance(j.inner_table, QueryUnit) for j in q.joins):
            raise ValueError("a unit over a FROM-subquery has no plan before the inner unit has run: its layout is sized from "
                             "the statistics of the inner result; execute() it")
        self._measure_inner_tables(q)
        return compile_query(self.storage, q)

    def _measure_inner_tables(self, q: QueryUnit):
        """For each join of `q` whose inner table is a joinable storage.DeviceTable and whose key is not yet in its key_multiplicity:
        one hdk_hip_key_multiplicity call on the table's block, the 32-byte record read back and kept.  A semi or anti
        join needs no number (the first row of a key wins the fill); a join that compile_query will refuse anyway (key
        lists, key types, an inner table without a key value) is left to it."""
        for j in q.joins:
            inner = self.storage.tables.get(j.inner_table) if isinstance(j.inner_table, str) else None
            if not isinstance(inner, DeviceTable) or not inner.joinable or j.type in ("semi", "anti"):
                continue
            icols = j.inner_cols
            if len(j.outer_keys) != len(icols) or not 1 <= len(icols) <= A.MAX_JOIN_KEYS or \
                    any(c not in inner.columns or not inner.columns[c].type.is_integer_like for c in icols):
                continue
            shape = join_key_shape(inner, j)
            if shape is None or shape.multiplicity_key in inner.key_multiplicity:
                continue
            inner.key_multiplicity[shape.multiplicity_key] = self._key_multiplicity(inner, shape)

    def _key_multiplicity(self, inner: DeviceTable, shape) -> tuple:
        """-> (max_matches, occupied) of the join key `shape` (a plan.JoinKeyShape) over the rows of `inner`, filed as the
        build of that join will file them.  A row outside the range the statistics give -- the build's -2, found before
        anything is built -- raises QueryMustRunOnCpu."""
        nk = len(shape.cols)
        keys = (A.MultiplicityKey * nk)()
        for i, c in enumerate(shape.cols):
            col = inner.columns[c]
            st = col.table_stats()
            mn, mx = (int(st.min), int(st.max)) if st.min is not None else (0, 0)
            # (nullable whatever the type says: the builds test every word against the type's NULL, JoinColumnTypeInfo)
            keys[i] = A.MultiplicityKey(inner.column_order.index(c), 1, (C.c_uint8 * 3)(), A.to_i64(col.type.null_value()),
                                        A.to_i64(mn), A.to_i64(mx), A.to_i64(mx + 1))
        flags = A.KEYS_NULLS_MATCH if shape.nulls_match else 0
        d_rec = self.mgr.alloc(C.sizeof(A.KeyMultiplicityResult), self.device_id)
        try:
            check(lib().hdk_hip_key_multiplicity(inner._base(), inner.out_capacity, len(inner.column_order), inner.num_rows, keys,
                                                 nk, shape.entry_count, shape.bucket, flags, d_rec.ptr, None, 0, self.device_id,
                                                 None))
            self.mgr.synchronizeStream(self.device_id)
            rec = self.mgr.to_host(d_rec.ptr, C.sizeof(A.KeyMultiplicityResult), self.device_id, np.uint64)
        finally:
            d_rec.free()
        max_matches, occupied, _, outside = (int(x) for x in rec)
        if outside:
            raise QueryMustRunOnCpu(f"stale statistics: {outside} rows of the registered result {inner.name!r} hold a join key "
                                    f"outside the range [{shape.min_key}, {shape.max_key}] its table would be sized from")
        return max_matches, occupied

    _subquery_ids = itertools.count()

    def register_columns(self, name: str, cols: DeviceColumns, columns=None, fragment_size: Optional[int] = None,
                         joinable: bool = False) -> DeviceTable:
        """Dense result columns as a table that the scan kernels read (hdk_hip_chunk_columns; the device form of
        ArrowStorage's import: sentinel rewrite, ArrowStorageUtils.cpp:176-213, and computeStats) -> the storage.DeviceTable,
        added to this executor's storage under `name`; `cols` stays valid and unmodified.  `columns` selects and orders the
        columns by name or index (default: all of them, at most 16).  Every column becomes an 8-byte storage column of its
        kind (storage.registered_column_type), its NULLs rewritten to that type's sentinel; the table owns one new block, a
        copy: the chunks of a fresh block start on 256-byte boundaries, as every chunk the scan kernels have met.
        `fragment_size` (default storage.DEFAULT_FRAGMENT_SIZE) is ROUNDED UP to a multiple of 32 for the same reason.
        The per-fragment statistics are read back after one stream synchronisation.
        A ValueError: duplicate or empty column names, cols.error_code != 0, freed columns, more than 16 columns, a column
        without an 8-byte storage form (a boolean, a DATE in days: leave it out with columns=), a name that is a table
        already.  The table is the outer table of a unit; with joinable=True it may also be the INNER table of a join, whose
        key multiplicity compile() then measures on the device (storage.DeviceTable.key_multiplicity) -- without it a join
        against the table keeps the refusal it always got.  drop_registered(name) frees it."""
        if not isinstance(name, str) or not name:
            raise ValueError("a registered table needs a name")
        if name in self.storage.tables:
            raise ValueError(f"{name!r} is already a table: drop it first")
        if cols.error_code != 0:
            raise ValueError(f"the columns carry error code {cols.error_code}: they are not a complete result")
        if cols.device_id != self.device_id:
            raise ValueError("the columns live on another device")
        by_name = {d.name: i for i, d in enumerate(cols.schema)}
        picked = []
        for c in (range(cols.num_cols) if columns is None else columns):
            if isinstance(c, str):
                if c not in by_name:
                    raise ValueError(f"columns= names no column: {c!r}")
                picked.append(by_name[c])
            elif isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < cols.num_cols:
                raise ValueError(f"columns= index {c!r} outside 0..{cols.num_cols - 1}")
            else:
                picked.append(int(c))
        if not 1 <= len(picked) <= A.MAX_CHUNK_COLUMNS:
            raise ValueError(f"{len(picked)} columns: a registered table takes 1..{A.MAX_CHUNK_COLUMNS} (select with columns=)")
        descs = [cols.schema[i] for i in picked]
        names = [d.name for d in descs]
        if any(not n for n in names) or len(set(names)) != len(names):
            raise ValueError(f"the column names {names} are empty or not unique: a table's columns are found by name")
        types = [registered_column_type(d) for d in descs]
        fragment_rows = int(fragment_size or DEFAULT_FRAGMENT_SIZE)
        if fragment_rows <= 0:
            raise ValueError("fragment_size must be positive")
        fragment_rows = (fragment_rows + 31) // 32 * 32
        n, nc = cols.num_rows, len(picked)
        src = cols._block_ptr() if n else None
        nfrag = max(1, -(-n // fragment_rows))
        out_capacity = max((n + 31) // 32 * 32, 32)
        sel = (A.ChunkCol * nc)()
        for j, (i, d, t) in enumerate(zip(picked, descs, types)):
            sel[j] = A.ChunkCol(i, int(d.is_fp), int(d.nullable), (C.c_uint8 * 2)(), A.to_i64(d.null_bits), A.to_i64(t.null_value()))
        block = self.mgr.alloc(nc * out_capacity * 8, self.device_id)
        try:
            d_stats = self.mgr.alloc(nc * nfrag * C.sizeof(A.ChunkStatsRecord), self.device_id)
            try:
                check(lib().hdk_hip_chunk_columns(src, cols.capacity if n else 0, cols.num_cols, n, sel, nc, fragment_rows,
                                                  block.ptr, out_capacity, d_stats.ptr, None, 0, self.device_id, None))
                self.mgr.synchronizeStream(self.device_id)
                rec = self.mgr.to_host(d_stats.ptr, nc * nfrag * 32, self.device_id, np.int64).reshape(nc, nfrag, 4)
            finally:
                d_stats.free()
            frag_rows = [min(fragment_rows, n - b) for b in range(0, n, fragment_rows)] or [0]
            table_cols = []
            for j, (d, t) in enumerate(zip(descs, types)):
                stats = [stats_from_record(t, int(r[0]), int(r[1]), int(r[2]), int(r[3])) for r in rec[j]]
                table_cols.append(Column(d.name, t, [], stats, d.dictionary))
            table = DeviceTable(name, table_cols, frag_rows, block, out_capacity, fragment_rows, self.device_id, joinable)
        except Exception:
            block.free()
            raise
        return self.storage.add_table(table)

    def drop_registered(self, name: str):
        """Remove a table that register_columns made and free its block, and with it every join table and fused join table
        built over it: both caches are keyed by the table's NAME, and a name registered again must not be served the hash
        table of its predecessor."""
        t = self.storage.tables.get(name)
        if not isinstance(t, DeviceTable):
            raise ValueError(f"{name!r} is not a registered result")
        self.storage.drop_table(name)
        for cache in (self._join_cache, self._fused_cache):
            for key in [k for k in cache if k[0] == name]:
                cache.pop(key).free()
        t.free()

    def _execute_subquery(self, q: QueryUnit, device_type, frag_ids, result, **kw):
        """A unit that reads a QueryUnit -- as its `table` (a FROM-subquery) or as the inner table of a join --: that unit
        runs with result="columns", all its stages included; its columns are registered under a private name and handed
        back; the unit above runs over that table like over any other, and the table is dropped -- also when a step raises.
        One subquery per call: the unit above comes back through execute() with the others.  An inner unit may itself
        read a subquery."""
        ji = next((i for i, j in enumerate(q.joins) if isinstance(j.inner_table, QueryUnit)), None)
        cols = self.execute(q.table if ji is None else q.joins[ji].inner_table, device_type, None, "columns")
        name = None
        try:
            try:
                name = "__subquery_%d" % next(self._subquery_ids)
                while name in self.storage.tables:
                    name = "__subquery_%d" % next(self._subquery_ids)
                self.register_columns(name, cols, joinable=ji is not None)
            finally:
                cols.free()
            if ji is None:
                above = dataclasses.replace(q, table=name)
            else:
                above = dataclasses.replace(q, joins=[dataclasses.replace(j, inner_table=name) if i == ji else j
                                                      for i, j in enumerate(q.joins)])
            return self.execute(above, device_type, frag_ids, result, **kw)
        finally:
            if name is not None and isinstance(self.storage.tables.get(name), DeviceTable):
                self.drop_registered(name)

    def _join_columns(self, inner, info):
        """JoinColumn / JoinColumnTypeInfo per key column: one JoinChunk per inner fragment."""
        jcs, tis, keep = [], [], []
        for k, col in enumerate(info["inner_cols"]):
            chunks = (A.JoinChunk * inner.num_fragments)()
            rid = 0
            for f in range(inner.num_fragments):
                chunks[f].col_buff = self.cache.chunk(inner, col, f).ptr
                chunks[f].num_elems = inner.frag_rows[f]
                chunks[f].row_id = rid
                rid += inner.frag_rows[f]
            raw = np.frombuffer(bytes(chunks), dtype=np.uint8)
            d_chunks = self.mgr.to_device(raw, self.device_id)
            keep.append(d_chunks)
            jcs.append(A.JoinColumn(d_chunks.ptr, raw.nbytes, inner.num_fragments, inner.num_rows, info["elem_szs"][k]))
            # JoinColumnTypeInfo as PerfectJoinHashTableBuilder fills it (Builders/PerfectHashTableBuilder.h:100-106):
            # {size, range min, range max, the column's own NULL, is_bitwise_eq, range max + 1, column kind}
            tis.append(A.JoinColumnTypeInfo(info["elem_szs"][k], info["mins"][k], info["maxs"][k], info["null_vals"][k],
                                            info["uses_bw_eq"], info["col_types"][k], info["translated_null_build"]))
        return jcs, tis, keep

    def _build_join_table(self, cp: CompiledPlan, ji: int, fuse_spec=None) -> DeviceBuffer:
        """HashJoin::getInstance / PerfectJoinHashTable::reify / BaselineJoinHashTable::reify for one
        device (QE/JoinHashTable/HashJoin.cpp:258-330): the table kind the plan names -- perfect or
        keyed, one-to-one or one-to-many -- built with the *_on_device entry points.  The plan chose
        one-to-one from the inner table's data; a duplicate showing up anyway (stale data) is reported
        like the reference's NeedsOneToManyHash."""
        info = cp.join_infos[ji]
        kind = info["kind"]
        key = (info["inner_table"], tuple(info["inner_cols"]), kind, info["uses_bw_eq"], info["for_semi_join"])
        if key in self._join_cache:
            return self._join_cache[key]
        L = lib()
        dev = self.device_id
        inner = self.storage.get(info["inner_table"])
        jcs, tis, keep = self._join_columns(inner, info)
        d_err = self.mgr.to_device(np.zeros(1, dtype=np.int32), dev)
        semi = info["for_semi_join"]
        fused_key = None
        if kind in (A.JOIN_ONE_TO_ONE, A.JOIN_ONE_TO_MANY):
            # HashEntryInfo{max - min + 1 (+ 1 for kBwEq), bucket_normalization}; the table has the NORMALISED count of
            # slots (initHashTableOnGpu, Builders/PerfectHashTableBuilder.h:82-130)
            hei = A.HashEntryInfo(info["hash_entry_count"], info["bucket"])
            entries = info["entry_count"]
            if entries <= 0 or entries > 2**31 - 1:
                raise QueryMustRunOnCpu("join key range too large for a perfect hash table (TooManyHashEntries)")
            if kind == A.JOIN_ONE_TO_ONE:
                table = self.mgr.alloc(entries * 4, dev)
                check(L.hdk_hip_init_hash_join_buff(table.ptr, entries, A.JOIN_INVALID_SLOT, dev, None))
                if fuse_spec is not None and fuse_spec[0][0] not in self._fused_cache:
                    # the table and its fused form in one sweep (hdk_hip_fill_hash_join_buff_fused: partitioned from a
                    # few million rows on, no gather through the row id)
                    (fkey, step), cols, stride = fuse_spec
                    ptrs, widths, kinds = step._payload_arrays(ji, cols)
                    fused = self.mgr.alloc(entries * stride * 8, dev)
                    sb = L.hdk_hip_join_build_scratch_bytes(inner.num_rows, entries, len(cols))
                    scratch = self.mgr.alloc(sb, dev) if sb else None
                    check(L.hdk_hip_fill_hash_join_buff_fused(table.ptr, A.JOIN_INVALID_SLOT, semi, d_err.ptr, jcs[0], tis[0],
                                                              max(info["bucket"], 1), ptrs, widths, kinds, len(cols), fused.ptr,
                                                              scratch.ptr if scratch else None, sb, dev, None))
                    self.mgr.synchronizeStream(dev)
                    if scratch:
                        scratch.free()
                    self._fused_cache[fkey] = fused
                    fused_key = fkey
                elif info["bucketized"]:
                    # (the reference always calls the bucketized fill for a one-to-one table, with bucket 1 for
                    # everything but a DATE key; the plain entry point is that call with bucket 1)
                    check(L.hdk_hip_fill_hash_join_buff_bucketized(table.ptr, A.JOIN_INVALID_SLOT, semi, d_err.ptr, jcs[0],
                                                                   tis[0], info["bucket"], dev, None))
                else:
                    check(L.hdk_hip_fill_hash_join_buff(table.ptr, A.JOIN_INVALID_SLOT, semi, d_err.ptr, jcs[0], tis[0],
                                                        dev, None))
            else:
                n32 = 2 * entries + inner.num_rows
                table = self.mgr.alloc(n32 * 4, dev)
                check(L.hdk_hip_init_hash_join_buff(table.ptr, n32, A.JOIN_INVALID_SLOT, dev, None))
                fill = L.hdk_hip_fill_one_to_many_hash_table_bucketized if info["bucketized"] else \
                    L.hdk_hip_fill_one_to_many_hash_table
                check(fill(table.ptr, hei, A.JOIN_INVALID_SLOT, jcs[0], tis[0], dev, None))
        else:
            kc, w, entries = len(info["inner_cols"]), info["key_width"], info["entry_count"]
            jc_arr = (A.JoinColumn * kc)(*jcs)
            ti_arr = (A.JoinColumnTypeInfo * kc)(*tis)
            one = kind == A.JOIN_KEYED_ONE_TO_ONE
            dict_bytes = entries * (kc + (1 if one else 0)) * w
            table = self.mgr.alloc(dict_bytes + (0 if one else (2 * entries + inner.num_rows) * 4), dev)
            check(L.hdk_hip_init_baseline_hash_join_buff(table.ptr, entries, kc, w, 1 if one else 0,
                                                         A.JOIN_INVALID_SLOT, dev, None))
            check(L.hdk_hip_fill_baseline_hash_join_buff(table.ptr, entries, A.JOIN_INVALID_SLOT, semi, kc, w,
                                                         1 if one else 0, d_err.ptr, jc_arr, ti_arr, dev, None))
            if not one:
                check(L.hdk_hip_fill_one_to_many_baseline_hash_table(table.ptr + dict_bytes, table.ptr, entries,
                                                                     A.JOIN_INVALID_SLOT, kc, w, jc_arr, ti_arr, dev, None))
        self.mgr.synchronizeStream(dev)
        err = int(self.mgr.to_host(d_err.ptr, 4, dev, np.int32)[0])
        d_err.free()
        for d in keep:
            d.free()
        if err != 0:
            table.free()
            if fused_key is not None:
                self._fused_cache.pop(fused_key).free()
            raise QueryMustRunOnCpu(f"join table build failed with code {err} (-1: duplicate key in a one-to-one "
                                    "table, PerfectHashTableBuilder.h:134-141 NeedsOneToManyHash; -2: stale metadata)")
        self._join_cache[key] = table
        return table

    def interrupt(self, value: int = 1):
        """Executor::interrupt (QE/GpuInterrupt.cpp): launches started with LAUNCH_CHECK_INTERRUPT stop with
        ERR_INTERRUPTED; interrupt(0) re-arms (DeviceKernel::initializeRuntimeInterrupter)."""
        check(lib().hdk_hip_set_interrupt(self.device_id, int(value)))

    def prepare(self, q, frag_ids: Optional[List[int]] = None, grid=0, flags=0,
                out_ptr: Optional[int] = None, watchdog_ms: int = 0) -> PreparedStep:
        cp = q if isinstance(q, CompiledPlan) else self.compile(q)
        outer = self.storage.get(cp.query.table)
        if frag_ids is None:
            frag_ids = list(range(outer.num_fragments))
        return PreparedStep(self, cp, frag_ids, grid=grid, flags=flags, out_ptr=out_ptr, watchdog_ms=watchdog_ms)

    def execute(self, q: QueryUnit, device_type: str = "GPU", frag_ids=None, result: str = "buffer", **kw):
        """-> ExecutionResult (the host copy of the buffer), or with result="columns" a DeviceColumns: the step's dense
        columns in device memory (PreparedStep.fetch_columns).  `q.table` and a join's `inner_table` may be a QueryUnit, a
        subquery (_execute_subquery): its result never leaves the device.  On a projection or a non-grouped QueryUnit, result_joins,
        result_setops, windows, select and the SortInfo are taken off the unit (plan.split_row_unit) and applied to its columns."""
        if device_type != "GPU":
            raise QueryMustRunOnCpu("hdk_amd ships the GPU path only; run device_type='CPU' on HDK itself")
        if result not in ("buffer", "columns"):
            raise ValueError(f"result must be 'buffer' or 'columns', not {result!r}")
        sq = q.query if isinstance(q, CompiledPlan) else q
        if isinstance(q, QueryUnit) and (isinstance(q.table, QueryUnit) or any(isinstance(j.inner_table, QueryUnit) for j in q.joins)):
            return self._execute_subquery(q, device_type, frag_ids, result, **kw)
        # a projection or a non-grouped unit: what compile_query refuses on it is applied to its dense columns below
        row_unit = isinstance(q, QueryUnit) and is_row_unit(q)
        if sq.result_setops and result == "buffer":
            raise ValueError("result_setops need result='columns': they combine the dense result columns, not a hash-table buffer")
        if (sq.result_joins or sq.result_setops) and not row_unit:
            if sq.result_joins and result == "buffer":
                raise ValueError("result_joins need result='columns': they join the dense result columns, not a hash-table buffer")
            if isinstance(q, CompiledPlan):
                raise ValueError("result_joins and result_setops are applied above compile_query: execute the QueryUnit itself")
            if not has_count_distinct(sq):
                # what follows the joins may name a joined column: the unit below them is compiled without it
                inner = dataclasses.replace(sq, result_joins=[], result_setops=[], having=[], windows=[], select=[], order_by=[],
                                            limit=None, offset=0)
                cols = self.execute(inner, device_type, frag_ids, "columns", **kw)
                return run_stages(cols, sq.having, sq.windows, sq.select, sq.order_by, sq.limit, sq.offset, sq.result_joins,
                                  sq.result_setops)
        if sq.windows and result == "buffer":
            raise ValueError("windows need result='columns': they read the dense result columns, not a hash-table buffer")
        if sq.select and result == "buffer":
            raise ValueError("select needs result='columns': it computes over the dense result columns, not a hash-table buffer")
        if has_count_distinct(sq):
            if result == "buffer":
                raise ValueError("count_distinct needs result='columns': it regroups the dense result columns of an inner "
                                 "GROUP BY, which no hash-table buffer holds")
            return self._execute_count_distinct(sq, frag_ids, **kw)
        sorts = bool(sq.order_by) or sq.limit is not None or bool(sq.offset)
        if sorts and result == "buffer":
            raise ValueError("order_by / limit / offset need result='columns': a hash-table buffer has no row order")
        if sq.having and result == "buffer":
            raise ValueError("having needs result='columns': it filters the dense result columns, not a hash-table buffer")
        if row_unit and (sq.result_joins or sq.result_setops or sq.windows or sq.select or sorts):
            if sq.result_joins and result == "buffer":
                raise ValueError("result_joins need result='columns': they join the dense result columns, not a hash-table buffer")
            if (sq.limit is not None and sq.limit < 0) or sq.offset < 0:
                raise ValueError("limit and offset must not be negative")
            cols = self.execute(split_row_unit(sq), device_type, frag_ids, "columns", **kw)
            return run_stages(cols, None, sq.windows, sq.select, sq.order_by, sq.limit, sq.offset, sq.result_joins,
                              sq.result_setops)
        # A QueryUnit whose open-addressing table the PLANNER sized (no baseline_entry_count): running out of slots means
        # the estimate was wrong (stale statistics, a key from an inner column) -- RelAlgExecutor::handleOutOfMemoryRetry
        # (QE/RelAlgExecutor.cpp:1713-1747) re-runs with a doubled max_groups_buffer_entry_guess, at most twice more, and
        # so does this.  A CompiledPlan or a caller-pinned entry count reports ERR_OUT_OF_SLOTS as before.
        retries_left = 2 if (isinstance(q, QueryUnit) and not q.baseline_entry_count) else 0
        guess = 0
        while True:
            step = self.prepare(q, frag_ids, **kw)
            try:
                if result == "columns":
                    step.enqueue()
                    return run_stages(step.fetch_columns(), step.cp.having, sq.windows, sq.select, sq.order_by, sq.limit,
                                      sq.offset)
                return step.run()
            except HdkHipError as e:
                if e.code != A.ERR_OUT_OF_SLOTS or step.cp.plan.query_kind != A.Q_BASELINE_HASH or retries_left == 0:
                    raise
                retries_left -= 1
                guess = max(2 * max(guess, int(step.cp.entry_count)), DEFAULT_MAX_GROUPS_BUFFER_ENTRY_GUESS)
                q = dataclasses.replace(q, baseline_entry_count=guess)
            finally:
                step.free()

    def _execute_count_distinct(self, q: QueryUnit, frag_ids=None, **kw) -> DeviceColumns:
        """COUNT(DISTINCT x) GROUP BY k in two steps (plan.split_count_distinct): the inner unit GROUP BY k, x as an
        ordinary plan with whatever kernels it is routed to, then DeviceColumns.group_by by k over its dense columns;
        HAVING and the SortInfo apply to the regrouped columns.  Every intermediate block is handed back."""
        inner, rg = split_count_distinct(q)
        cols = self.execute(inner, frag_ids=frag_ids, result="columns", **kw)
        out = _stage(cols, lambda c: c.group_by(rg.keys, rg.outs))
        return run_stages(out, rg.having, rg.windows, rg.select, rg.order_by, rg.limit, rg.offset, q.result_joins,
                          q.result_setops)
