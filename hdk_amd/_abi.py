"""ctypes mirror of include/hdk_hip.h (the C ABI's PODs and constants).

Pure interface definition: no compute, no library loading (that is `_lib.py`).
Field order and types must match include/hdk_hip.h exactly; tests/test_abi.py checks sizes
against the compiled library (`hdk_hip_sizeof_*`).
"""
import ctypes as C

# --- limits (hdk_hip.h) ---------------------------------------------------------------------
MAX_COLS = 24
MAX_KEYS = 4
MAX_TARGETS = 8
MAX_QUALS = 6
MAX_JOINS = 2
MAX_JOIN_KEYS = 3
MAX_EXPR_STEPS = 3
MAX_FILTER_OPS = 16
MAX_ORDER_ENTRIES = 8
MAX_HAVING_LEAVES = 8
MAX_GROUP_KEYS = 8
MAX_GROUP_OUTS = 16
MAX_WINDOW_KEYS = 8
MAX_WINDOW_OUTS = 8
MAX_PROJECT_OUTS = 8
MAX_PROJECT_OPS = 48
MAX_PROJECT_STACK = 6
MAX_PROJECT_INPUTS = 8
MAX_JOIN_COLUMNS_KEYS = 8  # hdk_hip_join_columns (MAX_JOIN_KEYS is the keyed storage-table join's)
MAX_JOIN_COLUMNS_OUTS = 32
JOIN_NULL_SAFE = 1  # hdk_hip_join_columns flags; its types are JOIN_INNER / JOIN_LEFT / JOIN_SEMI / JOIN_ANTI below
MAX_SETOP_COLUMNS = 8
MAX_SETOP_OUTS = 16
CONCAT_TAG_FIRST = 1  # hdk_hip_concat_columns flags
MAX_CHUNK_COLUMNS = 16  # hdk_hip_chunk_columns
KEYS_NULLS_MATCH = 1  # hdk_hip_key_multiplicity flags
SETOP_UNION, SETOP_INTERSECT, SETOP_INTERSECT_ALL, SETOP_EXCEPT, SETOP_EXCEPT_ALL = range(5)  # hdk_hip_setop
JOIN_NO_ROW = 0xFFFFFFFF  # rperm_out of an output row without a partner
SORT_NO_SELECT = 1  # hdk_hip_sort_columns flags
F_AND, F_OR, F_NOT = 64, 65, 66
PLAN_ABI = 4

# --- sentinels: reference omniscidb/Shared/InlineNullValues.h:33-39, QueryEngine/GpuRtConstants.h:29-32
EMPTY_KEY_64 = 2**63 - 1
EMPTY_KEY_32 = 2**31 - 1
EMPTY_KEY_16 = 2**15 - 1
EMPTY_KEY_8 = 2**7 - 1
NULL_BIGINT = -(2**63)
NULL_INT = -(2**31)
NULL_SMALLINT = -(2**15)
NULL_TINYINT = -(2**7)
NULL_DOUBLE_BITS = 0x0010000000000000  # DBL_MIN
NULL_FLOAT_BITS = 0x00800000  # FLT_MIN
FP_SLOT_NONE, FP_SLOT_DOUBLE, FP_SLOT_FLOAT = 0, 1, 2  # hdk_hip_fp_slot (target.arg_is_fp)
JOIN_INVALID_SLOT = -1

# --- status codes (reference QueryEngine/Execute.h:1019-1031 + library-level) ----------------
OK = 0
ERR_DIV_BY_ZERO = 1
ERR_OUT_OF_GPU_MEM = 2
ERR_OUT_OF_SLOTS = 3
ERR_OVERFLOW_OR_UNDERFLOW = 7
ERR_OUT_OF_TIME = 9
ERR_INTERRUPTED = 10
ERR_SINGLE_VALUE_FOUND_MULTIPLE_VALUES = 15
ERR_UNSUPPORTED = 100
ERR_INVALID_ARG = 101
ERR_RUNTIME = 102
ERR_EXCHANGE_INCOMPLETE = 103

# --- enums -----------------------------------------------------------------------------------
VC_INT, VC_FP = 0, 1
COL_INT, COL_UNSIGNED, COL_FLOAT, COL_DOUBLE, COL_SMALL_DATE = 0, 1, 2, 3, 4
LEAF_NONE, LEAF_COL, LEAF_INT, LEAF_FP = 0, 1, 2, 3
(OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_MOD, OP_EXTRACT_YEAR, OP_SCALE_DOWN, OP_FLOOR_DIV,
 OP_CAST_INT_TO_FP, OP_CAST_FP_TO_INT) = range(1, 11)
CMP_EQ, CMP_NE, CMP_LT, CMP_GT, CMP_LE, CMP_GE = range(1, 7)
JOIN_ONE_TO_ONE, JOIN_ONE_TO_MANY, JOIN_ONE_TO_ONE_FUSED, JOIN_KEYED_ONE_TO_ONE, JOIN_KEYED_ONE_TO_MANY = 0, 1, 2, 3, 4
JOIN_INNER, JOIN_LEFT, JOIN_SEMI, JOIN_ANTI = 0, 1, 2, 3
JOIN_NULL_NONE, JOIN_NULL_NULLABLE, JOIN_NULL_BITWISE = 0, 1, 2
Q_NON_GROUPED, Q_PERFECT_HASH, Q_BASELINE_HASH, Q_PROJECTION = 0, 1, 2, 3
AGG_COUNT, AGG_SUM, AGG_MIN, AGG_MAX, AGG_AVG, AGG_ID, AGG_SINGLE_VALUE = 0, 1, 2, 3, 4, 5, 6
# hdk_hip_window_kind (the order of the reference's WindowFunctionKind) and hdk_hip_window_frame
(WIN_ROW_NUMBER, WIN_RANK, WIN_DENSE_RANK, WIN_PERCENT_RANK, WIN_CUME_DIST, WIN_NTILE, WIN_LAG, WIN_LEAD, WIN_FIRST_VALUE,
 WIN_LAST_VALUE, WIN_AVG, WIN_MIN, WIN_MAX, WIN_SUM, WIN_COUNT) = range(15)
FRAME_ROWS, FRAME_RANGE, FRAME_PARTITION = 0, 1, 2
# hdk_hip_project_code and hdk_hip_project_flag
(P_PUSH_COL, P_PUSH_INT, P_PUSH_FP, P_PUSH_NULL_INT, P_PUSH_NULL_FP, P_ADD_I, P_SUB_I, P_MUL_I, P_DIV_I, P_MOD_I, P_ADD_F,
 P_SUB_F, P_MUL_F, P_DIV_F, P_CAST_I2F, P_CAST_F2I, P_CMP_I, P_CMP_F, P_AND, P_OR, P_NOT, P_IS_NULL, P_SELECT) = range(1, 24)
P_FLAG_NULLABLE, P_FLAG_FP = 1, 2
JC_SMALL_DATE, JC_SIGNED, JC_UNSIGNED, JC_DOUBLE = 0, 1, 2, 3
(KP_COL_BUFFERS, KP_NUM_FRAGMENTS, KP_LITERALS, KP_NUM_ROWS, KP_FRAG_ROW_OFFSETS, KP_MAX_MATCHED,
 KP_TOTAL_MATCHED, KP_INIT_AGG_VALS, KP_GROUPBY_BUF, KP_ERROR_CODE, KP_NUM_TABLES,
 KP_JOIN_HASH_TABLES, KP_COUNT) = range(13)
LAUNCH_FORCE_GLOBAL_ATOMICS = 1
LAUNCH_RECORD_EVENTS = 2
LAUNCH_FORCE_GENERIC = 4
LAUNCH_FORCE_SCALAR = 8
LAUNCH_FORCE_PARTITIONED = 16
LAUNCH_WIDE_TUPLES = 1024
LAUNCH_ACCUMULATE = 2048
LAUNCH_PLAN_RESIDENT = 32
LAUNCH_CHECK_INTERRUPT = 64
LAUNCH_INIT_OUTPUT = 128
LAUNCH_CLUSTER_PROBES = 256
LAUNCH_NO_CLUSTER_PROBES = 512


class Col(C.Structure):
    _fields_ = [("buf_idx", C.c_int32), ("table", C.c_int32), ("width", C.c_int32),
                ("kind", C.c_int32),
                # ChunkStats of the column over the launch's fragments (DataMgr/ChunkMetadata.h); has_stats = 0: unknown
                ("has_stats", C.c_int32), ("has_nulls", C.c_int32), ("min_val", C.c_int64), ("max_val", C.c_int64)]


class Leaf(C.Structure):
    _fields_ = [("kind", C.c_int32), ("col", C.c_int32), ("ival", C.c_int64),
                ("null_val", C.c_int64), ("nullable", C.c_int32), ("pad_", C.c_int32)]


class Step(C.Structure):
    _fields_ = [("op", C.c_int32), ("out_class", C.c_int32), ("rhs", Leaf),
                ("null_out", C.c_int64), ("check_width", C.c_int32), ("pad_", C.c_int32)]


class Expr(C.Structure):
    _fields_ = [("vclass", C.c_int32), ("nsteps", C.c_int32), ("leaf0", Leaf),
                ("steps", Step * MAX_EXPR_STEPS), ("null_val", C.c_int64),
                ("nullable", C.c_int32), ("pad_", C.c_int32)]


class Qual(C.Structure):
    _fields_ = [("lhs", Expr), ("rhs", Leaf), ("cmp", C.c_int32), ("after_joins", C.c_int32)]


class Join(C.Structure):
    _fields_ = [("outer_key", Expr), ("min_key", C.c_int64), ("max_key", C.c_int64),
                ("null_val", C.c_int64), ("translated_null", C.c_int64), ("bucket", C.c_int64),
                ("kind", C.c_int32), ("type", C.c_int32), ("null_mode", C.c_int32),
                ("table_idx", C.c_int32), ("fused_stride", C.c_int32), ("key_component_count", C.c_int32),
                ("entry_count", C.c_int64), ("key_component_width", C.c_int32), ("pad_", C.c_int32),
                ("extra_keys", Expr * (MAX_JOIN_KEYS - 1))]


class Target(C.Structure):
    _fields_ = [("agg", C.c_int32), ("has_arg", C.c_int32), ("arg", Expr),
                ("skip_null", C.c_int32), ("slot_width", C.c_int32), ("slot_off", C.c_int32),
                ("slot2_width", C.c_int32), ("slot2_off", C.c_int32), ("arg_is_fp", C.c_int32),
                ("key_idx", C.c_int32), ("pad_", C.c_int32), ("null_val", C.c_int64)]


class Plan(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("query_kind", C.c_int32),
                ("num_cols", C.c_int32), ("cols", Col * MAX_COLS),
                ("num_quals", C.c_int32), ("quals", Qual * MAX_QUALS),
                ("num_filter_ops", C.c_int32), ("filter_after_joins", C.c_int32),
                ("filter_ops", C.c_uint8 * MAX_FILTER_OPS),
                ("num_joins", C.c_int32), ("joins", Join * MAX_JOINS),
                ("key_count", C.c_int32), ("keys", Expr * MAX_KEYS),
                ("key_min", C.c_int64 * MAX_KEYS), ("key_bucket", C.c_int64 * MAX_KEYS),
                ("key_card", C.c_int64 * MAX_KEYS), ("key_null_translated", C.c_int64 * MAX_KEYS),
                ("key_has_nulls", C.c_int32 * MAX_KEYS),
                ("entry_count", C.c_uint32), ("key_width", C.c_int32), ("keyless", C.c_int32),
                ("idx_target_as_key", C.c_int32),
                ("output_columnar", C.c_int32), ("row_size_quad", C.c_uint32),
                ("num_targets", C.c_int32), ("targets", Target * MAX_TARGETS)]


class ExchangeShape(C.Structure):
    """hdk_hip_exchange_shape: geometry of the multi-GPU tuple exchange (include/hdk_hip.h)."""
    _fields_ = [("num_owners", C.c_uint32), ("owner_entry_count", C.c_uint32), ("tuple_bytes", C.c_uint32),
                ("coarse_per_owner", C.c_uint32), ("regions_log2", C.c_uint32), ("reserved_", C.c_uint32),
                ("sub_slab_tuples", C.c_uint64), ("segment_header_bytes", C.c_uint64), ("segment_bytes", C.c_uint64),
                ("rows_bound", C.c_uint64), ("scatter_workspace_bytes", C.c_uint64),
                ("aggregate_workspace_bytes", C.c_uint64)]


class OrderEntry(C.Structure):
    """hdk_hip_order_entry: one ORDER BY entry over dense result columns (hdk_hip_sort_columns)."""
    _fields_ = [("col", C.c_int32), ("is_desc", C.c_uint8), ("nulls_first", C.c_uint8), ("is_fp", C.c_uint8),
                ("nullable", C.c_uint8), ("null_bits", C.c_int64)]


class HavingLeaf(C.Structure):
    """hdk_hip_having_leaf: one comparison of a HAVING predicate over dense result columns (hdk_hip_filter_columns):
    column lhs_col <cmp> column rhs_col or the literal rhs_lit.  A side is NULL when it is nullable and its word equals
    null_bits (a literal never is); cmp_fp compares as doubles, an int64 side converted with (double)."""
    _fields_ = [("lhs_col", C.c_int32), ("rhs_col", C.c_int32), ("cmp", C.c_uint8), ("rhs_is_col", C.c_uint8),
                ("cmp_fp", C.c_uint8), ("lhs_is_fp", C.c_uint8), ("lhs_nullable", C.c_uint8), ("rhs_is_fp", C.c_uint8),
                ("rhs_nullable", C.c_uint8), ("pad_", C.c_uint8), ("lhs_null_bits", C.c_int64),
                ("rhs_null_bits", C.c_int64), ("rhs_lit", C.c_int64)]


class GroupOut(C.Structure):
    """hdk_hip_group_out: one output of a GROUP BY over dense result columns (hdk_hip_group_columns): ID of a key column,
    COUNT (col < 0: the rows of the run), SUM, MIN or MAX of column `col`, whose word is NULL when the out is nullable and
    the word equals null_bits."""
    _fields_ = [("col", C.c_int32), ("kind", C.c_uint8), ("is_fp", C.c_uint8), ("nullable", C.c_uint8), ("pad_", C.c_uint8),
                ("null_bits", C.c_int64)]


class WindowOut(C.Structure):
    """hdk_hip_window_out: one output of hdk_hip_window_columns: a ranking kind, LAG / LEAD (param = k), NTILE (param = n),
    FIRST_VALUE / LAST_VALUE or an aggregate of column `col` over the frame, whose word is NULL when the out is nullable and
    the word equals null_bits."""
    _fields_ = [("col", C.c_int32), ("kind", C.c_uint8), ("frame", C.c_uint8), ("is_fp", C.c_uint8), ("nullable", C.c_uint8),
                ("null_bits", C.c_int64), ("param", C.c_int64)]


class ProjectOp(C.Structure):
    """hdk_hip_project_op: one postfix op of hdk_hip_project_columns.  flags: P_FLAG_* for P_PUSH_COL, the CMP_* code for
    P_CMP_I / P_CMP_F; imm: the column's in-band NULL, or the literal (a double's bits for P_PUSH_FP)."""
    _fields_ = [("code", C.c_uint8), ("check_width", C.c_uint8), ("flags", C.c_uint8), ("pad_", C.c_uint8), ("col", C.c_uint32),
                ("imm", C.c_int64)]


class ProjectOut(C.Structure):
    """hdk_hip_project_out: one output of hdk_hip_project_columns: ops[first_op .. first_op + num_ops) leave its value, a
    NULL result stores null_bits."""
    _fields_ = [("first_op", C.c_int32), ("num_ops", C.c_int32), ("is_fp", C.c_uint8), ("nullable", C.c_uint8),
                ("pad_", C.c_uint8 * 6), ("null_bits", C.c_int64)]


class JoinKey(C.Structure):
    """hdk_hip_join_key: one key of hdk_hip_join_columns: left column lcol = right column rcol, int64 words; a word is NULL
    when its side is nullable and the word equals that side's null_bits."""
    _fields_ = [("lcol", C.c_int32), ("rcol", C.c_int32), ("lnullable", C.c_uint8), ("rnullable", C.c_uint8),
                ("pad_", C.c_uint8 * 6), ("lnull_bits", C.c_int64), ("rnull_bits", C.c_int64)]


class JoinOut(C.Structure):
    """hdk_hip_join_out: one output column of hdk_hip_join_columns: column `col` of the left (side 0) or right (side 1)
    block; null_bits is what a right out holds for a LEFT join's row without a partner."""
    _fields_ = [("side", C.c_uint8), ("pad_", C.c_uint8 * 3), ("col", C.c_int32), ("null_bits", C.c_int64)]


class SetopCol(C.Structure):
    """hdk_hip_setop_col: one column pair of hdk_hip_concat_columns: left column lcol and right column rcol become one output
    column; a word that is NULL on its side (side nullable, word equal to that side's null_bits) is written as
    out_null_bits."""
    _fields_ = [("lcol", C.c_int32), ("rcol", C.c_int32), ("lnullable", C.c_uint8), ("rnullable", C.c_uint8),
                ("pad_", C.c_uint8 * 6), ("lnull_bits", C.c_int64), ("rnull_bits", C.c_int64), ("out_null_bits", C.c_int64)]


class ChunkCol(C.Structure):
    """hdk_hip_chunk_col: one selected column of hdk_hip_chunk_columns: input column `col`; a word of a nullable column that
    equals null_bits is written as out_null_bits, the NULL of the 8-byte storage type."""
    _fields_ = [("col", C.c_int32), ("is_fp", C.c_uint8), ("nullable", C.c_uint8), ("pad_", C.c_uint8 * 2),
                ("null_bits", C.c_int64), ("out_null_bits", C.c_int64)]


class ChunkStatsRecord(C.Structure):
    """hdk_hip_chunk_stats: what hdk_hip_chunk_columns leaves per (column, fragment); min_bits / max_bits are meaningful
    only when value_count > 0 (an fp fragment of NaNs only: min_bits = +inf, max_bits = -inf)."""
    _fields_ = [("min_bits", C.c_int64), ("max_bits", C.c_int64), ("null_count", C.c_uint64), ("value_count", C.c_uint64)]


class MultiplicityKey(C.Structure):
    """hdk_hip_multiplicity_key: one key column of hdk_hip_key_multiplicity; min_val / max_val / translated_null are the
    JoinColumnTypeInfo of the perfect table (read on the perfect route only)."""
    _fields_ = [("col", C.c_int32), ("nullable", C.c_uint8), ("pad_", C.c_uint8 * 3), ("null_bits", C.c_int64),
                ("min_val", C.c_int64), ("max_val", C.c_int64), ("translated_null", C.c_int64)]


class KeyMultiplicityResult(C.Structure):
    """hdk_hip_key_multiplicity_result: the record hdk_hip_key_multiplicity leaves."""
    _fields_ = [("max_matches", C.c_uint64), ("occupied", C.c_uint64), ("rows_filed", C.c_uint64),
                ("rows_out_of_range", C.c_uint64)]


class KernelOptions(C.Structure):
    _fields_ = [("grid_dim_x", C.c_uint32), ("block_dim_x", C.c_uint32),
                ("shared_mem_bytes", C.c_uint32), ("flags", C.c_uint32), ("total_rows", C.c_uint64),
                ("watchdog_ms", C.c_uint32), ("reserved_", C.c_uint32)]


class DeviceProperties(C.Structure):
    _fields_ = [("global_mem", C.c_size_t), ("num_cu", C.c_int32),
                ("max_threads_per_block", C.c_int32), ("wavefront_size", C.c_int32),
                ("grid_size", C.c_int32), ("shared_mem_per_block", C.c_size_t),
                ("has_shared_memory_atomics", C.c_int32), ("can_load_async", C.c_int32),
                ("has_fp64", C.c_int32), ("clock_khz", C.c_int32),
                ("memory_clock_khz", C.c_int32), ("memory_bus_width", C.c_int32),
                ("arch_name", C.c_char * 64)]


class JoinChunk(C.Structure):
    _fields_ = [("col_buff", C.c_void_p), ("num_elems", C.c_size_t), ("row_id", C.c_size_t)]


class JoinColumn(C.Structure):
    _fields_ = [("col_chunks_buff", C.c_void_p), ("col_chunks_buff_sz", C.c_size_t),
                ("num_chunks", C.c_size_t), ("num_elems", C.c_size_t), ("elem_sz", C.c_size_t)]


class JoinColumnTypeInfo(C.Structure):
    _fields_ = [("elem_sz", C.c_size_t), ("min_val", C.c_int64), ("max_val", C.c_int64),
                ("null_val", C.c_int64), ("uses_bw_eq", C.c_int32), ("column_type", C.c_int32),
                ("translated_null_val", C.c_int64)]


class HashEntryInfo(C.Structure):
    _fields_ = [("hash_entry_count", C.c_size_t), ("bucket_normalization", C.c_int64)]


def to_i64(v: int) -> int:
    """Wrap a Python int into the signed 64-bit range (two's complement)."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v
