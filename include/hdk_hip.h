/*
 * hdk_hip.h -- C ABI of the MI355X (gfx950) operator library for HDK's per-fragment hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers / sizes / PODs, returns an int32 status
 * (0 = ok; 1..16 = HDK's own Executor error codes, reference omniscidb/QueryEngine/Execute.h:1019-1031;
 * <0 = out of slots, as in RuntimeFunctions.cpp:1123-1135) and never lets an exception cross the
 * boundary.  `hdk_hip_last_error()` returns a thread-local message for the last non-zero status.
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference
 * root, `QE/` = omniscidb/QueryEngine/).  INTEGRATION.md shows the HDK-side bindings
 * (HipMgr : GpuMgr, HipKernel : DeviceKernel, the *_on_device free functions).
 *
 * The JIT'ed row function that HDK generates per query (QE/RowFuncBuilder.cpp,
 * QE/QueryTemplateGenerator.cpp) is replaced by a POD *plan* (`hdk_hip_plan`) interpreted by a
 * fixed library of hand-written kernels; shapes the library does not cover are rejected with
 * HDK_HIP_ERR_UNSUPPORTED so the caller can take HDK's existing QueryMustRunOnCpu retry
 * (QE/RelAlgExecutor.cpp:183-192).
 */
#ifndef HDK_HIP_H
#define HDK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Constants shared with the reference
 * ---------------------------------------------------------------------------------------- */
#define HDK_EMPTY_KEY_64 INT64_MAX /* QE/GpuRtConstants.h:29 */
#define HDK_EMPTY_KEY_32 INT32_MAX /* :30 */
#define HDK_EMPTY_KEY_16 INT16_MAX /* :31 */
#define HDK_EMPTY_KEY_8 INT8_MAX   /* :32 */
#define HDK_NULL_BIGINT INT64_MIN  /* Shared/InlineNullValues.h:37 */
#define HDK_NULL_INT INT32_MIN
#define HDK_NULL_SMALLINT INT16_MIN
#define HDK_NULL_TINYINT INT8_MIN
/* NULL_DOUBLE = DBL_MIN, NULL_FLOAT = FLT_MIN (smallest positive normal), compared bit-wise. */
#define HDK_NULL_DOUBLE_BITS INT64_C(0x0010000000000000)
#define HDK_NULL_FLOAT_BITS INT32_C(0x00800000)
#define HDK_JOIN_INVALID_SLOT (-1) /* QE/JoinHashTable/Runtime/JoinHashTableQueryRuntime.cpp:38 */

/* status / error codes: QE/Execute.h:1019-1031 */
#define HDK_HIP_OK 0
#define HDK_HIP_ERR_DIV_BY_ZERO 1
#define HDK_HIP_ERR_OUT_OF_GPU_MEM 2
#define HDK_HIP_ERR_OUT_OF_SLOTS 3
#define HDK_HIP_ERR_OVERFLOW_OR_UNDERFLOW 7
#define HDK_HIP_ERR_OUT_OF_TIME 9
#define HDK_HIP_ERR_INTERRUPTED 10
#define HDK_HIP_ERR_SINGLE_VALUE_FOUND_MULTIPLE_VALUES 15
/* library-level failures (not produced by HDK's runtime): */
#define HDK_HIP_ERR_UNSUPPORTED 100 /* plan shape outside the fixed library -> QueryMustRunOnCpu */
#define HDK_HIP_ERR_INVALID_ARG 101
#define HDK_HIP_ERR_RUNTIME 102 /* a HIP runtime call failed; see hdk_hip_last_error() */
#define HDK_HIP_ERR_EXCHANGE_INCOMPLETE 103 /* device code of hdk_hip_aggregate_from_ranks: a rank's segment was flagged
                                               (a sub-slab overflowed: skewed keys; stale column statistics; or the
                                               scatter was interrupted), or the owner's spill list overflowed (its
                                               table is all but full) -- redo the step with the table exchange.  A
                                               heavy hitter that only overflows the OWNER's slabs is not an error: the
                                               owner then applies its inbox with atomics (hdk_part_owner_fallback) */
#define HDK_HIP_ERR_JOIN_SLOT_TAKEN (-1) /* one-to-one build hit a duplicate key (JoinHashImpl.h:55-66) */

const char* hdk_hip_last_error(void);
/* Library/ABI version (major*1000+minor). */
int32_t hdk_hip_version(void);

/* ------------------------------------------------------------------------------------------
 * HipMgr -- device manager under BufferProvider.
 * Replaces CudaMgr/L0Manager behind `struct GpuMgr` (omniscidb/DataMgr/GpuMgr.h:29-79,
 * omniscidb/CudaMgr/CudaMgr.h:83-260); one function per virtual.  There is no handle: state is a
 * per-device table (stream, properties) initialised lazily and thread-safe.
 * ---------------------------------------------------------------------------------------- */
int32_t hdk_hip_mgr_get_device_count(int32_t* count);               /* GpuMgr::getDeviceCount */
int32_t hdk_hip_mgr_set_context(int32_t device_num);                /* GpuMgr::setContext */
int32_t hdk_hip_mgr_allocate_device_mem(size_t num_bytes, int32_t device_num,
                                        int8_t** device_ptr);       /* GpuMgr::allocateDeviceMem;
                                                                       OOM -> ERR_OUT_OF_GPU_MEM */
int32_t hdk_hip_mgr_free_device_mem(int8_t* device_ptr);            /* GpuMgr::freeDeviceMem */
int32_t hdk_hip_mgr_allocate_pinned_host_mem(size_t num_bytes, int8_t** host_ptr); /* CudaMgr.h:120 */
int32_t hdk_hip_mgr_free_pinned_host_mem(int8_t* host_ptr);
int32_t hdk_hip_mgr_copy_host_to_device(int8_t* device_ptr, const int8_t* host_ptr, size_t num_bytes,
                                        int32_t device_num);        /* GpuMgr::copyHostToDevice */
int32_t hdk_hip_mgr_copy_host_to_device_async(int8_t* device_ptr, const int8_t* host_ptr,
                                              size_t num_bytes, int32_t device_num);
int32_t hdk_hip_mgr_synchronize_stream(int32_t device_num);         /* GpuMgr::synchronizeStream */
int32_t hdk_hip_mgr_copy_device_to_host(int8_t* host_ptr, const int8_t* device_ptr, size_t num_bytes,
                                        int32_t device_num);        /* GpuMgr::copyDeviceToHost */
int32_t hdk_hip_mgr_copy_device_to_device(int8_t* dest_ptr, int8_t* src_ptr, size_t num_bytes,
                                          int32_t dest_device_num, int32_t src_device_num);
int32_t hdk_hip_mgr_zero_device_mem(int8_t* device_ptr, size_t num_bytes, int32_t device_num);
int32_t hdk_hip_mgr_set_device_mem(int8_t* device_ptr, unsigned char uc, size_t num_bytes,
                                   int32_t device_num);
int32_t hdk_hip_mgr_synchronize_devices(void);                      /* GpuMgr::synchronizeDevices */
/* The per-device stream the manager's async copies and (when `stream`==NULL) the kernels use. */
int32_t hdk_hip_mgr_get_stream(int32_t device_num, void** stream);

typedef struct hdk_hip_device_properties { /* CudaMgr.h:43-66 `DeviceProperties` */
  size_t global_mem;                /* GpuMgr::getTotalMem */
  int32_t num_cu;                   /* GpuMgr::getMinEUNumForAllDevices (256 on MI355X) */
  int32_t max_threads_per_block;    /* GpuMgr::getMaxBlockSize */
  int32_t wavefront_size;           /* GpuMgr::getSubGroupSize -> 64 on CDNA4 */
  int32_t grid_size;                /* GpuMgr::getGridSize: blocks a persistent launch uses */
  size_t shared_mem_per_block;      /* GpuMgr::getMinSharedMemoryPerBlockForAllDevices */
  int32_t has_shared_memory_atomics;/* GpuMgr::hasSharedMemoryAtomicsSupport -> 1 */
  int32_t can_load_async;           /* GpuMgr::canLoadAsync -> 1 */
  int32_t has_fp64;                 /* GpuMgr::hasFP64Support -> 1 */
  int32_t clock_khz;
  int32_t memory_clock_khz;
  int32_t memory_bus_width;
  char arch_name[64];               /* "gfx950..." */
} hdk_hip_device_properties;
int32_t hdk_hip_mgr_get_device_properties(int32_t device_num, hdk_hip_device_properties* out);
/* Measurement helper (no reference counterpart): what plain streaming kernels reach on this device -- a 16 B/lane
 * copy (bytes read + written per second) and a 16 B/lane read, best of `reps` over `bytes` of scratch.  bench.py
 * reports them as roofline.peak_measured next to the nominal 8 TB/s. */
int32_t hdk_hip_mgr_measure_hbm(int32_t device_num, size_t bytes, int32_t reps, double* copy_gbps, double* read_gbps);

/* ------------------------------------------------------------------------------------------
 * Output-buffer initialisation (kernel #1 of every group-by launch).
 * Replaces init_group_by_buffer_on_device / init_columnar_group_by_buffer_on_device
 * (QE/GpuInitGroups.h:23-48, kernels QE/GpuInitGroups.cu:17-232).  Same arguments minus the
 * platform enum, plus device + stream.  block/grid sizes are accepted for signature parity and
 * only used as hints.
 * ---------------------------------------------------------------------------------------- */
int32_t hdk_hip_init_group_by_buffer(int64_t* groups_buffer, const int64_t* init_vals,
                                     uint32_t groups_buffer_entry_count, uint32_t key_count,
                                     uint32_t key_width, uint32_t row_size_quad, int32_t keyless,
                                     int8_t warp_size, size_t block_size_x, size_t grid_size_x,
                                     int32_t device_id, void* stream);
int32_t hdk_hip_init_columnar_group_by_buffer(int64_t* groups_buffer, const int64_t* init_vals,
                                              uint32_t groups_buffer_entry_count, uint32_t key_count,
                                              uint32_t agg_col_count, const int8_t* col_sizes,
                                              int32_t need_padding, int32_t keyless, int8_t key_size,
                                              size_t block_size_x, size_t grid_size_x,
                                              int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * The plan: POD replacement for the JIT'ed row function.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_MAX_COLS 24
#define HDK_HIP_MAX_KEYS 4
#define HDK_HIP_MAX_TARGETS 8
#define HDK_HIP_MAX_QUALS 6
#define HDK_HIP_MAX_JOINS 2
#define HDK_HIP_MAX_JOIN_KEYS 3 /* key components of a keyed (composite-key) join */
#define HDK_HIP_MAX_EXPR_STEPS 3
#define HDK_HIP_MAX_FILTER_OPS 16
enum hdk_hip_filter_op { HDK_F_AND = 64, HDK_F_OR = 65, HDK_F_NOT = 66 }; /* < 64: push quals[op] */

enum hdk_hip_value_class { HDK_VC_INT = 0, HDK_VC_FP = 1 };

/* How a fixed-width column element is decoded (QE/DecodersImpl.h:30-150). */
enum hdk_hip_col_kind {
  HDK_COL_INT = 0,      /* fixed_width_int_decode: sign-extend 1/2/4/8 bytes */
  HDK_COL_UNSIGNED = 1, /* fixed_width_unsigned_decode (dictionary ids of 1/2 bytes) */
  HDK_COL_FLOAT = 2,    /* fixed_width_float_decode, widened to double */
  HDK_COL_DOUBLE = 3,   /* fixed_width_double_decode */
  HDK_COL_SMALL_DATE = 4 /* fixed_width_small_date_decode (QE/DecodersImpl.h:151-159; chosen by get_col_decoder for a DATE
                           stored in days, QE/ColumnIR.cpp:46-49): a 2- or 4-byte day count, read as epoch SECONDS
                           (x 86400); the column's narrow NULL (INT16_MIN / INT32_MIN, QE/Codec.cpp:86-87) becomes
                           NULL_BIGINT.  Read by the plan interpreters only (no specialised kernel takes such a column) */
};

typedef struct hdk_hip_col {
  int32_t buf_idx;   /* index into col_buffers[frag][...] (the COL_BUFFERS kernel param) */
  int32_t table;     /* 0 = outer table (row = pos); j>0 = inner table of join j-1 (row = matched id);
                        -j (j>0) = PAYLOAD word `buf_idx` of join j-1's fused table (see
                        HDK_JOIN_ONE_TO_ONE_FUSED): no column buffer is read */
  int32_t width;     /* bytes per element */
  int32_t kind;      /* hdk_hip_col_kind */
  /* Statistics of the column over the fragments of the launch: the ChunkStats {min, max, has_nulls} every chunk's
   * metadata carries (omniscidb/DataMgr/ChunkMetadata.h) and the reference's planner reads through
   * getExpressionRange (QE/ExpressionRange.cpp) to choose hash layouts.  Here they also let a multi-pass strategy
   * move a column in fewer bytes than its physical width (8-byte tuples in the radix-partitioned group-by when key
   * and argument both fit 32 bits).  Optional: has_stats = 0 means unknown.  They must hold for every element read;
   * the kernels that rely on them notice a value outside and redo the launch at full width (no wrong result from
   * stale metadata, only a slower one). */
  int32_t has_stats; /* 1: min_val / max_val / has_nulls below are valid (integer columns only) */
  int32_t has_nulls; /* ChunkStats::has_nulls: some element is the in-band NULL */
  int64_t min_val;   /* bounds of the non-NULL elements */
  int64_t max_val;
} hdk_hip_col;

/* Expression: a short left-to-right chain  acc = leaf0; acc = op_i(acc, leaf_i)  i < nsteps.
 * Integer values are carried as int64, fp as double.  NULLs stay in-band exactly like the
 * reference's *_nullable runtime functions (QE/RuntimeFunctions.cpp:49-230): each step names the
 * sentinel of its inputs and of its result. */
enum hdk_hip_leaf_kind { HDK_LEAF_NONE = 0, HDK_LEAF_COL = 1, HDK_LEAF_INT = 2, HDK_LEAF_FP = 3 };
typedef struct hdk_hip_leaf {
  int32_t kind;     /* hdk_hip_leaf_kind */
  int32_t col;      /* index into plan->cols when kind == HDK_LEAF_COL */
  int64_t ival;     /* literal (int), or bit pattern of the double literal */
  int64_t null_val; /* in-band NULL of this leaf, widened (int) or double bits (fp); */
  int32_t nullable; /* 0 => the leaf can never be NULL (null_val ignored) */
  int32_t pad_;
} hdk_hip_leaf;

enum hdk_hip_op {
  HDK_OP_ADD = 1, HDK_OP_SUB, HDK_OP_MUL, HDK_OP_DIV, HDK_OP_MOD, /* DEF_ARITH_NULLABLE */
  HDK_OP_EXTRACT_YEAR,     /* omniscidb/Utils/ExtractFromTime.cpp: extract_year on epoch seconds */
  HDK_OP_SCALE_DOWN,       /* scale_decimal_down_[not_]nullable (RuntimeFunctions.cpp:245-262) */
  HDK_OP_FLOOR_DIV,        /* floor_div_[nullable_]lhs (:266-279) */
  HDK_OP_CAST_INT_TO_FP,   /* cast_int64_t_to_double_nullable (:311-345) */
  HDK_OP_CAST_FP_TO_INT    /* DEF_ROUND_NULLABLE(double,int64_t) */
};
typedef struct hdk_hip_step {
  int32_t op;        /* hdk_hip_op */
  int32_t out_class; /* hdk_hip_value_class of the result */
  hdk_hip_leaf rhs;  /* second operand (unused by unary ops) */
  int64_t null_out;  /* in-band NULL of the result */
  int32_t check_width; /* + - * on integers: byte width (1/2/4/8) of the operation's SQL type; a result outside that
                          type's range ends the query with ERR_OVERFLOW_OR_UNDERFLOW, like the checked arithmetic the
                          reference generates (QE/ArithmeticIR.cpp:277-520; NULL operands are not checked).  0: unchecked */
  int32_t pad_;
} hdk_hip_step;
typedef struct hdk_hip_expr {
  int32_t vclass;    /* value class of the final result */
  int32_t nsteps;
  hdk_hip_leaf leaf0;
  hdk_hip_step steps[HDK_HIP_MAX_EXPR_STEPS];
  int64_t null_val;  /* in-band NULL of the final result */
  int32_t nullable;  /* whether the result may be NULL */
  int32_t pad_;
} hdk_hip_expr;

/* Filter conjunct `lhs cmp rhs`, three-valued (DEF_CMP_NULLABLE, RuntimeFunctions.cpp:83-117);
 * a row passes when every conjunct is TRUE (logical_and, :357-372; NULL does not pass). */
enum hdk_hip_cmp { HDK_CMP_EQ = 1, HDK_CMP_NE, HDK_CMP_LT, HDK_CMP_GT, HDK_CMP_LE, HDK_CMP_GE };
typedef struct hdk_hip_qual {
  hdk_hip_expr lhs;
  hdk_hip_leaf rhs;
  int32_t cmp;
  int32_t after_joins; /* 0: reads outer-table columns only, evaluated before any probe (the reference
                          hoists such filters in front of the join loops, IRCodegen.cpp:569-570);
                          1: reads joined columns, evaluated once per matching row combination */
} hdk_hip_qual;

/* Equi-join probe.  Perfect-hash tables: hash_join_idx family (QE/GroupByRuntime.cpp:274-366);
 * keyed ("baseline") tables: baseline_hash_join_idx_{32,64}
 * (QE/JoinHashTable/Runtime/JoinHashTableQueryRuntime.cpp:42-98).  The join loops follow
 * Executor::buildJoinLoops (QE/IRCodegen.cpp:497-667): a one-to-one table yields at most one inner
 * row (JoinLoopKind::Singleton), a one-to-many table a set of them (JoinLoopKind::Set, the matching
 * set of HashJoin::codegenMatchingSet, QE/JoinHashTable/HashJoin.cpp:149-197); a LEFT join with no
 * match runs the rest of the row once with every column of the inner table NULL. */
enum hdk_hip_join_kind {
  HDK_JOIN_ONE_TO_ONE = 0,  /* the reference's table: int32 row id per slot (PerfectHashTableBuilder.h:35-38) */
  HDK_JOIN_ONE_TO_MANY = 1, /* int32 [offsets(entry_count) | counts(entry_count) | row ids]
                               (fill_one_to_many_hash_table, HashJoinRuntime.cpp:770-853) */
  /* MI355X addition (no reference counterpart): int64 entries [row id | payload 1 | ... ] per slot,
   * `fused_stride` quads apart, built by hdk_hip_build_fused_join_table from the reference table and
   * the referenced inner columns.  One 16..32-B gather per probing row replaces the dependent
   * slot -> row id -> inner column chain (two cache lines) of the reference layout. */
  HDK_JOIN_ONE_TO_ONE_FUSED = 2,
  /* keyed tables (wide or composite keys), key components `key_component_width` bytes wide:
   *   one-to-one : entry_count x [key components | row id]        (width-sized row id)
   *   one-to-many: entry_count x [key components], then int32 [offsets | counts | row ids]
   * (BaselineJoinHashTable layout, QE/JoinHashTable/Runtime/HashJoinRuntime.cpp:357-507,855-1000) */
  HDK_JOIN_KEYED_ONE_TO_ONE = 3,
  HDK_JOIN_KEYED_ONE_TO_MANY = 4
};
enum hdk_hip_join_type {
  HDK_JOIN_INNER = 0,
  HDK_JOIN_LEFT = 1,
  /* JoinType::SEMI / ANTI (Shared/sqldefs.h:33; JoinLoop::codegen, QE/LoopControlFlow/JoinLoop.cpp:254-262): the table
   * is a one-to-one table filled with for_semi_join = 1 (first row of a key wins, duplicates are not an error:
   * fill_hashtable_for_semi_join, JoinHashImpl.h:68-77).  SEMI runs the rest of the row when the probe finds a slot
   * (exactly like INNER over that table: every outer row at most once), ANTI when it finds none (`slot_lookup_result
   * < 0`); an ANTI join's inner columns are never read. */
  HDK_JOIN_SEMI = 2,
  HDK_JOIN_ANTI = 3
};
enum hdk_hip_join_null { HDK_JOIN_NULL_NONE = 0, HDK_JOIN_NULL_NULLABLE = 1, HDK_JOIN_NULL_BITWISE = 2 };
typedef struct hdk_hip_join {
  hdk_hip_expr outer_key;
  int64_t min_key;
  int64_t max_key;
  int64_t null_val;
  int64_t translated_null; /* [bucketized_]hash_join_idx_bitwise: the key a NULL probes with -- what getHashJoinArgs passes
                              (QE/JoinHashTable/PerfectJoinHashTable.cpp:803-810): max_key + 1, or for a bucketized (DATE)
                              key max_key / bucket + 1 */
  int64_t bucket;          /* bucket_normalization (DATE keys: 86400, PerfectJoinHashTable.cpp:81); 0/1 => plain.  The
                              table then has ceil((max - min + 1 [+ 1 when NULLs match]) / bucket) slots
                              (HashEntryInfo::getNormalizedHashEntryCount, HashJoinRuntime.h:46-55) and `entry_count` of a
                              one-to-many table is that number */
  int32_t kind;            /* hdk_hip_join_kind */
  int32_t type;            /* hdk_hip_join_type */
  int32_t null_mode;       /* hdk_hip_join_null */
  int32_t table_idx;       /* which entry of JOIN_HASH_TABLES */
  int32_t fused_stride;    /* HDK_JOIN_ONE_TO_ONE_FUSED: int64 words per slot (1 + payload columns) */
  int32_t key_component_count; /* keyed tables: 1 + number of `extra_keys` in use */
  int64_t entry_count;     /* slots of a one-to-many or keyed table */
  int32_t key_component_width; /* keyed tables: 4 or 8 */
  int32_t pad_;
  hdk_hip_expr extra_keys[HDK_HIP_MAX_JOIN_KEYS - 1]; /* keyed tables: outer-side components 2.. */
} hdk_hip_join;

/* Query shape: RS/QueryMemoryDescriptor.h `QueryDescriptionType`. */
enum hdk_hip_query_kind {
  HDK_Q_NON_GROUPED = 0,        /* NonGroupedAggregate */
  HDK_Q_PERFECT_HASH = 1,       /* GroupByPerfectHash */
  HDK_Q_BASELINE_HASH = 2,      /* GroupByBaselineHash */
  HDK_Q_PROJECTION = 3          /* Projection: filter/project, one output row per passing input row.
                                   Layout (RS/QueryMemoryDescriptor.cpp:314-342): row-wise
                                   [int64 row position | slots], columnar [int64 positions | slot
                                   columns at their logical widths]; rows land at atomically claimed
                                   positions (TOTAL_MATCHED), `entry_count` = MAX_MATCHED rows. */
};

enum hdk_hip_agg {
  HDK_AGG_COUNT = 0, HDK_AGG_SUM = 1, HDK_AGG_MIN = 2, HDK_AGG_MAX = 3, HDK_AGG_AVG = 4,
  HDK_AGG_ID = 5, /* non-aggregate target, written with agg_id (QE/RuntimeFunctions.cpp:473-476).
                    Group-by plans: a projected group-by key, `key_idx` names it and `arg` repeats its
                    expression.  Projection plans: any expression `arg`, key_idx = -1. */
  HDK_AGG_SINGLE_VALUE = 6 /* SINGLE_VALUE(x) (hdk::ir::AggType::kSingleValue): the slot starts at the argument's NULL,
                    the first non-NULL value is stored, a DIFFERENT non-NULL value ends the launch with
                    HDK_HIP_ERR_SINGLE_VALUE_FOUND_MULTIPLE_VALUES (checked_single_agg_id[_int32|_double|_float],
                    QE/RuntimeFunctions.cpp:489-506,567-583,743-760; *_shared, QE/cuda_mapd_rt.cu:670-782; partial
                    results: reduceOneSlotSingleValue, QE/ResultSetReduction.cpp:1186-1230).  `skip_null` = 1 and
                    `null_val` = the slot's initial value; 4- or 8-byte slots.  Plans with such a target run on the
                    global-atomics kernel (hdk_scan_agg_global). */
};
enum hdk_hip_fp_slot { HDK_FP_SLOT_NONE = 0, HDK_FP_SLOT_DOUBLE = 1, HDK_FP_SLOT_FLOAT = 2 };
typedef struct hdk_hip_target {
  int32_t agg;        /* hdk_hip_agg */
  int32_t has_arg;    /* 0 => COUNT(*) */
  hdk_hip_expr arg;
  int32_t skip_null;  /* TargetInfo::skip_null_val -> *_skip_val runtime (RuntimeFunctions.cpp:612-875) */
  int32_t slot_width; /* 4 or 8: padded slot width of the first slot (RS/ColSlotContext); 0 for a projected
                         group key of a GroupByBaselineHash plan, which has no slot and is read back
                         from the key columns (target_groupby_indices, QE/MemoryLayoutBuilder.cpp:921-927;
                         ColSlotContext::addSlotForColumn(0, 0), RS/ColSlotContext.cpp:43-48) */
  int32_t slot_off;   /* row-wise: byte offset of the first slot inside the row (after keys);
                         columnar: byte offset of the slot column from the buffer start */
  int32_t slot2_width;/* AVG: width of the count slot */
  int32_t slot2_off;  /* AVG: offset of the count slot */
  int32_t arg_is_fp;  /* hdk_hip_fp_slot: 0 integer slot; 1 the slot holds a double bit pattern; 2 float accumulator
                         (takes_float_argument, Shared/TargetInfo.h:170-179: SUM / MIN / MAX / AVG over a FLOAT
                         argument): the slot's LOW 4 BYTES hold a float whatever its padded width, updated like
                         agg_{sum,min,max}_float[_skip_val] (QE/RuntimeFunctions.cpp:770-875); the other bytes of an
                         8-byte slot keep the init pattern.  Values travel through the scan as doubles (HDK_COL_FLOAT
                         widens), so `null_val` is the float sentinel WIDENED to double; the slot's own sentinel is its
                         float bits, and INIT_AGG_VALS carries that sign-extended from 32 bits, as the reference's
                         init_agg_val_vec does (QE/OutputBufferInitialization.cpp:52-65) */
  int32_t key_idx;    /* HDK_AGG_ID: index of the projected group-by key */
  int32_t pad_;
  int64_t null_val;   /* skip value == init value of the slot for nullable args (slot-typed bits) */
} hdk_hip_target;

typedef struct hdk_hip_plan {
  uint32_t abi_version;     /* must be HDK_HIP_PLAN_ABI */
  int32_t query_kind;       /* hdk_hip_query_kind */
  /* inputs */
  int32_t num_cols;
  hdk_hip_col cols[HDK_HIP_MAX_COLS];
  int32_t num_quals;
  hdk_hip_qual quals[HDK_HIP_MAX_QUALS];
  /* Filter as a boolean expression over the conjuncts above, in postfix order (AND / OR / NOT with the reference's
   * three-valued logical_and / logical_or / logical_not, QE/RuntimeFunctions.cpp:357-384): a byte < HDK_F_AND pushes
   * the value of quals[byte] (TRUE / FALSE / NULL), HDK_F_AND and HDK_F_OR combine the two topmost values, HDK_F_NOT
   * negates the topmost; a row passes when the result is TRUE.  num_filter_ops == 0: the plain conjunction of all
   * quals (each staged by its own after_joins).  With a program the whole filter is evaluated at one stage:
   * filter_after_joins. */
  int32_t num_filter_ops;
  int32_t filter_after_joins;
  uint8_t filter_ops[HDK_HIP_MAX_FILTER_OPS];
  int32_t num_joins;
  hdk_hip_join joins[HDK_HIP_MAX_JOINS];
  /* group-by keys */
  int32_t key_count;
  hdk_hip_expr keys[HDK_HIP_MAX_KEYS];
  int64_t key_min[HDK_HIP_MAX_KEYS];       /* perfect hash: ColRangeInfo.min */
  int64_t key_bucket[HDK_HIP_MAX_KEYS];    /* ColRangeInfo.bucket (0 => none) */
  int64_t key_card[HDK_HIP_MAX_KEYS];      /* getBucketedCardinality (multi-col stride factors) */
  int64_t key_null_translated[HDK_HIP_MAX_KEYS]; /* max + (bucket?bucket:1) (RowFuncBuilder.cpp:456-461) */
  int32_t key_has_nulls[HDK_HIP_MAX_KEYS]; /* translate NULL keys (perfect hash only) */
  /* output layout (subset of RS/QueryMemoryDescriptor) */
  uint32_t entry_count;
  int32_t key_width;        /* effective key width in the buffer: 4 or 8 (perfect hash: 8) */
  int32_t keyless;          /* hasKeylessHash */
  int32_t idx_target_as_key;/* keyless: SLOT index whose init value marks an empty entry
                               (QueryMemoryDescriptor::getTargetIdxForKey; AVG counts as 2 slots) */
  int32_t output_columnar;  /* didOutputColumnar */
  uint32_t row_size_quad;   /* row-wise: row bytes / 8 (keys + slots) */
  int32_t num_targets;
  hdk_hip_target targets[HDK_HIP_MAX_TARGETS];
} hdk_hip_plan;
#define HDK_HIP_PLAN_ABI 4u

/* ------------------------------------------------------------------------------------------
 * Kernel launch.
 * Replaces DeviceKernel::launch(const KernelOptions&, std::vector<int8_t*>& kernelParams)
 * (QE/DeviceKernel.h:33-61) for the JIT'ed `multifrag_query[_hoisted_literals]`
 * (QE/RuntimeFunctions.cpp:1692-1768).  `params` holds exactly the reference's 12 *device*
 * pointers in the order of QE/QueryExecutionContext.h:111-125, laid out as
 * QueryExecutionContext::prepareKernelParams builds them (QE/QueryExecutionContext.cpp:788-964).
 * ---------------------------------------------------------------------------------------- */
enum hdk_hip_kern_param {
  HDK_KP_COL_BUFFERS = 0,   /* const int8_t***  [num_fragments][num_cols] */
  HDK_KP_NUM_FRAGMENTS,     /* const uint64_t*  */
  HDK_KP_LITERALS,          /* const int8_t*    (unused: literals live in the plan) */
  HDK_KP_NUM_ROWS,          /* const int64_t*   [num_fragments * num_tables] */
  HDK_KP_FRAG_ROW_OFFSETS,  /* const uint64_t*  [num_fragments * num_tables] */
  HDK_KP_MAX_MATCHED,       /* const int32_t*   */
  HDK_KP_TOTAL_MATCHED,     /* int32_t*         */
  HDK_KP_INIT_AGG_VALS,     /* const int64_t*   */
  HDK_KP_GROUPBY_BUF,       /* int64_t**        group-by: [0] = the shared output buffer;
                                                non-grouped: out_vec, [i] = slot of target i */
  HDK_KP_ERROR_CODE,        /* int32_t*         [grid*block]; entry 0 is written */
  HDK_KP_NUM_TABLES,        /* const uint32_t*  */
  HDK_KP_JOIN_HASH_TABLES,  /* 1 table: the table itself; >1: const int64_t* array of tables */
  HDK_KP_COUNT
};

typedef struct hdk_hip_kernel_options { /* KernelOptions, QE/DeviceKernel.h:33-43 */
  uint32_t grid_dim_x;  /* 0 => library default (persistent grid sized from the CU count) */
  uint32_t block_dim_x; /* 0 => library default */
  uint32_t shared_mem_bytes; /* ignored: LDS use is decided by the kernel choice */
  uint32_t flags;       /* HDK_HIP_LAUNCH_* */
  uint64_t total_rows;  /* upper bound on the outer rows of this launch (sum of NUM_ROWS), 0 = unknown.  NUM_ROWS is
                           device memory; multi-pass strategies size their stream-ordered scratch from this instead
                           of reading it back: the radix-partitioned group-by (skipped when 0) and the selection
                           bitmask the filter/project counting pass hands to its writing pass (when 0, or for rows
                           past the bound, the writing pass evaluates the filter again) */
  uint32_t watchdog_ms; /* > 0: the launch's kernels give up with ERR_OUT_OF_TIME once this much time has passed
                           since the launch reached the device (dynamic watchdog: QE/DynamicWatchdog.cpp:36-84,
                           QE/cuda_mapd_rt.cu:105-135; the reference counts cycles, this counts the 100 MHz
                           s_memrealtime clock) */
  uint32_t reserved_;
} hdk_hip_kernel_options;
#define HDK_HIP_LAUNCH_CHECK_INTERRUPT 64u     /* poll the device's interrupt flag (hdk_hip_set_interrupt) once per
                                                  tile and stop with ERR_INTERRUPTED when it is set
                                                  (check_interrupt, QE/cuda_mapd_rt.cu:137-148) */
#define HDK_HIP_LAUNCH_INIT_OUTPUT 128u        /* row-wise group-by plans: the output buffer is NOT initialised yet -- the
                                                  launch writes the image hdk_hip_init_group_by_buffer would have (EMPTY
                                                  keys, INIT_AGG_VALS) itself.  The radix-partitioned group-by builds each
                                                  region's image in LDS instead of loading it and stores every region, which
                                                  saves one write and one read of the whole table (a 200 M-entry table is
                                                  3.2 GB); every other strategy simply runs the init kernel first.  Never
                                                  set it when launching into a buffer that holds an earlier launch's groups */
#define HDK_HIP_LAUNCH_CLUSTER_PROBES 256u      /* aggregate plans with ONE inner one-to-one perfect-hash join over 8-byte outer
                                                  columns: permute the outer rows by join-key range first (scan_cluster.h), so
                                                  that the probes of consecutive rows share a slice of the table that stays in L2
                                                  instead of costing one 128-byte memory line each.  Off unless asked for: with
                                                  the batched interpreter as the consumer the pre-pass (32 B/row of traffic)
                                                  costs more than the locality returns (C3: 2.2 + 4.2 ms against 5.0 ms) */
#define HDK_HIP_LAUNCH_NO_CLUSTER_PROBES 512u   /* overrides the flag above */
#define HDK_HIP_LAUNCH_ACCUMULATE 2048u         /* hdk_hip_aggregate_from_ranks: GROUPBY_BUF[0] already holds an owner table (an
                                                  earlier CHUNK of the same exchange put it there): merge this call's tuples
                                                  into it instead of writing the table completely -- what lets a rank's rows be
                                                  exchanged in chunks, scatter of chunk k + 1 beside the all-to-all of chunk k
                                                  beside the aggregation of chunk k - 1 */
#define HDK_HIP_LAUNCH_WIDE_TUPLES 1024u       /* multi-pass strategies: do NOT narrow tuples from the column statistics (8-byte
                                                  tuples of the radix-partitioned group-by / the tuple exchange).  The
                                                  statistics are per rank: ranks of one exchange must agree on the tuple
                                                  width, so a rank whose columns would allow 8 bytes sets this when another
                                                  rank's do not (hdk_amd/distributed.py: TupleExchange) */
#define HDK_HIP_LAUNCH_FORCE_PARTITIONED 16u   /* take the radix-partitioned group-by whenever the plan shape
                                                  allows it, whatever the table size (testing) */
#define HDK_HIP_LAUNCH_PLAN_RESIDENT 32u       /* the head of `workspace` already holds this plan (an earlier
                                                  launch with the same workspace put it there): skip the
                                                  host-to-device copy -- what makes a launch capturable as
                                                  pure kernel nodes (hdk_hip_graph_*) */
#define HDK_HIP_LAUNCH_FORCE_GLOBAL_ATOMICS 1u /* skip the LDS-privatised strategy (testing) */
#define HDK_HIP_LAUNCH_FORCE_GENERIC 4u        /* use the (batched) plan-interpreter kernel even when a
                                                  specialised kernel matches (testing) */
#define HDK_HIP_LAUNCH_FORCE_SCALAR 8u         /* use the row-at-a-time interpreter kernel (testing) */
#define HDK_HIP_LAUNCH_RECORD_EVENTS 2u        /* bracket the scan kernel with HIP events on the launch
                                                  stream (DeviceClock, QE/DeviceKernel.cpp:25-43) */

/* Runtime interrupt (Executor::interrupt -> the `runtime_interrupt_flag` of the GPU module, QE/GpuInterrupt.cpp,
 * QE/cuda_mapd_rt.cu:137-148): value != 0 makes every running and future launch on `device_id` that was started with
 * HDK_HIP_LAUNCH_CHECK_INTERRUPT record ERR_INTERRUPTED and stop at its next tile; 0 re-arms (what
 * DeviceKernel::initializeRuntimeInterrupter does before a launch).  Written on a stream of its own, so it overtakes
 * the kernels it is meant to stop. */
int32_t hdk_hip_set_interrupt(int32_t device_id, int32_t value);

/* Host-only check of a plan: ABI version, every count, index, width and enumerator a kernel or a matcher reads
 * (column widths and tables, leaf column indices, expression steps, comparison / join / aggregate kinds, slot
 * offsets inside the row, the filter program).  Every entry point that takes a plan runs it first; a malformed plan
 * gets HDK_HIP_ERR_INVALID_ARG (or _UNSUPPORTED) and a message, never an out-of-bounds read.  No device is touched.
 * layout_only != 0: only what describes the OUTPUT buffer (query kind, keys' count and width, targets' aggregates and
 * slots, entry count) -- what hdk_hip_reduce_buffers, hdk_hip_partition_baseline* and hdk_hip_baseline_table_quads
 * need and check; a caller that reduces buffers may leave columns, filters, joins and expressions unset, as the
 * reference's ResultSetReduction works from the QueryMemoryDescriptor alone. */
int32_t hdk_hip_validate_plan(const hdk_hip_plan* plan, int32_t layout_only);
/* Bytes of device scratch `hdk_hip_launch` needs for this plan (per-block partial tables). */
int32_t hdk_hip_workspace_size(const hdk_hip_plan* plan, const hdk_hip_kernel_options* ko,
                               int32_t device_id, size_t* bytes);
/* Enqueue the scan -> filter -> join-probe -> group/aggregate pass over all fragments described by
 * `params` on `stream` (NULL = the manager's stream for `device_id`).  Asynchronous: results and
 * error codes are complete when the stream is.  The output buffer must already be initialised
 * (hdk_hip_init_*_group_by_buffer, or INIT_AGG_VALS copies for non-grouped out slots).
 * The launch MERGES into what the buffer holds, whatever earlier launch (of any route, under any flag or switch) or
 * hdk_hip_reduce_buffers put it there: groups the launch does not meet stay as they are, COUNT / SUM / AVG add to the stored
 * value, MIN / MAX combine with it, a slot that still holds its NULL sentinel takes the launch's first value, a new group is
 * claimed where the reference's probe sequence finds it.  Launches over disjoint row sets into one buffer therefore equal
 * one launch over all the rows (tests/test_gpu_relaunch.py, every aggregate route).  HDK_HIP_LAUNCH_INIT_OUTPUT is the one
 * exception: it overwrites the buffer with the empty image first.
 * Error codes (ERROR_CODE[0], an int32 the caller zeroes before the launch): a row raises HDK_HIP_ERR_DIV_BY_ZERO (integer / and
 * %, floating-point / by 0.0 or -0.0) or HDK_HIP_ERR_OVERFLOW_OR_UNDERFLOW (a checked + - * whose exact result leaves the
 * step's SQL type of check_width bytes) only if the reference's row function evaluates the step for it: the row passes the
 * filters, has a partner in every INNER join, and neither operand is NULL (an inner column of a LEFT join without a partner
 * reads as NULL).  A result equal to the smallest or the largest value of the type raises nothing.  When several codes are
 * raised in one launch -- by different rows, or together with OUT_OF_SLOTS, OUT_OF_TIME or INTERRUPTED -- the word holds the
 * numerically LARGEST positive code (every kernel records with an atomic maximum; the reference keeps the first code a thread
 * happens to store, which is no more specified).  After a positive code the contents of the output buffer are unspecified:
 * later passes of a multi-pass route and an armed fallback kernel may or may not have run.  The launch leaves nothing else
 * behind: the next launch with the same workspace, plan and parameters is not affected by it
 * (tests/test_gpu_error_cases.py, every route that evaluates an arithmetic step). */
int32_t hdk_hip_launch(const hdk_hip_plan* plan, int8_t* const params[HDK_KP_COUNT],
                       const hdk_hip_kernel_options* ko, int32_t device_id, void* stream,
                       void* workspace, size_t workspace_bytes);
/* hipGraph capture of a launch sequence (no reference counterpart: the reference launches kernel by kernel
 * through cuLaunchKernel, CudaMgr/DeviceKernel.cpp).  For callers that issue one small step at a time and
 * wait for it, the step is launch latency; recording the sequence removes the per-kernel submission.
 * (Measured here with back-to-back asynchronous steps of 1 M rows the replay is NOT faster -- 25.8 vs
 * 20.7 us, scripts/small_query_latency.py -- so the Python executor does not use it by default.)  Record the
 * sequence once and replay it:
 *     hdk_hip_graph_begin_capture(dev, stream);
 *       hdk_hip_init_*_group_by_buffer(..., stream);
 *       hdk_hip_launch(plan, params, ko with HDK_HIP_LAUNCH_PLAN_RESIDENT, dev, stream, ws, ws_bytes);
 *     hdk_hip_graph_end_capture(dev, stream, &graph);       then per execution:  hdk_hip_graph_launch(graph, dev, stream)
 * Only sequences made of kernels are capturable: the LDS-strategy launches (perfect hash / non-grouped) with
 * PLAN_RESIDENT and without RECORD_EVENTS.  `stream` NULL = the manager's stream. */
int32_t hdk_hip_graph_begin_capture(int32_t device_id, void* stream);
int32_t hdk_hip_graph_end_capture(int32_t device_id, void* stream, void** graph_exec);
int32_t hdk_hip_graph_launch(void* graph_exec, int32_t device_id, void* stream);
int32_t hdk_hip_graph_destroy(void* graph_exec);

/* Elapsed milliseconds of every scan kernel launched with HDK_HIP_LAUNCH_RECORD_EVENTS on
 * `device_id` since the last call (waits for them); at most `capacity` values are written, `*count`
 * receives how many there were. */
int32_t hdk_hip_collect_scan_times(int32_t device_id, float* ms_out, int32_t capacity, int32_t* count);
/* Names of the device kernels a launch of `plan` dispatches (for profiling), comma separated.
 * device_id HDK_HIP_DEVICE_ASSUMED_MI355X: answered for an MI355X (256 CUs, 160 KB of LDS per block) without touching
 * a device -- routing is host arithmetic, and a CPU-only test-suite can pin it. */
#define HDK_HIP_DEVICE_ASSUMED_MI355X (-355)
int32_t hdk_hip_describe_launch(const hdk_hip_plan* plan, const hdk_hip_kernel_options* ko,
                                int32_t device_id, char* out, size_t out_len);

/* ------------------------------------------------------------------------------------------
 * Partial-result reduction on device.
 * Replaces the host-side ResultSetReduction::reduce (QE/ResultSetReduction.cpp:174-330:
 * perfect hash = slot-wise reduceOneSlot :1234-1330; baseline = reduceOneEntryBaseline :694-731)
 * for per-GPU / per-launch partial buffers that already sit in HBM (e.g. after an RCCL
 * all-gather).  `that_bufs[i]` are merged into `this_buf`; layouts come from `plan`.
 * For HDK_Q_BASELINE_HASH `this_entry_count` may exceed `plan->entry_count` (Execute.cpp:1241-1253), and `this_buf`
 * may be a fresh (initialised) table or the output of ANY launch of this library: every kernel, the
 * radix-partitioned group-by included, leaves a group on the reference's probe sequence
 * (key_hash % entry_count, then linearly on), which is where the re-insert looks for it
 * (tests/test_gpu_baseline.py::test_reduce_and_relaunch_into_a_partitioned_table).
 * ---------------------------------------------------------------------------------------- */
int32_t hdk_hip_reduce_buffers(const hdk_hip_plan* plan, int64_t* this_buf, uint32_t this_entry_count,
                               const int64_t* const* that_bufs, const uint32_t* that_entry_counts,
                               int32_t num_that, const int64_t* init_vals, int32_t* dev_error,
                               int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU exchange step of a baseline-hash group-by.  No reference counterpart:
 * the reference copies every device's partial ResultSet to the host and re-inserts the entries
 * there (Executor::reduceMultiDeviceResultSets, QE/Execute.cpp:1224-1336, with
 * reduceOneEntryBaseline, QE/ResultSetReduction.cpp:694-731).  Here the non-empty entries of a
 * rank's table are split by owner = mulhi32(key_hash(key), num_owners) into `num_owners` compact
 * tables that keep the plan's layout (row-wise or columnar) with entry_count = counts[o]; after an
 * all-to-all each owner folds what it received with hdk_hip_reduce_buffers, and the result is the
 * concatenation of the owners' disjoint tables.
 *   hdk_hip_baseline_table_quads     size (int64 words) of a table of `entry_count` entries
 *   hdk_hip_partition_baseline_count entries per owner -> HOST array counts[num_owners] (synchronises)
 *   hdk_hip_partition_baseline       scatter into seg_bufs[o] (HOST array of device pointers, each
 *                                    hdk_hip_baseline_table_quads(counts[o]) words); `counts` is the
 *                                    HOST array the count step returned
 * `init_vals` is the HOST array of hdk_hip_reduce_buffers (keyless tables cannot be baseline, but the
 * emptiness rule is shared).
 * ---------------------------------------------------------------------------------------- */
int32_t hdk_hip_baseline_table_quads(const hdk_hip_plan* plan, uint32_t entry_count, int64_t* quads);
int32_t hdk_hip_partition_baseline_count(const hdk_hip_plan* plan, const int64_t* buf, uint32_t entry_count,
                                         const int64_t* init_vals, int32_t num_owners, uint32_t* counts,
                                         int32_t device_id, void* stream);
int32_t hdk_hip_partition_baseline(const hdk_hip_plan* plan, const int64_t* buf, uint32_t entry_count,
                                   const int64_t* init_vals, int32_t num_owners, const uint32_t* counts,
                                   int64_t* const* seg_bufs, int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Columnar results on the device.
 * Replaces, for a ResultSet whose storage sits in HBM, ColumnarResults::materializeAllColumnsGroupBy with its two stages
 * locateAndCountEntries / compactAndCopyEntries (omniscidb/ResultSetRegistry/ColumnarResults.cpp:691-1010), which the
 * reference runs on the host after copying the whole buffer, empty entries included.  A group-by buffer in the plan's
 * layout (HDK_Q_PERFECT_HASH or HDK_Q_BASELINE_HASH: row-wise or columnar, keyless, 4- or 8-byte keys and slots,
 * zero-width slots of projected baseline keys; any other query kind is HDK_HIP_ERR_UNSUPPORTED) becomes one dense 8-byte
 * column per target: column t starts at out_cols + t * capacity, and row r of every column is the r-th non-empty entry
 * in ascending entry index -- ResultSet iteration order.  An entry is empty as ResultSetStorage::isEmptyEntry[Columnar]
 * says (omniscidb/ResultSet/ResultSetStorage.cpp:439-521).  A value is what iteration returns for the target:
 *   HDK_AGG_ID                      the slot, sign-extended; with slot_width == 0 key column key_idx (a 4-byte key
 *                                   sign-extended, an fp key's bit pattern unchanged)
 *   COUNT, integer SUM / MIN / MAX / SINGLE_VALUE
 *                                   the slot sign-extended from its width (an in-band NULL stays in band)
 *   arg_is_fp DOUBLE, not AVG       the slot's 8 bytes
 *   arg_is_fp FLOAT, not AVG        the float in the slot's low 4 bytes widened to double; with skip_null,
 *                                   HDK_NULL_FLOAT_BITS becomes HDK_NULL_DOUBLE_BITS
 *   AVG                             pair_to_double (omniscidb/ResultSet/ResultSetBufferAccessors.h:168-190):
 *                                   double(dividend) / double(count), dividend = (double)int64 sum, the double's bits or
 *                                   the widened float; HDK_NULL_DOUBLE_BITS when count == 0
 * `entry_count` is that of THIS buffer and may differ from plan->entry_count (a reduced baseline table);  `init_vals` is
 * the HOST array of hdk_hip_reduce_buffers (keyless emptiness).  `*row_count` (device) always receives the TRUE number of
 * non-empty entries; rows at or beyond `capacity` are not written, and nothing outside [0, min(rows, capacity)) of a
 * column is touched.  out_cols == NULL: count only.  `workspace`: hdk_hip_result_columns_workspace_bytes(entry_count)
 * bytes of device memory (host arithmetic only: 4 bytes per tile of 4 096 entries), or NULL -- the library then takes it
 * from the stream's memory pool (hipMallocAsync), as the fused join build does.  Asynchronous on `stream`; the host
 * never waits.
 * ---------------------------------------------------------------------------------------- */
size_t hdk_hip_result_columns_workspace_bytes(uint32_t entry_count);
int32_t hdk_hip_columnarize_result(const hdk_hip_plan* plan, const int64_t* buf, uint32_t entry_count,
                                   const int64_t* init_vals, int64_t* out_cols, uint64_t capacity, uint64_t* row_count,
                                   void* workspace, size_t workspace_bytes, int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Columnar results on the device: projections and non-grouped results.
 * Replaces, for a ResultSet whose storage sits in HBM, ColumnarResults::materializeAllColumnsProjection with
 * copyAllNonLazyColumns / materializeAllColumnsDirectly (omniscidb/ResultSetRegistry/ColumnarResults.cpp:520-620), which the
 * reference runs on the host after copying the whole buffer.  The other half of the scan path (HDK_Q_PROJECTION or
 * HDK_Q_NON_GROUPED; a group-by plan is HDK_HIP_ERR_UNSUPPORTED and goes through hdk_hip_columnarize_result) becomes the
 * same dense form: one 8-byte column per target, column t at out_cols + t * capacity.
 *   HDK_Q_PROJECTION   rows = min(max(*total_matched, 0), entry_count), read ON THE DEVICE (`total_matched` is the launch's
 *                      TOTAL_MATCHED word; a step that ran out of output rows has total_matched > entry_count).  Row r of
 *                      every column is buffer row r -- ResultSet iteration order; rows are never reordered.  Both layouts:
 *                      row-wise [int64 row position | one 8-byte slot per target], copied as they are, and columnar
 *                      [positions: entry_count x 8 | one column per target at its width 1 / 2 / 4 / 8, each start aligned
 *                      to 8], a narrow slot SIGN-EXTENDED to 64 bits (a narrow NULL sentinel arrives sign-extended), a
 *                      double's 8 bytes copied.  `pos_out` (device, `capacity` rows, or NULL) receives the row positions.
 *   HDK_Q_NON_GROUPED  entry_count must be 1, total_matched and pos_out NULL; rows = 1.  Slot i is buf[i] (AVG owns two);
 *                      one value per target by the rules hdk_hip_columnarize_result documents for a slot: a FLOAT
 *                      accumulator widened to double (HDK_NULL_FLOAT_BITS -> HDK_NULL_DOUBLE_BITS under skip_null), AVG
 *                      through pair_to_double (HDK_NULL_DOUBLE_BITS at count 0), anything else the slot.
 * `*row_count` (device) always receives the TRUE row count; rows at or beyond `capacity` are not written and nothing outside
 * [0, min(rows, capacity)) of a column or of pos_out is touched; buffer rows at or beyond that are not read.
 * out_cols == NULL: count only (pos_out is not written either).  No workspace, no atomics.  Asynchronous on `stream`; the
 * host never waits.
 * ---------------------------------------------------------------------------------------- */
int32_t hdk_hip_columnarize_rows(const hdk_hip_plan* plan, const int64_t* buf, uint32_t entry_count,
                                 const int32_t* total_matched, int64_t* out_cols, uint64_t capacity, int64_t* pos_out,
                                 uint64_t* row_count, int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * ORDER BY / LIMIT / OFFSET over dense result columns on the device.
 * Replaces, for a result whose columns sit in HBM, ResultSet::sort with doBaselineSort and its GPU sorts
 * (omniscidb/QueryEngine/ResultSetSort.cpp:64-188, ResultSetSortImpl.cu, TopKSort.cu); the order entries, limit and
 * offset are RelAlgExecutionUnit's SortInfo.  Input: `num_cols` columns of `num_rows` 8-byte words, column t at
 * cols + t * capacity, NULLs in band -- what hdk_hip_columnarize_result writes.  Output: column t at
 * out_cols + t * out_capacity.  With out_rows = min(limit ? limit : infinity, num_rows > offset ? num_rows - offset : 0)
 * (host arithmetic, hence not returned), rows [0, out_rows) of every output column receive input rows perm[offset + r] and
 * perm_out[r] (when not NULL) that input row index -- the reference's permutation buffer.  Nothing at or beyond out_rows is
 * written, the input is not modified, and out_cols must not overlap cols.
 * Order: ResultSetComparator (ResultSetSort.cpp:329-480), entry by entry from the first: both NULL -> next entry; one
 * NULL -> nulls_first decides, whatever is_desc says; equal words -> next entry; otherwise (l < r) != is_desc, compared as
 * int64 or, with is_fp, as doubles.  A word is NULL when the entry is nullable and the word equals null_bits.
 * Rows equal on every entry come out in ascending input row index (the reference leaves the order among ties open: a
 * stable result is one of its valid results, and it is the same on every run).  Doubles are ordered by the usual
 * order-preserving bit transform, which differs from operator< in two places: -0.0 comes BEFORE +0.0 (the reference calls
 * them a tie), and NaNs are ordered by bit pattern beyond the infinities (sign bit set: before -inf; clear: after +inf).
 * A LIMIT with offset + limit <= num_rows / 8 first selects the candidate rows by the first entry (radix select, ties at
 * the threshold kept) and sorts only those; the result is word for word that of the full sort, which
 * HDK_HIP_SORT_NO_SELECT forces.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL cols / order / out_cols,
 * num_order outside 1..HDK_HIP_MAX_ORDER_ENTRIES, an entry's col outside [0, num_cols), num_rows >= 2^32, num_rows >
 * capacity, out_capacity < out_rows, overlapping blocks, a workspace that is too small.  num_rows == 0 or out_rows == 0:
 * HDK_HIP_OK, nothing is launched.
 * `workspace`: hdk_hip_sort_columns_workspace_bytes(num_rows, num_order) bytes of device memory (host arithmetic only:
 * two (8-byte key, 4-byte row) pairs and 1/4 byte of digit counters per row, plus 4 KiB), or NULL -- the library then takes
 * it from the stream's memory pool (hipMallocAsync), as hdk_hip_columnarize_result does.
 * SYNCHRONISES `stream`: once per order entry the host reads 16 bytes back (which digits of the keys differ at all, so
 * that only those radix passes are launched), and once more on the selection path (the number of candidates).  The final
 * passes and the gather are asynchronous: the output is complete when `stream` has drained.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_MAX_ORDER_ENTRIES 8
#define HDK_HIP_SORT_NO_SELECT 1u /* flags: always the full sort, never the top-N selection (tests, A/B) */

typedef struct hdk_hip_order_entry {
  int32_t col;         /* 0-based column = target index (the reference's tle_no - 1) */
  uint8_t is_desc;
  uint8_t nulls_first;
  uint8_t is_fp;       /* words are doubles, compared as doubles; else int64 */
  uint8_t nullable;    /* 0: null_bits is an ordinary value */
  int64_t null_bits;   /* the column's in-band NULL as the dense column holds it */
} hdk_hip_order_entry;

size_t hdk_hip_sort_columns_workspace_bytes(uint64_t num_rows, int32_t num_order);
int32_t hdk_hip_sort_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                             const hdk_hip_order_entry* order, int32_t num_order, uint64_t offset, uint64_t limit,
                             uint32_t flags, int64_t* out_cols, uint64_t out_capacity, uint32_t* perm_out, void* workspace,
                             size_t workspace_bytes, int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * HAVING over dense result columns on the device: the rows on which a predicate is TRUE, compacted.
 * Replaces, for a result whose columns sit in HBM, the reference's filter step over a temporary table (the previous
 * step's ResultSet materialised as ColumnarResults), whose comparisons are DEF_CMP_NULLABLE*
 * (omniscidb/QueryEngine/RuntimeFunctions.cpp:83-117) combined by logical_not / logical_and / logical_or (:355-384).
 * Input: `num_cols` columns of `num_rows` 8-byte words, column t at cols + t * capacity, NULLs in band -- what
 * hdk_hip_columnarize_result and hdk_hip_sort_columns write.
 * Predicate: `num_leaves` (1..HDK_HIP_MAX_HAVING_LEAVES) comparisons and a postfix program `ops` over them of up to
 * HDK_HIP_MAX_FILTER_OPS bytes in the encoding of hdk_hip_plan::filter_ops: a byte < HDK_F_AND pushes the value of
 * leaves[byte] (TRUE / FALSE / NULL), HDK_F_AND and HDK_F_OR combine the two topmost values, HDK_F_NOT negates the
 * topmost.  num_ops == 0: the plain conjunction of all leaves.  A row passes only when the result is TRUE; NULL and
 * FALSE both drop it.
 * Leaf: column lhs_col <cmp> column rhs_col (rhs_is_col) or the literal rhs_lit (an int64, or a double's bits with
 * rhs_is_fp).  A side is NULL when it is nullable and its word EQUALS null_bits -- a bit compare, the rule of
 * hdk_hip_order_entry; a literal is never NULL; a leaf with a NULL side is NULL.  With cmp_fp the sides are compared as
 * doubles, an int64 side (is_fp == 0) converted with (double) as the reference's cast would; without it the words are
 * compared as int64 and is_fp is not looked at.
 * Doubles compare with the C operators, UNLIKE hdk_hip_sort_columns' order: -0.0 == +0.0 holds, and any comparison
 * with a NaN is false except <> (HDK_CMP_NE), which is true.
 * Output: column t at out_cols + t * out_capacity; passing rows keep their input order (stable).  *row_count (device)
 * ALWAYS receives the true number of passing rows; rows at or beyond out_capacity are not written, and nothing outside
 * [0, min(rows, out_capacity)) of an output column is touched.  out_cols == NULL: count only (perm_out is ignored).
 * perm_out (device, may be NULL; out_capacity entries) receives the input row index of each output row.  The input is
 * not modified, and no two of cols, out_cols, perm_out, row_count and workspace may overlap (a block the call does not
 * touch -- out_cols and perm_out with out_capacity == 0 or in a count-only call -- has no bytes and overlaps nothing).
 * `workspace`: hdk_hip_filter_columns_workspace_bytes(num_rows) bytes of device memory, 8-byte aligned (host arithmetic only: one pass
 * bit per row and 4 bytes per tile of 4 096 rows, both rounded up to whole tiles, plus at most 512 bytes), or NULL -- the
 * library then takes it from the stream's memory pool (hipMallocAsync), as its two siblings do.
 * ASYNCHRONOUS on `stream`: three launches (count, scan, compact) ordered by the stream alone; the host never waits
 * (as hdk_hip_columnarize_result, unlike hdk_hip_sort_columns).  Output and *row_count are complete when `stream` has
 * drained.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL cols / leaves /
 * row_count, num_leaves outside 1..8, a column index outside [0, num_cols), a cmp outside hdk_hip_cmp, a malformed
 * program (more than HDK_HIP_MAX_FILTER_OPS ops, an unknown byte, stack underflow, a leaf index >= num_leaves, a final
 * stack depth other than 1), num_rows >= 2^32, num_rows > capacity, overlapping blocks, a workspace that is too small
 * or not 8-byte aligned.
 * num_rows == 0: *row_count = 0 is stored on the stream, nothing else is launched.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_MAX_HAVING_LEAVES 8

typedef struct hdk_hip_having_leaf {
  int32_t lhs_col;        /* 0-based column = target index */
  int32_t rhs_col;        /* with rhs_is_col */
  uint8_t cmp;            /* hdk_hip_cmp */
  uint8_t rhs_is_col;     /* 0: the right-hand side is rhs_lit */
  uint8_t cmp_fp;         /* compare as doubles (a side is fp, or the literal is); else as int64 */
  uint8_t lhs_is_fp;      /* the column's words are doubles */
  uint8_t lhs_nullable;   /* 0: lhs_null_bits is an ordinary value */
  uint8_t rhs_is_fp;      /* the column's words, or rhs_lit, are a double('s bits) */
  uint8_t rhs_nullable;   /* a column only: a literal is never NULL */
  uint8_t pad_;
  int64_t lhs_null_bits;  /* the column's in-band NULL as the dense column holds it */
  int64_t rhs_null_bits;
  int64_t rhs_lit;
} hdk_hip_having_leaf;

size_t hdk_hip_filter_columns_workspace_bytes(uint64_t num_rows);
int32_t hdk_hip_filter_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                               const hdk_hip_having_leaf* leaves, int32_t num_leaves, const uint8_t* ops, int32_t num_ops,
                               int64_t* out_cols, uint64_t out_capacity, uint64_t* row_count, uint32_t* perm_out,
                               void* workspace, size_t workspace_bytes, int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * GROUP BY over dense result columns on the device: one row per run of adjacent rows with equal keys.
 * The device form, for a result whose columns sit in HBM, of the reference's per-slot merge of partial results
 * (reduceOneSlot, omniscidb/QueryEngine/ResultSetReduction.cpp) with the NULL rules of the _skip_val functions
 * (omniscidb/QueryEngine/RuntimeFunctions.cpp:612-681, 841-867): a second aggregation step over a first step's result
 * (a roll-up, SELECT DISTINCT, the outer half of COUNT(DISTINCT)).
 * Input: `num_cols` columns of `num_rows` 8-byte words, column t at cols + t * capacity, NULLs in band -- what
 * hdk_hip_columnarize_result, hdk_hip_filter_columns and hdk_hip_sort_columns write.  Rows with equal keys must be
 * ADJACENT: a precondition, which hdk_hip_sort_columns on the key columns establishes.  A RUN is a maximal stretch of
 * adjacent rows whose words in every one of the `num_keys` (1..HDK_HIP_MAX_GROUP_KEYS) columns key_cols[] are BIT-EQUAL:
 * NULL equals NULL, -0.0 differs from +0.0, NaNs are compared by pattern -- how the group-by tables compare 8-byte keys,
 * and the equivalence that the sort's total order makes adjacent.  Unsorted input is not an error: every run becomes a row.
 * Output: one row per run, in input order; output column j (of `num_outs`, 1..HDK_HIP_MAX_GROUP_OUTS) at
 * out_cols + j * out_capacity, in the order of `outs`:
 *   HDK_AGG_ID      the run's word of column `col`, which must be one of key_cols (SELECT DISTINCT k: outs = [ID(k)]; a key
 *                   need not be projected)
 *   HDK_AGG_COUNT   col < 0: COUNT(*), the rows of the run; else the words of `col` that are not NULL.  An int64, never NULL
 *   HDK_AGG_SUM     over the non-NULL words: int64 two's-complement wrapping addition, or (is_fp) a sum of doubles in an
 *                   unspecified association (the same on every run of the same call)
 *   HDK_AGG_MIN / HDK_AGG_MAX   over the non-NULL words by < / > on int64 or (is_fp) on doubles
 * A word is NULL when the out is nullable and the word EQUALS null_bits (a bit compare, the rule of hdk_hip_order_entry);
 * with nullable == 0 every word is a value.  SUM / MIN / MAX of a run without a non-NULL word give null_bits.  Whether a
 * run has a value is tracked beside the value, so a sum that happens to equal null_bits is still stored as that sum (and
 * reads as NULL to whoever reads the column afterwards, as in the reference).  A NaN inside an aggregated double column
 * leaves that run's SUM / MIN / MAX unspecified.
 * *row_count (device) ALWAYS receives the true number of runs; rows at or beyond out_capacity are not written, and nothing
 * outside [0, min(runs, out_capacity)) of an output column is touched.  out_cols == NULL (or out_capacity == 0): count
 * only.  The input is not modified, and no two of cols, out_cols, row_count and workspace may overlap (out_cols in a
 * count-only call has no bytes and overlaps nothing).
 * `workspace`: hdk_hip_group_columns_workspace_bytes(num_rows, num_outs) bytes of device memory, 8-byte aligned (host
 * arithmetic only: per tile of 4 096 rows 4 bytes and 12 bytes per out, plus at most 1 KiB), or NULL -- the library then
 * takes it from the stream's memory pool (hipMallocAsync), as its siblings do.
 * ASYNCHRONOUS on `stream`: four launches (count, scan, carry scan, reduce; two in a count-only call) ordered by the stream
 * alone; the host never waits (as hdk_hip_filter_columns).  Output and *row_count are complete when `stream` has drained.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL cols / key_cols / outs /
 * row_count, num_keys outside 1..8, num_outs outside 1..16, a column index outside [0, num_cols) (col < 0 is COUNT(*) for
 * HDK_AGG_COUNT only), an ID whose column is not a key, a kind outside the five, num_rows >= 2^32, num_rows > capacity,
 * overlapping blocks, a workspace that is too small or not 8-byte aligned.
 * num_rows == 0: *row_count = 0 is stored on the stream, nothing else is launched.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_MAX_GROUP_KEYS 8
#define HDK_HIP_MAX_GROUP_OUTS 16

typedef struct hdk_hip_group_out {
  int32_t col;        /* input column; ignored for COUNT(*) (col < 0) */
  uint8_t kind;       /* HDK_AGG_ID: the run's value of a KEY column (col must be in key_cols);
                         HDK_AGG_COUNT (col < 0: rows of the run; else non-NULL words), HDK_AGG_SUM, HDK_AGG_MIN, HDK_AGG_MAX */
  uint8_t is_fp;      /* words are doubles (SUM / MIN / MAX as doubles); else int64 */
  uint8_t nullable;   /* 0: null_bits is an ordinary value */
  uint8_t pad_;
  int64_t null_bits;  /* the input column's in-band NULL, as in hdk_hip_order_entry */
} hdk_hip_group_out;

size_t hdk_hip_group_columns_workspace_bytes(uint64_t num_rows, int32_t num_outs);
int32_t hdk_hip_group_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                              const int32_t* key_cols, int32_t num_keys, const hdk_hip_group_out* outs, int32_t num_outs,
                              int64_t* out_cols, uint64_t out_capacity, uint64_t* row_count, void* workspace,
                              size_t workspace_bytes, int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Window functions over dense result columns on the device: one word per input row and output.
 * The device form, for a result whose columns sit in HBM, of the reference's window step over the previous step's
 * materialised result (WindowFunctionContext, omniscidb/QueryEngine/WindowContext.cpp and WindowFunctionIR.cpp; the kinds
 * are hdk::ir::WindowFunctionKind, omniscidb/IR/OpTypeEnums.h:95-112, in the same order).
 * Input: `num_cols` columns of `num_rows` 8-byte words, column t at cols + t * capacity, NULLs in band -- what
 * hdk_hip_columnarize_result, hdk_hip_filter_columns, hdk_hip_sort_columns and hdk_hip_group_columns write.
 * A PARTITION is a maximal stretch of adjacent rows whose words in every one of the `num_part` (0..HDK_HIP_MAX_WINDOW_KEYS)
 * columns part_cols[] are BIT-EQUAL (the equivalence of hdk_hip_group_columns: NULL equals NULL); num_part == 0 makes the
 * whole input one partition.  A PEER GROUP is a maximal stretch inside a partition whose words in every one of the
 * `num_order` (0..HDK_HIP_MAX_WINDOW_KEYS) columns order_cols[] are bit-equal too; num_order == 0 makes every row of a
 * partition a peer.  Adjacency is a PRECONDITION, which hdk_hip_sort_columns on (partition keys, order entries)
 * establishes; unsorted input is not an error: every stretch becomes a partition.  Order keys are read for equality
 * only: direction and NULL placement belong to the sort.
 * Deviation from the reference: bit equality differs from the reference's comparator for -0.0 / +0.0 (two peer groups
 * here) and for NaNs (compared by pattern) -- the deviation that the sort's total order already makes.
 * Output: exactly `num_rows` rows in input row order, output j (of `num_outs`, 1..HDK_HIP_MAX_WINDOW_OUTS) at
 * out_cols + j * out_capacity; only the window columns are written.  out_capacity >= num_rows; nothing at or beyond
 * num_rows is touched, the input is not modified, and no two of cols, out_cols and workspace may overlap.
 * For a row r (0-based input row index): start / end are the first and last row of its partition, pstart / pend of its
 * peer group, size = end - start + 1.  The word written for row r:
 *   HDK_WIN_ROW_NUMBER    r - start + 1
 *   HDK_WIN_RANK          pstart - start + 1                                   (index_to_rank, WindowContext.cpp:124-137)
 *   HDK_WIN_DENSE_RANK    the peer groups of the partition up to and including r's                        (:140-153)
 *   HDK_WIN_PERCENT_RANK  a double: size == 1 ? 0 : (rank - 1) / (size - 1)                               (:156-170)
 *   HDK_WIN_CUME_DIST     a double: (pend - start + 1) / size                                             (:173-191)
 *   HDK_WIN_NTILE         param = n >= 1; the reference's rule, not the SQL standard's:
 *                         (r - start) / ceil(size / n) + 1                                                (:194-206)
 *   HDK_WIN_LAG / LEAD    param = k >= 0: the word of `col` at row r - k / r + k when that row is inside [start, end],
 *                         else null_bits (apply_lag_to_partition, :266-285).  The word is copied unexamined
 *   HDK_WIN_FIRST_VALUE   the word of `col` at start
 *   HDK_WIN_LAST_VALUE    the word of `col` at the frame's last row
 *   HDK_WIN_COUNT / SUM / MIN / MAX / AVG   over the frame of r with the NULL rules of hdk_hip_group_columns: COUNT with
 *                         col < 0 is COUNT(*), COUNT is never NULL; a word is NULL when the out is nullable and the word
 *                         EQUALS null_bits; SUM / MIN / MAX give null_bits while the frame has no non-NULL word (whether it
 *                         has one travels beside the value: a sum equal to the sentinel stays a sum); an int64 SUM wraps; a
 *                         SUM of doubles has an unspecified association, the same on every run of the same call; AVG is
 *                         always a double, (double)sum / (double)count as the reference's pair_to_double, and
 *                         HDK_NULL_DOUBLE_BITS while the count is 0
 * `frame` is read by the aggregates and by LAST_VALUE only.  Every frame starts at `start`; its last row is
 *   HDK_FRAME_ROWS        r       (the reference's running MIN / MAX and its LAST_VALUE)
 *   HDK_FRAME_RANGE       pend    (all peers receive the same word, bit for bit: the reference's peer handling for SUM /
 *                                  COUNT / AVG, window_function_requires_peer_handling, WindowContext.cpp:425-441)
 *   HDK_FRAME_PARTITION   end     (every row of the partition receives the same word: the reference without order keys)
 * With num_order == 0, RANGE and PARTITION coincide.  `col` is ignored for the six ranking kinds.
 * `workspace`: hdk_hip_window_columns_workspace_bytes(num_rows, num_outs) bytes of device memory, 8-byte aligned (host
 * arithmetic only: 12 bytes per row -- the directory: the last row of every partition and peer group and the ordinal of
 * every partition's last peer group --, per tile of 4 096 rows 8 bytes and 12 bytes per out, plus at most 2 KiB), or NULL --
 * the library then takes it from the stream's memory pool (hipMallocAsync), as its siblings do.
 * ASYNCHRONOUS on `stream`: up to seven launches (count, two scans, carry scan, directory, rows, and a broadcast when an
 * aggregate has a RANGE or PARTITION frame) ordered by the stream alone; the host never waits.  The output is complete
 * when `stream` has drained.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL cols / outs / out_cols,
 * a NULL part_cols with num_part > 0 or order_cols with num_order > 0, num_part or num_order outside 0..8, num_outs outside
 * 1..8, num_cols < 1, a column index outside [0, num_cols) (col < 0 is COUNT(*) for HDK_WIN_COUNT only), a kind or frame
 * outside the enums, param < 0 or an NTILE param < 1, num_rows >= 2^32, num_rows > capacity, out_capacity < num_rows,
 * overlapping blocks, a workspace that is too small or not 8-byte aligned.
 * num_rows == 0: HDK_HIP_OK, nothing is launched.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_MAX_WINDOW_KEYS 8
#define HDK_HIP_MAX_WINDOW_OUTS 8

typedef enum hdk_hip_window_kind {
  HDK_WIN_ROW_NUMBER = 0, HDK_WIN_RANK = 1, HDK_WIN_DENSE_RANK = 2, HDK_WIN_PERCENT_RANK = 3, HDK_WIN_CUME_DIST = 4,
  HDK_WIN_NTILE = 5, HDK_WIN_LAG = 6, HDK_WIN_LEAD = 7, HDK_WIN_FIRST_VALUE = 8, HDK_WIN_LAST_VALUE = 9, HDK_WIN_AVG = 10,
  HDK_WIN_MIN = 11, HDK_WIN_MAX = 12, HDK_WIN_SUM = 13, HDK_WIN_COUNT = 14
} hdk_hip_window_kind;

typedef enum hdk_hip_window_frame { HDK_FRAME_ROWS = 0, HDK_FRAME_RANGE = 1, HDK_FRAME_PARTITION = 2 } hdk_hip_window_frame;

typedef struct hdk_hip_window_out {
  int32_t col;        /* input column; ignored for the ranking kinds and for COUNT(*) (col < 0) */
  uint8_t kind;       /* hdk_hip_window_kind */
  uint8_t frame;      /* hdk_hip_window_frame: read by the aggregates and by LAST_VALUE */
  uint8_t is_fp;      /* words are doubles (SUM / MIN / MAX / AVG as doubles); else int64 */
  uint8_t nullable;   /* 0: null_bits is an ordinary value */
  int64_t null_bits;  /* the input column's in-band NULL, as in hdk_hip_group_out */
  int64_t param;      /* NTILE: n; LAG / LEAD: k */
} hdk_hip_window_out;

size_t hdk_hip_window_columns_workspace_bytes(uint64_t num_rows, int32_t num_outs);
int32_t hdk_hip_window_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                               const int32_t* part_cols, int32_t num_part, const int32_t* order_cols, int32_t num_order,
                               const hdk_hip_window_out* outs, int32_t num_outs, int64_t* out_cols, uint64_t out_capacity,
                               void* workspace, size_t workspace_bytes, int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Projection over dense result columns on the device: computed columns, one word per input row and output.
 * The device form, for a result whose columns sit in HBM, of the reference's project step over the previous step's
 * materialised result: its nullable arithmetic (DEF_ARITH_NULLABLE*, omniscidb/QueryEngine/RuntimeFunctions.cpp:49-80) with
 * the checked + - * and the division guard of QE/ArithmeticIR.cpp:277-634, the casts (:311-345), DEF_CMP_NULLABLE*
 * (:83-117), logical_not / logical_and / logical_or (:355-384) and CASE (codegenCase, QE/CaseIR.cpp).
 * Input: `num_cols` columns of `num_rows` 8-byte words, column t at cols + t * capacity, NULLs in band -- what the other
 * *_columns calls write.
 * Output: out j (of `num_outs`, 1..HDK_HIP_MAX_PROJECT_OUTS) at out_cols + j * out_capacity: exactly `num_rows` words in
 * input row order.  Nothing at or beyond row num_rows and nothing outside the num_outs columns is written; the input is
 * not modified; no two of cols, out_cols and error_code_dev may overlap.
 * A PROGRAM is a postfix sequence of typed ops over a value stack; out j owns ops[first_op .. first_op + num_ops) and
 * starts on an empty stack.  A call takes at most HDK_HIP_MAX_PROJECT_OPS ops over all outs, a stack of at most
 * HDK_HIP_MAX_PROJECT_STACK values and at most HDK_HIP_MAX_PROJECT_INPUTS distinct input columns.  Every stack value is a
 * 64-bit word, a NULL bit and a pending-error mark; its class -- INT (an int64), FP (a double's bits) or BOOL -- is
 * static, and the library type-checks every program on the host: mixed arithmetic needs explicit casts.
 *   HDK_P_PUSH_COL        the word of column `col` (flags: HDK_P_FLAG_FP = the class is FP, else INT; HDK_P_FLAG_NULLABLE =
 *                         the value is NULL when the word is BIT-EQUAL to imm, the rule of hdk_hip_filter_columns)
 *   HDK_P_PUSH_INT / _FP  imm, an int64 / the bits of a double; never NULL
 *   HDK_P_PUSH_NULL_INT / _FP   a NULL of that class
 *   HDK_P_ADD_I SUB_I MUL_I DIV_I MOD_I   b = pop, a = pop, push a op b, as hdk_hip_expr's steps: a NULL operand gives NULL
 *                         and nothing is checked; + - * wrap, and with check_width 1 / 2 / 4 / 8 (0: unchecked) a result
 *                         outside the signed type of that many bytes raises HDK_HIP_ERR_OVERFLOW_OR_UNDERFLOW; / and % raise
 *                         HDK_HIP_ERR_DIV_BY_ZERO on b == 0, truncate towards zero, INT64_MIN / -1 = INT64_MIN, x % -1 = 0
 *   HDK_P_ADD_F SUB_F MUL_F DIV_F   on doubles, unfused; DIV_F raises HDK_HIP_ERR_DIV_BY_ZERO on b == 0.0 (either zero)
 *   HDK_P_CAST_I2F        (double) a;  HDK_P_CAST_F2I   (int64_t)(d + (d < 0 ? -0.5 : 0.5)), as HDK_OP_CAST_FP_TO_INT (a
 *                         NaN or a double outside int64 gives an unspecified word)
 *   HDK_P_CMP_I / CMP_F   b = pop, a = pop, push the BOOL a <cmp> b with the hdk_hip_cmp in `flags`; NULL when an operand
 *                         is; doubles compare with the C operators (-0.0 == +0.0; with a NaN only <> is true)
 *   HDK_P_AND / OR / NOT  three-valued, on BOOLs
 *   HDK_P_IS_NULL         a BOOL that is never NULL, of a value of any class
 *   HDK_P_SELECT          e = pop, t = pop, c = pop (a BOOL; t and e of one class): push t when c is TRUE, e when c is FALSE
 *                         or NULL.  CASE with several WHENs nests it: the ELSE side is the next SELECT
 * An out must leave exactly one INT (is_fp == 0) or FP (is_fp == 1) value; a NULL result stores null_bits (whatever
 * `nullable` says: it only describes the column to its next reader).  An out that is a single HDK_P_PUSH_COL is a
 * pass-through: the word is copied unexamined.
 * ERRORS ARE LAZY, as the reference's CASE is (a branch is evaluated in its own block): an op that would raise MARKS its
 * result with the code instead (the marked value itself is unspecified), and an op with a marked operand gives a marked
 * result (the larger code of two) -- except that HDK_P_SELECT keeps the marks of its condition and of the CHOSEN branch
 * only, and HDK_P_AND / HDK_P_OR give an unmarked result when an unmarked operand alone decides it (FALSE / TRUE).  A mark
 * that reaches an out raises.  So CASE WHEN n = 0 THEN NULL ELSE s / n END never raises.  Deviation: the reference's planner
 * short-circuits AND / OR on one chosen side, and also when that side is NULL; here a NULL side does not hide the other
 * side's error.
 * Reporting: the call first stores *error_code_dev = 0 (device memory, stream-ordered); rows that raise then leave the
 * numerically largest code raised (one atomic max per block that saw any).  After an error the output words are
 * unspecified.  error_code_dev may be NULL only when no op of the call can raise (no / or %, every check_width 0).
 * ASYNCHRONOUS on `stream`: one store and one launch; no workspace; the host never waits.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL cols / ops / outs /
 * out_cols, num_cols < 1, num_outs outside 1..8, num_ops outside 1..48, an out whose op range is empty or outside the ops, an
 * unknown code, check_width not 0 / 1 / 2 / 4 / 8, a cmp outside hdk_hip_cmp, stack underflow or a depth above 6, an
 * operand of the wrong class, an out that leaves no value, more than one, a BOOL or a class that is not its is_fp,
 * col >= num_cols, more than 8 distinct columns, num_rows >= 2^32, capacity or out_capacity below num_rows, overlapping
 * blocks, a NULL error_code_dev with a program that can raise.
 * num_rows == 0: nothing but *error_code_dev is touched.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_MAX_PROJECT_OUTS 8
#define HDK_HIP_MAX_PROJECT_OPS 48
#define HDK_HIP_MAX_PROJECT_STACK 6
#define HDK_HIP_MAX_PROJECT_INPUTS 8

typedef enum hdk_hip_project_code {
  HDK_P_PUSH_COL = 1, HDK_P_PUSH_INT, HDK_P_PUSH_FP, HDK_P_PUSH_NULL_INT, HDK_P_PUSH_NULL_FP,
  HDK_P_ADD_I, HDK_P_SUB_I, HDK_P_MUL_I, HDK_P_DIV_I, HDK_P_MOD_I,
  HDK_P_ADD_F, HDK_P_SUB_F, HDK_P_MUL_F, HDK_P_DIV_F,
  HDK_P_CAST_I2F, HDK_P_CAST_F2I, HDK_P_CMP_I, HDK_P_CMP_F,
  HDK_P_AND, HDK_P_OR, HDK_P_NOT, HDK_P_IS_NULL, HDK_P_SELECT
} hdk_hip_project_code;
enum hdk_hip_project_flag { HDK_P_FLAG_NULLABLE = 1, HDK_P_FLAG_FP = 2 }; /* of HDK_P_PUSH_COL */

typedef struct hdk_hip_project_op {
  uint8_t code;         /* hdk_hip_project_code */
  uint8_t check_width;  /* ADD_I / SUB_I / MUL_I: bytes of the checked SQL type, 0 = unchecked */
  uint8_t flags;        /* PUSH_COL: hdk_hip_project_flag bits; CMP_I / CMP_F: the hdk_hip_cmp */
  uint8_t pad_;
  uint32_t col;         /* PUSH_COL: the input column */
  int64_t imm;          /* PUSH_COL: the column's in-band NULL; PUSH_INT / PUSH_FP: the value */
} hdk_hip_project_op;

typedef struct hdk_hip_project_out {
  int32_t first_op;     /* the out's program: ops[first_op .. first_op + num_ops) */
  int32_t num_ops;
  uint8_t is_fp;        /* the program leaves an FP value; else an INT */
  uint8_t nullable;     /* describes the column; a NULL result stores null_bits either way */
  uint8_t pad_[6];
  int64_t null_bits;
} hdk_hip_project_out;

int32_t hdk_hip_project_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                                const hdk_hip_project_op* ops, int32_t num_ops, const hdk_hip_project_out* outs,
                                int32_t num_outs, int64_t* out_cols, uint64_t out_capacity, int32_t* error_code_dev,
                                int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Equi-join of two blocks of dense result columns on the device (sort-merge).
 * The device form, for results whose columns sit in HBM, of the reference's join against a previous step's result: a
 * registered ResultSet is fetched as ColumnarResults and handed to the hash-table builders like any table
 * (ColumnFetcher::makeJoinColumn, omniscidb/QueryEngine/ColumnFetcher.cpp:111); the join types are JoinType's INNER, LEFT,
 * SEMI and ANTI (omniscidb/Shared/sqldefs.h:33), here hdk_hip_join_type as hdk_hip_join uses it.
 * Inputs: two blocks of dense columns, left (`lnum_cols` columns of `lnum_rows` 8-byte words, column t at
 * lcols + t * lcapacity) and right (the same with r), NULLs in band -- what the other *_columns calls write.  rcols may be
 * NULL when rnum_rows == 0.
 * Keys: `num_keys` (1..HDK_HIP_MAX_JOIN_COLUMNS_KEYS) pairs of columns, int64 words only (the reference hashes integers and
 * dictionary ids; doubles have no equality that this library's sort and its comparisons agree on).  A word is NULL when
 * its side is nullable and the word EQUALS that side's null_bits (a bit compare, the rule of hdk_hip_order_entry); the two
 * sides may use different sentinels: equality is on (is NULL, value) pairs, never on raw words.
 * Match: a left row matches a right row when every key is non-NULL on both sides and equal; with HDK_HIP_JOIN_NULL_SAFE
 * (IS NOT DISTINCT FROM) a NULL also matches a NULL.
 * PRECONDITION (as hdk_hip_group_columns has one): the RIGHT rows are ascending on the key columns, in the order that
 * hdk_hip_sort_columns gives for the entries (rcol, is_desc 0, nulls_first 0, is_fp 0, rnullable, rnull_bits) -- NULLs
 * last per column.  The left rows may be in any order.  A right side that is not sorted is not an error and gives
 * unspecified rows; even then nothing outside the permitted output range is written and *row_count is the number of rows
 * the write pass emits: both passes read the same stored per-row (right start, emit offset) pairs.
 * Type: a left row with m matching right rows emits m rows (HDK_JOIN_INNER), max(m, 1) (HDK_JOIN_LEFT), m > 0 ? 1 : 0
 * (HDK_JOIN_SEMI) or m == 0 ? 1 : 0 (HDK_JOIN_ANTI).
 * Output: column j (of `num_outs`, 1..HDK_HIP_MAX_JOIN_COLUMNS_OUTS) at out_cols + j * out_capacity holds the word of
 * column `col` of the left (side 0) or right (side 1) row of each output row.  Right outs are invalid for SEMI / ANTI; in a
 * LEFT join an unmatched row's right outs receive that out's null_bits.  Output rows follow left row order and the matches
 * of one left row follow right row order: the result is deterministic, word for word.
 * *row_count (device) ALWAYS receives the true number of output rows, also when that is >= 2^32; a count-only call
 * (out_cols == NULL or out_capacity == 0) is valid for any such size.  Rows at or beyond out_capacity are not written,
 * nothing outside [0, min(rows, out_capacity)) of an output column or perm is touched, and out_capacity is below 2^32.
 * lperm_out / rperm_out (device, may be NULL; out_capacity entries) receive the left / right input row index of each output
 * row; rperm_out is 0xFFFFFFFF for a row without a partner (an unmatched LEFT row, every ANTI row) and the FIRST matching
 * right row for SEMI.  The inputs are not modified, and no two of the two blocks, out_cols, the perms, row_count and
 * workspace may overlap (a block the call does not touch has no bytes and overlaps nothing).
 * `workspace`: hdk_hip_join_columns_workspace_bytes(lnum_rows) bytes of device memory, 8-byte aligned (host arithmetic only:
 * 12 bytes per left row and 8 bytes per segment of 1 024 left rows, plus at most 1 KiB), or NULL -- the library then takes
 * it from the stream's memory pool (hipMallocAsync), as its siblings do.
 * ASYNCHRONOUS on `stream`: three launches (count, 64-bit scan, expand; two in a count-only call) ordered by the stream
 * alone -- no atomics, no look-back; the host never waits.  Output and *row_count are complete when `stream` has drained.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL lcols / keys / outs /
 * row_count (rcols with rnum_rows > 0), lnum_cols or rnum_cols < 1, num_keys outside 1..8, num_outs outside 1..32, a column
 * index outside its side's columns, side > 1, a right out in SEMI / ANTI, a type outside hdk_hip_join_type, an unknown flag,
 * either row count >= 2^32, rows > capacity, out_capacity >= 2^32, overlapping blocks, a workspace that is too small or not
 * 8-byte aligned.
 * lnum_rows == 0: *row_count = 0 is stored on the stream, nothing else is launched, and a workspace of any size is
 * accepted (none is used).  rnum_rows == 0 is an ordinary call in which every m is 0.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_MAX_JOIN_COLUMNS_KEYS 8 /* (HDK_HIP_MAX_JOIN_KEYS is the keyed storage-table join's) */
#define HDK_HIP_MAX_JOIN_COLUMNS_OUTS 32
#define HDK_HIP_JOIN_NULL_SAFE 1u /* flags: a NULL key matches a NULL key (IS NOT DISTINCT FROM) */

typedef struct hdk_hip_join_key {
  int32_t lcol;        /* key column of the left block */
  int32_t rcol;        /* key column of the right block */
  uint8_t lnullable;   /* 0: lnull_bits is an ordinary value */
  uint8_t rnullable;
  uint8_t pad_[6];
  int64_t lnull_bits;  /* the left column's in-band NULL, as in hdk_hip_order_entry */
  int64_t rnull_bits;
} hdk_hip_join_key;

typedef struct hdk_hip_join_out {
  uint8_t side;        /* 0: a column of the left block; 1: of the right block */
  uint8_t pad_[3];
  int32_t col;
  int64_t null_bits;   /* side 1 in a LEFT join: the word of a row without a partner */
} hdk_hip_join_out;

size_t hdk_hip_join_columns_workspace_bytes(uint64_t lnum_rows);
int32_t hdk_hip_join_columns(const int64_t* lcols, uint64_t lcapacity, int32_t lnum_cols, uint64_t lnum_rows,
                             const int64_t* rcols, uint64_t rcapacity, int32_t rnum_cols, uint64_t rnum_rows,
                             const hdk_hip_join_key* keys, int32_t num_keys, int32_t type, uint32_t flags,
                             const hdk_hip_join_out* outs, int32_t num_outs, int64_t* out_cols, uint64_t out_capacity,
                             uint64_t* row_count, uint32_t* lperm_out, uint32_t* rperm_out, void* workspace,
                             size_t workspace_bytes, int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Set operations over dense result columns on the device: UNION ALL as one copy, and UNION / INTERSECT [ALL] / EXCEPT [ALL]
 * as one walk over sorted runs.
 * The device form, for results whose columns sit in HBM, of the reference's LogicalUnion step over two previous steps'
 * results (RelAlgExecutor::executeUnion, omniscidb/QueryEngine/RelAlgExecutor.cpp), widened to SQL's other set operations.
 * Rows are compared as WHOLE rows, word by word, doubles included.
 *
 * hdk_hip_concat_columns -- UNION ALL.
 * Inputs: two blocks of dense columns, left (`lnum_cols` columns of `lnum_rows` 8-byte words, column t at
 * lcols + t * lcapacity) and right (the same with r), NULLs in band -- what the other *_columns calls write.  The columns of
 * a side without rows may be NULL.  `pairs`: `num_cols` (1..HDK_HIP_MAX_SETOP_COLUMNS) pairs of a left and a right column.
 * Output: rows [0, lnum_rows) are the left rows and rows [lnum_rows, lnum_rows + rnum_rows) the right rows, both in input
 * order.  A word that is NULL on its side (the side is nullable and the word EQUALS that side's null_bits, a bit compare) is
 * written as out_null_bits; every other word is written unchanged -- so a non-NULL word that equals out_null_bits reads as
 * NULL afterwards, the in-band rule of every *_columns call.  side_col < 0: pair j is output column j at
 * out_cols + j * out_capacity.  side_col in [0, num_cols]: the output has num_cols + 1 columns, column side_col receives 0
 * for every left row and 1 for every right row (with HDK_HIP_CONCAT_TAG_FIRST in `flags`: 1 for the left rows and 0 for the
 * right rows, the tag hdk_hip_setop_columns expects when ITS right operand is passed here as the left block), and pair j is
 * output column j + (j >= side_col).  Nothing outside rows [0, lnum_rows + rnum_rows) of an output column is touched.
 * ASYNCHRONOUS on `stream`: one launch, no workspace; the host never waits.  The inputs are not modified and may overlap each
 * other; out_cols may overlap neither.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL pairs / out_cols (lcols or
 * rcols with rows on that side), lnum_cols or rnum_cols < 1, num_cols outside 1..8, a column index outside its side's columns,
 * side_col > num_cols, an unknown flag, lnum_rows + rnum_rows >= 2^32, rows > capacity, out_capacity below
 * lnum_rows + rnum_rows, out_cols overlapping an input.
 * Both sides empty: nothing is launched.
 *
 * hdk_hip_setop_columns -- the rows that a set operation keeps, over ONE block that holds the rows of both operands and a tag.
 * Input: `num_cols` columns of `num_rows` 8-byte words, column t at cols + t * capacity.  key_cols[num_keys]
 * (1..HDK_HIP_MAX_SETOP_COLUMNS) are the compared columns; a word of column `tag_col` (not a key) that is NOT 0 marks a row of
 * the RIGHT operand, a 0 a row of the LEFT operand.  A RUN is a maximal stretch of adjacent rows that are BIT-EQUAL on every
 * key column -- exactly the equivalence of hdk_hip_group_columns: NULL equals NULL, -0.0 differs from +0.0, NaNs are compared
 * by pattern.
 * PRECONDITION (as hdk_hip_group_columns and hdk_hip_join_columns have theirs): equal rows are ADJACENT, and inside a run the
 * rows with a non-zero tag word PRECEDE the rows with tag 0.  hdk_hip_sort_columns (stable: ties keep their input order) on
 * all key columns of a block whose right rows were concatenated FIRST establishes it.  A block that violates it is not an
 * error and gives unspecified rows; even then nothing outside the permitted output range is written, *row_count is the number
 * of rows the write pass emits and is at most num_rows: both passes read the same stored per-row keep bits.
 * With rb = the right rows and lb = the left rows BEFORE a row in its run, the row is kept iff
 *   HDK_SETOP_UNION           rb + lb == 0   (the run's first row, whichever side: one row per distinct row)
 *   HDK_SETOP_INTERSECT       left row, lb == 0, rb > 0
 *   HDK_SETOP_INTERSECT_ALL   left row, lb < rb          (min(l, r) rows of a run with l left and r right rows)
 *   HDK_SETOP_EXCEPT          left row, lb == 0, rb == 0
 *   HDK_SETOP_EXCEPT_ALL      left row, lb >= rb         (max(l - r, 0) rows)
 * Output: the kept rows in input order; output column j (of `num_outs`, 1..HDK_HIP_MAX_SETOP_OUTS) at
 * out_cols + j * out_capacity holds their words of input column out_cols_idx[j] (any column: a subset of the keys, the tag).
 * *row_count (device) ALWAYS receives the true number of kept rows; rows at or beyond out_capacity are not written, and
 * nothing outside [0, min(kept, out_capacity)) of an output column is touched.  out_cols == NULL (or out_capacity == 0):
 * count only.  The input is not modified, and no two of cols, out_cols, row_count and workspace may overlap (out_cols in a
 * count-only call has no bytes and overlaps nothing).
 * `workspace`: hdk_hip_setop_columns_workspace_bytes(num_rows) bytes of device memory, 8-byte aligned (host arithmetic only:
 * per tile of 4 096 rows 512 bytes of keep bits -- one bit per row -- and 20 bytes of counters, plus at most 1.5 KiB), or
 * NULL -- the library then takes it from the stream's memory pool (hipMallocAsync), as its siblings do.
 * ASYNCHRONOUS on `stream`: six launches (summary, scan, carry scan, keep, scan, compact; five in a count-only call) ordered
 * by the stream alone -- no atomics, no look-back; the host never waits.  Output and *row_count are complete when `stream`
 * has drained.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL cols / key_cols /
 * out_cols_idx / row_count, num_cols < 1, num_keys outside 1..8, num_outs outside 1..16, an op outside hdk_hip_setop, a column
 * index outside [0, num_cols), a tag_col that is a key, num_rows >= 2^32, num_rows > capacity, overlapping blocks, a
 * workspace that is too small or not 8-byte aligned.
 * num_rows == 0: *row_count = 0 is stored on the stream, nothing else is launched.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_MAX_SETOP_COLUMNS 8 /* the limit of hdk_hip_sort_columns' entries and hdk_hip_group_columns' keys */
#define HDK_HIP_MAX_SETOP_OUTS 16
#define HDK_HIP_CONCAT_TAG_FIRST 1u /* flags: the side column holds 1 for the left block's rows and 0 for the right's */

typedef enum hdk_hip_setop {
  HDK_SETOP_UNION = 0,
  HDK_SETOP_INTERSECT = 1,
  HDK_SETOP_INTERSECT_ALL = 2,
  HDK_SETOP_EXCEPT = 3,
  HDK_SETOP_EXCEPT_ALL = 4
} hdk_hip_setop;

typedef struct hdk_hip_setop_col {
  int32_t lcol;          /* column of the left block */
  int32_t rcol;          /* column of the right block */
  uint8_t lnullable;     /* 0: lnull_bits is an ordinary value */
  uint8_t rnullable;
  uint8_t pad_[6];
  int64_t lnull_bits;    /* the left column's in-band NULL, as in hdk_hip_order_entry */
  int64_t rnull_bits;
  int64_t out_null_bits; /* what a NULL of either side is written as */
} hdk_hip_setop_col;

int32_t hdk_hip_concat_columns(const int64_t* lcols, uint64_t lcapacity, int32_t lnum_cols, uint64_t lnum_rows,
                               const int64_t* rcols, uint64_t rcapacity, int32_t rnum_cols, uint64_t rnum_rows,
                               const hdk_hip_setop_col* pairs, int32_t num_cols, int32_t side_col, uint32_t flags,
                               int64_t* out_cols, uint64_t out_capacity, int32_t device_id, void* stream);
size_t hdk_hip_setop_columns_workspace_bytes(uint64_t num_rows);
int32_t hdk_hip_setop_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                              const int32_t* key_cols, int32_t num_keys, int32_t tag_col, int32_t op,
                              const int32_t* out_cols_idx, int32_t num_outs, int64_t* out_cols, uint64_t out_capacity,
                              uint64_t* row_count, void* workspace, size_t workspace_bytes, int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense result columns as the chunks of a table: the copy, the sentinel rewrite and the chunk statistics that make a
 * device result the INPUT of a scan step.
 * The device form, for a result whose columns sit in HBM, of what ArrowStorage does when a table is imported: null values
 * rewritten to the column type's in-band sentinel (omniscidb/ArrowStorage/ArrowStorageUtils.cpp:176-213) and the
 * per-fragment chunk metadata min / max / has_nulls (ArrowStorage's computeStats) from which the planner sizes every layout
 * (ColRangeInfo, ExpressionRange).
 *
 * Input: `num_cols_in` dense columns of `num_rows` 8-byte words, column t at cols + t * capacity, NULLs in band -- what the
 * other *_columns calls write.  `sel`: `num_cols` (1..HDK_HIP_MAX_CHUNK_COLUMNS) selected columns, in output order; a column
 * may be selected more than once.
 * Copy: output column j at out_cols + j * out_capacity holds rows [0, num_rows) of input column sel[j].col.  A word of a
 * nullable column that EQUALS null_bits (a bit compare) is written as out_null_bits; every other word is written unchanged --
 * so a non-NULL word that equals out_null_bits reads as NULL afterwards, the in-band rule of every *_columns call.  A word of
 * a column that is not nullable is never rewritten and never counted as NULL.  Nothing outside rows [0, num_rows) of an
 * output column is touched; the input is not modified.
 * The output is a COPY by design: input column t starts at an address that is only 8-byte aligned, while the scan kernels
 * read chunks that start on 256-byte boundaries.  With out_cols 256-byte aligned, fragment_rows % 32 == 0 and
 * out_capacity % 32 == 0 every chunk out_cols + j * out_capacity + f * fragment_rows is.
 * Statistics: num_fragments = max(1, ceil(num_rows / fragment_rows)); fragment f of a column is rows
 * [f * fragment_rows, min((f + 1) * fragment_rows, num_rows)).  stats[j * num_fragments + f] (device) receives, over the
 * OUTPUT words of that fragment: null_count -- the words of a nullable column that equal out_null_bits, i.e. what reads as
 * NULL afterwards --, value_count -- all other words --, and the min and max of those other words: compared as signed int64,
 * or for an is_fp column compared as doubles with the BIT PATTERN of the winning value stored.  An fp word that is a NaN is not
 * NULL and counts in value_count but takes no part in min / max -- a deviation from numpy's min(), which propagates a NaN.
 * -0.0 and +0.0 compare equal; either may be stored.  min_bits / max_bits are meaningful only when value_count > 0; an fp
 * fragment whose values are all NaN leaves min_bits = +inf and max_bits = -inf (min > max: no value took part).
 * `workspace`: hdk_hip_chunk_columns_workspace_bytes(num_rows, fragment_rows, num_cols) bytes of device memory, 8-byte aligned
 * (host arithmetic only: one 32-byte partial per column and tile of 4 096 rows, tiles cut at fragment boundaries -- every
 * fragment but the last has ceil(fragment_rows / 4 096) tiles, the last those of its own rows -- rounded up to 256 bytes), or
 * NULL -- the library then takes it from the stream's memory pool (hipMallocAsync), as its siblings do.
 * ASYNCHRONOUS on `stream`: two launches (the streaming copy that leaves the partials, the fold per column and fragment)
 * ordered by the stream alone -- no atomics, no look-back; the host never waits.  Output and stats are complete when
 * `stream` has drained.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL sel / out_cols / stats
 * (cols with rows), num_cols outside 1..16, a column index outside [0, num_cols_in), fragment_rows 0 or not a multiple of
 * 32, num_rows >= 2^32, num_rows > capacity or > out_capacity, out_capacity not a multiple of 32 when num_cols > 1, out_cols
 * overlapping cols (or any two of cols, out_cols, stats and workspace overlapping), a workspace that is too small or not
 * 8-byte aligned.
 * num_rows == 0: one all-zero stats record per column is stored on the stream, nothing else is launched.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_MAX_CHUNK_COLUMNS 16

typedef struct hdk_hip_chunk_col {
  int32_t col;           /* column of the input block */
  uint8_t is_fp;         /* min / max compare the words as doubles */
  uint8_t nullable;      /* 0: null_bits is an ordinary value */
  uint8_t pad_[2];
  int64_t null_bits;     /* the input column's in-band NULL, as in hdk_hip_order_entry */
  int64_t out_null_bits; /* what a NULL is written as: the NULL of the 8-byte storage type */
} hdk_hip_chunk_col;

typedef struct hdk_hip_chunk_stats {
  int64_t min_bits;
  int64_t max_bits;
  uint64_t null_count;
  uint64_t value_count;
} hdk_hip_chunk_stats;

size_t hdk_hip_chunk_columns_workspace_bytes(uint64_t num_rows, uint64_t fragment_rows, int32_t num_cols);
int32_t hdk_hip_chunk_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols_in, uint64_t num_rows,
                              const hdk_hip_chunk_col* sel, int32_t num_cols, uint64_t fragment_rows, int64_t* out_cols,
                              uint64_t out_capacity, hdk_hip_chunk_stats* stats, void* workspace, size_t workspace_bytes,
                              int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * The key multiplicity of a join key over dense columns: what the planner must know of an INNER table that lies in HBM.
 * The reference finds out whether a one-to-one table will do by trying the fill (fill_one_to_one_hashtable returns -1 ->
 * NeedsOneToManyHash, Builders/PerfectHashTableBuilder.h:134-141) and sizes a projection from the table it then has; here the
 * plan names the table kind up front, so the largest matching set is measured first.  The call files every row exactly as the
 * builds of this library will and leaves one record: max_matches -- the most rows filed under one key --, occupied -- the keys
 * that hold a row --, rows_filed and rows_out_of_range.
 *
 * Input: `num_cols` dense columns of `num_rows` 8-byte words, column t at cols + t * capacity -- the block of a table made by
 * hdk_hip_chunk_columns, or what any *_columns call writes.  `keys`: 1..HDK_HIP_MAX_JOIN_KEYS descriptors.  A word of a
 * nullable key column that EQUALS null_bits (a bit compare) is NULL; a word of a column that is not nullable never is.
 * Perfect route (num_keys == 1, entry_count > 0: the normalised slot count of the perfect table, `bucket` its
 * bucket_normalization), a restatement of fill_hash_join_buff_impl (HashJoinRuntime.cpp:197-240): a NULL word is dropped, or
 * with HDK_HIP_KEYS_NULLS_MATCH (the kBwEq build) filed under translated_null (= max + 1); a non-NULL word outside
 * [min_val, max_val], or a word whose slot (word - min_val) / bucket is not below entry_count, counts in rows_out_of_range
 * and is not filed -- the builds answer -2 there (stale statistics).  max_matches is the largest number of rows in one slot,
 * occupied the number of slots that hold a row.  Method: a histogram of entry_count 32-bit counters in the workspace (the
 * size of the one-to-one table the caller allocates anyway, with the same 2^31 - 1 limit), zeroed on the stream; one
 * streaming pass over tiles of 4 096 rows with one non-returning atomic add per filed row, or ONE add of the lane count for
 * 64 rows whose filing lanes all name the same slot (a column of one key, the long equal runs of a result that arrives
 * sorted); a pass that reduces the histogram to one partial per block; a fold.  No atomics on the record.  ASYNCHRONOUS on
 * `stream`: the host never waits; the record is complete when `stream` has drained.
 * Sorted route (entry_count == 0: composite keys, and a single key whose range exceeds 2^31 - 1 slots -- the plans that take
 * a keyed table): a row with a NULL in any component is skipped, as hdk_hip_fill_baseline_hash_join_buff skips it; rows match
 * when every component word is equal; min_val / max_val / translated_null / bucket / the flag are not read.  The key columns
 * are sorted by hdk_hip_sort_columns into a temporary that holds EVERY column up to the highest key column (that call copies
 * whole blocks), and a longest-run pass over the sorted keys leaves one summary per tile of 4 096 rows -- (leading open run,
 * trailing open run, best closed run, all-one-run flag, runs closed) --, folded with the associative combine.  A run whose
 * rows carry a NULL component has weight 0.  occupied is the number of runs of weight > 0, rows_out_of_range is 0.
 * This route SYNCHRONISES `stream` where hdk_hip_sort_columns does (once per key); the run pass and the fold are asynchronous.
 * `workspace`: hdk_hip_key_multiplicity_workspace_bytes(num_rows, keys, num_keys, entry_count) bytes of device memory, 8-byte
 * aligned (host arithmetic only; perfect: entry_count * 4 rounded up to 256 plus 64 KiB of partials; sorted: the temporary of
 * (highest key column + 1) columns of num_rows rounded up to 32 words, the sort's own workspace and 32 bytes per tile; 0 for
 * num_rows == 0 or arguments the call would refuse), or NULL -- the library then takes it from the stream's memory pool.
 * Errors, all found before any device is touched (HDK_HIP_ERR_INVALID_ARG with a message): a NULL keys / result (cols with
 * rows), num_keys outside 1..3, a key column outside [0, num_cols), num_rows >= 2^32, num_rows > capacity, entry_count < 0 or
 * > 2^31 - 1, entry_count > 0 with more than one key, bucket < 1, unknown flags, a workspace that is too small or not 8-byte
 * aligned, result not 8-byte aligned, any two of cols, result and workspace overlapping.
 * num_rows == 0: an all-zero record is stored on the stream, nothing is launched.  The input is never modified.
 * ---------------------------------------------------------------------------------------- */
#define HDK_HIP_KEYS_NULLS_MATCH 1u /* flags: NULL keys are filed under translated_null (the kBwEq build) */

typedef struct hdk_hip_multiplicity_key {
  int32_t col;             /* column of the input block */
  uint8_t nullable;        /* 0: null_bits is an ordinary value */
  uint8_t pad_[3];
  int64_t null_bits;       /* the column's in-band NULL */
  int64_t min_val;         /* perfect route: the range the table was sized from (JoinColumnTypeInfo) */
  int64_t max_val;
  int64_t translated_null; /* perfect route with HDK_HIP_KEYS_NULLS_MATCH: max_val + 1 */
} hdk_hip_multiplicity_key;

typedef struct hdk_hip_key_multiplicity_result {
  uint64_t max_matches;
  uint64_t occupied;
  uint64_t rows_filed;
  uint64_t rows_out_of_range;
} hdk_hip_key_multiplicity_result;

size_t hdk_hip_key_multiplicity_workspace_bytes(uint64_t num_rows, const hdk_hip_multiplicity_key* keys, int32_t num_keys,
                                                int64_t entry_count);
int32_t hdk_hip_key_multiplicity(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                                 const hdk_hip_multiplicity_key* keys, int32_t num_keys, int64_t entry_count, int64_t bucket,
                                 uint32_t flags, hdk_hip_key_multiplicity_result* result, void* workspace, size_t workspace_bytes,
                                 int32_t device_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Environment switches (MI355X addition; no reference counterpart: the reference's knobs are Config fields,
 * Shared/Config.h).  libhdk_hip.so reads its HDK_HIP_* variables (tests and A/B measurements, none needed
 * in production) ONCE per process, at the first launch that asks for one -- never per launch, so a host that calls
 * setenv() while queries run races with nothing.  A caller that changes them on purpose (the test harness) asks for a
 * re-read; not to be called while another thread is inside a launch.
 * ---------------------------------------------------------------------------------------- */
void hdk_hip_reload_switches(void);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU open-addressing group-by by TUPLE exchange (MI355X addition; replaces, for plans of the
 * radix-partitioned shape, per-device tables + host merge: Executor::reduceMultiDeviceResultSets,
 * QE/Execute.cpp:1224-1336, reduceOneEntryBaseline, QE/ResultSetReduction.cpp:694-731).  Keys are split by owner =
 * mulhi32(key_hash(key), num_owners); owner o ends with an open-addressing table of `owner_entry_count` entries in
 * the plan's layout holding exactly its keys, each group where the reference's probe sequence
 * (key_hash % owner_entry_count, then linearly on) finds it; the query result is the concatenation of the owners'
 * tables.  One step of rank r:
 *     hdk_hip_exchange_shape_for(plan, ko, G, owner_entry_count, &shape)      the same on every rank (host only)
 *     hdk_hip_scatter_to_owners(plan, params, ko, &shape, send, ...)          pass 1 over the rank's fragments:
 *                                                                              (filtered) rows -> tuples -> G segments
 *     all-to-all with EQUAL splits of shape.segment_bytes (RCCL over xGMI; segment o of `send` goes to rank o and
 *                                                          lands as segment r of its `recv`) -- sizes are static,
 *                                                          no counts are exchanged and the host never waits
 *     hdk_hip_aggregate_from_ranks(plan, params, ko, &shape, recv, ...)       passes 2-4 over the G received segments
 *                                                                              into GROUPBY_BUF[0] (the owner's table,
 *                                                                              initialised by the call itself)
 * Tuples are as narrow as the plan's column statistics allow (8 bytes when key and argument fit 32 bits each, else
 * 16 / 24).  `ko->total_rows` must be the SAME upper bound on a rank's outer rows on every rank (it sizes the
 * segments).  Skewed keys (one owner sub-slab overflowing), stale statistics or an interrupt flag the segments; the
 * owner's call then leaves ERROR_CODE = HDK_HIP_ERR_EXCHANGE_INCOMPLETE and the caller redoes the step with partial
 * tables (hdk_hip_launch + hdk_hip_partition_baseline + hdk_hip_reduce_buffers), which has no such limit.
 * Plans outside the radix-partitioned shape (hdk_scan_agg_baseline_direct's: row-wise, 1-2 plain integer key columns,
 * plain-column arguments, `column cmp literal` filters) get HDK_HIP_ERR_UNSUPPORTED from shape_for.
 * `stream` of the two calls must be the stream the all-to-all runs on, or be ordered with it by the caller: NULL means the
 * manager's own stream, which is ordered neither with the legacy default stream nor with a communicator's.
 * ---------------------------------------------------------------------------------------- */
typedef struct hdk_hip_exchange_shape {
  uint32_t num_owners;         /* G, 1 ... 32 (one owner: a rank exchanging with itself -- every kernel and the collective run,
                                  which is how a one-GPU box exercises the RCCL all-to-all) */
  uint32_t owner_entry_count;  /* entries of every owner's table */
  uint32_t tuple_bytes;        /* 8, 16 or 24 */
  uint32_t coarse_per_owner;   /* level-1 bins per owner (G x this <= 256) */
  uint32_t regions_log2;       /* regions of the owner's table per coarse slab = 1 << this */
  uint32_t reserved_;
  uint64_t sub_slab_tuples;    /* capacity of one (coarse slab, XCD) sub-slab */
  uint64_t segment_header_bytes; /* header: uint32 tuples per (coarse slab, XCD) sub-slab, a flag word (0 = complete) and a
                                    tag word (tuple bytes | coarse_per_owner << 8) that the owner checks against its own
                                    shape: a sender that chose another tuple width makes the exchange INCOMPLETE */
  uint64_t segment_bytes;      /* one rank -> owner segment: header + coarse_per_owner x 8 sub-slabs; `send` and `recv`
                                  are num_owners segments each */
  uint64_t rows_bound;         /* ko->total_rows the shape was made for */
  uint64_t scatter_workspace_bytes;   /* `workspace` of hdk_hip_scatter_to_owners */
  uint64_t aggregate_workspace_bytes; /* `workspace` of hdk_hip_aggregate_from_ranks */
} hdk_hip_exchange_shape;
int32_t hdk_hip_exchange_shape_for(const hdk_hip_plan* plan, const hdk_hip_kernel_options* ko, int32_t num_owners,
                                   uint32_t owner_entry_count, int32_t device_id, hdk_hip_exchange_shape* shape);
/* `params`: the 12 launch pointers of hdk_hip_launch (GROUPBY_BUF unused); `send`: num_owners x segment_bytes of device
 * memory, 256-byte aligned.  Honours HDK_HIP_LAUNCH_CHECK_INTERRUPT / watchdog_ms / RECORD_EVENTS of `ko`. */
int32_t hdk_hip_scatter_to_owners(const hdk_hip_plan* plan, int8_t* const params[HDK_KP_COUNT],
                                  const hdk_hip_kernel_options* ko, const hdk_hip_exchange_shape* shape, int8_t* send,
                                  int32_t device_id, void* stream, void* workspace, size_t workspace_bytes);
/* `params`: GROUPBY_BUF[0] = the owner's table (hdk_hip_baseline_table_quads(plan, owner_entry_count) words, written
 * completely: no initialisation needed), INIT_AGG_VALS and ERROR_CODE as for hdk_hip_launch; the other entries are
 * not read.  `recv`: the num_owners segments this owner received, in rank order. */
int32_t hdk_hip_aggregate_from_ranks(const hdk_hip_plan* plan, int8_t* const params[HDK_KP_COUNT],
                                     const hdk_hip_kernel_options* ko, const hdk_hip_exchange_shape* shape,
                                     const int8_t* recv, int32_t device_id, void* stream, void* workspace,
                                     size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * Hash-join table build (perfect hash).
 * Replaces the *_on_device free functions of QE/JoinHashTable/Runtime/HashJoinRuntime.h:66-68,
 * 158-200 (GPU bodies QE/JoinHashTable/Runtime/HashJoinRuntimeGpu.cu:32-190).  The structs carry the same fields
 * as the reference's PODs (HashJoinRuntime.h:43-57,100-124) but are NOT layout-compatible with them: fixed-width
 * members, `bool` widened to int32, and hdk_hip_join_column_type_info keeps column_type in front of
 * translated_null_val (the reference: `translated_null_val, uses_bw_eq, column_type`).  Convert field by field
 * (hdk_amd/glue/HipRuntimeOnDevice.h: to_abi / to_abi_column), never by memcpy.
 * ---------------------------------------------------------------------------------------- */
typedef struct hdk_hip_join_chunk {  /* JoinChunk */
  const int8_t* col_buff;
  size_t num_elems;
  size_t row_id;
} hdk_hip_join_chunk;
typedef struct hdk_hip_join_column { /* JoinColumn */
  const int8_t* col_chunks_buff;     /* device array of hdk_hip_join_chunk */
  size_t col_chunks_buff_sz;
  size_t num_chunks;
  size_t num_elems;
  size_t elem_sz;
} hdk_hip_join_column;
enum hdk_hip_column_type { HDK_JC_SMALL_DATE = 0, HDK_JC_SIGNED = 1, HDK_JC_UNSIGNED = 2, HDK_JC_DOUBLE = 3 };
typedef struct hdk_hip_join_column_type_info { /* JoinColumnTypeInfo */
  size_t elem_sz;
  int64_t min_val;
  int64_t max_val;
  int64_t null_val;
  int32_t uses_bw_eq;
  int32_t column_type; /* hdk_hip_column_type */
  int64_t translated_null_val;
} hdk_hip_join_column_type_info;
typedef struct hdk_hip_hash_entry_info { /* HashEntryInfo */
  size_t hash_entry_count;
  int64_t bucket_normalization;
} hdk_hip_hash_entry_info;

/* init_hash_join_buff_on_device (HashJoinRuntime.h:66-68) */
int32_t hdk_hip_init_hash_join_buff(int32_t* buff, int64_t entry_count, int32_t invalid_slot_val,
                                    int32_t device_id, void* stream);
/* fill_hash_join_buff_on_device[_bucketized] (HashJoinRuntime.h:158-171): one-to-one; on a duplicate
 * key `*dev_err_buff` becomes -1 (the caller then rebuilds one-to-many, PerfectHashTableBuilder.h:134-141).
 * ONE call fills ONE table: from 2 M rows on (and a table of at most 16 slots per row) the fill goes through slot-range
 * partitions whose build pass writes EVERY slot of `buff` (the claimed row id, or `invalid_slot_val`), so entries of an
 * earlier call into the same buffer do not survive -- the reference's callers (PerfectHashTableBuilder::initOneToOneHashTable
 * OnGpu) hand the whole JoinColumn to one call as well. */
int32_t hdk_hip_fill_hash_join_buff(int32_t* buff, int32_t invalid_slot_val, int32_t for_semi_join,
                                    int32_t* dev_err_buff, hdk_hip_join_column join_column,
                                    hdk_hip_join_column_type_info type_info, int32_t device_id,
                                    void* stream);
int32_t hdk_hip_fill_hash_join_buff_bucketized(int32_t* buff, int32_t invalid_slot_val,
                                               int32_t for_semi_join, int32_t* dev_err_buff,
                                               hdk_hip_join_column join_column,
                                               hdk_hip_join_column_type_info type_info,
                                               int64_t bucket_normalization, int32_t device_id,
                                               void* stream);
/* fill_one_to_many_hash_table_on_device[_bucketized] (HashJoinRuntime.h:188-200): layout
 * [pos | count | row ids] of int32 (Builders/PerfectHashTableBuilder.h:35-38). `buff` must have been
 * initialised with hdk_hip_init_hash_join_buff over 2*entries + num_elems slots' first 2*entries. */
int32_t hdk_hip_fill_one_to_many_hash_table(int32_t* buff, hdk_hip_hash_entry_info hash_entry_info,
                                            int32_t invalid_slot_val, hdk_hip_join_column join_column,
                                            hdk_hip_join_column_type_info type_info, int32_t device_id,
                                            void* stream);
int32_t hdk_hip_fill_one_to_many_hash_table_bucketized(int32_t* buff,
                                                       hdk_hip_hash_entry_info hash_entry_info,
                                                       int32_t invalid_slot_val,
                                                       hdk_hip_join_column join_column,
                                                       hdk_hip_join_column_type_info type_info,
                                                       int32_t device_id, void* stream);

/* Keyed ("baseline") join tables for composite or wide keys -- the *_on_device_{32,64} functions of
 * HashJoinRuntime.h:181-204,225-281 (GPU bodies HashJoinRuntimeGpu.cu:192-330), with the
 * GenericKeyHandler (HashJoinKeyHandlers.h:36-100) passed as its two arrays: `join_column_per_key`
 * and `type_info_per_key` are HOST arrays of `key_component_count` entries; `key_component_width`
 * (4 or 8) selects the _32 / _64 form.  A row with a NULL component is skipped.
 *   init : keys = EMPTY_KEY, payload (with_val_slot) = invalid_slot_val
 *   fill : one-to-one table (with_val_slot=1; *dev_err_buff becomes -1 on a duplicate key, -2 when
 *          the table is full) or just the composite-key dictionary (with_val_slot=0)
 *   fill_one_to_many : `buff` = int32 [offsets | counts | row ids] right after the dictionary
 *          `composite_key_dict` (which fill with_val_slot=0 built) */
int32_t hdk_hip_init_baseline_hash_join_buff(int8_t* hash_buff, int64_t entry_count, size_t key_component_count,
                                             int32_t key_component_width, int32_t with_val_slot,
                                             int32_t invalid_slot_val, int32_t device_id, void* stream);
int32_t hdk_hip_fill_baseline_hash_join_buff(int8_t* hash_buff, int64_t entry_count, int32_t invalid_slot_val,
                                             int32_t for_semi_join, size_t key_component_count,
                                             int32_t key_component_width, int32_t with_val_slot,
                                             int32_t* dev_err_buff, const hdk_hip_join_column* join_column_per_key,
                                             const hdk_hip_join_column_type_info* type_info_per_key,
                                             int32_t device_id, void* stream);
int32_t hdk_hip_fill_one_to_many_baseline_hash_table(int32_t* buff, const int8_t* composite_key_dict,
                                                     int64_t hash_entry_count, int32_t invalid_slot_val,
                                                     size_t key_component_count, int32_t key_component_width,
                                                     const hdk_hip_join_column* join_column_per_key,
                                                     const hdk_hip_join_column_type_info* type_info_per_key,
                                                     int32_t device_id, void* stream);

/* Build a fused join table (HDK_JOIN_ONE_TO_ONE_FUSED) from a one-to-one table:
 *   out[slot * (1 + ncols) + 0]     = table[slot]                      (row id or invalid)
 *   out[slot * (1 + ncols) + 1 + c] = decode(inner_cols[c][row id])     (0 when the slot is empty)
 * `inner_cols` / `widths` / `kinds` are HOST arrays of ncols device pointers / element widths /
 * hdk_hip_col_kind; inner columns must be linearised (one buffer per column). */
int32_t hdk_hip_build_fused_join_table(const int32_t* table, int64_t entry_count, const int8_t* const* inner_cols,
                                       const int32_t* widths, const int32_t* kinds, int32_t ncols, int64_t* out,
                                       int32_t device_id, void* stream);

/* A one-to-one table AND its fused form in one sweep over the inner rows (MI355X addition; the table is what
 * fill_hash_join_buff_on_device_bucketized leaves, QE/JoinHashTable/Runtime/HashJoinRuntimeGpu.cu:57-75, the fused form
 * what hdk_hip_build_fused_join_table derives from it).  From a few million rows on, and unless the table is built for a
 * semi join, the rows are PARTITIONED by slot range (one or two radix levels) and each 32 768-slot slice is built in LDS
 * and written front to back, payloads travelling with the rows: no random atomics (1e8 of them cost 4.4 ms), no gather
 * through the row id (2.9 ms per 1e8 slots).  hdk_hip_fill_hash_join_buff[_bucketized] take the same route for the table
 * alone.  A taken slot is -1 and a key outside [min, max] -2 in *dev_err_buff, as there; `buff` must have been initialised
 * (hdk_hip_init_hash_join_buff).  `scratch`: hdk_hip_join_build_scratch_bytes(rows, slots, ncols) bytes of device memory
 * (0: this table is not partitioned, none needed), or NULL -- the library then takes it from the stream's memory pool
 * (hipMallocAsync).  HDK_HIP_BUILD_PARTITION_MIN_ROWS overrides the threshold (0 = never partition). */
size_t hdk_hip_join_build_scratch_bytes(int64_t num_rows, int64_t entry_count, int32_t ncols);
int32_t hdk_hip_fill_hash_join_buff_fused(int32_t* buff, int32_t invalid_slot_val, int32_t for_semi_join, int32_t* dev_err_buff,
                                          hdk_hip_join_column join_column, hdk_hip_join_column_type_info type_info,
                                          int64_t bucket_normalization, const int8_t* const* inner_cols, const int32_t* widths,
                                          const int32_t* kinds, int32_t ncols, int64_t* fused_out, void* scratch,
                                          size_t scratch_bytes, int32_t device_id, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDK_HIP_H */
