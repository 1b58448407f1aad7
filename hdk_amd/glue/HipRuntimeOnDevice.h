// HipRuntimeOnDevice.h -- HDK-side forwards for the free functions the executor and the join-table
// builders call with GpuMgrPlatform-style dispatch (reference QE/GpuInitGroupsImpl.cpp:86-159 switches
// on the platform; QE/JoinHashTable/Runtime/HashJoinRuntime.h:66-68,158-200 are CUDA-only today).
// Each forward keeps the reference's name and argument list and adds (device_id, stream = nullptr).
// PODs: the reference's JoinChunk/JoinColumn/JoinColumnTypeInfo/HashEntryInfo are layout-compatible
// with hdk_hip_join_* except JoinColumnTypeInfo (bool/enum members): `to_abi` converts it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "hdk_hip.h"

namespace hip_rt {

inline void check(int32_t status) {
  if (status != HDK_HIP_OK) {
    throw std::runtime_error(std::string("hdk_hip: ") + hdk_hip_last_error());
  }
}

// init_group_by_buffer_on_device(..., GpuMgrPlatform::HIP) -> here (QE/GpuInitGroups.h:23-34)
inline void init_group_by_buffer_on_device_hip(int64_t* groups_buffer, const int64_t* init_vals,
                                               const uint32_t groups_buffer_entry_count, const uint32_t key_count,
                                               const uint32_t key_width, const uint32_t agg_col_count /*row_size_quad*/,
                                               const bool keyless, const int8_t warp_size, const size_t block_size_x,
                                               const size_t grid_size_x, const int device_id) {
  check(hdk_hip_init_group_by_buffer(groups_buffer, init_vals, groups_buffer_entry_count, key_count, key_width,
                                     agg_col_count, keyless, warp_size, block_size_x, grid_size_x, device_id, nullptr));
}

// init_columnar_group_by_buffer_on_device(..., GpuMgrPlatform::HIP) (QE/GpuInitGroups.h:36-48)
inline void init_columnar_group_by_buffer_on_device_hip(int64_t* groups_buffer, const int64_t* init_vals,
                                                        const uint32_t groups_buffer_entry_count,
                                                        const uint32_t key_count, const uint32_t agg_col_count,
                                                        const int8_t* col_sizes, const bool need_padding,
                                                        const bool keyless, const int8_t key_size,
                                                        const size_t block_size_x, const size_t grid_size_x,
                                                        const int device_id) {
  check(hdk_hip_init_columnar_group_by_buffer(groups_buffer, init_vals, groups_buffer_entry_count, key_count,
                                              agg_col_count, col_sizes, need_padding, keyless, key_size, block_size_x,
                                              grid_size_x, device_id, nullptr));
}

// JoinColumnTypeInfo (HashJoinRuntime.h:114-122) -> ABI POD
template <class RefTypeInfo>
inline hdk_hip_join_column_type_info to_abi(const RefTypeInfo& t) {
  hdk_hip_join_column_type_info o;
  o.elem_sz = t.elem_sz;
  o.min_val = t.min_val;
  o.max_val = t.max_val;
  o.null_val = t.null_val;
  o.uses_bw_eq = t.uses_bw_eq ? 1 : 0;
  o.column_type = static_cast<int32_t>(t.column_type);  // SmallDate=0, Signed=1, Unsigned=2, Double=3
  o.translated_null_val = t.translated_null_val;
  return o;
}
template <class RefJoinColumn>
inline hdk_hip_join_column to_abi_column(const RefJoinColumn& c) {
  hdk_hip_join_column o;
  o.col_chunks_buff = c.col_chunks_buff;
  o.col_chunks_buff_sz = c.col_chunks_buff_sz;
  o.num_chunks = c.num_chunks;
  o.num_elems = c.num_elems;
  o.elem_sz = c.elem_sz;
  return o;
}

inline void init_hash_join_buff_on_device(int32_t* buff, const int64_t entry_count, const int32_t invalid_slot_val,
                                          const int device_id) {
  check(hdk_hip_init_hash_join_buff(buff, entry_count, invalid_slot_val, device_id, nullptr));
}

template <class RefJoinColumn, class RefTypeInfo>
inline void fill_hash_join_buff_on_device(int32_t* buff, const int32_t invalid_slot_val, const bool for_semi_join,
                                          int* dev_err_buff, const RefJoinColumn& join_column,
                                          const RefTypeInfo& type_info, const int device_id) {
  check(hdk_hip_fill_hash_join_buff(buff, invalid_slot_val, for_semi_join, dev_err_buff, to_abi_column(join_column),
                                    to_abi(type_info), device_id, nullptr));
}

template <class RefJoinColumn, class RefTypeInfo>
inline void fill_hash_join_buff_on_device_bucketized(int32_t* buff, const int32_t invalid_slot_val,
                                                     const bool for_semi_join, int* dev_err_buff,
                                                     const RefJoinColumn& join_column, const RefTypeInfo& type_info,
                                                     const int64_t bucket_normalization, const int device_id) {
  check(hdk_hip_fill_hash_join_buff_bucketized(buff, invalid_slot_val, for_semi_join, dev_err_buff,
                                               to_abi_column(join_column), to_abi(type_info), bucket_normalization,
                                               device_id, nullptr));
}

// The table AND its fused form ([row id | payload words], HDK_JOIN_ONE_TO_ONE_FUSED) in one sweep over the inner rows: what
// PerfectJoinHashTableBuilder::initOneToOneHashTableOnGpu (Builders/PerfectHashTableBuilder.h:82-141) calls in place of
// fill_hash_join_buff_on_device_bucketized when the plan's kernels read the fused table.  `scratch` comes from the
// BufferProvider (hdk_hip_join_build_scratch_bytes(rows, slots, ncols) bytes; 0 = none needed) or is NULL (stream pool).
template <class RefJoinColumn, class RefTypeInfo>
inline void fill_hash_join_buff_fused_on_device(int32_t* buff, const int32_t invalid_slot_val, const bool for_semi_join,
                                                int* dev_err_buff, const RefJoinColumn& join_column,
                                                const RefTypeInfo& type_info, const int64_t bucket_normalization,
                                                const int8_t* const* inner_cols, const int32_t* widths, const int32_t* kinds,
                                                const int32_t ncols, int64_t* fused_out, int8_t* scratch,
                                                const size_t scratch_bytes, const int device_id) {
  check(hdk_hip_fill_hash_join_buff_fused(buff, invalid_slot_val, for_semi_join, dev_err_buff, to_abi_column(join_column),
                                          to_abi(type_info), bucket_normalization, inner_cols, widths, kinds, ncols, fused_out,
                                          scratch, scratch_bytes, device_id, nullptr));
}

template <class RefHashEntryInfo, class RefJoinColumn, class RefTypeInfo>
inline void fill_one_to_many_hash_table_on_device(int32_t* buff, const RefHashEntryInfo& hash_entry_info,
                                                  const int32_t invalid_slot_val, const RefJoinColumn& join_column,
                                                  const RefTypeInfo& type_info, const int device_id) {
  hdk_hip_hash_entry_info h{hash_entry_info.hash_entry_count, hash_entry_info.bucket_normalization};
  check(hdk_hip_fill_one_to_many_hash_table(buff, h, invalid_slot_val, to_abi_column(join_column), to_abi(type_info),
                                            device_id, nullptr));
}

// ---- keyed ("baseline") join tables: *_on_device_{32,64} of HashJoinRuntime.h:181-204,225-281 ----------
// The reference passes a device-resident GenericKeyHandler; the ABI takes its two arrays on the host
// (join_column_per_key / type_info_per_key, HashJoinKeyHandlers.h:36-50), so the HDK-side builder
// (BaselineJoinHashTableBuilder::initHashTableOnGpu) forwards the vectors it already owns.
template <int W>  // key component width in bytes: 4 -> *_32, 8 -> *_64
inline void init_baseline_hash_join_buff_on_device(int8_t* hash_join_buff, const int64_t entry_count,
                                                   const size_t key_component_count, const bool with_val_slot,
                                                   const int32_t invalid_slot_val, const int device_id) {
  check(hdk_hip_init_baseline_hash_join_buff(hash_join_buff, entry_count, key_component_count, W, with_val_slot,
                                             invalid_slot_val, device_id, nullptr));
}

template <int W, class RefJoinColumn, class RefTypeInfo>
inline void fill_baseline_hash_join_buff_on_device(int8_t* hash_buff, const int64_t entry_count,
                                                   const int32_t invalid_slot_val, const bool for_semi_join,
                                                   const size_t key_component_count, const bool with_val_slot,
                                                   int* dev_err_buff, const RefJoinColumn* join_column_per_key,
                                                   const RefTypeInfo* type_info_per_key, const int device_id) {
  hdk_hip_join_column cols[HDK_HIP_MAX_JOIN_KEYS];
  hdk_hip_join_column_type_info tis[HDK_HIP_MAX_JOIN_KEYS];
  if (key_component_count > HDK_HIP_MAX_JOIN_KEYS) {
    throw std::runtime_error("hdk_hip: more key components than the fixed kernel library takes");
  }
  for (size_t k = 0; k < key_component_count; ++k) {
    cols[k] = to_abi_column(join_column_per_key[k]);
    tis[k] = to_abi(type_info_per_key[k]);
  }
  check(hdk_hip_fill_baseline_hash_join_buff(hash_buff, entry_count, invalid_slot_val, for_semi_join,
                                             key_component_count, W, with_val_slot, dev_err_buff, cols, tis, device_id,
                                             nullptr));
}

template <int W, class RefJoinColumn, class RefTypeInfo>
inline void fill_one_to_many_baseline_hash_table_on_device(int32_t* buff, const int8_t* composite_key_dict,
                                                           const int64_t hash_entry_count,
                                                           const int32_t invalid_slot_val,
                                                           const size_t key_component_count,
                                                           const RefJoinColumn* join_column_per_key,
                                                           const RefTypeInfo* type_info_per_key, const int device_id) {
  hdk_hip_join_column cols[HDK_HIP_MAX_JOIN_KEYS];
  hdk_hip_join_column_type_info tis[HDK_HIP_MAX_JOIN_KEYS];
  if (key_component_count > HDK_HIP_MAX_JOIN_KEYS) {
    throw std::runtime_error("hdk_hip: more key components than the fixed kernel library takes");
  }
  for (size_t k = 0; k < key_component_count; ++k) {
    cols[k] = to_abi_column(join_column_per_key[k]);
    tis[k] = to_abi(type_info_per_key[k]);
  }
  check(hdk_hip_fill_one_to_many_baseline_hash_table(buff, composite_key_dict, hash_entry_count, invalid_slot_val,
                                                     key_component_count, W, cols, tis, device_id, nullptr));
}

// ColumnarResults for a ResultSet whose storage is on the device: what the ColumnarResults constructor
// (ResultSetRegistry/ColumnarResults.cpp:66-123) would call in place of materializeAllColumnsGroupBy (:691-1010) when
// rows.getDeviceType() is GPU.  `plan` describes the buffer's layout (HipPlanBuilder.h, from the QueryMemoryDescriptor),
// `init_vals` is ResultSetStorage::target_init_vals_ (a host vector), `entry_count` that of the buffer handed in.
// Column t of the result starts at out_cols + t * capacity; *row_count_dev (device memory) receives the number of
// non-empty entries, also when out_cols is null (count only) or the capacity is smaller.  `workspace` comes from the
// BufferProvider (columnar_results_workspace_bytes(entry_count) bytes) or is null (the stream's memory pool).
inline size_t columnar_results_workspace_bytes(const uint32_t entry_count) {
  return hdk_hip_result_columns_workspace_bytes(entry_count);
}
inline void columnarize_result_on_device(const hdk_hip_plan& plan, const int64_t* groups_buffer, const uint32_t entry_count,
                                         const int64_t* init_vals, int64_t* out_cols, const size_t capacity,
                                         uint64_t* row_count_dev, int8_t* workspace, const size_t workspace_bytes,
                                         const int device_id) {
  check(hdk_hip_columnarize_result(&plan, groups_buffer, entry_count, init_vals, out_cols, static_cast<uint64_t>(capacity),
                                   row_count_dev, workspace, workspace_bytes, device_id, nullptr));
}

// The same for a projection ResultSet or a non-grouped result on the device: what the ColumnarResults constructor would call
// in place of materializeAllColumnsProjection with copyAllNonLazyColumns / materializeAllColumnsDirectly (ResultSetRegistry/
// ColumnarResults.cpp:520-620).  `total_matched_dev` is the launch's TOTAL_MATCHED word (device memory; null for a
// non-grouped result, whose entry_count is 1): the rows are the first min(max(*total_matched_dev, 0), entry_count) of the
// buffer, in their order.  Column t starts at out_cols + t * capacity; pos_out (device, may be null; `capacity` rows)
// receives the row positions; *row_count_dev always receives the true count.  No workspace; asynchronous on the device's
// stream, the host never waits.
inline void columnarize_rows_on_device(const hdk_hip_plan& plan, const int64_t* buffer, const uint32_t entry_count,
                                       const int32_t* total_matched_dev, int64_t* out_cols, const size_t capacity,
                                       int64_t* pos_out, uint64_t* row_count_dev, const int device_id) {
  check(hdk_hip_columnarize_rows(&plan, buffer, entry_count, total_matched_dev, out_cols, static_cast<uint64_t>(capacity),
                                 pos_out, row_count_dev, device_id, nullptr));
}

// ResultSet::sort for a result whose dense columns are on the device: what doBaselineSort (QueryEngine/ResultSetSort.cpp:
// 64-188) does with ResultSetSortImpl.cu / TopKSort.cu.  `order` is RelAlgExecutionUnit::sort_info.order_entries restated
// (col = tle_no - 1; is_fp / nullable / null_bits from the target's type), `limit` / `offset` are SortInfo's (0 = no
// limit).  Column t of the input starts at cols + t * capacity, of the output at out_cols + t * out_capacity;
// perm_out (device, may be null) receives the permutation.  `workspace` comes from the BufferProvider
// (sort_columns_workspace_bytes(num_rows, num_order) bytes) or is null (the stream's memory pool).  Synchronises the
// stream while it runs (include/hdk_hip.h); the output is complete when the stream has drained.
inline size_t sort_columns_workspace_bytes(const size_t num_rows, const int num_order) {
  return hdk_hip_sort_columns_workspace_bytes(static_cast<uint64_t>(num_rows), num_order);
}
inline void sort_columns_on_device(const int64_t* cols, const size_t capacity, const int num_cols, const size_t num_rows,
                                   const hdk_hip_order_entry* order, const int num_order, const size_t offset,
                                   const size_t limit, int64_t* out_cols, const size_t out_capacity, uint32_t* perm_out,
                                   int8_t* workspace, const size_t workspace_bytes, const int device_id) {
  check(hdk_hip_sort_columns(cols, static_cast<uint64_t>(capacity), num_cols, static_cast<uint64_t>(num_rows), order, num_order,
                             static_cast<uint64_t>(offset), static_cast<uint64_t>(limit), 0u, out_cols,
                             static_cast<uint64_t>(out_capacity), perm_out, workspace, workspace_bytes, device_id, nullptr));
}

// HAVING for a result whose dense columns are on the device: the reference's filter step over the previous step's result
// (a temporary table of ColumnarResults), with DEF_CMP_NULLABLE* comparisons under logical_and / logical_or / logical_not
// (QueryEngine/RuntimeFunctions.cpp:83-117, :355-384).  `leaves` restate the comparisons (target index, hdk_hip_cmp, a
// literal or a second target, and per side is_fp / nullable / null_bits from the target's type), `ops` is the postfix
// program over them in the encoding of hdk_hip_plan::filter_ops (num_ops == 0: the conjunction of all leaves).  Rows on
// which the predicate is TRUE are written in input order to out_cols + t * out_capacity; *row_count_dev (device) always
// receives their true number, rows at or beyond out_capacity are not written, out_cols == nullptr counts only; perm_out
// (device, may be null) receives the input row of each output row.  `workspace` comes from the BufferProvider
// (filter_columns_workspace_bytes(num_rows) bytes) or is null (the stream's memory pool).  Asynchronous on the device's
// stream, like columnarize_result_on_device: the host never waits.
inline size_t filter_columns_workspace_bytes(const size_t num_rows) {
  return hdk_hip_filter_columns_workspace_bytes(static_cast<uint64_t>(num_rows));
}
inline void filter_columns_on_device(const int64_t* cols, const size_t capacity, const int num_cols, const size_t num_rows,
                                     const hdk_hip_having_leaf* leaves, const int num_leaves, const uint8_t* ops,
                                     const int num_ops, int64_t* out_cols, const size_t out_capacity, uint64_t* row_count_dev,
                                     uint32_t* perm_out, int8_t* workspace, const size_t workspace_bytes, const int device_id) {
  check(hdk_hip_filter_columns(cols, static_cast<uint64_t>(capacity), num_cols, static_cast<uint64_t>(num_rows), leaves, num_leaves,
                               ops, num_ops, out_cols, static_cast<uint64_t>(out_capacity), row_count_dev, perm_out, workspace,
                               workspace_bytes, device_id, nullptr));
}

// GROUP BY for a result whose dense columns are on the device and sorted by the keys (sort_columns_on_device): the merge of
// partial results per slot (reduceOneSlot, QueryEngine/ResultSetReduction.cpp) with the _skip_val NULL rules, as a second
// aggregation step -- a roll-up, SELECT DISTINCT, the outer half of COUNT(DISTINCT).  One row per run of adjacent rows
// whose words in the `key_cols` are bit-equal, in input order, column j of `outs` at out_cols + j * out_capacity;
// *row_count_dev (device) always receives the true number of runs, rows at or beyond out_capacity are not written,
// out_cols == nullptr counts only.  `workspace` comes from the BufferProvider (group_columns_workspace_bytes(num_rows,
// num_outs) bytes) or is null (the stream's memory pool).  Asynchronous on the device's stream: the host never waits.
inline size_t group_columns_workspace_bytes(const size_t num_rows, const int num_outs) {
  return hdk_hip_group_columns_workspace_bytes(static_cast<uint64_t>(num_rows), num_outs);
}
inline void group_columns_on_device(const int64_t* cols, const size_t capacity, const int num_cols, const size_t num_rows,
                                    const int32_t* key_cols, const int num_keys, const hdk_hip_group_out* outs, const int num_outs,
                                    int64_t* out_cols, const size_t out_capacity, uint64_t* row_count_dev, int8_t* workspace,
                                    const size_t workspace_bytes, const int device_id) {
  check(hdk_hip_group_columns(cols, static_cast<uint64_t>(capacity), num_cols, static_cast<uint64_t>(num_rows), key_cols, num_keys,
                              outs, num_outs, out_cols, static_cast<uint64_t>(out_capacity), row_count_dev, workspace, workspace_bytes,
                              device_id, nullptr));
}

// The window step for a result whose dense columns are on the device and sorted by (partition keys, order entries)
// (sort_columns_on_device): WindowFunctionContext's per-partition computation (QueryEngine/WindowContext.cpp) over the
// previous step's materialised result.  One word per input row and out, in input row order, column j of `outs` at
// out_cols + j * out_capacity (out_capacity >= num_rows); partitions and peer groups are stretches of adjacent rows whose
// words in `part_cols` (and `order_cols`) are bit-equal.  `workspace` comes from the BufferProvider
// (window_columns_workspace_bytes(num_rows, num_outs) bytes) or is null (the stream's memory pool).  Asynchronous on the
// device's stream: the host never waits.
inline size_t window_columns_workspace_bytes(const size_t num_rows, const int num_outs) {
  return hdk_hip_window_columns_workspace_bytes(static_cast<uint64_t>(num_rows), num_outs);
}
inline void window_columns_on_device(const int64_t* cols, const size_t capacity, const int num_cols, const size_t num_rows,
                                     const int32_t* part_cols, const int num_part, const int32_t* order_cols, const int num_order,
                                     const hdk_hip_window_out* outs, const int num_outs, int64_t* out_cols,
                                     const size_t out_capacity, int8_t* workspace, const size_t workspace_bytes,
                                     const int device_id) {
  check(hdk_hip_window_columns(cols, static_cast<uint64_t>(capacity), num_cols, static_cast<uint64_t>(num_rows), part_cols, num_part,
                               order_cols, num_order, outs, num_outs, out_cols, static_cast<uint64_t>(out_capacity), workspace,
                               workspace_bytes, device_id, nullptr));
}

// The project step for a result whose dense columns are on the device: computed columns over the previous step's
// materialised result, with the reference's nullable arithmetic, checked + - *, division guard, casts, comparisons,
// three-valued logic and CASE (hdk_hip_project_columns in hdk_hip.h has the op set).  `ops` holds the postfix programs of
// the `num_outs` outs (hdk_hip_project_out names each out's range); out j lands at out_cols + j * out_capacity, num_rows
// words in input row order.  `error_code` is the step's ERROR_CODE word in device memory: the call stores 0 and rows that
// raise leave ERR_DIV_BY_ZERO / ERR_OVERFLOW_OR_UNDERFLOW there, to be read once the stream has drained, as after a
// kernel launch.  No workspace.  Asynchronous on the device's stream: the host never waits.
inline void project_columns_on_device(const int64_t* cols, const size_t capacity, const int num_cols, const size_t num_rows,
                                      const hdk_hip_project_op* ops, const int num_ops, const hdk_hip_project_out* outs,
                                      const int num_outs, int64_t* out_cols, const size_t out_capacity, int32_t* error_code,
                                      const int device_id) {
  check(hdk_hip_project_columns(cols, static_cast<uint64_t>(capacity), num_cols, static_cast<uint64_t>(num_rows), ops, num_ops, outs,
                                num_outs, out_cols, static_cast<uint64_t>(out_capacity), error_code, device_id, nullptr));
}

// The join step for two results whose dense columns are on the device, the right one sorted by its key columns
// (sort_columns_on_device, ascending, NULLs last): what the reference does by fetching a registered ResultSet as
// ColumnarResults and handing it to the hash-table builders (ColumnFetcher::makeJoinColumn, QueryEngine/ColumnFetcher.cpp:111),
// as a sort-merge equi-join.  `type` is a hdk_hip_join_type (INNER, LEFT, SEMI, ANTI), `flags` 0 or
// HDK_HIP_JOIN_NULL_SAFE; output rows follow left row order, the matches of one left row right row order, column j of
// `outs` at out_cols + j * out_capacity.  *row_count_dev (device) always receives the true number of output rows (64-bit),
// rows at or beyond out_capacity are not written, out_cols == nullptr counts only; lperm_out / rperm_out (may be null)
// receive each output row's input row indices.  `workspace` comes from the BufferProvider
// (join_columns_workspace_bytes(lnum_rows) bytes) or is null (the stream's memory pool).  Asynchronous on the device's
// stream: the host never waits.
inline size_t join_columns_workspace_bytes(const size_t lnum_rows) {
  return hdk_hip_join_columns_workspace_bytes(static_cast<uint64_t>(lnum_rows));
}
inline void join_columns_on_device(const int64_t* lcols, const size_t lcapacity, const int lnum_cols, const size_t lnum_rows,
                                   const int64_t* rcols, const size_t rcapacity, const int rnum_cols, const size_t rnum_rows,
                                   const hdk_hip_join_key* keys, const int num_keys, const int type, const uint32_t flags,
                                   const hdk_hip_join_out* outs, const int num_outs, int64_t* out_cols, const size_t out_capacity,
                                   uint64_t* row_count_dev, uint32_t* lperm_out, uint32_t* rperm_out, int8_t* workspace,
                                   const size_t workspace_bytes, const int device_id) {
  check(hdk_hip_join_columns(lcols, static_cast<uint64_t>(lcapacity), lnum_cols, static_cast<uint64_t>(lnum_rows), rcols,
                             static_cast<uint64_t>(rcapacity), rnum_cols, static_cast<uint64_t>(rnum_rows), keys, num_keys, type,
                             flags, outs, num_outs, out_cols, static_cast<uint64_t>(out_capacity), row_count_dev, lperm_out,
                             rperm_out, workspace, workspace_bytes, device_id, nullptr));
}

// Set operations of two results that sit in HBM: the device form of LogicalUnion over two previous steps' results
// (RelAlgExecutor::executeUnion, QueryEngine/RelAlgExecutor.cpp), widened to INTERSECT [ALL] and EXCEPT [ALL].
// concat_columns_on_device is UNION ALL: the left rows, then the right rows, each side's in-band NULL rewritten to
// pairs[j].out_null_bits; side_col >= 0 adds a column that holds 0 for left and 1 for right rows (HDK_HIP_CONCAT_TAG_FIRST in
// `flags`: 1 and 0).  setop_columns_on_device walks ONE block in which equal rows are adjacent and, inside a run, the rows
// with a non-zero word in `tag_col` precede the rows with tag 0 -- what a stable hdk_hip_sort_columns on all compared
// columns makes of a block whose RIGHT operand was concatenated first with HDK_HIP_CONCAT_TAG_FIRST -- and writes the rows
// that `op` (a hdk_hip_setop) keeps, in input order, column j at out_cols + j * out_capacity.  *row_count_dev (device)
// always receives the true number of kept rows, rows at or beyond out_capacity are not written, out_cols == nullptr counts
// only.  `workspace` comes from the BufferProvider (setop_columns_workspace_bytes(num_rows) bytes) or is null (the stream's
// memory pool).  Both are asynchronous on the device's stream: the host never waits.
inline void concat_columns_on_device(const int64_t* lcols, const size_t lcapacity, const int lnum_cols, const size_t lnum_rows,
                                     const int64_t* rcols, const size_t rcapacity, const int rnum_cols, const size_t rnum_rows,
                                     const hdk_hip_setop_col* pairs, const int num_cols, const int side_col, const uint32_t flags,
                                     int64_t* out_cols, const size_t out_capacity, const int device_id) {
  check(hdk_hip_concat_columns(lcols, static_cast<uint64_t>(lcapacity), lnum_cols, static_cast<uint64_t>(lnum_rows), rcols,
                               static_cast<uint64_t>(rcapacity), rnum_cols, static_cast<uint64_t>(rnum_rows), pairs, num_cols,
                               side_col, flags, out_cols, static_cast<uint64_t>(out_capacity), device_id, nullptr));
}
inline size_t setop_columns_workspace_bytes(const size_t num_rows) {
  return hdk_hip_setop_columns_workspace_bytes(static_cast<uint64_t>(num_rows));
}
inline void setop_columns_on_device(const int64_t* cols, const size_t capacity, const int num_cols, const size_t num_rows,
                                    const int32_t* key_cols, const int num_keys, const int tag_col, const int op,
                                    const int32_t* out_cols_idx, const int num_outs, int64_t* out_cols, const size_t out_capacity,
                                    uint64_t* row_count_dev, int8_t* workspace, const size_t workspace_bytes,
                                    const int device_id) {
  check(hdk_hip_setop_columns(cols, static_cast<uint64_t>(capacity), num_cols, static_cast<uint64_t>(num_rows), key_cols, num_keys,
                              tag_col, op, out_cols_idx, num_outs, out_cols, static_cast<uint64_t>(out_capacity), row_count_dev,
                              workspace, workspace_bytes, device_id, nullptr));
}

// A result that sits in HBM as the input of the next step's SCAN: the device form of what ArrowStorage does on import -- the
// sentinel rewrite (ArrowStorage/ArrowStorageUtils.cpp:176-213) and the chunk metadata (ArrowStorage's computeStats).
// chunk_columns_on_device copies the selected dense columns into `out_cols` (a fresh, 256-byte-aligned block: column j at
// out_cols + j * out_capacity, fragment f of it fragment_rows * f rows further on), writes each nullable column's in-band
// NULL as sel[j].out_null_bits -- the NULL of the 8-byte storage type -- and leaves one hdk_hip_chunk_stats per (column,
// fragment) in `stats_dev` (device, [num_cols][max(1, ceil(num_rows / fragment_rows))]): min / max / null_count /
// value_count, from which ChunkMetadata is filled once the stream has drained.  fragment_rows and (with more than one
// column) out_capacity are multiples of 32.  `workspace` comes from the BufferProvider
// (chunk_columns_workspace_bytes(num_rows, fragment_rows, num_cols) bytes) or is null (the stream's memory pool).
// Asynchronous on the device's stream: the host never waits.
inline size_t chunk_columns_workspace_bytes(const size_t num_rows, const size_t fragment_rows, const int num_cols) {
  return hdk_hip_chunk_columns_workspace_bytes(static_cast<uint64_t>(num_rows), static_cast<uint64_t>(fragment_rows), num_cols);
}
inline void chunk_columns_on_device(const int64_t* cols, const size_t capacity, const int num_cols_in, const size_t num_rows,
                                    const hdk_hip_chunk_col* sel, const int num_cols, const size_t fragment_rows,
                                    int64_t* out_cols, const size_t out_capacity, hdk_hip_chunk_stats* stats_dev,
                                    int8_t* workspace, const size_t workspace_bytes, const int device_id) {
  check(hdk_hip_chunk_columns(cols, static_cast<uint64_t>(capacity), num_cols_in, static_cast<uint64_t>(num_rows), sel, num_cols,
                              static_cast<uint64_t>(fragment_rows), out_cols, static_cast<uint64_t>(out_capacity), stats_dev,
                              workspace, workspace_bytes, device_id, nullptr));
}

}  // namespace hip_rt
