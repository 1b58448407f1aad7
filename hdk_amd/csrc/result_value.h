// result_value.h -- one slot of an output buffer -> the 8-byte value that ResultSet iteration returns for its target.
// Shared by result_columns.hip (group-by buffers) and row_columns.hip (non-grouped results): slots sign-extended from
// their width, a float accumulator read from the low 4 bytes of its slot and widened, AVG through pair_to_double
// (omniscidb/ResultSet/ResultSetBufferAccessors.h:168-190).
#pragma once
#include "column_primitives.h"

namespace hdk {

enum RcOp : uint32_t {
  RC_COPY = 0,            // the slot (or key), sign-extended; doubles keep their bits
  RC_FLOAT = 1,           // float in the low 4 bytes -> double
  RC_FLOAT_NULLABLE = 2,  // ... and NULL_FLOAT -> NULL_DOUBLE
  RC_AVG_INT = 3,         // pair_to_double: (double)sum / (double)count, NULL_DOUBLE for count 0
  RC_AVG_DOUBLE = 4,
  RC_AVG_FLOAT = 5
};

// how a target's slot (AVG: its two slots) becomes a value
inline RcOp rc_op_of(const hdk_hip_target& tg) {
  if (tg.agg == HDK_AGG_AVG) {
    return tg.arg_is_fp == HDK_FP_SLOT_FLOAT ? RC_AVG_FLOAT : tg.arg_is_fp ? RC_AVG_DOUBLE : RC_AVG_INT;
  }
  if (tg.arg_is_fp == HDK_FP_SLOT_FLOAT && tg.agg != HDK_AGG_COUNT && tg.agg != HDK_AGG_ID) {
    return tg.skip_null ? RC_FLOAT_NULLABLE : RC_FLOAT;
  }
  return RC_COPY;
}

// the table is read once per pass and is larger than the last-level cache: every load is non-temporal (nt_load)
HDK_DEV int64_t rc_load_sext(const int8_t* base, size_t off, uint32_t width) {
  switch (width) {
    case 1:
      return nt_load<int8_t>(base, off);
    case 2:
      return nt_load<int16_t>(base, off);
    case 4:
      return nt_load<int32_t>(base, off);
    default:
      return nt_load<int64_t>(base, off);
  }
}

HDK_DEV int64_t rc_value(uint32_t op, int64_t a, int64_t b) {
  if (op == RC_COPY) {
    return a;
  }
  const int32_t fbits = static_cast<int32_t>(a);
  if (op == RC_FLOAT || op == RC_FLOAT_NULLABLE) {
    if (op == RC_FLOAT_NULLABLE && fbits == HDK_NULL_FLOAT_BITS) {
      return HDK_NULL_DOUBLE_BITS;
    }
    return double_to_bits(static_cast<double>(__int_as_float(fbits)));
  }
  if (b == 0) {
    return HDK_NULL_DOUBLE_BITS;
  }
  const double dividend = op == RC_AVG_INT      ? static_cast<double>(a)
                          : op == RC_AVG_DOUBLE ? bits_to_double(a)
                                                : static_cast<double>(__int_as_float(fbits));
  return double_to_bits(dividend / static_cast<double>(b));
}

}  // namespace hdk
