// project_columns.hip -- computed columns over dense 8-byte result columns in HBM: one word per input row and out.
//
// Device form of the reference's project step over a temporary table (the previous step's ResultSet, materialised as
// ColumnarResults): DEF_ARITH_NULLABLE* (omniscidb/QueryEngine/RuntimeFunctions.cpp:49-80) behind the overflow checks and
// the division guard of QE/ArithmeticIR.cpp:277-634, the casts (:311-345), DEF_CMP_NULLABLE* (:83-117), logical_not /
// logical_and / logical_or (:355-384) and CASE (QE/CaseIR.cpp).  The integer arithmetic is device_common.h's eval_expr:
// the same checked_arith, the same division and modulo.
//
// One launch, a persistent grid over tiles of kPcTile rows; no block ever waits for another block.  The programs travel
// as a POD kernel argument (PcDesc): the op loop reads them from scalar registers, every branch on an op is a scalar
// branch, and the per-row loops sit inside the cases.  A tile first loads every DISTINCT input column once (the host
// renames the columns of the call to 0 .. nin - 1), then runs the outs one after the other on a value stack that lives
// in registers: st.v[0] is the top, a push shifts the slots down and a pop shifts them up, so no slot is ever indexed by
// a run-time value (which would put the stack in scratch memory).  NULL bits and error marks are one bit per row of the
// lane (bit j = its j-th row of the tile).  Three instantiations -- stack 2 / 4 / 6 with 2 / 4 / 8 input columns -- keep
// short programs from paying registers for six slots; the host picks the smallest that holds the call.
// Traffic: 8 bytes per row and distinct input column read, 8 bytes per row and out written.
#include <string.h>

#include "column_primitives.h"
#include "host_common.h"

namespace hdk {

constexpr int kPcBlock = kTileBlock;
constexpr int kPcItems = 4;  // rows per thread and tile
constexpr uint32_t kPcTile = kPcBlock * kPcItems;
constexpr int kPcWaves = kPcBlock / kWave;
constexpr uint32_t kPcAllRows = (1u << kPcItems) - 1u;

enum PcOutFlag : uint32_t { PC_OUT_PASS = 1u };  // a bare PUSH_COL: the word is copied unexamined

struct PcOut {
  uint32_t first, count;
  uint32_t flags, pad_;
  int64_t null_bits;
};

struct PcDesc {
  uint32_t nouts, nin;
  uint32_t in_col[HDK_HIP_MAX_PROJECT_INPUTS];  // the distinct input columns; an op's `col` indexes this list
  PcOut out[HDK_HIP_MAX_PROJECT_OUTS];
  hdk_hip_project_op op[HDK_HIP_MAX_PROJECT_OPS];
};

// D values of kPcItems rows each, slot 0 the top.  nul / e1 / e7: bit j = row j is NULL / carries a pending
// HDK_HIP_ERR_DIV_BY_ZERO / a pending HDK_HIP_ERR_OVERFLOW_OR_UNDERFLOW.  A BOOL holds 0 or 1 in its word.
template <int D>
struct PcStack {
  int64_t v[D][kPcItems];
  uint32_t nul[D], e1[D], e7[D];

  HDK_DEV void push() {
#pragma unroll
    for (int k = D - 1; k > 0; --k) {
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        v[k][j] = v[k - 1][j];
      }
      nul[k] = nul[k - 1];
      e1[k] = e1[k - 1];
      e7[k] = e7[k - 1];
    }
    nul[0] = 0;
    e1[0] = 0;
    e7[0] = 0;
  }
  // slots FROM + 1 .. move up by FROM: the result of an op that read FROM + 1 values already stands in slot 0
  template <int FROM>
  HDK_DEV void drop() {
#pragma unroll
    for (int k = 1; k + FROM < D; ++k) {
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        v[k][j] = v[k + FROM][j];
      }
      nul[k] = nul[k + FROM];
      e1[k] = e1[k + FROM];
      e7[k] = e7[k + FROM];
    }
  }
  // bit j: the BOOL in slot k is TRUE / FALSE (and not NULL)
  HDK_DEV uint32_t truths(int k) const {
    uint32_t t = 0;
#pragma unroll
    for (int j = 0; j < kPcItems; ++j) {
      t |= v[k][j] != 0 ? 1u << j : 0u;
    }
    return t & ~nul[k];
  }
  HDK_DEV void set_bool(uint32_t t) {
#pragma unroll
    for (int j = 0; j < kPcItems; ++j) {
      v[0][j] = (t >> j) & 1u;
    }
  }
};

template <bool FP>
HDK_DEV uint32_t pc_compare(uint32_t cmp, const int64_t (&a)[kPcItems], const int64_t (&b)[kPcItems]) {
  uint32_t m = 0;
#define HDK_PC_BITS(OP)                                                                                 \
  _Pragma("unroll") for (int j = 0; j < kPcItems; ++j) {                                                \
    const bool t = FP ? bits_to_double(a[j]) OP bits_to_double(b[j]) : a[j] OP b[j];                    \
    m |= t ? 1u << j : 0u;                                                                              \
  }
  switch (cmp) {
    case HDK_CMP_EQ: HDK_PC_BITS(==) break;
    case HDK_CMP_NE: HDK_PC_BITS(!=) break;
    case HDK_CMP_LT: HDK_PC_BITS(<) break;
    case HDK_CMP_GT: HDK_PC_BITS(>) break;
    case HDK_CMP_LE: HDK_PC_BITS(<=) break;
    default: HDK_PC_BITS(>=) break;
  }
#undef HDK_PC_BITS
  return m;
}

// one op on the stack: a = slot 1, b = slot 0 for the binary ops (the op is wave-uniform)
template <int D, int NIN>
HDK_DEV void pc_step(PcStack<D>& st, const hdk_hip_project_op& op, const int64_t (&in)[NIN][kPcItems]) {
  switch (op.code) {
    case HDK_P_PUSH_COL: {
      st.push();
      uint32_t isnull = 0;
#pragma unroll
      for (int k = 0; k < NIN; ++k) {
        if (op.col == static_cast<uint32_t>(k)) {
#pragma unroll
          for (int j = 0; j < kPcItems; ++j) {
            st.v[0][j] = in[k][j];
            isnull |= in[k][j] == op.imm ? 1u << j : 0u;
          }
        }
      }
      st.nul[0] = (op.flags & HDK_P_FLAG_NULLABLE) ? isnull : 0u;
      break;
    }
    case HDK_P_PUSH_INT:
    case HDK_P_PUSH_FP:
    case HDK_P_PUSH_NULL_INT:
    case HDK_P_PUSH_NULL_FP:
      st.push();
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        st.v[0][j] = op.code <= HDK_P_PUSH_FP ? op.imm : 0;
      }
      st.nul[0] = op.code <= HDK_P_PUSH_FP ? 0u : kPcAllRows;
      break;
    case HDK_P_ADD_I:
    case HDK_P_SUB_I:
    case HDK_P_MUL_I: {
      const int aop = op.code == HDK_P_ADD_I ? HDK_OP_ADD : op.code == HDK_P_SUB_I ? HDK_OP_SUB : HDK_OP_MUL;
      uint32_t ovf = 0;
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        int64_t r;
        ovf |= checked_arith(aop, st.v[1][j], st.v[0][j], op.check_width, &r) ? 1u << j : 0u;
        st.v[0][j] = r;
      }
      st.nul[0] |= st.nul[1];
      st.e1[0] |= st.e1[1];
      st.e7[0] |= st.e7[1] | (ovf & ~st.nul[0]);  // (a NULL operand: nothing is checked)
      st.template drop<1>();
      break;
    }
    case HDK_P_DIV_I:
    case HDK_P_MOD_I: {
      uint32_t zero = 0;
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        const int64_t a = st.v[1][j], b = st.v[0][j];
        zero |= b == 0 ? 1u << j : 0u;
        const int64_t den = b == 0 || b == -1 ? 1 : b;  // (neither INT64_MIN / -1 nor x / 0 reaches the divider)
        if (op.code == HDK_P_DIV_I) {
          // a / -1 = -a wrapping: INT64_MIN stays INT64_MIN
          st.v[0][j] = b == -1 ? static_cast<int64_t>(0ull - static_cast<uint64_t>(a)) : a / den;
        } else {
          st.v[0][j] = b == -1 ? 0 : a % den;
        }
      }
      st.nul[0] |= st.nul[1];
      st.e1[0] |= st.e1[1] | (zero & ~st.nul[0]);
      st.e7[0] |= st.e7[1];
      st.template drop<1>();
      break;
    }
    case HDK_P_ADD_F:
    case HDK_P_SUB_F:
    case HDK_P_MUL_F:
    case HDK_P_DIV_F: {
      uint32_t zero = 0;
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        const double a = bits_to_double(st.v[1][j]), b = bits_to_double(st.v[0][j]);
        double r;
        if (op.code == HDK_P_ADD_F) {
          r = a + b;
        } else if (op.code == HDK_P_SUB_F) {
          r = a - b;
        } else if (op.code == HDK_P_MUL_F) {
          r = a * b;
        } else {
          r = a / b;
          zero |= b == 0.0 ? 1u << j : 0u;
        }
        st.v[0][j] = double_to_bits(r);
      }
      st.nul[0] |= st.nul[1];
      st.e1[0] |= st.e1[1] | (zero & ~st.nul[0]);
      st.e7[0] |= st.e7[1];
      st.template drop<1>();
      break;
    }
    case HDK_P_CAST_I2F:
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        st.v[0][j] = double_to_bits(static_cast<double>(st.v[0][j]));
      }
      break;
    case HDK_P_CAST_F2I:
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        const double d = bits_to_double(st.v[0][j]);
        st.v[0][j] = static_cast<int64_t>(d + (d < 0.0 ? -0.5 : 0.5));
      }
      break;
    case HDK_P_CMP_I:
    case HDK_P_CMP_F: {
      const uint32_t t = op.code == HDK_P_CMP_F ? pc_compare<true>(op.flags, st.v[1], st.v[0])
                                                : pc_compare<false>(op.flags, st.v[1], st.v[0]);
      st.set_bool(t);
      st.nul[0] |= st.nul[1];
      st.e1[0] |= st.e1[1];
      st.e7[0] |= st.e7[1];
      st.template drop<1>();
      break;
    }
    case HDK_P_AND:
    case HDK_P_OR: {
      const uint32_t ta = st.truths(1), tb = st.truths(0);
      const uint32_t fa = ~(ta | st.nul[1]), fb = ~(tb | st.nul[0]);
      const uint32_t ma = st.e1[1] | st.e7[1], mb = st.e1[0] | st.e7[0];  // marked rows
      uint32_t rt, rn, decided;
      if (op.code == HDK_P_AND) {
        rt = ta & tb;
        rn = ~(rt | fa | fb);
        decided = (fa & ~ma) | (fb & ~mb);  // an unmarked FALSE decides alone
      } else {
        rt = ta | tb;
        rn = ~rt & (st.nul[0] | st.nul[1]);
        decided = (ta & ~ma) | (tb & ~mb);  // an unmarked TRUE
      }
      st.set_bool(rt);
      st.nul[0] = rn & kPcAllRows;
      st.e1[0] = (st.e1[0] | st.e1[1]) & ~decided;
      st.e7[0] = (st.e7[0] | st.e7[1]) & ~decided;
      st.template drop<1>();
      break;
    }
    case HDK_P_NOT:
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        st.v[0][j] = st.v[0][j] == 0;  // NULL stays NULL, TRUE <-> FALSE
      }
      break;
    case HDK_P_IS_NULL:
      st.set_bool(st.nul[0]);
      st.nul[0] = 0;
      break;
    default:  // HDK_P_SELECT: else = slot 0, then = slot 1, cond = slot 2
      if constexpr (D >= 3) {
        const uint32_t take = st.truths(2);
#pragma unroll
        for (int j = 0; j < kPcItems; ++j) {
          st.v[0][j] = (take >> j) & 1u ? st.v[1][j] : st.v[0][j];
        }
        st.nul[0] = (take & st.nul[1]) | (~take & st.nul[0]);
        st.e1[0] = st.e1[2] | (take & st.e1[1]) | (~take & st.e1[0]);
        st.e7[0] = st.e7[2] | (take & st.e7[1]) | (~take & st.e7[0]);
        st.template drop<2>();
      }
      break;
  }
}

// Row r of a tile belongs to thread r % kPcBlock, item r / kPcBlock: consecutive lanes read and write consecutive rows.
// (tile * kPcTile + kPcTile - 1 never exceeds 2^32 - 1: tile < ceil(n / kPcTile), n < 2^32.)
template <int D, int NIN>
__global__ __launch_bounds__(kPcBlock) void hdk_project_rows(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n,
                                                              PcDesc d, uint32_t ntiles, int64_t* __restrict__ out,
                                                              uint64_t out_capacity, int32_t* __restrict__ error_code) {
  __shared__ int32_t s_err[kPcWaves];
  uint32_t seen1 = 0, seen7 = 0;  // rows of this lane whose out carried a mark
  PcStack<D> st;
#pragma unroll
  for (int k = 0; k < D; ++k) {
#pragma unroll
    for (int j = 0; j < kPcItems; ++j) {
      st.v[k][j] = 0;
    }
    st.nul[k] = 0;
    st.e1[k] = 0;
    st.e7[k] = 0;
  }
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t r0 = tile * kPcTile + threadIdx.x;
    int64_t in[NIN][kPcItems];
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        in[k][j] = 0;
      }
      if (static_cast<uint32_t>(k) < d.nin) {
        const int64_t* col = cols + static_cast<uint64_t>(d.in_col[k]) * capacity;
#pragma unroll
        for (int j = 0; j < kPcItems; ++j) {
          // (a row past the end reads the last row instead: the loads of a tile are issued together, and such a row
          // computes, and raises, what the last row does; it is not stored)
          const uint32_t r = r0 + static_cast<uint32_t>(j) * kPcBlock;
          in[k][j] = nt_load<int64_t>(col + (r < n ? r : n - 1), 0);
        }
      }
    }
    for (uint32_t jo = 0; jo < d.nouts; ++jo) {
      const PcOut o = d.out[jo];
      for (uint32_t i = o.first; i < o.first + o.count; ++i) {
        pc_step<D, NIN>(st, d.op[i], in);
      }
      int64_t* dst = out + static_cast<uint64_t>(jo) * out_capacity;
      const uint32_t isnull = (o.flags & PC_OUT_PASS) ? 0u : st.nul[0];
#pragma unroll
      for (int j = 0; j < kPcItems; ++j) {
        const uint32_t r = r0 + static_cast<uint32_t>(j) * kPcBlock;
        if (r < n) {
          dst[r] = (isnull >> j) & 1u ? o.null_bits : st.v[0][j];
        }
      }
      seen1 |= st.e1[0];
      seen7 |= st.e7[0];
      st.template drop<1>();  // the out's value leaves: the stack is empty again
    }
  }
  if (error_code) {  // (kernel-uniform)
    const bool w7 = __builtin_amdgcn_ballot_w64(seen7 != 0) != 0;
    const bool w1 = __builtin_amdgcn_ballot_w64(seen1 != 0) != 0;
    if ((threadIdx.x & (kWave - 1)) == 0) {
      s_err[threadIdx.x / kWave] = w7 ? HDK_HIP_ERR_OVERFLOW_OR_UNDERFLOW : w1 ? HDK_HIP_ERR_DIV_BY_ZERO : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int32_t worst = 0;
#pragma unroll
      for (int w = 0; w < kPcWaves; ++w) {
        worst = s_err[w] > worst ? s_err[w] : worst;
      }
      record_error(error_code, worst);  // the numerically largest code wins: one atomic per block that saw any
    }
  }
}

enum PcClass : uint8_t { PC_INT = 0, PC_FP = 1, PC_BOOL = 2 };

struct PcCheck {
  int max_depth = 0;
  bool can_raise = false;
};

// the program of one out is well typed: every operand there and of its class, one INT / FP value left
static const char* pc_check_program(const hdk_hip_project_op* ops, int32_t count, int32_t num_cols, bool out_fp, PcCheck* chk) {
  uint8_t cls[HDK_HIP_MAX_PROJECT_STACK];
  int depth = 0;
  for (int32_t i = 0; i < count; ++i) {
    const hdk_hip_project_op& op = ops[i];
    int pops = 0;
    uint8_t want = PC_INT, gives = PC_INT;
    switch (op.code) {
      case HDK_P_PUSH_COL:
        if (op.col >= static_cast<uint32_t>(num_cols)) return "names a column >= num_cols";
        gives = (op.flags & HDK_P_FLAG_FP) ? PC_FP : PC_INT;
        break;
      case HDK_P_PUSH_INT:
      case HDK_P_PUSH_NULL_INT: gives = PC_INT; break;
      case HDK_P_PUSH_FP:
      case HDK_P_PUSH_NULL_FP: gives = PC_FP; break;
      case HDK_P_ADD_I:
      case HDK_P_SUB_I:
      case HDK_P_MUL_I:
        if (op.check_width != 0 && op.check_width != 1 && op.check_width != 2 && op.check_width != 4 && op.check_width != 8) {
          return "has a check_width that is not 0, 1, 2, 4 or 8";
        }
        chk->can_raise |= op.check_width != 0;
        pops = 2, want = PC_INT, gives = PC_INT;
        break;
      case HDK_P_DIV_I:
      case HDK_P_MOD_I:
        chk->can_raise = true;
        pops = 2, want = PC_INT, gives = PC_INT;
        break;
      case HDK_P_DIV_F: chk->can_raise = true; [[fallthrough]];
      case HDK_P_ADD_F:
      case HDK_P_SUB_F:
      case HDK_P_MUL_F: pops = 2, want = PC_FP, gives = PC_FP; break;
      case HDK_P_CAST_I2F: pops = 1, want = PC_INT, gives = PC_FP; break;
      case HDK_P_CAST_F2I: pops = 1, want = PC_FP, gives = PC_INT; break;
      case HDK_P_CMP_I:
      case HDK_P_CMP_F:
        if (op.flags < HDK_CMP_EQ || op.flags > HDK_CMP_GE) return "has a comparison outside hdk_hip_cmp";
        pops = 2, want = op.code == HDK_P_CMP_F ? PC_FP : PC_INT, gives = PC_BOOL;
        break;
      case HDK_P_AND:
      case HDK_P_OR: pops = 2, want = PC_BOOL, gives = PC_BOOL; break;
      case HDK_P_NOT: pops = 1, want = PC_BOOL, gives = PC_BOOL; break;
      case HDK_P_IS_NULL:
        if (depth < 1) return "underflows its stack";
        pops = 1, want = cls[depth - 1], gives = PC_BOOL;
        break;
      case HDK_P_SELECT:
        if (depth < 3) return "underflows its stack";
        if (cls[depth - 3] != PC_BOOL) return "has an operand of the wrong class (the condition of a SELECT is no BOOL)";
        if (cls[depth - 2] != cls[depth - 1]) return "has an operand of the wrong class (the branches of a SELECT differ)";
        gives = cls[depth - 1];
        depth -= 3;
        break;
      default: return "holds an unknown code";
    }
    if (depth < pops) return "underflows its stack";
    for (int k = 0; k < pops; ++k) {
      if (cls[depth - 1 - k] != want) return "has an operand of the wrong class";
    }
    depth -= pops;
    if (depth >= HDK_HIP_MAX_PROJECT_STACK) return "needs a stack deeper than HDK_HIP_MAX_PROJECT_STACK";
    cls[depth++] = gives;
    chk->max_depth = depth > chk->max_depth ? depth : chk->max_depth;
  }
  if (depth != 1) return "does not leave exactly one value (final stack depth != 1)";
  if (cls[0] == PC_BOOL) return "leaves a BOOL";
  if ((cls[0] == PC_FP) != out_fp) return "leaves a value whose class is not the out's is_fp";
  return nullptr;
}

}  // namespace hdk

using namespace hdk;

extern "C" int32_t hdk_hip_project_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                                           const hdk_hip_project_op* ops, int32_t num_ops, const hdk_hip_project_out* outs,
                                           int32_t num_outs, int64_t* out_cols, uint64_t out_capacity, int32_t* error_code_dev,
                                           int32_t device_id, void* stream) {
  HDK_REQUIRE(cols && ops && outs && out_cols,
              "hdk_hip_project_columns: NULL argument (cols, ops, outs and out_cols are required)");
  HDK_REQUIRE(num_cols >= 1, "hdk_hip_project_columns: num_cols %d", num_cols);
  HDK_REQUIRE(num_outs >= 1 && num_outs <= HDK_HIP_MAX_PROJECT_OUTS, "hdk_hip_project_columns: num_outs %d outside 1..%d", num_outs,
              HDK_HIP_MAX_PROJECT_OUTS);
  HDK_REQUIRE(num_ops >= 1 && num_ops <= HDK_HIP_MAX_PROJECT_OPS, "hdk_hip_project_columns: num_ops %d outside 1..%d", num_ops,
              HDK_HIP_MAX_PROJECT_OPS);
  PcDesc d;
  memset(&d, 0, sizeof(d));
  PcCheck chk;
  for (int32_t j = 0; j < num_outs; ++j) {
    const hdk_hip_project_out& o = outs[j];
    HDK_REQUIRE(o.first_op >= 0 && o.num_ops >= 1 && o.first_op <= num_ops - o.num_ops,
                "hdk_hip_project_columns: out %d owns ops [%d, %d + %d) of %d", j, o.first_op, o.first_op, o.num_ops, num_ops);
    const char* why = pc_check_program(ops + o.first_op, o.num_ops, num_cols, o.is_fp != 0, &chk);
    HDK_REQUIRE(!why, "hdk_hip_project_columns: malformed program of out %d: it %s", j, why);
    PcOut& q = d.out[j];
    q.first = static_cast<uint32_t>(o.first_op);
    q.count = static_cast<uint32_t>(o.num_ops);
    q.flags = o.num_ops == 1 && ops[o.first_op].code == HDK_P_PUSH_COL ? PC_OUT_PASS : 0u;
    q.null_bits = o.null_bits;
  }
  // the distinct input columns in order of first appearance; the ops name them by their place in that list
  for (int32_t i = 0; i < num_ops; ++i) {
    d.op[i] = ops[i];
    if (ops[i].code != HDK_P_PUSH_COL) continue;
    HDK_REQUIRE(ops[i].col < static_cast<uint32_t>(num_cols), "hdk_hip_project_columns: op %d names column %u of %d", i, ops[i].col,
                num_cols);
    uint32_t k = 0;
    while (k < d.nin && d.in_col[k] != ops[i].col) ++k;
    if (k == d.nin) {
      HDK_REQUIRE(d.nin < HDK_HIP_MAX_PROJECT_INPUTS, "hdk_hip_project_columns: more than %d distinct input columns",
                  HDK_HIP_MAX_PROJECT_INPUTS);
      d.in_col[d.nin++] = ops[i].col;
    }
    d.op[i].col = k;
  }
  d.nouts = static_cast<uint32_t>(num_outs);
  HDK_REQUIRE(num_rows < (uint64_t(1) << 32), "hdk_hip_project_columns: num_rows %llu does not fit 32-bit row indices",
              static_cast<unsigned long long>(num_rows));
  HDK_REQUIRE(num_rows <= capacity, "hdk_hip_project_columns: num_rows %llu exceeds the capacity %llu",
              static_cast<unsigned long long>(num_rows), static_cast<unsigned long long>(capacity));
  HDK_REQUIRE(num_rows <= out_capacity, "hdk_hip_project_columns: num_rows %llu exceeds the out_capacity %llu",
              static_cast<unsigned long long>(num_rows), static_cast<unsigned long long>(out_capacity));
  HDK_REQUIRE(error_code_dev || !chk.can_raise,
              "hdk_hip_project_columns: error_code_dev is NULL and a program can raise (a division, a modulo or a checked + - *)");
  {
    const MemBlock blk[] = {
        {"cols", reinterpret_cast<uintptr_t>(cols), static_cast<uint64_t>(num_cols) * capacity * 8},
        {"out_cols", reinterpret_cast<uintptr_t>(out_cols), static_cast<uint64_t>(num_outs) * out_capacity * 8},
        {"error_code_dev", reinterpret_cast<uintptr_t>(error_code_dev), error_code_dev ? 4u : 0u},
    };
    const int32_t bad = require_disjoint("hdk_hip_project_columns", blk, sizeof(blk) / sizeof(blk[0]));
    if (bad) return bad;
  }
  hipStream_t s;
  const int32_t st = device_enter(device_id, stream, &s);
  if (st) return st;
  if (error_code_dev) {
    HDK_HIP_CHECK(hipMemsetAsync(error_code_dev, 0, sizeof(int32_t), s));
  }
  if (num_rows == 0) {
    return HDK_HIP_OK;
  }
  const uint32_t n = static_cast<uint32_t>(num_rows);
  const uint32_t ntiles = static_cast<uint32_t>((num_rows + kPcTile - 1) / kPcTile);
  const dim3 grid(persistent_grid(device_props(device_id), ntiles)), block(kPcBlock);
  if (chk.max_depth <= 2 && d.nin <= 2) {
    hipLaunchKernelGGL((hdk_project_rows<2, 2>), grid, block, 0, s, cols, capacity, n, d, ntiles, out_cols, out_capacity,
                       error_code_dev);
  } else if (chk.max_depth <= 4 && d.nin <= 4) {
    hipLaunchKernelGGL((hdk_project_rows<4, 4>), grid, block, 0, s, cols, capacity, n, d, ntiles, out_cols, out_capacity,
                       error_code_dev);
  } else {
    hipLaunchKernelGGL((hdk_project_rows<HDK_HIP_MAX_PROJECT_STACK, HDK_HIP_MAX_PROJECT_INPUTS>), grid, block, 0, s, cols, capacity,
                       n, d, ntiles, out_cols, out_capacity, error_code_dev);
  }
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
