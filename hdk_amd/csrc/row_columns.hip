// row_columns.hip -- a projection buffer or a non-grouped result in HBM -> dense 8-byte columns in HBM.
//
// Device form of ColumnarResults::materializeAllColumnsProjection with copyAllNonLazyColumns / materializeAllColumnsDirectly
// (omniscidb/ResultSetRegistry/ColumnarResults.cpp:520-620), which the reference runs on the host over a copy of the whole
// buffer.  The sibling of result_columns.hip for the other half of the scan path: a projection buffer has no empty
// entries -- its first min(TOTAL_MATCHED, entry_count) rows are the result, in ResultSet iteration order -- so there is
// nothing to count, scan or rank.  One launch, a pure byte mover:
//   hdk_rows_row16      row-wise, one target (16-byte rows): one 16-byte load per lane and row, kept in registers
//   hdk_rows_lds<W>     row-wise, W = 3 .. 9 words per row, staged through LDS: coalesced 16-byte loads, read back transposed
//   hdk_rows_walk<W>    the same rows in a buffer that is not 16-byte aligned: each lane walks its own rows word by word
//   hdk_rows_columnar   columnar: (tile, column) pairs; a narrow column is read in aligned 8-byte groups and sign-extended
//   hdk_rows_scalars    a non-grouped result: one wave, one value per target (result_value.h)
// Every block reads TOTAL_MATCHED itself (the host never waits for it), one thread of block 0 writes *row_count, and tiles
// at or beyond min(rows, capacity) are not read.  All buffer loads are non-temporal and all byte offsets 64-bit.
// Traffic: the consumed rows once plus 8 x rows x (targets [+ positions]) written.
#include <string.h>

#include "host_common.h"
#include "result_value.h"
#include "switches.h"

namespace hdk {

constexpr int kRwBlock = kTileBlock;
constexpr int kRwItems = 16;  // rows per thread and tile
constexpr uint32_t kRwTile = kRwBlock * kRwItems;
constexpr int kRwMaxWords = HDK_HIP_MAX_TARGETS + 1;  // words of a row-wise row / columns of a columnar buffer, positions included

// rows of the result that this call materialises: min(min(max(*total_matched, 0), entry_count), capacity); the true count
// goes to *row_count (one thread of block 0)
HDK_DEV uint64_t rw_rows(const int32_t* __restrict__ total_matched, uint32_t entry_count, uint64_t capacity,
                         uint64_t* __restrict__ row_count) {
  const int32_t tm = *total_matched;
  const uint32_t rows = tm <= 0 ? 0u : (static_cast<uint32_t>(tm) < entry_count ? static_cast<uint32_t>(tm) : entry_count);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *row_count = rows;
  }
  return rows < capacity ? rows : capacity;
}

// Row r of a tile belongs to thread r % kRwBlock, item r / kRwBlock: consecutive lanes take consecutive rows, so every
// store instruction of a wave covers 512 contiguous bytes of one output column.
__global__ __launch_bounds__(kRwBlock) void hdk_rows_row16(const int8_t* __restrict__ buf, uint32_t entry_count,
                                                           const int32_t* __restrict__ total_matched,
                                                           int64_t* __restrict__ out, uint64_t capacity,
                                                           int64_t* __restrict__ pos_out, uint64_t* __restrict__ row_count) {
  const uint64_t n = rw_rows(total_matched, entry_count, capacity, row_count);
  for (uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * kRwTile; r0 < n; r0 += static_cast<uint64_t>(gridDim.x) * kRwTile) {
    bf_i64x2 row[kRwItems];
#pragma unroll
    for (int j = 0; j < kRwItems; ++j) {
      // (a row past the end reads the last row instead, so that the loads of a tile are issued together)
      const uint64_t r = r0 + threadIdx.x + static_cast<uint32_t>(j) * kRwBlock;
      row[j] = nt_load<bf_i64x2>(buf, (r < n ? r : n - 1) * 16);
    }
#pragma unroll
    for (int j = 0; j < kRwItems; ++j) {
      const uint64_t r = r0 + threadIdx.x + static_cast<uint32_t>(j) * kRwBlock;
      if (r < n) {
        if (pos_out) pos_out[r] = row[j].x;
        out[r] = row[j].y;
      }
    }
  }
}

// word w of row r goes to pos_out (w == 0, when asked for) or to column w - 1
template <int W>
HDK_DEV void rw_store_row(const int64_t (&v)[W], uint64_t r, int64_t* __restrict__ out, uint64_t capacity,
                          int64_t* __restrict__ pos_out) {
  if (pos_out) pos_out[r] = v[0];
#pragma unroll
  for (int w = 1; w < W; ++w) {
    out[static_cast<uint64_t>(w - 1) * capacity + r] = v[w];
  }
}

constexpr int kRwWalkBatch = 4;  // rows a lane has in flight (4 x W loads)

// rows [r0, r0 + count * kRwBlock) of which those below n exist: each lane walks its rows, kRwWalkBatch at a time
template <int W>
HDK_DEV void rw_walk(const int8_t* __restrict__ buf, uint64_t r0, int count, uint64_t n, int64_t* __restrict__ out,
                     uint64_t capacity, int64_t* __restrict__ pos_out) {
  for (int j0 = 0; j0 < count; j0 += kRwWalkBatch) {
    int64_t v[kRwWalkBatch][W];
#pragma unroll
    for (int j = 0; j < kRwWalkBatch; ++j) {
      const uint64_t r = r0 + threadIdx.x + static_cast<uint32_t>(j0 + j) * kRwBlock;
      const uint64_t rc = r < n ? r : n - 1;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        v[j][w] = nt_load<int64_t>(buf, (rc * W + w) * 8);
      }
    }
#pragma unroll
    for (int j = 0; j < kRwWalkBatch; ++j) {
      const uint64_t r = r0 + threadIdx.x + static_cast<uint32_t>(j0 + j) * kRwBlock;
      if (r < n && j0 + j < count) {
        rw_store_row<W>(v[j], r, out, capacity, pos_out);
      }
    }
  }
}

template <int W>
__global__ __launch_bounds__(kRwBlock) void hdk_rows_walk(const int8_t* __restrict__ buf, uint32_t entry_count,
                                                          const int32_t* __restrict__ total_matched,
                                                          int64_t* __restrict__ out, uint64_t capacity,
                                                          int64_t* __restrict__ pos_out, uint64_t* __restrict__ row_count) {
  const uint64_t n = rw_rows(total_matched, entry_count, capacity, row_count);
  for (uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * kRwTile; r0 < n; r0 += static_cast<uint64_t>(gridDim.x) * kRwTile) {
    rw_walk<W>(buf, r0, kRwItems, n, out, capacity, pos_out);
  }
}

// LDS pitch of a staged row in 8-byte words: odd, so that the rows of 32 consecutive lanes start in 32 different 8-byte
// bank pairs (ds_read_b64 banks by (address / 4) % 64, i.e. by word % 32, within a 32-lane half; pitch x lane % 32 is a
// permutation of 0 .. 31 exactly when the pitch is odd).  Even W pays one padding word per row.
constexpr int rw_pitch(int w) { return w | 1; }

// A tile goes through LDS in kRwItems steps of kRwBlock rows: the step's rows are one contiguous, 16-byte aligned range
// of 128 x W 16-byte chunks, loaded chunk c by thread c % kRwBlock (coalesced) and stored at the pitch; then thread i reads
// row i back.  A step that is not full (the ragged end) is walked instead: its last chunk could reach past the buffer.
template <int W>
__global__ __launch_bounds__(kRwBlock) void hdk_rows_lds(const int8_t* __restrict__ buf, uint32_t entry_count,
                                                         const int32_t* __restrict__ total_matched,
                                                         int64_t* __restrict__ out, uint64_t capacity,
                                                         int64_t* __restrict__ pos_out, uint64_t* __restrict__ row_count) {
  constexpr int P = rw_pitch(W);
  constexpr int kChunks = kRwBlock * W / 2;                       // 16-byte chunks of a step
  constexpr int kTrips = (kChunks + kRwBlock - 1) / kRwBlock;     // chunks per thread
  __shared__ int64_t s_rows[kRwBlock * P];
  const uint64_t n = rw_rows(total_matched, entry_count, capacity, row_count);
  for (uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kRwTile; t0 < n; t0 += static_cast<uint64_t>(gridDim.x) * kRwTile) {
    for (int step = 0; step < kRwItems; ++step) {
      const uint64_t r0 = t0 + static_cast<uint32_t>(step) * kRwBlock;
      if (r0 >= n) {
        break;  // (block-uniform, as is the branch below)
      }
      if (r0 + kRwBlock > n) {
        rw_walk<W>(buf, r0, 1, n, out, capacity, pos_out);
        break;
      }
      bf_i64x2 c[kTrips];
#pragma unroll
      for (int k = 0; k < kTrips; ++k) {
        const uint32_t ch = threadIdx.x + static_cast<uint32_t>(k) * kRwBlock;
        c[k] = nt_load<bf_i64x2>(buf, r0 * (W * 8) + static_cast<uint64_t>(ch < kChunks ? ch : kChunks - 1) * 16);
      }
#pragma unroll
      for (int k = 0; k < kTrips; ++k) {
        const uint32_t ch = threadIdx.x + static_cast<uint32_t>(k) * kRwBlock;
        if (ch < kChunks) {
          const uint32_t g = 2 * ch;  // word of the step: row g / W, word g % W
          s_rows[(g / W) * P + g % W] = c[k].x;
          s_rows[((g + 1) / W) * P + (g + 1) % W] = c[k].y;
        }
      }
      __syncthreads();
      int64_t v[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        v[w] = s_rows[threadIdx.x * P + w];
      }
      rw_store_row<W>(v, r0 + threadIdx.x, out, capacity, pos_out);
      __syncthreads();  // the next step overwrites the rows
    }
  }
}

struct RwColumnar {
  uint64_t off[kRwMaxWords];    // bytes from the buffer start; columns [0, ncols) are the targets, then the positions
  uint32_t width[kRwMaxWords];  // 1 / 2 / 4 / 8
  uint32_t ncols;               // targets
  uint32_t npairs;              // columns per tile: ncols, + 1 when the positions are asked for
};

// the V = 8 / WIDTH values of an aligned 8-byte group, value `sub` sign-extended
template <int WIDTH>
HDK_DEV int64_t rw_group_value(int64_t group, uint32_t sub) {
  if (WIDTH == 8) {
    return group;
  }
  const uint64_t q = static_cast<uint64_t>(group) >> (sub * (8u * WIDTH));
  constexpr uint32_t drop = 64u - 8u * WIDTH;
  return static_cast<int64_t>(q << drop) >> drop;
}

// One full tile of one column.  A wave owns 64 x V consecutive values per trip: lane l loads their l-th 8-byte group, and
// store s of the trip covers values [64 s, 64 s + 64) of them -- 512 contiguous bytes of the output -- which lie in the
// groups of lanes [64 s / V, 64 (s + 1) / V): lane l takes value l % V of the group of lane 64 s / V + l / V.
template <int WIDTH>
HDK_DEV void rw_column_tile(const int8_t* __restrict__ col, uint64_t r0, int64_t* __restrict__ dst) {
  constexpr int V = 8 / WIDTH;                       // values per group
  constexpr int kTrips = kRwItems / V;               // groups per thread and tile
  constexpr uint32_t kWaveVals = kWave * V;          // values of a wave per trip
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int64_t g[kTrips];
#pragma unroll
  for (int k = 0; k < kTrips; ++k) {
    const uint64_t first = r0 + (static_cast<uint32_t>(k) * (kRwBlock / kWave) + wave) * kWaveVals;
    g[k] = nt_load<int64_t>(col, first * WIDTH + lane * 8);
  }
#pragma unroll
  for (int k = 0; k < kTrips; ++k) {
    const uint64_t first = r0 + (static_cast<uint32_t>(k) * (kRwBlock / kWave) + wave) * kWaveVals;
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const int64_t grp = V == 1 ? g[k] : __shfl(g[k], static_cast<int>(s * (kWave / V) + lane / V), kWave);
      dst[first + static_cast<uint32_t>(s) * kWave + lane] = rw_group_value<WIDTH>(grp, lane % V);
    }
  }
}

__global__ __launch_bounds__(kRwBlock) void hdk_rows_columnar(const int8_t* __restrict__ buf, uint32_t entry_count,
                                                              const int32_t* __restrict__ total_matched, RwColumnar d,
                                                              int64_t* __restrict__ out, uint64_t capacity,
                                                              int64_t* __restrict__ pos_out, uint64_t* __restrict__ row_count) {
  const uint64_t n = rw_rows(total_matched, entry_count, capacity, row_count);
  const uint64_t ntiles = (n + kRwTile - 1) / kRwTile;
  for (uint64_t pair = blockIdx.x; pair < ntiles * d.npairs; pair += gridDim.x) {
    const uint64_t r0 = pair / d.npairs * kRwTile;
    const uint32_t c = static_cast<uint32_t>(pair % d.npairs);
    uint64_t off = 0;
    uint32_t width = 8;
#pragma unroll
    for (int t = 0; t < kRwMaxWords; ++t) {  // (a constant index: the descriptor stays in scalar registers)
      if (static_cast<uint32_t>(t) == c) {
        off = d.off[t];
        width = d.width[t];
      }
    }
    const int8_t* col = buf + off;
    int64_t* dst = c < d.ncols ? out + static_cast<uint64_t>(c) * capacity : pos_out;
    if (r0 + kRwTile <= n) {
      switch (width) {
        case 1:
          rw_column_tile<1>(col, r0, dst);
          break;
        case 2:
          rw_column_tile<2>(col, r0, dst);
          break;
        case 4:
          rw_column_tile<4>(col, r0, dst);
          break;
        default:
          rw_column_tile<8>(col, r0, dst);
          break;
      }
    } else {  // the ragged last tile, per value
#pragma unroll 4
      for (int j = 0; j < kRwItems; ++j) {
        const uint64_t r = r0 + threadIdx.x + static_cast<uint32_t>(j) * kRwBlock;
        if (r < n) {
          dst[r] = rc_load_sext(col, r * width, width);
        }
      }
    }
  }
}

struct RwScalars {
  uint32_t ncols;
  uint32_t op[HDK_HIP_MAX_TARGETS];
  uint32_t slot[HDK_HIP_MAX_TARGETS];  // the target's first slot; AVG's count is the next one
};

// a non-grouped result: slot i at buf + i (QueryExecutionContext.cpp:452-458's out_vec), lane t makes target t's value
__global__ __launch_bounds__(kWave) void hdk_rows_scalars(const int64_t* __restrict__ buf, RwScalars d, int64_t* __restrict__ out,
                                                          uint64_t capacity, uint64_t* __restrict__ row_count) {
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    *row_count = 1;
  }
  if (!out || capacity == 0) {
    return;
  }
  uint32_t op = RC_COPY, slot = 0;
#pragma unroll
  for (int k = 0; k < HDK_HIP_MAX_TARGETS; ++k) {
    if (static_cast<uint32_t>(k) == t) {
      op = d.op[k];
      slot = d.slot[k];
    }
  }
  if (t < d.ncols) {
    const int64_t a = nt_load<int64_t>(buf, static_cast<size_t>(slot) * 8);
    const int64_t b = op >= RC_AVG_INT ? nt_load<int64_t>(buf, static_cast<size_t>(slot + 1) * 8) : 1;
    out[static_cast<uint64_t>(t) * capacity] = rc_value(op, a, b);
  }
}

int32_t validate_plan_layout(const hdk_hip_plan* p);  // scan_agg.hip: the layout half of the plan check

typedef void (*RwRowKernel)(const int8_t*, uint32_t, const int32_t*, int64_t*, uint64_t, int64_t*, uint64_t*);

template <int W>
static RwRowKernel rw_row_kernel_of(bool lds) {
  return lds ? hdk_rows_lds<W> : hdk_rows_walk<W>;
}

// Measured per row width: the staged form wins at every width from 3 words on (by 14 % at 3 words on the
// scan's own buffer, by 20 - 30 % from 7), so it is taken wherever its 16-byte loads are aligned; the walk stays for a
// buffer that is not, and for the ragged end.  HDK_HIP_ROWS_VARIANT=walk / lds forces one of the two (A/B measurements).
static RwRowKernel rw_row_kernel(uint32_t words, bool aligned16) {
  const char* sw = hdk_sw(SW_ROWS_VARIANT);
  bool lds = words >= 3;
  if (sw && !strcmp(sw, "walk")) lds = false;
  if (sw && !strcmp(sw, "lds")) lds = true;
  lds = lds && aligned16;  // (the staged form loads 16 bytes at a time)
  switch (words) {
    case 2:
      return hdk_rows_walk<2>;  // (a 16-byte row in a buffer that is not 16-byte aligned)
    case 3:
      return rw_row_kernel_of<3>(lds);
    case 4:
      return rw_row_kernel_of<4>(lds);
    case 5:
      return rw_row_kernel_of<5>(lds);
    case 6:
      return rw_row_kernel_of<6>(lds);
    case 7:
      return rw_row_kernel_of<7>(lds);
    case 8:
      return rw_row_kernel_of<8>(lds);
    default:
      return rw_row_kernel_of<9>(lds);
  }
}

}  // namespace hdk

using namespace hdk;

extern "C" int32_t hdk_hip_columnarize_rows(const hdk_hip_plan* plan, const int64_t* buf, uint32_t entry_count,
                                            const int32_t* total_matched, int64_t* out_cols, uint64_t capacity,
                                            int64_t* pos_out, uint64_t* row_count, int32_t device_id, void* stream) {
  int32_t st = validate_plan_layout(plan);
  if (st) return st;
  if (plan->query_kind != HDK_Q_PROJECTION && plan->query_kind != HDK_Q_NON_GROUPED) {
    set_error("hdk_hip_columnarize_rows takes projection buffers and non-grouped results; a group-by buffer goes through "
              "hdk_hip_columnarize_result");
    return HDK_HIP_ERR_UNSUPPORTED;
  }
  HDK_REQUIRE(buf, "buf is NULL");
  HDK_REQUIRE(row_count, "row_count is NULL");
  HDK_REQUIRE(reinterpret_cast<uintptr_t>(buf) % 8 == 0 && reinterpret_cast<uintptr_t>(out_cols) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(pos_out) % 8 == 0,
              "buf, out_cols and pos_out must be 8-byte aligned");
  const int nt = plan->num_targets;
  HDK_REQUIRE(nt >= 1 && nt <= HDK_HIP_MAX_TARGETS, "num_targets %d outside 1 .. %d", nt, HDK_HIP_MAX_TARGETS);
  if (!out_cols) {
    capacity = 0;  // count only: pos_out is not written either
  }
  hipStream_t s;
  if (plan->query_kind == HDK_Q_NON_GROUPED) {
    HDK_REQUIRE(entry_count == 1, "entry_count %u: a non-grouped result has one row", entry_count);
    HDK_REQUIRE(!pos_out, "pos_out: a non-grouped result has no row positions");
    RwScalars d;
    memset(&d, 0, sizeof(d));
    d.ncols = static_cast<uint32_t>(nt);
    uint32_t slot = 0;
    for (int t = 0; t < nt; ++t) {
      const hdk_hip_target& tg = plan->targets[t];
      HDK_REQUIRE(tg.slot_width == 8 && (tg.agg != HDK_AGG_AVG || tg.slot2_width == 8),
                  "target %d: a non-grouped result has 8-byte slots", t);
      d.op[t] = rc_op_of(tg);
      d.slot[t] = slot;
      slot += tg.agg == HDK_AGG_AVG ? 2 : 1;
    }
    st = device_enter(device_id, stream, &s);
    if (st) return st;
    hipLaunchKernelGGL(hdk_rows_scalars, dim3(1), dim3(kWave), 0, s, buf, d, out_cols, capacity, row_count);
    HDK_HIP_CHECK(hipGetLastError());
    return HDK_HIP_OK;
  }
  HDK_REQUIRE(total_matched, "total_matched is NULL");
  HDK_REQUIRE(entry_count < (1u << 31), "entry_count %u: a projection holds fewer than 2^31 rows", entry_count);
  st = device_enter(device_id, stream, &s);
  if (st) return st;
  const int8_t* table = reinterpret_cast<const int8_t*>(buf);
  const uint64_t bound = entry_count < capacity ? entry_count : capacity;  // rows this call can write
  const uint64_t ntiles = (bound + kRwTile - 1) / kRwTile;
  const dim3 block(kRwBlock);
  if (plan->output_columnar) {
    RwColumnar d;
    memset(&d, 0, sizeof(d));
    d.ncols = static_cast<uint32_t>(nt);
    d.npairs = d.ncols + (pos_out ? 1u : 0u);
    for (int t = 0; t < nt; ++t) {
      const int32_t w = plan->targets[t].slot_width;
      HDK_REQUIRE(plan->targets[t].agg == HDK_AGG_ID && (w == 1 || w == 2 || w == 4 || w == 8),
                  "target %d: a projection's slot is 1, 2, 4 or 8 bytes wide, not %d", t, w);
      d.off[t] = columnar_slot_off(plan, entry_count, t);
      d.width[t] = static_cast<uint32_t>(w);
    }
    d.off[nt] = 0;  // the positions
    d.width[nt] = 8;
    const unsigned grid = persistent_grid(device_props(device_id), ntiles * d.npairs);
    hipLaunchKernelGGL(hdk_rows_columnar, dim3(grid ? grid : 1), block, 0, s, table, entry_count, total_matched, d, out_cols,
                       capacity, pos_out, row_count);
  } else {
    const uint32_t words = plan->row_size_quad;
    HDK_REQUIRE(words == static_cast<uint32_t>(nt) + 1, "row_size_quad %u: a projection row is its position and %d 8-byte slots",
                words, nt);
    for (int t = 0; t < nt; ++t) {
      HDK_REQUIRE(plan->targets[t].agg == HDK_AGG_ID && plan->targets[t].slot_width == 8 && plan->targets[t].slot_off == 8 * (t + 1),
                  "target %d: a row-wise projection keeps target t in word t + 1 of the row", t);
    }
    const bool aligned16 = reinterpret_cast<uintptr_t>(buf) % 16 == 0;
    const unsigned grid = persistent_grid(device_props(device_id), ntiles);
    RwRowKernel k = words == 2 && aligned16 ? hdk_rows_row16 : rw_row_kernel(words, aligned16);
    hipLaunchKernelGGL(k, dim3(grid ? grid : 1), block, 0, s, table, entry_count, total_matched, out_cols, capacity, pos_out,
                       row_count);
  }
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
