// result_columns.hip -- a group-by buffer in HBM -> dense 8-byte columns in HBM.
//
// Device form of ColumnarResults::materializeAllColumnsGroupBy (omniscidb/ResultSetRegistry/ColumnarResults.cpp:691-1010),
// which the reference runs on the host in two stages: locateAndCountEntries (which entries are non-empty, how many come
// before each) and compactAndCopyEntries (one dense column per target, entry order kept).  Values are what ResultSet
// iteration returns: slots sign-extended from their width, a float accumulator read from the low 4 bytes of its slot
// and widened, AVG through pair_to_double (omniscidb/ResultSet/ResultSetBufferAccessors.h:168-190).  Emptiness is
// ResultSetStorage::isEmptyEntry[Columnar] (RS/ResultSetStorage.cpp:439-521; group_buffer.h).
//
// Three launches on one stream, ordered by nothing but the stream (no block ever waits for another block):
//   hdk_result_count    persistent grid over tiles of kRcTile entries: non-empty entries per tile -> workspace
//   hdk_counts_scan<4>  one block (column_scan.hip): exclusive scan of the tile counts in place, the total -> *row_count
//   hdk_result_compact  per tile: flags again, rank = tile offset + ballot/mbcnt rank, every column written at its rank;
//                       tiles without a group are skipped unread (a sparse perfect-hash table costs one pass, not two)
// The host decodes the plan once into a POD (RcDesc) that travels as a kernel argument: the entry loops read it from
// scalar registers and never touch the plan.  Traffic: row-wise, the table twice plus the output; columnar, the first
// key column (or the keyless slot column) plus the table plus the output.
#include <string.h>

#include "column_primitives.h"
#include "group_buffer.h"
#include "host_common.h"
#include "result_value.h"

namespace hdk {

constexpr int kRcBlock = kTileBlock;
constexpr int kRcItems = 16;  // entries per thread and tile
constexpr uint32_t kRcTile = kRcBlock * kRcItems;
constexpr int kRcWaves = kRcBlock / kWave;
constexpr int kRcParts = kRcItems * kRcWaves;  // (item, wave) partial counts of a tile, in entry order
static_assert(kRcParts == kWave, "one wave scans the partial counts of a tile");
constexpr ScanPer kRcScanPer = SCAN_PER_4;  // tile counts per thread and trip of the scan

struct RcCol {
  uint64_t off, off2;  // bytes from the buffer start (row-wise: inside the row) of the slot / of AVG's count slot
  uint32_t stride, stride2;
  uint32_t width, width2;
  uint32_t op;
  uint32_t pad_;
};

struct RcDesc {
  EmptyProbe probe;
  uint32_t ncols;
  uint32_t pad_;
  RcCol col[HDK_HIP_MAX_TARGETS];
};

// the `width` bytes at byte `off` of a 16-byte row held in registers, sign-extended (a slot never straddles a quad)
HDK_DEV int64_t row16_word(const bf_i64x2& v, uint32_t off, uint32_t width) {
  const uint64_t q = static_cast<uint64_t>(off >= 8 ? v.y : v.x) >> ((off & 7u) * 8u);
  const uint32_t drop = 64u - 8u * width;
  return static_cast<int64_t>(q << drop) >> drop;
}

// Entry e of a tile belongs to thread e % kRcBlock, item e / kRcBlock: consecutive lanes read consecutive entries.
// (tile * kRcTile + 4095 never exceeds 2^32 - 1: tile < ceil(entry_count / kRcTile), entry_count < 2^32.)
template <bool ROW16>
__global__ __launch_bounds__(kRcBlock) void hdk_result_count(const int8_t* __restrict__ buf, uint32_t entry_count,
                                                              EmptyProbe probe, uint32_t ntiles,
                                                              uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t s_wave[kRcWaves];
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t e0 = tile * kRcTile + threadIdx.x;
    int64_t word[kRcItems];
#pragma unroll
    for (int j = 0; j < kRcItems; ++j) {
      // (an entry past the end reads the last entry instead, so that the loads of a tile are issued together)
      const uint32_t e = e0 + static_cast<uint32_t>(j) * kRcBlock;
      const size_t ec = e < entry_count ? e : entry_count - 1;
      if (ROW16) {
        word[j] = row16_word(nt_load<bf_i64x2>(buf, ec * 16), static_cast<uint32_t>(probe.base), probe.width);
      } else {
        word[j] = rc_load_sext(buf, probe.base + ec * probe.stride, probe.width);
      }
    }
    uint32_t n = 0;  // of this wave
#pragma unroll
    for (int j = 0; j < kRcItems; ++j) {
      const uint32_t e = e0 + static_cast<uint32_t>(j) * kRcBlock;
      n += static_cast<uint32_t>(__popcll(__builtin_amdgcn_ballot_w64(e < entry_count && word[j] != probe.empty)));
    }
    block_store_tile_count(s_wave, n, tile_counts + tile);
  }
}

template <bool ROW16>
__global__ __launch_bounds__(kRcBlock) void hdk_result_compact(const int8_t* __restrict__ buf, uint32_t entry_count,
                                                                RcDesc d, uint32_t ntiles,
                                                                const uint32_t* __restrict__ tile_offs,
                                                                int64_t* __restrict__ out, uint64_t capacity) {
  // two arrays: a wave may still read this tile's bases while another already writes the next tile's counts
  __shared__ uint32_t s_cnt[kRcParts], s_base[kRcParts];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t first = tile_offs[tile];
    if (tile_offs[tile + 1] == first || first >= capacity) {
      continue;  // no group in this tile, or all of them past the capacity (block-uniform)
    }
    const uint32_t e0 = tile * kRcTile + threadIdx.x;
    bf_i64x2 row[ROW16 ? kRcItems : 1];
    int64_t word[kRcItems];
#pragma unroll
    for (int j = 0; j < kRcItems; ++j) {
      const uint32_t e = e0 + static_cast<uint32_t>(j) * kRcBlock;
      const size_t ec = e < entry_count ? e : entry_count - 1;
      if (ROW16) {
        row[j] = nt_load<bf_i64x2>(buf, ec * 16);
        word[j] = row16_word(row[j], static_cast<uint32_t>(d.probe.base), d.probe.width);
      } else {
        word[j] = rc_load_sext(buf, d.probe.base + ec * d.probe.stride, d.probe.width);
      }
    }
    uint32_t flags = 0;
#pragma unroll
    for (int j = 0; j < kRcItems; ++j) {
      const uint32_t e = e0 + static_cast<uint32_t>(j) * kRcBlock;
      const bool f = e < entry_count && word[j] != d.probe.empty;
      const uint64_t mask = __builtin_amdgcn_ballot_w64(f);
      if (lane == 0) {
        s_cnt[j * kRcWaves + wave] = static_cast<uint32_t>(__popcll(mask));
      }
      flags |= static_cast<uint32_t>(f) << j;
    }
    __syncthreads();
    if (wave == 0) {  // exclusive scan of the kRcParts partial counts, which lie in entry order
      const uint32_t c = s_cnt[lane];
      s_base[lane] = wave_inclusive_sum(c, lane) - c;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRcItems; ++j) {
      const bool f = (flags >> j) & 1u;
      const uint64_t mask = __builtin_amdgcn_ballot_w64(f);
      const uint64_t r = static_cast<uint64_t>(first) + s_base[j * kRcWaves + wave] + lane_rank(mask);
      if (!f || r >= capacity) {
        continue;
      }
      const size_t e = e0 + static_cast<uint32_t>(j) * kRcBlock;
#pragma unroll
      for (int t = 0; t < HDK_HIP_MAX_TARGETS; ++t) {
        if (static_cast<uint32_t>(t) >= d.ncols) {
          break;
        }
        const RcCol& c = d.col[t];
        int64_t a, b = 1;
        if (ROW16) {
          a = row16_word(row[j], static_cast<uint32_t>(c.off), c.width);
          if (c.op >= RC_AVG_INT) b = row16_word(row[j], static_cast<uint32_t>(c.off2), c.width2);
        } else {
          a = rc_load_sext(buf, c.off + e * c.stride, c.width);
          if (c.op >= RC_AVG_INT) b = rc_load_sext(buf, c.off2 + e * c.stride2, c.width2);
        }
        out[static_cast<size_t>(t) * capacity + r] = rc_value(c.op, a, b);
      }
    }
  }
}

int32_t validate_plan_layout(const hdk_hip_plan* p);  // scan_agg.hip: the layout half of the plan check

static size_t rc_tiles(uint32_t entry_count) { return (static_cast<size_t>(entry_count) + kRcTile - 1) / kRcTile; }

// the plan, decoded for a buffer of `entry_count` entries (which may differ from the plan's)
static void rc_desc_of(const hdk_hip_plan* p, uint32_t entry_count, const int64_t* init_vals, RcDesc* d) {
  memset(d, 0, sizeof(*d));
  d->probe = empty_probe_of(p, entry_count, init_vals);
  d->ncols = static_cast<uint32_t>(p->num_targets);
  const uint32_t row_bytes = p->row_size_quad * 8u;
  int s = 0;
  for (int t = 0; t < p->num_targets; ++t) {
    const hdk_hip_target& tg = p->targets[t];
    RcCol& c = d->col[t];
    if (tg.slot_width == 0) {
      // a projected key without a slot: key column key_idx (target_groupby_indices)
      if (p->output_columnar) {
        c.off = static_cast<uint64_t>(tg.key_idx) * align8(static_cast<size_t>(entry_count) * 8);
        c.stride = 8;
        c.width = 8;
      } else {
        c.off = static_cast<uint64_t>(tg.key_idx) * static_cast<uint32_t>(p->key_width);
        c.stride = row_bytes;
        c.width = static_cast<uint32_t>(p->key_width);
      }
    } else if (p->output_columnar) {
      c.off = columnar_slot_off(p, entry_count, s);
      c.stride = c.width = static_cast<uint32_t>(tg.slot_width);
    } else {
      c.off = static_cast<uint64_t>(tg.slot_off);
      c.stride = row_bytes;
      c.width = static_cast<uint32_t>(tg.slot_width);
    }
    c.op = rc_op_of(tg);
    if (tg.agg == HDK_AGG_AVG) {
      c.width2 = static_cast<uint32_t>(tg.slot2_width);
      if (p->output_columnar) {
        c.off2 = columnar_slot_off(p, entry_count, s + 1);
        c.stride2 = c.width2;
      } else {
        c.off2 = static_cast<uint64_t>(tg.slot2_off);
        c.stride2 = row_bytes;
      }
    }
    s += tg.agg == HDK_AGG_AVG ? 2 : 1;
  }
}

}  // namespace hdk

using namespace hdk;

extern "C" size_t hdk_hip_result_columns_workspace_bytes(uint32_t entry_count) {
  return align256((rc_tiles(entry_count) + 1) * sizeof(uint32_t));
}

extern "C" int32_t hdk_hip_columnarize_result(const hdk_hip_plan* plan, const int64_t* buf, uint32_t entry_count,
                                              const int64_t* init_vals, int64_t* out_cols, uint64_t capacity,
                                              uint64_t* row_count, void* workspace, size_t workspace_bytes,
                                              int32_t device_id, void* stream) {
  int32_t st = validate_plan_layout(plan);
  if (st) return st;
  if (plan->query_kind != HDK_Q_PERFECT_HASH && plan->query_kind != HDK_Q_BASELINE_HASH) {
    set_error("hdk_hip_columnarize_result takes group-by buffers (perfect or baseline hash); a %s result stays on the host path",
              plan->query_kind == HDK_Q_PROJECTION ? "projection" : "non-grouped");
    return HDK_HIP_ERR_UNSUPPORTED;
  }
  HDK_REQUIRE(buf && init_vals, "NULL argument");
  HDK_REQUIRE(row_count, "row_count is NULL");
  const size_t need = hdk_hip_result_columns_workspace_bytes(entry_count);
  HDK_REQUIRE(!workspace || workspace_bytes >= need, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t s;
  st = device_enter(device_id, stream, &s);
  if (st) return st;
  RcDesc d;
  rc_desc_of(plan, entry_count, init_vals, &d);
  AsyncScratch mem(s);
  st = acquire_workspace(mem, &workspace, need);
  if (st) return st;
  uint32_t* tiles = static_cast<uint32_t*>(workspace);
  const uint32_t ntiles = static_cast<uint32_t>(rc_tiles(entry_count));
  const int8_t* table = reinterpret_cast<const int8_t*>(buf);
  const bool row16 = !plan->output_columnar && plan->row_size_quad == 2 && reinterpret_cast<uintptr_t>(buf) % 16 == 0;
  const dim3 grid(persistent_grid(device_props(device_id), ntiles)), block(kRcBlock);
  if (ntiles) {
    if (row16) {
      hipLaunchKernelGGL(hdk_result_count<true>, grid, block, 0, s, table, entry_count, d.probe, ntiles, tiles);
    } else {
      hipLaunchKernelGGL(hdk_result_count<false>, grid, block, 0, s, table, entry_count, d.probe, ntiles, tiles);
    }
  }
  launch_counts_scan(tiles, ntiles, kRcScanPer, row_count, s);
  if (ntiles && out_cols && capacity) {
    if (row16) {
      hipLaunchKernelGGL(hdk_result_compact<true>, grid, block, 0, s, table, entry_count, d, ntiles, tiles, out_cols, capacity);
    } else {
      hipLaunchKernelGGL(hdk_result_compact<false>, grid, block, 0, s, table, entry_count, d, ntiles, tiles, out_cols, capacity);
    }
  }
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
