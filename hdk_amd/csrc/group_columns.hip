// group_columns.hip -- GROUP BY over dense 8-byte result columns in HBM: one output row per run of adjacent rows with
// bit-equal key words, the aggregates a segmented reduction over the run.
//
// Device form of the reference's per-slot merge of partial results (reduceOneSlot, omniscidb/QueryEngine/
// ResultSetReduction.cpp) with the NULL rules of the _skip_val functions (QE/RuntimeFunctions.cpp:612-681, 841-867), over
// what hdk_hip_columnarize_result, hdk_hip_filter_columns and hdk_hip_sort_columns write.  A row is a TAIL when it is the
// last row or when some key word differs from the next row's; a run's output row belongs to its tail, so partial values
// only ever flow forward.
//
// Four launches on one stream, ordered by nothing but the stream (no global atomics, no look-back, no flags):
//   hdk_group_count       persistent grid over tiles of kGcTile rows: the tile's number of tails -> counts[tile]; unless
//                         the call only counts, per aggregate the tile's OPEN SUFFIX -- the partial over the rows after
//                         the tile's last tail (the whole tile when it has none) -- by a masked block reduction that
//                         loads only the 64-row items the suffix reaches into
//   hdk_counts_scan<4>    one block (column_scan.hip): exclusive offsets in place, the total -> *row_count.  A tile has a
//                         tail exactly when its offset differs from the next tile's: that is the has-tail flag
//   hdk_group_carry_scan  one block per aggregate: the segmented exclusive scan of the open suffixes over the tiles,
//                         carry_in[t] = has_tail[t-1] ? suffix[t-1] : combine(carry_in[t-1], suffix[t-1]), in place; in
//                         trips of kGcCarryTrip tiles, the carry going from trip to trip
//   hdk_group_reduce      per tile (one without a tail is skipped unread): the tails again, then per output a segmented
//                         inclusive reduction -- a wave-level segmented scan per 64-row item, lane 63 carried to the next
//                         item, the waves chained through LDS, carry_in applied to the tile's first open run -- and at
//                         every tail one word stored at offset[tile] + rank
// Row layout: wave w of a block owns rows [w * 1024, (w + 1) * 1024) of its tile and its item j the 64 consecutive rows
// from w * 1024 + j * 64, so a ballot is the flag word of those rows and rows follow each other lane by lane, item by
// item, wave by wave.
// "No value yet": beside every accumulator travels the number of non-NULL words it has seen (for COUNT that number IS
// the value).  NULL words enter a reduction as the operator's identity; a run whose count is 0 at its tail gives
// null_bits.  The count goes through every combine step -- item to item, wave to wave, the tile's open suffix, the carry
// scan -- so a run whose rows in one tile are all NULL takes its value from whichever tile has one, and a sum that
// happens to equal the sentinel stays a value.
// The geometry, the tails, the operators, the open suffix and the carry scan are column_segments.h's, shared with
// window_columns.hip.
// Traffic for n rows, k key columns, a aggregated columns, r runs: count 8nk (+ the suffix items of the aggregated
// columns, at least one item per wave and column), reduce 8n(k + a) read + 8r per output written.
#include <string.h>

#include "column_segments.h"
#include "host_common.h"

namespace hdk {

struct GcDesc {
  uint32_t nkeys, nouts;
  uint32_t key_col[HDK_HIP_MAX_GROUP_KEYS];
  GcOut out[HDK_HIP_MAX_GROUP_OUTS];
};

// sufv == NULL: the call only counts
__global__ __launch_bounds__(kGcBlock) void hdk_group_count(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, GcDesc d,
                                                             uint32_t ntiles, uint32_t* __restrict__ tile_counts,
                                                             int64_t* __restrict__ sufv, uint32_t* __restrict__ sufc) {
  __shared__ uint32_t s_wave[kGcWaves];
  __shared__ int64_t s_v[kGcWaves];
  __shared__ uint32_t s_c[kGcWaves], s_t[kGcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t r0 = gc_row0(tile, wave, lane);
    const uint32_t tails = gc_tails(cols, capacity, n, d, r0, lane);
    block_store_tile_count(s_wave, gc_count_tails(tails), tile_counts + tile);
    if (!sufv) {
      continue;
    }
    for (uint32_t a = 0; a < d.nouts; ++a) {
      const GcOut o = d.out[a];
      const int64_t* col = cols + static_cast<uint64_t>(o.col) * capacity;
      int64_t* dv = sufv + static_cast<uint64_t>(a) * ntiles + tile;
      uint32_t* dc = sufc + static_cast<uint64_t>(a) * ntiles + tile;
#define HDK_GC_CASE(OP) \
  case OP: gc_open_suffix<OP>(col, n, o, r0, lane, wave, tails, s_v, s_c, s_t, dv, dc); break;
      switch (o.op) {
        HDK_GC_CASE(GC_COUNT_STAR)
        HDK_GC_CASE(GC_COUNT)
        HDK_GC_CASE(GC_SUM_I)
        HDK_GC_CASE(GC_SUM_F)
        HDK_GC_CASE(GC_MIN_I)
        HDK_GC_CASE(GC_MIN_F)
        HDK_GC_CASE(GC_MAX_I)
        HDK_GC_CASE(GC_MAX_F)
        default: break;  // GC_ID: a key word has no partial
      }
#undef HDK_GC_CASE
    }
  }
}

// one block per aggregate: column_segments.h's segmented exclusive scan of its open suffixes
__global__ __launch_bounds__(kGcCarryBlock) void hdk_group_carry_scan(GcDesc d, uint32_t ntiles, const uint32_t* __restrict__ offs,
                                                                       int64_t* __restrict__ sufv, uint32_t* __restrict__ sufc) {
  const uint32_t a = blockIdx.x;
  int64_t* v = sufv + static_cast<uint64_t>(a) * ntiles;
  uint32_t* c = sufc + static_cast<uint64_t>(a) * ntiles;
#define HDK_GC_CASE(OP) \
  case OP: gc_carry_scan<OP>(ntiles, offs, v, c); break;
  switch (d.out[a].op) {
    HDK_GC_CASE(GC_COUNT_STAR)
    HDK_GC_CASE(GC_COUNT)
    HDK_GC_CASE(GC_SUM_I)
    HDK_GC_CASE(GC_SUM_F)
    HDK_GC_CASE(GC_MIN_I)
    HDK_GC_CASE(GC_MIN_F)
    HDK_GC_CASE(GC_MAX_I)
    HDK_GC_CASE(GC_MAX_F)
    default: break;
  }
#undef HDK_GC_CASE
}

// HDK_AGG_ID: the key word of every tail
HDK_DEV void gc_store_keys(const int64_t* __restrict__ col, uint32_t r0, uint32_t lane, uint32_t tails, uint64_t base,
                           int64_t* __restrict__ dst, uint64_t out_capacity) {
  uint32_t before = 0;
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    const uint64_t mj = gc_item_tails(tails, j);
    const uint64_t rank = base + before + lane_rank(mj);
    if (((tails >> j) & 1u) && rank < out_capacity) {
      dst[rank] = gc_load(col + r0 + static_cast<uint32_t>(j) * kWave);
    }
    before += static_cast<uint32_t>(__popcll(mj));
  }
}

// One aggregate over one tile.  Every wave runs its 16 items in row order with the partial of the run that is open at
// the end of an item carried to the next (from lane 63, unless that lane is a tail).  The wave's first tail cannot be
// stored yet -- its run may have begun in an earlier wave or tile --: its lane keeps it back until the waves have
// exchanged what they end with, and adds what enters the wave.  `base`: the output row of this wave's first tail.
template <uint32_t OP>
HDK_DEV void gc_reduce_out(const int64_t* __restrict__ col, uint32_t n, const GcOut& o, uint32_t r0, uint32_t lane, uint32_t wave,
                           uint32_t tails, uint64_t base, int64_t in_v, uint32_t in_c, int64_t (&s_v)[kGcWaves],
                           uint32_t (&s_c)[kGcWaves], uint32_t (&s_t)[kGcWaves], int64_t* __restrict__ dst, uint64_t out_capacity) {
  int64_t v[kGcItems];
  if constexpr (OP != GC_COUNT_STAR) {
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
      v[j] = gc_load(col + (r < n ? r : n - 1));
    }
  }
  int64_t carry_v = gc_identity<OP>();  // of the run that is open where item j begins (wave-uniform)
  uint32_t carry_c = 0;
  bool seen = false;  // a tail in an earlier item of this wave
  uint32_t before = 0;
  int64_t first_v = 0;  // the wave's first tail, on the lane that holds it
  uint32_t first_c = 0;
  uint64_t first_rank = ~uint64_t(0);
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
    bool has = r < n;
    if constexpr (OP != GC_COUNT_STAR) {
      has = has && !(o.nullable && v[j] == o.null_bits);
    }
    const uint64_t nn = __builtin_amdgcn_ballot_w64(has);
    const uint64_t mj = gc_item_tails(tails, j);
    const uint64_t below = mj & ((uint64_t(1) << lane) - 1);  // the tails before this lane
    const uint32_t s = below ? 64u - static_cast<uint32_t>(__clzll(static_cast<long long>(below))) : 0u;  // where this lane's run starts
    int64_t x = gc_identity<OP>();
    if constexpr (!gc_counts<OP>()) {
      x = has ? v[j] : x;
#pragma unroll
      for (int dd = 1; dd < kWave; dd <<= 1) {
        const int64_t up = gc_shfl_up(x, dd);
        if (lane >= s + static_cast<uint32_t>(dd)) {
          x = gc_combine<OP>(up, x);
        }
      }
    }
    // the non-NULL words of lanes s .. lane
    uint32_t c = static_cast<uint32_t>(__popcll(nn & (~uint64_t(0) >> (63u - lane)) & (~uint64_t(0) << s)));
    if (below == 0) {  // the run reaches back into the item before
      x = gc_combine<OP>(carry_v, x);
      c += carry_c;
    }
    if ((mj >> lane) & 1u) {
      const uint64_t rank = base + before + lane_rank(mj);
      if (!seen && below == 0) {
        first_v = x;
        first_c = c;
        first_rank = rank;
      } else if (rank < out_capacity) {
        dst[rank] = gc_result<OP>(x, c, o.null_bits);
      }
    }
    const bool closed = (mj >> (kWave - 1)) & 1u;
    const int64_t last_v = gc_lane63(x);
    const uint32_t last_c = __builtin_amdgcn_readlane(c, kWave - 1);
    carry_v = closed ? gc_identity<OP>() : last_v;
    carry_c = closed ? 0u : last_c;
    seen = seen || mj != 0;
    before += static_cast<uint32_t>(__popcll(mj));
  }
  if (lane == 0) {
    s_v[wave] = carry_v;
    s_c[wave] = carry_c;
    s_t[wave] = seen;
  }
  __syncthreads();
  // what enters this wave: the tile's carry_in through the waves before it
#pragma unroll
  for (int w = 0; w < kGcWaves - 1; ++w) {
    if (static_cast<uint32_t>(w) < wave) {
      in_v = s_t[w] ? s_v[w] : gc_combine<OP>(in_v, s_v[w]);
      in_c = s_t[w] ? s_c[w] : in_c + s_c[w];
    }
  }
  if (first_rank < out_capacity) {
    dst[first_rank] = gc_result<OP>(gc_combine<OP>(in_v, first_v), in_c + first_c, o.null_bits);
  }
  __syncthreads();
}

__global__ __launch_bounds__(kGcBlock) void hdk_group_reduce(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, GcDesc d,
                                                              uint32_t ntiles, const uint32_t* __restrict__ tile_offs,
                                                              const int64_t* __restrict__ carv, const uint32_t* __restrict__ carc,
                                                              int64_t* __restrict__ out, uint64_t out_capacity) {
  __shared__ uint32_t s_wave[kGcWaves];
  __shared__ int64_t s_v[kGcWaves];
  __shared__ uint32_t s_c[kGcWaves], s_t[kGcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t first = tile_offs[tile];
    if (tile_offs[tile + 1] == first || first >= out_capacity) {
      continue;  // no tail in this tile, or all of them past the capacity (block-uniform)
    }
    const uint32_t r0 = gc_row0(tile, wave, lane);
    const uint32_t tails = gc_tails(cols, capacity, n, d, r0, lane);
    const uint32_t wave_tails = gc_count_tails(tails);
    const uint64_t base = gc_wave_base(s_wave, first, wave_tails, lane, wave);
    for (uint32_t a = 0; a < d.nouts; ++a) {
      const GcOut o = d.out[a];
      const int64_t* col = cols + static_cast<uint64_t>(o.col) * capacity;
      int64_t* dst = out + static_cast<uint64_t>(a) * out_capacity;
      if (o.op == GC_ID) {
        gc_store_keys(col, r0, lane, tails, base, dst, out_capacity);
        continue;
      }
      const int64_t in_v = carv[static_cast<uint64_t>(a) * ntiles + tile];
      const uint32_t in_c = carc[static_cast<uint64_t>(a) * ntiles + tile];
#define HDK_GC_CASE(OP) \
  case OP: gc_reduce_out<OP>(col, n, o, r0, lane, wave, tails, base, in_v, in_c, s_v, s_c, s_t, dst, out_capacity); break;
      switch (o.op) {
        HDK_GC_CASE(GC_COUNT_STAR)
        HDK_GC_CASE(GC_COUNT)
        HDK_GC_CASE(GC_SUM_I)
        HDK_GC_CASE(GC_SUM_F)
        HDK_GC_CASE(GC_MIN_I)
        HDK_GC_CASE(GC_MIN_F)
        HDK_GC_CASE(GC_MAX_I)
        HDK_GC_CASE(GC_MAX_F)
        default: break;
      }
#undef HDK_GC_CASE
    }
  }
}

static size_t gc_tiles(uint64_t num_rows) { return static_cast<size_t>((num_rows + kGcTile - 1) / kGcTile); }
static size_t gc_counts_bytes(size_t ntiles) { return align256((ntiles + 1) * sizeof(uint32_t)); }
static size_t gc_values_bytes(size_t ntiles, int32_t num_outs) { return align256(ntiles * static_cast<size_t>(num_outs) * sizeof(int64_t)); }

}  // namespace hdk

using namespace hdk;

// [tile counters + 1][num_outs x ntiles partial values][num_outs x ntiles non-NULL counts]
extern "C" size_t hdk_hip_group_columns_workspace_bytes(uint64_t num_rows, int32_t num_outs) {
  const size_t ntiles = gc_tiles(num_rows);
  const int32_t outs = num_outs < 0 ? 0 : num_outs;
  return gc_counts_bytes(ntiles) + gc_values_bytes(ntiles, outs) + align256(ntiles * static_cast<size_t>(outs) * sizeof(uint32_t));
}

extern "C" int32_t hdk_hip_group_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                                         const int32_t* key_cols, int32_t num_keys, const hdk_hip_group_out* outs, int32_t num_outs,
                                         int64_t* out_cols, uint64_t out_capacity, uint64_t* row_count, void* workspace,
                                         size_t workspace_bytes, int32_t device_id, void* stream) {
  HDK_REQUIRE(cols && key_cols && outs && row_count,
              "hdk_hip_group_columns: NULL argument (cols, key_cols, outs and row_count are required)");
  HDK_REQUIRE(num_cols >= 1, "hdk_hip_group_columns: num_cols %d", num_cols);
  HDK_REQUIRE(num_keys >= 1 && num_keys <= HDK_HIP_MAX_GROUP_KEYS, "hdk_hip_group_columns: num_keys %d outside 1..%d", num_keys,
              HDK_HIP_MAX_GROUP_KEYS);
  HDK_REQUIRE(num_outs >= 1 && num_outs <= HDK_HIP_MAX_GROUP_OUTS, "hdk_hip_group_columns: num_outs %d outside 1..%d", num_outs,
              HDK_HIP_MAX_GROUP_OUTS);
  GcDesc d;
  memset(&d, 0, sizeof(d));
  d.nkeys = static_cast<uint32_t>(num_keys);
  d.nouts = static_cast<uint32_t>(num_outs);
  for (int32_t k = 0; k < num_keys; ++k) {
    HDK_REQUIRE(key_cols[k] >= 0 && key_cols[k] < num_cols, "hdk_hip_group_columns: key %d names column %d of %d", k, key_cols[k],
                num_cols);
    d.key_col[k] = static_cast<uint32_t>(key_cols[k]);
  }
  for (int32_t i = 0; i < num_outs; ++i) {
    const hdk_hip_group_out& o = outs[i];
    HDK_REQUIRE(o.kind == HDK_AGG_ID || o.kind == HDK_AGG_COUNT || o.kind == HDK_AGG_SUM || o.kind == HDK_AGG_MIN ||
                    o.kind == HDK_AGG_MAX,
                "hdk_hip_group_columns: out %d has kind %d (ID, COUNT, SUM, MIN or MAX)", i, static_cast<int>(o.kind));
    const bool count_star = o.kind == HDK_AGG_COUNT && o.col < 0;
    HDK_REQUIRE(count_star || (o.col >= 0 && o.col < num_cols), "hdk_hip_group_columns: out %d names column %d of %d", i, o.col,
                num_cols);
    GcOut& g = d.out[i];
    g.col = count_star ? 0u : static_cast<uint32_t>(o.col);
    g.nullable = o.nullable ? 1u : 0u;
    g.null_bits = o.null_bits;
    if (o.kind == HDK_AGG_ID) {
      bool is_key = false;
      for (int32_t k = 0; k < num_keys; ++k) {
        is_key = is_key || key_cols[k] == o.col;
      }
      HDK_REQUIRE(is_key, "hdk_hip_group_columns: out %d is an ID of column %d, which is not a key column", i, o.col);
      g.op = GC_ID;
    } else if (o.kind == HDK_AGG_COUNT) {
      // (a column that cannot be NULL counts its rows: no load)
      g.op = count_star || !o.nullable ? GC_COUNT_STAR : GC_COUNT;
    } else if (o.kind == HDK_AGG_SUM) {
      g.op = o.is_fp ? GC_SUM_F : GC_SUM_I;
    } else if (o.kind == HDK_AGG_MIN) {
      g.op = o.is_fp ? GC_MIN_F : GC_MIN_I;
    } else {
      g.op = o.is_fp ? GC_MAX_F : GC_MAX_I;
    }
  }
  HDK_REQUIRE(num_rows < (uint64_t(1) << 32), "hdk_hip_group_columns: num_rows %llu does not fit 32-bit row indices",
              static_cast<unsigned long long>(num_rows));
  HDK_REQUIRE(num_rows <= capacity, "hdk_hip_group_columns: num_rows %llu exceeds the capacity %llu",
              static_cast<unsigned long long>(num_rows), static_cast<unsigned long long>(capacity));
  const size_t need = hdk_hip_group_columns_workspace_bytes(num_rows, num_outs);
  HDK_REQUIRE(!workspace || workspace_bytes >= need, "hdk_hip_group_columns: workspace of %zu bytes, %zu needed", workspace_bytes,
              need);
  HDK_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "hdk_hip_group_columns: workspace %p is not 8-byte aligned",
              workspace);
  const bool writes = out_cols && out_capacity;
  {
    // every block the call reads or writes; a block nothing is written to (out_capacity == 0, count only) has no bytes
    const MemBlock blk[] = {
        {"cols", reinterpret_cast<uintptr_t>(cols), static_cast<uint64_t>(num_cols) * capacity * 8},
        {"out_cols", reinterpret_cast<uintptr_t>(out_cols), writes ? static_cast<uint64_t>(num_outs) * out_capacity * 8 : 0},
        {"row_count", reinterpret_cast<uintptr_t>(row_count), 8},
        {"workspace", reinterpret_cast<uintptr_t>(workspace), workspace ? static_cast<uint64_t>(need) : 0},
    };
    const int32_t bad = require_disjoint("hdk_hip_group_columns", blk, sizeof(blk) / sizeof(blk[0]));
    if (bad) return bad;
  }
  hipStream_t s;
  int32_t st = device_enter(device_id, stream, &s);
  if (st) return st;
  if (num_rows == 0) {
    HDK_HIP_CHECK(hipMemsetAsync(row_count, 0, sizeof(uint64_t), s));
    return HDK_HIP_OK;
  }
  AsyncScratch mem(s);
  st = acquire_workspace(mem, &workspace, need);
  if (st) return st;
  const uint32_t ntiles = static_cast<uint32_t>(gc_tiles(num_rows));
  uint32_t* tiles = static_cast<uint32_t*>(workspace);
  int64_t* sufv = reinterpret_cast<int64_t*>(static_cast<int8_t*>(workspace) + gc_counts_bytes(ntiles));
  uint32_t* sufc = reinterpret_cast<uint32_t*>(reinterpret_cast<int8_t*>(sufv) + gc_values_bytes(ntiles, num_outs));
  const dim3 grid(persistent_grid(device_props(device_id), ntiles)), block(kGcBlock);
  hipLaunchKernelGGL(hdk_group_count, grid, block, 0, s, cols, capacity, static_cast<uint32_t>(num_rows), d, ntiles, tiles,
                     writes ? sufv : nullptr, writes ? sufc : nullptr);
  launch_counts_scan(tiles, ntiles, kGcScanPer, row_count, s);
  if (writes) {
    hipLaunchKernelGGL(hdk_group_carry_scan, dim3(static_cast<unsigned>(num_outs)), dim3(kGcCarryBlock), 0, s, d, ntiles, tiles, sufv,
                       sufc);
    hipLaunchKernelGGL(hdk_group_reduce, grid, block, 0, s, cols, capacity, static_cast<uint32_t>(num_rows), d, ntiles, tiles, sufv,
                       sufc, out_cols, out_capacity);
  }
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
