// chunk_columns.hip -- dense result columns -> the chunks of a table that the scan kernels read, with their statistics.
//
//   hdk_hip_chunk_columns   copies the selected columns into a block whose fragments start on 256-byte boundaries, rewrites
//                           each column's in-band NULL to the NULL of an 8-byte storage column, and leaves min / max /
//                           null_count / value_count per (column, fragment): the device form of what ArrowStorage does on
//                           import (the sentinel rewrite of ArrowStorageUtils.cpp:176-213 and computeStats).
//
// Two launches ordered by the stream alone: a streaming pass over tiles of 4 096 rows that never span two fragments
// (registers -> wave reduction -> LDS -> one 32-byte partial per column, fragment and tile), and a fold of each
// (column, fragment)'s partials.  No atomics, no look-back, no host wait.
#include <string.h>

#include "column_primitives.h"
#include "host_common.h"

namespace hdk {

constexpr int kCkBlock = kTileBlock;
constexpr int kCkItems = 16;  // rows per thread and tile
constexpr uint32_t kCkTile = kCkBlock * kCkItems;
constexpr int kCkFoldBlock = kWave;  // one wave folds one (column, fragment)
constexpr uint32_t kCkFoldGridMax = 1u << 20;

static_assert(sizeof(hdk_hip_chunk_stats) == 32, "a partial is one 32-byte record");

constexpr uint32_t kCkFp = 1, kCkNullable = 2;

struct CkCol {
  uint32_t col;
  uint32_t flags;  // kCkFp | kCkNullable
  int64_t null_bits;
  int64_t out_null;
};

struct CkDesc {
  uint32_t ncols;
  uint32_t fp_mask;  // bit j: output column j compares as doubles
  CkCol col[HDK_HIP_MAX_CHUNK_COLUMNS];
};

// the identities of min / max: no word compares below / above them, and a NaN compares neither way
template <bool FP>
HDK_DEV int64_t ck_min_identity() {
  return FP ? static_cast<int64_t>(0x7FF0000000000000ull) : INT64_MAX;  // +inf
}
template <bool FP>
HDK_DEV int64_t ck_max_identity() {
  return FP ? static_cast<int64_t>(0xFFF0000000000000ull) : INT64_MIN;  // -inf
}

// min / max of two words of a column: signed int64, or doubles by value with the winner's bit pattern kept (a NaN
// compares neither way and never wins)
template <bool FP>
HDK_DEV int64_t ck_min(int64_t a, int64_t b) {
  if (FP) {
    return bits_to_double(b) < bits_to_double(a) ? b : a;
  }
  return b < a ? b : a;
}
template <bool FP>
HDK_DEV int64_t ck_max(int64_t a, int64_t b) {
  if (FP) {
    return bits_to_double(b) > bits_to_double(a) ? b : a;
  }
  return b > a ? b : a;
}

template <bool FP>
HDK_DEV void ck_wave_minmax(int64_t& mn, int64_t& mx) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    mn = ck_min<FP>(mn, __shfl_xor(static_cast<long long>(mn), d, kWave));
    mx = ck_max<FP>(mx, __shfl_xor(static_cast<long long>(mx), d, kWave));
  }
}

HDK_DEV uint32_t ck_wave_sum(uint32_t v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    v += __shfl_xor(v, d, kWave);
  }
  return v;
}

struct CkShared {
  int64_t mn[kTileWaves];
  int64_t mx[kTileWaves];
  uint32_t nulls[kTileWaves];
  uint32_t values[kTileWaves];
};

// rows [r0, end) of one column: copy with the NULL rewrite, and the tile's partial.  end - r0 <= kCkTile.
template <bool FP>
HDK_DEV void ck_tile_column(const int64_t* __restrict__ src, int64_t* __restrict__ dst, uint64_t r0, uint64_t end, const CkCol q,
                            CkShared& sh, hdk_hip_chunk_stats* __restrict__ part) {
  const bool nullable = (q.flags & kCkNullable) != 0;
  int64_t v[kCkItems];
#pragma unroll
  for (int j = 0; j < kCkItems; ++j) {
    const uint64_t r = r0 + threadIdx.x + static_cast<uint32_t>(j) * kCkBlock;
    v[j] = nt_load<int64_t>(src + (r < end ? r : end - 1), 0);  // (a tile has a row: end > r0; a lane past it re-reads the last)
  }
  int64_t mn = ck_min_identity<FP>(), mx = ck_max_identity<FP>();
  uint32_t nulls = 0, values = 0;
#pragma unroll
  for (int j = 0; j < kCkItems; ++j) {
    const uint64_t r = r0 + threadIdx.x + static_cast<uint32_t>(j) * kCkBlock;
    const bool live = r < end;
    const int64_t w = (nullable && v[j] == q.null_bits) ? q.out_null : v[j];
    if (live) {
      dst[r] = w;
    }
    // what reads as NULL afterwards is counted as NULL: the rewritten words and a word that equals out_null already
    const bool is_null = nullable && w == q.out_null;
    nulls += live && is_null ? 1u : 0u;
    if (live && !is_null) {
      ++values;
      mn = ck_min<FP>(mn, w);
      mx = ck_max<FP>(mx, w);
    }
  }
  ck_wave_minmax<FP>(mn, mx);
  nulls = ck_wave_sum(nulls);
  values = ck_wave_sum(values);
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
    sh.mn[wave] = mn;
    sh.mx[wave] = mx;
    sh.nulls[wave] = nulls;
    sh.values[wave] = values;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    hdk_hip_chunk_stats p;
    p.min_bits = sh.mn[0];
    p.max_bits = sh.mx[0];
    p.null_count = sh.nulls[0];
    p.value_count = sh.values[0];
#pragma unroll
    for (int w = 1; w < kTileWaves; ++w) {
      p.min_bits = ck_min<FP>(p.min_bits, sh.mn[w]);
      p.max_bits = ck_max<FP>(p.max_bits, sh.mx[w]);
      p.null_count += sh.nulls[w];
      p.value_count += sh.values[w];
    }
    *part = p;
  }
}

// Tile t belongs to fragment t / tpf (every fragment but the last has tpf tiles, the last at most tpf) and starts at row
// fragment * fragment_rows + (t % tpf) * kCkTile.  Partial of (column c, tile t): part[c * ntiles + t].
// The LDS words alternate between two sets from one (tile, column) step to the next: thread 0 still reads one set while
// the other waves fill the other, and the barrier of the step in between separates the two uses of a set.
__global__ __launch_bounds__(kCkBlock) void hdk_chunk_columns(const int64_t* __restrict__ cols, uint64_t capacity, uint64_t num_rows,
                                                               uint64_t fragment_rows, uint32_t tpf, uint32_t ntiles, CkDesc d,
                                                               int64_t* __restrict__ out, uint64_t out_capacity,
                                                               hdk_hip_chunk_stats* __restrict__ part) {
  __shared__ CkShared sh[2];
  uint32_t step = 0;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t f = tile / tpf, k = tile - f * tpf;
    const uint64_t fbegin = static_cast<uint64_t>(f) * fragment_rows;
    const uint64_t fend = fbegin + fragment_rows < num_rows ? fbegin + fragment_rows : num_rows;
    const uint64_t r0 = fbegin + static_cast<uint64_t>(k) * kCkTile;
    const uint64_t end = r0 + kCkTile < fend ? r0 + kCkTile : fend;
#pragma unroll 1
    for (uint32_t c = 0; c < d.ncols; ++c, ++step) {  // (wave-uniform: the description comes from scalar registers)
      const CkCol q = d.col[c];
      const int64_t* src = cols + static_cast<uint64_t>(q.col) * capacity;
      int64_t* dst = out + static_cast<uint64_t>(c) * out_capacity;
      hdk_hip_chunk_stats* p = part + static_cast<uint64_t>(c) * ntiles + tile;
      if (q.flags & kCkFp) {
        ck_tile_column<true>(src, dst, r0, end, q, sh[step & 1], p);
      } else {
        ck_tile_column<false>(src, dst, r0, end, q, sh[step & 1], p);
      }
    }
  }
}

// stats[c * nfrag + f] = the fold of the partials of fragment f's tiles; one wave per (column, fragment)
__global__ __launch_bounds__(kCkFoldBlock) void hdk_chunk_fold(const hdk_hip_chunk_stats* __restrict__ part, uint32_t ntiles,
                                                                uint32_t tpf, uint32_t nfrag, uint32_t ncols, uint32_t fp_mask,
                                                                hdk_hip_chunk_stats* __restrict__ stats) {
  const uint64_t pairs = static_cast<uint64_t>(ncols) * nfrag;
  for (uint64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
    const uint32_t c = static_cast<uint32_t>(pair / nfrag), f = static_cast<uint32_t>(pair - static_cast<uint64_t>(c) * nfrag);
    const bool fp = (fp_mask >> c) & 1u;
    const uint64_t t0 = static_cast<uint64_t>(f) * tpf;
    const uint64_t t1 = t0 + tpf < ntiles ? t0 + tpf : ntiles;
    const hdk_hip_chunk_stats* src = part + static_cast<uint64_t>(c) * ntiles;
    int64_t mn = fp ? ck_min_identity<true>() : ck_min_identity<false>();
    int64_t mx = fp ? ck_max_identity<true>() : ck_max_identity<false>();
    uint64_t nulls = 0, values = 0;
    for (uint64_t t = t0 + threadIdx.x; t < t1; t += kCkFoldBlock) {
      const hdk_hip_chunk_stats p = src[t];
      mn = fp ? ck_min<true>(mn, p.min_bits) : ck_min<false>(mn, p.min_bits);
      mx = fp ? ck_max<true>(mx, p.max_bits) : ck_max<false>(mx, p.max_bits);
      nulls += p.null_count;
      values += p.value_count;
    }
    if (fp) {
      ck_wave_minmax<true>(mn, mx);
    } else {
      ck_wave_minmax<false>(mn, mx);
    }
#pragma unroll
    for (int dlt = kWave / 2; dlt >= 1; dlt >>= 1) {
      nulls += __shfl_xor(static_cast<unsigned long long>(nulls), dlt, kWave);
      values += __shfl_xor(static_cast<unsigned long long>(values), dlt, kWave);
    }
    if (threadIdx.x == 0) {
      hdk_hip_chunk_stats s;
      s.min_bits = mn;
      s.max_bits = mx;
      s.null_count = nulls;
      s.value_count = values;
      stats[pair] = s;
    }
  }
}

static uint64_t ck_fragments(uint64_t num_rows, uint64_t fragment_rows) {
  const uint64_t n = (num_rows + fragment_rows - 1) / fragment_rows;
  return n ? n : 1;
}
static uint64_t ck_tiles_of(uint64_t rows) { return (rows + kCkTile - 1) / kCkTile; }
// every fragment but the last has ck_tiles_of(fragment_rows) tiles; the last has those of its own rows
static uint64_t ck_tiles(uint64_t num_rows, uint64_t fragment_rows) {
  if (num_rows == 0) return 0;
  const uint64_t nfrag = ck_fragments(num_rows, fragment_rows);
  return (nfrag - 1) * ck_tiles_of(fragment_rows) + ck_tiles_of(num_rows - (nfrag - 1) * fragment_rows);
}

}  // namespace hdk

using namespace hdk;

extern "C" size_t hdk_hip_chunk_columns_workspace_bytes(uint64_t num_rows, uint64_t fragment_rows, int32_t num_cols) {
  if (fragment_rows == 0 || num_cols < 1) return 0;
  return align256(static_cast<size_t>(num_cols) * ck_tiles(num_rows, fragment_rows) * sizeof(hdk_hip_chunk_stats));
}

extern "C" int32_t hdk_hip_chunk_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols_in, uint64_t num_rows,
                                         const hdk_hip_chunk_col* sel, int32_t num_cols, uint64_t fragment_rows, int64_t* out_cols,
                                         uint64_t out_capacity, hdk_hip_chunk_stats* stats, void* workspace, size_t workspace_bytes,
                                         int32_t device_id, void* stream) {
  HDK_REQUIRE(sel && out_cols && stats && (cols || num_rows == 0),
              "hdk_hip_chunk_columns: NULL argument (sel, out_cols and stats are required, and cols when there are rows)");
  HDK_REQUIRE(num_cols >= 1 && num_cols <= HDK_HIP_MAX_CHUNK_COLUMNS, "hdk_hip_chunk_columns: num_cols %d outside 1..%d", num_cols,
              HDK_HIP_MAX_CHUNK_COLUMNS);
  CkDesc d;
  memset(&d, 0, sizeof(d));
  d.ncols = static_cast<uint32_t>(num_cols);
  for (int32_t j = 0; j < num_cols; ++j) {
    const hdk_hip_chunk_col& c = sel[j];
    HDK_REQUIRE(c.col >= 0 && c.col < num_cols_in, "hdk_hip_chunk_columns: selection %d names column %d of %d", j, c.col,
                num_cols_in);
    CkCol& q = d.col[j];
    q.col = static_cast<uint32_t>(c.col);
    q.flags = (c.is_fp ? kCkFp : 0u) | (c.nullable ? kCkNullable : 0u);
    q.null_bits = c.null_bits;
    q.out_null = c.out_null_bits;
    d.fp_mask |= c.is_fp ? 1u << j : 0u;
  }
  HDK_REQUIRE(fragment_rows > 0 && fragment_rows % 32 == 0,
              "hdk_hip_chunk_columns: fragment_rows %llu is not a positive multiple of 32 (every chunk starts 256-byte aligned)",
              static_cast<unsigned long long>(fragment_rows));
  HDK_REQUIRE(num_rows < (uint64_t(1) << 32), "hdk_hip_chunk_columns: num_rows %llu does not fit 32-bit row indices",
              static_cast<unsigned long long>(num_rows));
  HDK_REQUIRE(num_rows <= capacity && num_rows <= out_capacity,
              "hdk_hip_chunk_columns: num_rows %llu exceeds the capacity %llu or the output capacity %llu",
              static_cast<unsigned long long>(num_rows), static_cast<unsigned long long>(capacity),
              static_cast<unsigned long long>(out_capacity));
  HDK_REQUIRE(num_cols == 1 || out_capacity % 32 == 0,
              "hdk_hip_chunk_columns: out_capacity %llu is not a multiple of 32 (every output column starts 256-byte aligned)",
              static_cast<unsigned long long>(out_capacity));
  const uint64_t nfrag = ck_fragments(num_rows, fragment_rows);
  const uint64_t ntiles = ck_tiles(num_rows, fragment_rows);
  const size_t need = hdk_hip_chunk_columns_workspace_bytes(num_rows, fragment_rows, num_cols);
  HDK_REQUIRE(!workspace || workspace_bytes >= need, "hdk_hip_chunk_columns: workspace of %zu bytes, %zu needed", workspace_bytes,
              need);
  HDK_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "hdk_hip_chunk_columns: workspace %p is not 8-byte aligned",
              workspace);
  {
    const MemBlock blk[] = {
        {"cols", reinterpret_cast<uintptr_t>(cols), num_rows ? static_cast<uint64_t>(num_cols_in) * capacity * 8 : 0},
        {"out_cols", reinterpret_cast<uintptr_t>(out_cols), num_rows ? static_cast<uint64_t>(num_cols) * out_capacity * 8 : 0},
        {"stats", reinterpret_cast<uintptr_t>(stats), static_cast<uint64_t>(num_cols) * nfrag * sizeof(hdk_hip_chunk_stats)},
        {"workspace", reinterpret_cast<uintptr_t>(workspace), workspace ? static_cast<uint64_t>(need) : 0},
    };
    const int32_t bad = require_disjoint("hdk_hip_chunk_columns", blk, sizeof(blk) / sizeof(blk[0]));
    if (bad) return bad;
  }
  hipStream_t s;
  int32_t st = device_enter(device_id, stream, &s);
  if (st) return st;
  if (num_rows == 0) {
    HDK_HIP_CHECK(hipMemsetAsync(stats, 0, static_cast<size_t>(num_cols) * sizeof(hdk_hip_chunk_stats), s));
    return HDK_HIP_OK;
  }
  AsyncScratch mem(s);
  st = acquire_workspace(mem, &workspace, need);
  if (st) return st;
  hdk_hip_chunk_stats* part = static_cast<hdk_hip_chunk_stats*>(workspace);
  const uint32_t tpf = static_cast<uint32_t>(ck_tiles_of(fragment_rows));
  const dim3 grid(persistent_grid(device_props(device_id), ntiles)), block(kCkBlock);
  hipLaunchKernelGGL(hdk_chunk_columns, grid, block, 0, s, cols, capacity, num_rows, fragment_rows, tpf, static_cast<uint32_t>(ntiles),
                     d, out_cols, out_capacity, part);
  const uint64_t pairs = static_cast<uint64_t>(num_cols) * nfrag;
  const dim3 fgrid(static_cast<unsigned>(pairs < kCkFoldGridMax ? pairs : kCkFoldGridMax)), fblock(kCkFoldBlock);
  hipLaunchKernelGGL(hdk_chunk_fold, fgrid, fblock, 0, s, part, static_cast<uint32_t>(ntiles), tpf, static_cast<uint32_t>(nfrag),
                     static_cast<uint32_t>(num_cols), d.fp_mask, stats);
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
