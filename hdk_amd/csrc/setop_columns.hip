// setop_columns.hip -- UNION / INTERSECT / EXCEPT over dense 8-byte result columns in HBM.
//
// Device form of the reference's LogicalUnion step over two previous steps' results (RelAlgExecutor::executeUnion,
// omniscidb/QueryEngine/RelAlgExecutor.cpp), widened to the other set operations of SQL.  Two entry points:
//   hdk_hip_concat_columns   UNION ALL: the rows of a second block appended to the rows of a first one, each side's in-band
//                            NULL rewritten to the output column's, and optionally one more column that says which block a
//                            row came from.  One launch of plain coalesced loads and stores.
//   hdk_hip_setop_columns    over ONE block in which equal rows are adjacent and, inside a run of equal rows, the rows with a
//                            non-zero tag word (the RIGHT operand's) come before the rows with tag 0 (the LEFT operand's):
//                            the rows that the operation keeps, compacted in input order.
// With the right rows in front every operation is a predicate on two forward, exclusive, segmented counters per row --
// rb, the right rows before it in its run, and lb, the left rows before it in its run:
//   UNION          rb + lb == 0                       INTERSECT ALL   left, lb <  rb
//   INTERSECT      left, lb == 0, rb >  0             EXCEPT ALL      left, lb >= rb
//   EXCEPT         left, lb == 0, rb == 0
// (at a left row rb is the run's whole right count), so nothing looks ahead to the end of a run.
//
// Six launches on one stream, ordered by nothing but the stream (no global atomics, no look-back, no flags):
//   hdk_setop_summary     persistent grid over tiles of kGcTile rows: the tile's number of tails -> tails[tile], and its OPEN
//                         SUFFIX -- the right and left rows after the tile's last tail (of the whole tile when it has none)
//                         -- as one packed word (right count << 32 | left count); only the 64-row items the suffix reaches
//                         into load the tag
//   hdk_counts_scan<4>    exclusive offsets of the tail counts: a tile has a tail exactly when its offset differs from the
//                         next tile's
//   hdk_setop_carry_scan  one block: column_segments.h's segmented exclusive scan of the packed suffixes (GC_SUM_I: both
//                         halves stay below 2^32, so they never meet) -> what enters every tile
//   hdk_setop_keep        per tile: the tails again, the tag bits, the carry through the waves before, then per 64-row item
//                         rb and lb of every lane as masked popcounts of the item's ballots (no shuffle scan), the
//                         predicate, one ballot per item stored as the keep mask of those 64 rows (masks[row / 64]) and
//                         the tile's kept count
//   hdk_counts_scan<4>    exclusive offsets of the kept counts, the total -> *row_count
//   hdk_setop_compact     per tile (one without a kept row is skipped unread): ranks from the stored masks, the kept rows'
//                         words gathered per out and stored
// A count-only call stops after the fifth.  The ranks of the compact pass come from the same stored masks as the counts,
// so a block that violates the precondition costs wrong rows and never an access outside the blocks.
// Traffic for n rows, k key columns, o outs, m kept rows: summary 8nk (+ the tag of the suffix items), keep 8n(k + 1) read
// + n/8 written, compact n/8 + 16mo.
#include <string.h>

#include "column_segments.h"
#include "host_common.h"

namespace hdk {

struct SoDesc {
  uint32_t nkeys, nouts;
  uint32_t tag_col, op;
  uint32_t key_col[HDK_HIP_MAX_SETOP_COLUMNS];
  uint32_t out_col[HDK_HIP_MAX_SETOP_OUTS];
};

constexpr int kSoWords = kGcItems * kGcWaves;  // keep masks of a tile, in row order: word wave * kGcItems + j
static_assert(kSoWords == kWave, "one wave scans the keep masks of a tile");

HDK_DEV int64_t so_pack(uint32_t rights, uint32_t lefts) {
  return static_cast<int64_t>((static_cast<uint64_t>(rights) << 32) | lefts);
}

// the lanes of a 64-row item behind its last tail (all of them when it has none)
HDK_DEV uint64_t so_behind(uint64_t mj) {
  if (!mj) return ~uint64_t(0);
  const int hb = 63 - __clzll(static_cast<long long>(mj));
  return hb == 63 ? 0 : ~uint64_t(0) << (hb + 1);
}

HDK_DEV uint64_t so_shfl64(uint64_t v, uint32_t src) {
  const uint32_t lo = __shfl(static_cast<uint32_t>(v), static_cast<int>(src), kWave);
  const uint32_t hi = __shfl(static_cast<uint32_t>(v >> 32), static_cast<int>(src), kWave);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

__global__ __launch_bounds__(kGcBlock) void hdk_setop_summary(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, SoDesc d,
                                                               uint32_t ntiles, uint32_t* __restrict__ tile_tails,
                                                               int64_t* __restrict__ sufv, uint32_t* __restrict__ sufc) {
  __shared__ uint32_t s_wave[kGcWaves];
  __shared__ int64_t s_v[kGcWaves];
  __shared__ uint32_t s_t[kGcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t* tag = cols + static_cast<uint64_t>(d.tag_col) * capacity;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t r0 = gc_row0(tile, wave, lane);
    const uint32_t tails = gc_tails(cols, capacity, n, d, r0, lane);
    block_store_tile_count(s_wave, gc_count_tails(tails), tile_tails + tile);
    uint32_t any = 0;  // bit j: item j holds a tail
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      any |= gc_item_tails(tails, j) ? 1u << j : 0u;
    }
    uint32_t rights = 0, lefts = 0;  // behind the wave's last tail
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      uint64_t sm = 0;
      if ((any >> j) <= 1u) {  // no tail in a later item
        sm = so_behind(gc_item_tails(tails, j));
      }
      if (sm) {  // (wave-uniform: every ballot below runs with all 64 lanes)
        const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
        const bool in = r < n && ((sm >> lane) & 1u);
        const int64_t w = gc_load(tag + (r < n ? r : n - 1));
        rights += static_cast<uint32_t>(__popcll(__builtin_amdgcn_ballot_w64(in && w != 0)));
        lefts += static_cast<uint32_t>(__popcll(__builtin_amdgcn_ballot_w64(in && w == 0)));
      }
    }
    if (lane == 0) {
      s_v[wave] = so_pack(rights, lefts);
      s_t[wave] = any;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t v = 0;
#pragma unroll
      for (int w = 0; w < kGcWaves; ++w) {
        v = s_t[w] ? s_v[w] : gc_combine<GC_SUM_I>(v, s_v[w]);
      }
      sufv[tile] = v;
      sufc[tile] = 0;  // (the scan carries a non-NULL count beside every value; a counter has none)
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kGcCarryBlock) void hdk_setop_carry_scan(uint32_t ntiles, const uint32_t* __restrict__ offs,
                                                                       int64_t* __restrict__ sufv, uint32_t* __restrict__ sufc) {
  gc_carry_scan<GC_SUM_I>(ntiles, offs, sufv, sufc);
}

template <uint32_t OP>
HDK_DEV bool so_keeps(bool valid, bool left, uint32_t rb, uint32_t lb) {
  if constexpr (OP == HDK_SETOP_UNION) return valid && rb + lb == 0;
  if constexpr (OP == HDK_SETOP_INTERSECT) return left && lb == 0 && rb > 0;
  if constexpr (OP == HDK_SETOP_INTERSECT_ALL) return left && lb < rb;
  if constexpr (OP == HDK_SETOP_EXCEPT) return left && lb == 0 && rb == 0;
  return left && lb >= rb;  // HDK_SETOP_EXCEPT_ALL
}

// The walk of one wave over its 16 items in row order: (cr, cl) are the right and left rows of the run that is open where
// item j begins (wave-uniform); a lane without a tail before it in its item adds them to what its item holds before it.
// -> the wave's kept rows; masks[j] = the keep mask of item j.
template <uint32_t OP>
HDK_DEV uint32_t so_walk(uint32_t tails, uint32_t right, uint32_t left, uint32_t lane, uint32_t cr, uint32_t cl,
                         uint64_t* __restrict__ masks) {
  uint32_t kept = 0;
  const uint64_t lower = (uint64_t(1) << lane) - 1;  // the lanes before this one
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    const uint64_t mj = gc_item_tails(tails, j);
    const uint64_t tj = __builtin_amdgcn_ballot_w64((right >> j) & 1u);
    const uint64_t lj = __builtin_amdgcn_ballot_w64((left >> j) & 1u);
    const uint64_t below = mj & lower;  // the tails before this lane
    const uint32_t s = below ? 64u - static_cast<uint32_t>(__clzll(static_cast<long long>(below))) : 0u;  // where this lane's run starts
    const uint64_t range = lower & (~uint64_t(0) << s);  // lanes s .. lane - 1
    uint32_t rb = static_cast<uint32_t>(__popcll(tj & range));
    uint32_t lb = static_cast<uint32_t>(__popcll(lj & range));
    if (below == 0) {  // the run reaches back into the item before
      rb += cr;
      lb += cl;
    }
    const bool is_left = (left >> j) & 1u;
    const bool valid = is_left || ((right >> j) & 1u);
    const uint64_t km = __builtin_amdgcn_ballot_w64(so_keeps<OP>(valid, is_left, rb, lb));
    if (lane == 0) {
      masks[j] = km;
    }
    kept += static_cast<uint32_t>(__popcll(km));
    const uint64_t sm = so_behind(mj);
    cr = (mj ? 0u : cr) + static_cast<uint32_t>(__popcll(tj & sm));
    cl = (mj ? 0u : cl) + static_cast<uint32_t>(__popcll(lj & sm));
  }
  return kept;
}

__global__ __launch_bounds__(kGcBlock) void hdk_setop_keep(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, SoDesc d,
                                                            uint32_t ntiles, const int64_t* __restrict__ carv,
                                                            uint64_t* __restrict__ masks, uint32_t* __restrict__ tile_kept) {
  __shared__ uint32_t s_wave[kGcWaves];
  __shared__ int64_t s_v[kGcWaves];
  __shared__ uint32_t s_t[kGcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t* tag = cols + static_cast<uint64_t>(d.tag_col) * capacity;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t r0 = gc_row0(tile, wave, lane);
    const uint32_t tails = gc_tails(cols, capacity, n, d, r0, lane);
    // bit j: this lane's row of item j is there and a right (tag != 0) / left (tag == 0) row
    uint32_t right = 0, left = 0;
    {
      int64_t t[kGcItems];
#pragma unroll
      for (int j = 0; j < kGcItems; ++j) {
        const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
        t[j] = gc_load(tag + (r < n ? r : n - 1));
      }
#pragma unroll
      for (int j = 0; j < kGcItems; ++j) {
        const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
        right |= r < n && t[j] != 0 ? 1u << j : 0u;
        left |= r < n && t[j] == 0 ? 1u << j : 0u;
      }
    }
    // what this wave ends with: the rows behind its last tail
    uint32_t er = 0, el = 0;
    bool seen = false;
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      const uint64_t mj = gc_item_tails(tails, j);
      const uint64_t tj = __builtin_amdgcn_ballot_w64((right >> j) & 1u);
      const uint64_t lj = __builtin_amdgcn_ballot_w64((left >> j) & 1u);
      const uint64_t sm = so_behind(mj);
      er = (mj ? 0u : er) + static_cast<uint32_t>(__popcll(tj & sm));
      el = (mj ? 0u : el) + static_cast<uint32_t>(__popcll(lj & sm));
      seen = seen || mj != 0;
    }
    if (lane == 0) {
      s_v[wave] = so_pack(er, el);
      s_t[wave] = seen;
    }
    __syncthreads();
    // what enters this wave: the tile's carry through the waves before it
    int64_t in = carv[tile];
#pragma unroll
    for (int w = 0; w < kGcWaves - 1; ++w) {
      if (static_cast<uint32_t>(w) < wave) {
        in = s_t[w] ? s_v[w] : gc_combine<GC_SUM_I>(in, s_v[w]);
      }
    }
    const uint32_t cr = static_cast<uint32_t>(static_cast<uint64_t>(in) >> 32), cl = static_cast<uint32_t>(in);
    uint64_t* wm = masks + static_cast<uint64_t>(tile) * kSoWords + wave * kGcItems;
    uint32_t kept = 0;
    switch (d.op) {  // (wave-uniform: the description comes from scalar registers)
      case HDK_SETOP_UNION: kept = so_walk<HDK_SETOP_UNION>(tails, right, left, lane, cr, cl, wm); break;
      case HDK_SETOP_INTERSECT: kept = so_walk<HDK_SETOP_INTERSECT>(tails, right, left, lane, cr, cl, wm); break;
      case HDK_SETOP_INTERSECT_ALL: kept = so_walk<HDK_SETOP_INTERSECT_ALL>(tails, right, left, lane, cr, cl, wm); break;
      case HDK_SETOP_EXCEPT: kept = so_walk<HDK_SETOP_EXCEPT>(tails, right, left, lane, cr, cl, wm); break;
      default: kept = so_walk<HDK_SETOP_EXCEPT_ALL>(tails, right, left, lane, cr, cl, wm); break;
    }
    block_store_tile_count(s_wave, kept, tile_kept + tile);  // (its barriers also free s_v and s_t for the next tile)
  }
}

// (no ballot here: the keep masks come from the keep pass; every wave scans the tile's 64 words for itself)
__global__ __launch_bounds__(kGcBlock) void hdk_setop_compact(const int64_t* __restrict__ cols, uint64_t capacity, SoDesc d,
                                                               uint32_t ntiles, const uint32_t* __restrict__ tile_offs,
                                                               const uint64_t* __restrict__ masks, int64_t* __restrict__ out,
                                                               uint64_t out_capacity) {
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t first = tile_offs[tile];
    if (tile_offs[tile + 1] == first || first >= out_capacity) {
      continue;  // no kept row in this tile, or all of them past the capacity (block-uniform)
    }
    const uint64_t word = masks[static_cast<uint64_t>(tile) * kSoWords + lane];
    const uint32_t c = static_cast<uint32_t>(__popcll(word));
    const uint32_t excl = wave_inclusive_sum(c, lane) - c;
    const uint64_t r0 = static_cast<uint64_t>(tile) * kGcTile + wave * kGcWaveRows + lane;
    uint32_t flags = 0;
    uint64_t rank[kGcItems];
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      const uint32_t w = wave * kGcItems + static_cast<uint32_t>(j);
      const uint64_t mask = so_shfl64(word, w);
      const uint32_t before = __shfl(excl, static_cast<int>(w), kWave);
      rank[j] = static_cast<uint64_t>(first) + before + lane_rank(mask);
      const bool f = ((mask >> lane) & 1u) && rank[j] < out_capacity;
      flags |= static_cast<uint32_t>(f) << j;
    }
    for (uint32_t t = 0; t < d.nouts; ++t) {
      const int64_t* src = cols + static_cast<uint64_t>(d.out_col[t]) * capacity;
      int64_t* dst = out + static_cast<uint64_t>(t) * out_capacity;
      int64_t v[kGcItems];
#pragma unroll
      for (int j = 0; j < kGcItems; ++j) {
        v[j] = 0;
        if ((flags >> j) & 1u) {  // (a kept row is a row below n: the keep pass sets no other bit)
          v[j] = gc_load(src + r0 + static_cast<uint32_t>(j) * kWave);
        }
      }
#pragma unroll
      for (int j = 0; j < kGcItems; ++j) {
        if ((flags >> j) & 1u) {
          dst[rank[j]] = v[j];
        }
      }
    }
  }
}

// ---- UNION ALL ----

struct CcCol {
  uint32_t lcol, rcol;
  uint32_t lnullable, rnullable;
  int64_t lnull, rnull, out_null;
};

struct CcDesc {
  uint32_t ncols;
  int32_t side_col;          // < 0: none
  int64_t first_side_word;   // what the side column holds for a row of the first block; the second block's rows hold the other of 0 / 1
  CcCol col[HDK_HIP_MAX_SETOP_COLUMNS];
};

constexpr int kCcBlock = kTileBlock;
constexpr int kCcItems = 4;  // rows per thread and tile
constexpr uint32_t kCcTile = kCcBlock * kCcItems;

// Output row r is row r of the first block for r < nl and row r - nl of the second otherwise; consecutive lanes move
// consecutive rows.  (64-bit row arithmetic: nl + nr stays below 2^32, a tile's last row index may not.)
__global__ __launch_bounds__(kCcBlock) void hdk_concat_columns(const int64_t* __restrict__ lcols, uint64_t lcapacity, uint64_t nl,
                                                                const int64_t* __restrict__ rcols, uint64_t rcapacity, uint64_t total,
                                                                CcDesc d, uint32_t ntiles, int64_t* __restrict__ out,
                                                                uint64_t out_capacity) {
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t r0 = static_cast<uint64_t>(tile) * kCcTile + threadIdx.x;
    for (uint32_t c = 0; c < d.ncols; ++c) {  // (wave-uniform: the description comes from scalar registers)
      const CcCol q = d.col[c];
      const int64_t* lsrc = lcols + static_cast<uint64_t>(q.lcol) * lcapacity;
      const int64_t* rsrc = rcols + static_cast<uint64_t>(q.rcol) * rcapacity;
      const uint32_t oc = c + (d.side_col >= 0 && c >= static_cast<uint32_t>(d.side_col) ? 1u : 0u);
      int64_t* dst = out + static_cast<uint64_t>(oc) * out_capacity;
      int64_t v[kCcItems];
#pragma unroll
      for (int j = 0; j < kCcItems; ++j) {
        const uint64_t r = r0 + static_cast<uint32_t>(j) * kCcBlock;
        v[j] = 0;
        if (r < total) {
          const bool first = r < nl;
          const int64_t w = gc_load(first ? lsrc + r : rsrc + (r - nl));
          const bool is_null = first ? (q.lnullable && w == q.lnull) : (q.rnullable && w == q.rnull);
          v[j] = is_null ? q.out_null : w;
        }
      }
#pragma unroll
      for (int j = 0; j < kCcItems; ++j) {
        const uint64_t r = r0 + static_cast<uint32_t>(j) * kCcBlock;
        if (r < total) {
          dst[r] = v[j];
        }
      }
    }
    if (d.side_col >= 0) {
      int64_t* dst = out + static_cast<uint64_t>(d.side_col) * out_capacity;
#pragma unroll
      for (int j = 0; j < kCcItems; ++j) {
        const uint64_t r = r0 + static_cast<uint32_t>(j) * kCcBlock;
        if (r < total) {
          dst[r] = r < nl ? d.first_side_word : 1 - d.first_side_word;
        }
      }
    }
  }
}

static size_t so_tiles(uint64_t num_rows) { return static_cast<size_t>((num_rows + kGcTile - 1) / kGcTile); }
static size_t so_counts_bytes(size_t ntiles) { return align256((ntiles + 1) * sizeof(uint32_t)); }

}  // namespace hdk

using namespace hdk;

extern "C" int32_t hdk_hip_concat_columns(const int64_t* lcols, uint64_t lcapacity, int32_t lnum_cols, uint64_t lnum_rows,
                                          const int64_t* rcols, uint64_t rcapacity, int32_t rnum_cols, uint64_t rnum_rows,
                                          const hdk_hip_setop_col* pairs, int32_t num_cols, int32_t side_col, uint32_t flags,
                                          int64_t* out_cols, uint64_t out_capacity, int32_t device_id, void* stream) {
  HDK_REQUIRE(pairs && out_cols && (lcols || lnum_rows == 0) && (rcols || rnum_rows == 0),
              "hdk_hip_concat_columns: NULL argument (pairs and out_cols are required, and the columns of a side that has rows)");
  HDK_REQUIRE(lnum_cols >= 1 && rnum_cols >= 1, "hdk_hip_concat_columns: lnum_cols %d, rnum_cols %d", lnum_cols, rnum_cols);
  HDK_REQUIRE(num_cols >= 1 && num_cols <= HDK_HIP_MAX_SETOP_COLUMNS, "hdk_hip_concat_columns: num_cols %d outside 1..%d", num_cols,
              HDK_HIP_MAX_SETOP_COLUMNS);
  HDK_REQUIRE(side_col < 0 || side_col <= num_cols, "hdk_hip_concat_columns: side_col %d of %d output columns", side_col,
              num_cols + 1);
  HDK_REQUIRE((flags & ~HDK_HIP_CONCAT_TAG_FIRST) == 0, "hdk_hip_concat_columns: unknown flags 0x%x", flags);
  CcDesc d;
  memset(&d, 0, sizeof(d));
  d.ncols = static_cast<uint32_t>(num_cols);
  d.side_col = side_col < 0 ? -1 : side_col;
  d.first_side_word = (flags & HDK_HIP_CONCAT_TAG_FIRST) ? 1 : 0;
  for (int32_t i = 0; i < num_cols; ++i) {
    const hdk_hip_setop_col& p = pairs[i];
    HDK_REQUIRE(p.lcol >= 0 && p.lcol < lnum_cols, "hdk_hip_concat_columns: pair %d names column %d of %d (left)", i, p.lcol,
                lnum_cols);
    HDK_REQUIRE(p.rcol >= 0 && p.rcol < rnum_cols, "hdk_hip_concat_columns: pair %d names column %d of %d (right)", i, p.rcol,
                rnum_cols);
    CcCol& q = d.col[i];
    q.lcol = static_cast<uint32_t>(p.lcol);
    q.rcol = static_cast<uint32_t>(p.rcol);
    q.lnullable = p.lnullable ? 1u : 0u;
    q.rnullable = p.rnullable ? 1u : 0u;
    q.lnull = p.lnull_bits;
    q.rnull = p.rnull_bits;
    q.out_null = p.out_null_bits;
  }
  HDK_REQUIRE(lnum_rows < (uint64_t(1) << 32) && rnum_rows < (uint64_t(1) << 32) && lnum_rows + rnum_rows < (uint64_t(1) << 32),
              "hdk_hip_concat_columns: %llu + %llu rows do not fit 32-bit row indices", static_cast<unsigned long long>(lnum_rows),
              static_cast<unsigned long long>(rnum_rows));
  HDK_REQUIRE(lnum_rows <= lcapacity && rnum_rows <= rcapacity,
              "hdk_hip_concat_columns: rows %llu / %llu exceed the capacities %llu / %llu", static_cast<unsigned long long>(lnum_rows),
              static_cast<unsigned long long>(rnum_rows), static_cast<unsigned long long>(lcapacity),
              static_cast<unsigned long long>(rcapacity));
  const uint64_t total = lnum_rows + rnum_rows;
  HDK_REQUIRE(out_capacity >= total, "hdk_hip_concat_columns: out_capacity %llu below the %llu output rows",
              static_cast<unsigned long long>(out_capacity), static_cast<unsigned long long>(total));
  {
    const uint64_t out_ncols = static_cast<uint64_t>(num_cols) + (side_col >= 0 ? 1 : 0);
    const MemBlock blk[] = {
        {"lcols", reinterpret_cast<uintptr_t>(lcols), lnum_rows ? static_cast<uint64_t>(lnum_cols) * lcapacity * 8 : 0},
        {"rcols", reinterpret_cast<uintptr_t>(rcols), rnum_rows ? static_cast<uint64_t>(rnum_cols) * rcapacity * 8 : 0},
        {"out_cols", reinterpret_cast<uintptr_t>(out_cols), total ? out_ncols * out_capacity * 8 : 0},
    };
    // (the two inputs are only read: they may be the same block or share columns)
    HDK_REQUIRE(!blk[0].bytes || !blk[2].bytes || blk[0].at + blk[0].bytes <= blk[2].at || blk[2].at + blk[2].bytes <= blk[0].at,
                "hdk_hip_concat_columns: out_cols overlaps lcols");
    HDK_REQUIRE(!blk[1].bytes || !blk[2].bytes || blk[1].at + blk[1].bytes <= blk[2].at || blk[2].at + blk[2].bytes <= blk[1].at,
                "hdk_hip_concat_columns: out_cols overlaps rcols");
  }
  hipStream_t s;
  int32_t st = device_enter(device_id, stream, &s);
  if (st) return st;
  if (total == 0) {
    return HDK_HIP_OK;
  }
  const uint32_t ntiles = static_cast<uint32_t>((total + kCcTile - 1) / kCcTile);
  const dim3 grid(persistent_grid(device_props(device_id), ntiles)), block(kCcBlock);
  // a side without rows is never dereferenced; give its base a value the address arithmetic may use
  const int64_t* lbase = lnum_rows ? lcols : out_cols;
  const int64_t* rbase = rnum_rows ? rcols : out_cols;
  hipLaunchKernelGGL(hdk_concat_columns, grid, block, 0, s, lbase, lnum_rows ? lcapacity : 0, lnum_rows, rbase,
                     rnum_rows ? rcapacity : 0, total, d, ntiles, out_cols, out_capacity);
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}

// [tail counters + 1][kept counters + 1][ntiles packed suffixes][ntiles scan counts][64 keep masks per tile]
extern "C" size_t hdk_hip_setop_columns_workspace_bytes(uint64_t num_rows) {
  const size_t ntiles = so_tiles(num_rows);
  return 2 * so_counts_bytes(ntiles) + align256(ntiles * sizeof(int64_t)) + align256(ntiles * sizeof(uint32_t)) +
         ntiles * kSoWords * sizeof(uint64_t);
}

extern "C" int32_t hdk_hip_setop_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                                         const int32_t* key_cols, int32_t num_keys, int32_t tag_col, int32_t op,
                                         const int32_t* out_cols_idx, int32_t num_outs, int64_t* out_cols, uint64_t out_capacity,
                                         uint64_t* row_count, void* workspace, size_t workspace_bytes, int32_t device_id,
                                         void* stream) {
  HDK_REQUIRE(cols && key_cols && out_cols_idx && row_count,
              "hdk_hip_setop_columns: NULL argument (cols, key_cols, out_cols_idx and row_count are required)");
  HDK_REQUIRE(num_cols >= 1, "hdk_hip_setop_columns: num_cols %d", num_cols);
  HDK_REQUIRE(num_keys >= 1 && num_keys <= HDK_HIP_MAX_SETOP_COLUMNS, "hdk_hip_setop_columns: num_keys %d outside 1..%d", num_keys,
              HDK_HIP_MAX_SETOP_COLUMNS);
  HDK_REQUIRE(num_outs >= 1 && num_outs <= HDK_HIP_MAX_SETOP_OUTS, "hdk_hip_setop_columns: num_outs %d outside 1..%d", num_outs,
              HDK_HIP_MAX_SETOP_OUTS);
  HDK_REQUIRE(op >= HDK_SETOP_UNION && op <= HDK_SETOP_EXCEPT_ALL, "hdk_hip_setop_columns: op %d outside hdk_hip_setop", op);
  HDK_REQUIRE(tag_col >= 0 && tag_col < num_cols, "hdk_hip_setop_columns: tag_col names column %d of %d", tag_col, num_cols);
  SoDesc d;
  memset(&d, 0, sizeof(d));
  d.nkeys = static_cast<uint32_t>(num_keys);
  d.nouts = static_cast<uint32_t>(num_outs);
  d.tag_col = static_cast<uint32_t>(tag_col);
  d.op = static_cast<uint32_t>(op);
  for (int32_t k = 0; k < num_keys; ++k) {
    HDK_REQUIRE(key_cols[k] >= 0 && key_cols[k] < num_cols, "hdk_hip_setop_columns: key %d names column %d of %d", k, key_cols[k],
                num_cols);
    HDK_REQUIRE(key_cols[k] != tag_col, "hdk_hip_setop_columns: key %d is the tag column %d", k, tag_col);
    d.key_col[k] = static_cast<uint32_t>(key_cols[k]);
  }
  for (int32_t i = 0; i < num_outs; ++i) {
    HDK_REQUIRE(out_cols_idx[i] >= 0 && out_cols_idx[i] < num_cols, "hdk_hip_setop_columns: out %d names column %d of %d", i,
                out_cols_idx[i], num_cols);
    d.out_col[i] = static_cast<uint32_t>(out_cols_idx[i]);
  }
  HDK_REQUIRE(num_rows < (uint64_t(1) << 32), "hdk_hip_setop_columns: num_rows %llu does not fit 32-bit row indices",
              static_cast<unsigned long long>(num_rows));
  HDK_REQUIRE(num_rows <= capacity, "hdk_hip_setop_columns: num_rows %llu exceeds the capacity %llu",
              static_cast<unsigned long long>(num_rows), static_cast<unsigned long long>(capacity));
  const size_t need = hdk_hip_setop_columns_workspace_bytes(num_rows);
  HDK_REQUIRE(!workspace || workspace_bytes >= need, "hdk_hip_setop_columns: workspace of %zu bytes, %zu needed", workspace_bytes,
              need);
  HDK_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "hdk_hip_setop_columns: workspace %p is not 8-byte aligned",
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
    const int32_t bad = require_disjoint("hdk_hip_setop_columns", blk, sizeof(blk) / sizeof(blk[0]));
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
  const uint32_t ntiles = static_cast<uint32_t>(so_tiles(num_rows));
  int8_t* at = static_cast<int8_t*>(workspace);
  uint32_t* tails = reinterpret_cast<uint32_t*>(at);
  at += so_counts_bytes(ntiles);
  uint32_t* kept = reinterpret_cast<uint32_t*>(at);
  at += so_counts_bytes(ntiles);
  int64_t* sufv = reinterpret_cast<int64_t*>(at);
  at += align256(ntiles * sizeof(int64_t));
  uint32_t* sufc = reinterpret_cast<uint32_t*>(at);
  at += align256(ntiles * sizeof(uint32_t));
  uint64_t* masks = reinterpret_cast<uint64_t*>(at);
  const uint32_t n = static_cast<uint32_t>(num_rows);
  const dim3 grid(persistent_grid(device_props(device_id), ntiles)), block(kGcBlock);
  hipLaunchKernelGGL(hdk_setop_summary, grid, block, 0, s, cols, capacity, n, d, ntiles, tails, sufv, sufc);
  launch_counts_scan(tails, ntiles, kGcScanPer, nullptr, s);
  hipLaunchKernelGGL(hdk_setop_carry_scan, dim3(1), dim3(kGcCarryBlock), 0, s, ntiles, tails, sufv, sufc);
  hipLaunchKernelGGL(hdk_setop_keep, grid, block, 0, s, cols, capacity, n, d, ntiles, sufv, masks, kept);
  launch_counts_scan(kept, ntiles, kGcScanPer, row_count, s);
  if (writes) {
    hipLaunchKernelGGL(hdk_setop_compact, grid, block, 0, s, cols, capacity, d, ntiles, kept, masks, out_cols, out_capacity);
  }
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
