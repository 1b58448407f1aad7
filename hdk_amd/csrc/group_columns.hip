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
// Traffic for n rows, k key columns, a aggregated columns, r runs: count 8nk (+ the suffix items of the aggregated
// columns, at least one item per wave and column), reduce 8n(k + a) read + 8r per output written.
#include <string.h>

#include "column_primitives.h"
#include "host_common.h"

namespace hdk {

constexpr int kGcBlock = kTileBlock;
constexpr int kGcItems = 16;  // 64-row items per wave and tile
constexpr uint32_t kGcTile = kGcBlock * kGcItems;
constexpr int kGcWaves = kGcBlock / kWave;
constexpr uint32_t kGcWaveRows = kWave * kGcItems;  // rows of a tile that one wave owns
constexpr ScanPer kGcScanPer = SCAN_PER_4;
constexpr int kGcCarryBlock = 1024;
constexpr int kGcCarryPer = 4;
constexpr uint32_t kGcCarryTrip = kGcCarryBlock * kGcCarryPer;  // tiles per trip of the carry scan

enum GcOp : uint32_t { GC_ID, GC_COUNT_STAR, GC_COUNT, GC_SUM_I, GC_SUM_F, GC_MIN_I, GC_MIN_F, GC_MAX_I, GC_MAX_F };

struct GcOut {
  uint32_t col, op;
  uint32_t nullable, pad_;
  int64_t null_bits;
};

struct GcDesc {
  uint32_t nkeys, nouts;
  uint32_t key_col[HDK_HIP_MAX_GROUP_KEYS];
  GcOut out[HDK_HIP_MAX_GROUP_OUTS];
};

// the columns are read once per pass: every load is non-temporal
HDK_DEV int64_t gc_load(const int64_t* p) { return nt_load<int64_t>(p, 0); }

// the value a NULL word (or a row that is not there) enters a reduction with
template <uint32_t OP>
HDK_DEV int64_t gc_identity() {
  if constexpr (OP == GC_SUM_F) return double_to_bits(-0.0);  // (-0.0 + x == x for every x, +0.0 and -0.0 included)
  if constexpr (OP == GC_MIN_I) return INT64_MAX;
  if constexpr (OP == GC_MAX_I) return INT64_MIN;
  if constexpr (OP == GC_MIN_F) return double_to_bits(__builtin_huge_val());
  if constexpr (OP == GC_MAX_F) return double_to_bits(-__builtin_huge_val());
  return 0;
}

template <uint32_t OP>
HDK_DEV int64_t gc_combine(int64_t a, int64_t b) {
  if constexpr (OP == GC_SUM_I) return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(b));
  if constexpr (OP == GC_SUM_F) return double_to_bits(bits_to_double(a) + bits_to_double(b));
  if constexpr (OP == GC_MIN_I) return b < a ? b : a;
  if constexpr (OP == GC_MAX_I) return b > a ? b : a;
  if constexpr (OP == GC_MIN_F) return bits_to_double(b) < bits_to_double(a) ? b : a;
  if constexpr (OP == GC_MAX_F) return bits_to_double(b) > bits_to_double(a) ? b : a;
  return a;  // the counts: their value is the non-NULL count that travels beside
}

template <uint32_t OP>
constexpr bool gc_counts() {
  return OP == GC_COUNT_STAR || OP == GC_COUNT;
}

// the word a tail stores: the count, or the value when the run had one
template <uint32_t OP>
HDK_DEV int64_t gc_result(int64_t v, uint32_t c, int64_t null_bits) {
  if constexpr (gc_counts<OP>()) return static_cast<int64_t>(c);
  return c ? v : null_bits;
}

HDK_DEV int64_t gc_shfl_up(int64_t v, int d) { return __shfl_up(static_cast<long long>(v), static_cast<unsigned>(d), kWave); }
HDK_DEV int64_t gc_shfl_xor(int64_t v, int d) { return __shfl_xor(static_cast<long long>(v), d, kWave); }
HDK_DEV int64_t gc_lane63(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(v), kWave - 1);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32), kWave - 1);
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

// first row of this lane in `tile`; its item j is row + j * 64.  (tile * kGcTile + 4095 never exceeds 2^32 - 1:
// tile < ceil(n / kGcTile), n < 2^32.)
HDK_DEV uint32_t gc_row0(uint32_t tile, uint32_t wave, uint32_t lane) { return tile * kGcTile + wave * kGcWaveRows + lane; }

// Bit j: this lane's row of item j is a tail (every lane of the wave calls this).  The next row's key word comes from
// the next lane; lane 63 loads it.  One row past the tile is read, and row n is masked by value: row n - 1 is a tail
// whatever follows it in the capacity.  The flag word of item j is gc_item_tails(tails, j): a ballot, recomputed where
// it is needed instead of being held in 32 scalar registers.
HDK_DEV uint32_t gc_tails(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, const GcDesc& d, uint32_t r0,
                          uint32_t lane) {
  uint32_t differs = 0;
  for (uint32_t k = 0; k < d.nkeys; ++k) {  // (wave-uniform: the description comes from scalar registers)
    const int64_t* col = cols + static_cast<uint64_t>(d.key_col[k]) * capacity;
    int64_t a[kGcItems], b[kGcItems];
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      // (a row past the end reads the last row instead, so that the loads of a tile are issued together)
      const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
      a[j] = gc_load(col + (r < n ? r : n - 1));
    }
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
      b[j] = 0;
      if (lane == kWave - 1) {
        b[j] = gc_load(col + (r < n - 1 ? r + 1 : n - 1));
      }
    }
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      const int64_t down = __shfl_down(static_cast<long long>(a[j]), 1u, kWave);
      const int64_t next = lane == kWave - 1 ? b[j] : down;
      differs |= a[j] != next ? 1u << j : 0u;
    }
  }
  uint32_t tails = 0;
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
    tails |= r < n && (r == n - 1 || ((differs >> j) & 1u)) ? 1u << j : 0u;
  }
  return tails;
}

// the tails among the 64 rows of this wave's item j (all 64 lanes call this together)
HDK_DEV uint64_t gc_item_tails(uint32_t tails, int j) { return __builtin_amdgcn_ballot_w64((tails >> j) & 1u); }

HDK_DEV uint32_t gc_count_tails(uint32_t tails) {  // of the wave
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    c += static_cast<uint32_t>(__popcll(gc_item_tails(tails, j)));
  }
  return c;
}

// The open suffix of one aggregate over one tile -> sufv[tile], sufc[tile]: a masked reduction.  Per wave the rows after
// its last tail (items without such a row are not loaded), the four waves combined in order by thread 0.
template <uint32_t OP>
HDK_DEV void gc_open_suffix(const int64_t* __restrict__ col, uint32_t n, const GcOut& o, uint32_t r0, uint32_t lane, uint32_t wave,
                            uint32_t tails, int64_t (&s_v)[kGcWaves], uint32_t (&s_c)[kGcWaves],
                            uint32_t (&s_t)[kGcWaves], int64_t* __restrict__ sufv, uint32_t* __restrict__ sufc) {
  uint32_t any = 0;  // bit j: item j holds a tail
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    any |= gc_item_tails(tails, j) ? 1u << j : 0u;
  }
  int64_t x = gc_identity<OP>();
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    // the lanes of item j behind the wave's last tail
    uint64_t sm = 0;
    if ((any >> j) <= 1u) {  // no tail in a later item
      sm = ~uint64_t(0);
      const uint64_t mj = gc_item_tails(tails, j);
      if (mj) {
        const int hb = 63 - __clzll(static_cast<long long>(mj));
        sm = hb == 63 ? 0 : ~uint64_t(0) << (hb + 1);
      }
    }
    if (sm) {  // (wave-uniform: every ballot below runs with all 64 lanes)
      const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
      bool has = r < n && ((sm >> lane) & 1u);
      if constexpr (OP != GC_COUNT_STAR) {
        const int64_t w = gc_load(col + (r < n ? r : n - 1));
        has = has && !(o.nullable && w == o.null_bits);
        x = has ? gc_combine<OP>(x, w) : x;
      }
      c += static_cast<uint32_t>(__popcll(__builtin_amdgcn_ballot_w64(has)));
    }
  }
  if constexpr (!gc_counts<OP>()) {
#pragma unroll
    for (int dd = kWave / 2; dd > 0; dd >>= 1) {
      x = gc_combine<OP>(x, gc_shfl_xor(x, dd));
    }
  }
  if (lane == 0) {
    s_v[wave] = x;
    s_c[wave] = c;
    s_t[wave] = any;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t v = gc_identity<OP>();
    uint32_t cc = 0;
#pragma unroll
    for (int w = 0; w < kGcWaves; ++w) {
      v = s_t[w] ? s_v[w] : gc_combine<OP>(v, s_v[w]);
      cc = s_t[w] ? s_c[w] : cc + s_c[w];
    }
    *sufv = v;
    *sufc = cc;
  }
  __syncthreads();
}

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

// One block per aggregate: suffix[t] -> carry_in[t] in place, a segmented exclusive scan.  The elements are (has_tail,
// value, count) and the operator (f1, x1) . (f2, x2) = (f1 | f2, f2 ? x2 : combine(x1, x2)) is associative, so a thread
// folds its kGcCarryPer tiles, the wave scans the threads, the waves are chained through LDS and the carry goes from trip
// to trip.  has_tail[t] is offs[t + 1] != offs[t] of the scanned counters.
template <uint32_t OP>
HDK_DEV void gc_carry_scan(uint32_t ntiles, const uint32_t* __restrict__ offs, int64_t* __restrict__ v, uint32_t* __restrict__ c) {
  constexpr int kWaves = kGcCarryBlock / kWave;
  __shared__ int64_t s_v[kWaves];
  __shared__ uint32_t s_c[kWaves], s_f[kWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int64_t carry_v = gc_identity<OP>();
  uint32_t carry_c = 0;
  for (uint32_t base = 0; base < ntiles; base += kGcCarryTrip) {
    const uint32_t i0 = base + threadIdx.x * kGcCarryPer;
    int64_t ev[kGcCarryPer];
    uint32_t ec[kGcCarryPer];
    bool ef[kGcCarryPer];
    int64_t tv = gc_identity<OP>();
    uint32_t tc = 0;
    bool tf = false;
#pragma unroll
    for (int k = 0; k < kGcCarryPer; ++k) {
      const uint32_t i = i0 + k;
      const bool in = i < ntiles;
      ev[k] = in ? v[i] : gc_identity<OP>();
      ec[k] = in ? c[i] : 0;
      ef[k] = in && offs[i + 1] != offs[i];
      tv = ef[k] ? ev[k] : gc_combine<OP>(tv, ev[k]);
      tc = ef[k] ? ec[k] : tc + ec[k];
      tf = tf || ef[k];
    }
    int64_t iv = tv;
    uint32_t ic = tc;
    bool fl = tf;
#pragma unroll
    for (int dd = 1; dd < kWave; dd <<= 1) {
      const int64_t uv = gc_shfl_up(iv, dd);
      const uint32_t uc = __shfl_up(ic, static_cast<unsigned>(dd), kWave);
      const int uf = __shfl_up(static_cast<int>(fl), static_cast<unsigned>(dd), kWave);
      if (lane >= static_cast<uint32_t>(dd)) {
        iv = fl ? iv : gc_combine<OP>(uv, iv);
        ic = fl ? ic : uc + ic;
        fl = fl || uf;
      }
    }
    if (lane == kWave - 1) {
      s_v[wave] = iv;
      s_c[wave] = ic;
      s_f[wave] = fl;
    }
    __syncthreads();
    // what enters this wave, and what leaves the trip
    int64_t pv = carry_v, nv = carry_v;
    uint32_t pc = carry_c, nc = carry_c;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int64_t wv = s_f[w] ? s_v[w] : gc_combine<OP>(nv, s_v[w]);
      const uint32_t wc = s_f[w] ? s_c[w] : nc + s_c[w];
      nv = wv;
      nc = wc;
      if (static_cast<uint32_t>(w) < wave) {
        pv = wv;
        pc = wc;
      }
    }
    // what enters this thread: the wave's, through the threads before it
    int64_t xv = gc_shfl_up(iv, 1);
    uint32_t xc = __shfl_up(ic, 1u, kWave);
    int xf = __shfl_up(static_cast<int>(fl), 1u, kWave);
    if (lane == 0) {
      xv = gc_identity<OP>();
      xc = 0;
      xf = 0;
    }
    int64_t rv = xf ? xv : gc_combine<OP>(pv, xv);
    uint32_t rc = xf ? xc : pc + xc;
#pragma unroll
    for (int k = 0; k < kGcCarryPer; ++k) {
      const uint32_t i = i0 + k;
      if (i < ntiles) {
        v[i] = rv;
        c[i] = rc;
      }
      rv = ef[k] ? ev[k] : gc_combine<OP>(rv, ev[k]);
      rc = ef[k] ? ec[k] : rc + ec[k];
    }
    carry_v = nv;
    carry_c = nc;
    __syncthreads();
  }
}

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
    if (lane == 0) {
      s_wave[wave] = wave_tails;
    }
    __syncthreads();
    uint64_t base = first;
#pragma unroll
    for (int w = 0; w < kGcWaves - 1; ++w) {
      base += static_cast<uint32_t>(w) < wave ? s_wave[w] : 0u;
    }
    __syncthreads();
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
