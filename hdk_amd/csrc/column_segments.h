// column_segments.h -- the segmented walk over dense 8-byte columns that group_columns.hip (one word per run) and
// window_columns.hip (one word per row) share: the tile geometry, tail detection, the operators with their identities,
// the open suffix of a tile and the carry scan over the tiles.
//
// A row is a TAIL when it is the last row or when some key word differs from the next row's.  Row layout: wave w of a
// block owns rows [w * 1024, (w + 1) * 1024) of its tile and its item j the 64 consecutive rows from w * 1024 + j * 64,
// so a ballot is the flag word of those rows and rows follow each other lane by lane, item by item, wave by wave.
// "No value yet": beside every accumulator travels the number of non-NULL words it has seen (for COUNT that number IS
// the value).  NULL words enter a reduction as the operator's identity; the count goes through every combine step.
#pragma once
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

// Bit j: some word of the key columns `keys` (a structure with nkeys and key_col[]) differs between this lane's row of
// item j and the row after it (every lane of the wave calls this).  The next row's key word comes from the next lane;
// lane 63 loads it.  One row past the tile is read; rows at and beyond n read row n - 1.
template <class Keys>
HDK_DEV uint32_t gc_differs(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, const Keys& keys, uint32_t r0,
                            uint32_t lane) {
  uint32_t differs = 0;
  for (uint32_t k = 0; k < keys.nkeys; ++k) {  // (wave-uniform: the description comes from scalar registers)
    const int64_t* col = cols + static_cast<uint64_t>(keys.key_col[k]) * capacity;
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
  return differs;
}

// Bit j: this lane's row of item j is a tail.  Row n is masked by value: row n - 1 is a tail whatever follows it in
// the capacity.
HDK_DEV uint32_t gc_tails_of(uint32_t differs, uint32_t n, uint32_t r0) {
  uint32_t tails = 0;
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
    tails |= r < n && (r == n - 1 || ((differs >> j) & 1u)) ? 1u << j : 0u;
  }
  return tails;
}

// The flag word of item j is gc_item_tails(tails, j): a ballot, recomputed where it is needed instead of being held in
// 32 scalar registers.
template <class Keys>
HDK_DEV uint32_t gc_tails(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, const Keys& keys, uint32_t r0,
                          uint32_t lane) {
  return gc_tails_of(gc_differs(cols, capacity, n, keys, r0, lane), n, r0);
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

// the output row (or directory slot) of this wave's first tail: the tile's offset plus the tails of the waves before
// (every thread calls this; s_wave is free again when it returns)
HDK_DEV uint64_t gc_wave_base(uint32_t (&s_wave)[kGcWaves], uint32_t first, uint32_t wave_tails, uint32_t lane, uint32_t wave) {
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
  return base;
}

// the aggregate operators: `case OP: ...` for each through HDK_GC_CASE, which the caller defines around the use
#define HDK_GC_AGG_CASES       \
  HDK_GC_CASE(GC_COUNT_STAR)   \
  HDK_GC_CASE(GC_COUNT)        \
  HDK_GC_CASE(GC_SUM_I)        \
  HDK_GC_CASE(GC_SUM_F)        \
  HDK_GC_CASE(GC_MIN_I)        \
  HDK_GC_CASE(GC_MIN_F)        \
  HDK_GC_CASE(GC_MAX_I)        \
  HDK_GC_CASE(GC_MAX_F)

}  // namespace hdk
