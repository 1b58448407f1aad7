// key_multiplicity.hip -- the key multiplicity of a join key over dense 8-byte columns: what the planner needs to know of
// an INNER table before it names the join table's kind (one-to-one or one-to-many) and sizes a projection's buffer.
//
//   hdk_hip_key_multiplicity   files every row exactly as the join builds will (join_build.hip) and leaves
//                              {max_matches, occupied, rows_filed, rows_out_of_range} in one 32-byte record.
//
// Perfect route (one key, entry_count > 0): a histogram of 32-bit counters, one per slot of the perfect table, zeroed on
// the stream; one streaming pass over tiles of 4 096 rows with one non-returning atomic add per filed row -- or ONE add
// of the lane count for a wave item whose filing lanes all name the same slot --; a pass over the histogram (registers
// -> wave reduction -> LDS -> one partial per block); a fold.  No atomics on the record, no host wait.
// Sorted route (entry_count == 0): the library's own sort on the key columns, then the longest run over the sorted keys
// on column_segments.h's tile geometry: one summary per tile, folded with an associative combine.
#include <string.h>

#include "column_segments.h"

namespace hdk {

constexpr int kKmBlock = kTileBlock;
constexpr int kKmItems = 16;  // rows per thread and tile
constexpr uint32_t kKmTile = kKmBlock * kKmItems;
constexpr uint32_t kKmGridMax = 2048;  // blocks of either pass: the workspace holds one partial per block and pass
constexpr int kKmFoldBlock = 256;

static_assert(sizeof(hdk_hip_key_multiplicity_result) == 32, "the result is one 32-byte record");
static_assert(kKmTile == kGcTile, "one tile size for both routes");

struct KmPartial {  // pass 1: {rows_filed, rows_out_of_range}; pass 2: {max_matches, occupied}
  uint64_t a, b;
};

struct KmKey {
  uint32_t col;
  uint32_t nullable;
  int64_t null_bits, min_val, max_val, translated_null;
};

HDK_DEV uint64_t km_wave_sum(uint64_t v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    v += __shfl_xor(static_cast<unsigned long long>(v), d, kWave);
  }
  return v;
}
HDK_DEV uint64_t km_wave_max(uint64_t v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    const uint64_t o = __shfl_xor(static_cast<unsigned long long>(v), d, kWave);
    v = o > v ? o : v;
  }
  return v;
}

// (a, b) of the block's threads -> *out: a summed, b summed or (MAX_A) a maximised
template <bool MAX_A>
HDK_DEV void km_block_partial(uint64_t a, uint64_t b, KmPartial* out) {
  __shared__ uint64_t s_a[kTileWaves], s_b[kTileWaves];
  a = MAX_A ? km_wave_max(a) : km_wave_sum(a);
  b = km_wave_sum(b);
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
    s_a[wave] = a;
    s_b[wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    KmPartial p = {s_a[0], s_b[0]};
#pragma unroll
    for (int w = 1; w < kTileWaves; ++w) {
      p.a = MAX_A ? (s_a[w] > p.a ? s_a[w] : p.a) : p.a + s_a[w];
      p.b += s_b[w];
    }
    *out = p;
  }
}

// ---- perfect route -------------------------------------------------------------------------------------------------------
// Files the rows as fill_hash_join_buff_impl does: a NULL word is dropped, or with NULLS_MATCH filed under translated_null;
// a non-NULL word outside [min_val, max_val] or a slot at or beyond entry_count is out of range (the builds' -2).
// hist[slot] += 1 per filed row; part[blockIdx.x] = {rows filed, rows out of range} of the block's tiles.
template <bool BUCKET>
__global__ __launch_bounds__(kKmBlock) void hdk_key_histogram(const int64_t* __restrict__ col, uint64_t num_rows, uint32_t ntiles,
                                                               KmKey k, uint64_t entry_count, uint64_t bucket, uint32_t nulls_match,
                                                               uint32_t* __restrict__ hist, KmPartial* __restrict__ part) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  uint64_t filed = 0, outside = 0;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t r0 = static_cast<uint64_t>(tile) * kKmTile;
    const uint64_t end = r0 + kKmTile < num_rows ? r0 + kKmTile : num_rows;
    int64_t v[kKmItems];
#pragma unroll
    for (int j = 0; j < kKmItems; ++j) {
      const uint64_t r = r0 + threadIdx.x + static_cast<uint32_t>(j) * kKmBlock;
      v[j] = nt_load<int64_t>(col + (r < end ? r : end - 1), 0);  // (a tile has a row; a lane past it re-reads the last)
    }
#pragma unroll
    for (int j = 0; j < kKmItems; ++j) {
      const uint64_t r = r0 + threadIdx.x + static_cast<uint32_t>(j) * kKmBlock;
      const bool live = r < end;
      const bool is_null = k.nullable && v[j] == k.null_bits;
      const int64_t elem = is_null ? k.translated_null : v[j];
      const bool in_range = is_null ? nulls_match != 0 : (elem >= k.min_val && elem <= k.max_val);
      uint64_t s = static_cast<uint64_t>(elem) - static_cast<uint64_t>(k.min_val);
      // (a translated NULL below min_val wraps to a huge slot and is out of range, as in the builds)
      if (BUCKET) {
        s /= bucket;
      }
      const bool dropped = is_null && !nulls_match;
      const bool files = live && in_range && s < entry_count;
      outside += live && !dropped && !files ? 1u : 0u;
      filed += files ? 1u : 0u;
      // One hot slot must not serialise the chip: when every filing lane of the wave names the same slot, one lane adds
      // the lane count.  (All 64 lanes are here: the ballots and the readlane are wave-uniform.)
      const uint32_t slot = static_cast<uint32_t>(s);
      const uint64_t fm = __builtin_amdgcn_ballot_w64(files);
      if (fm) {
        const uint32_t lead = static_cast<uint32_t>(__ffsll(static_cast<long long>(fm)) - 1);
        const uint32_t s0 = __builtin_amdgcn_readlane(slot, lead);
        const uint64_t differ = __builtin_amdgcn_ballot_w64(files && slot != s0);
        if (differ == 0) {
          if (lane == lead) {
            atomicAdd(hist + s0, static_cast<uint32_t>(__popcll(fm)));
          }
        } else if (files) {
          atomicAdd(hist + slot, 1u);
        }
      }
    }
  }
  km_block_partial<false>(filed, outside, part + blockIdx.x);
}

// part[blockIdx.x] = {the largest counter, the counters that are not zero} of the block's share of the histogram
__global__ __launch_bounds__(kKmBlock) void hdk_key_histogram_reduce(const uint32_t* __restrict__ hist, uint64_t entry_count,
                                                                      KmPartial* __restrict__ part) {
  uint32_t mx = 0;
  uint64_t occupied = 0;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kKmBlock;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kKmBlock + threadIdx.x; i < entry_count; i += stride) {
    const uint32_t c = hist[i];
    mx = c > mx ? c : mx;
    occupied += c ? 1u : 0u;
  }
  km_block_partial<true>(mx, occupied, part + blockIdx.x);
}

// one block: the record from the partials of both passes
__global__ __launch_bounds__(kKmFoldBlock) void hdk_key_histogram_fold(const KmPartial* __restrict__ rows, uint32_t nrows,
                                                                        const KmPartial* __restrict__ slots, uint32_t nslots,
                                                                        hdk_hip_key_multiplicity_result* __restrict__ result) {
  __shared__ uint64_t s[4][kKmFoldBlock / kWave];
  uint64_t filed = 0, outside = 0, mx = 0, occupied = 0;
  for (uint32_t i = threadIdx.x; i < nrows; i += kKmFoldBlock) {
    filed += rows[i].a;
    outside += rows[i].b;
  }
  for (uint32_t i = threadIdx.x; i < nslots; i += kKmFoldBlock) {
    mx = slots[i].a > mx ? slots[i].a : mx;
    occupied += slots[i].b;
  }
  filed = km_wave_sum(filed);
  outside = km_wave_sum(outside);
  mx = km_wave_max(mx);
  occupied = km_wave_sum(occupied);
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
    s[0][wave] = mx;
    s[1][wave] = occupied;
    s[2][wave] = filed;
    s[3][wave] = outside;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    hdk_hip_key_multiplicity_result r = {0, 0, 0, 0};
    for (int w = 0; w < kKmFoldBlock / kWave; ++w) {
      r.max_matches = s[0][w] > r.max_matches ? s[0][w] : r.max_matches;
      r.occupied += s[1][w];
      r.rows_filed += s[2][w];
      r.rows_out_of_range += s[3][w];
    }
    *result = r;
  }
}

// ---- sorted route --------------------------------------------------------------------------------------------------------
// The summary of a stretch of rows.  A run ends at a TAIL; its weight is the number of its rows, or 0 when they carry a
// NULL component.  all_one: the stretch holds no tail and `lead` is the weight of all its rows.  Otherwise `lead` is the
// weight of the rows up to the first tail (the end of a run that may have begun earlier), `trail` that of the rows behind
// the last tail (a run that is still open), `best` the heaviest and `closed` the number of weight > 0 among the runs that
// begin and end inside the stretch.  `filed` is the weight of all rows.
struct KmRuns {
  uint32_t lead, trail, best, closed;
  uint32_t filed, all_one;
  uint32_t pad_[2];
};
static_assert(sizeof(KmRuns) == 32, "a tile summary is one 32-byte record");

// a followed by b; associative
HDK_DEV KmRuns km_combine(const KmRuns& a, const KmRuns& b) {
  KmRuns r;
  r.pad_[0] = r.pad_[1] = 0;
  r.filed = a.filed + b.filed;
  if (a.all_one) {
    r = b;
    r.filed = a.filed + b.filed;
    r.lead = a.lead + b.lead;
    r.trail = b.all_one ? r.lead : b.trail;
    return r;
  }
  if (b.all_one) {
    r = a;
    r.filed = a.filed + b.filed;
    r.trail = a.trail + b.lead;
    return r;
  }
  const uint32_t mid = a.trail + b.lead;  // the run that a left open and b ends
  const uint32_t ab = a.best > b.best ? a.best : b.best;
  r.lead = a.lead;
  r.trail = b.trail;
  r.best = mid > ab ? mid : ab;
  r.closed = a.closed + b.closed + (mid ? 1u : 0u);
  r.all_one = 0;
  return r;
}

HDK_DEV KmRuns km_no_rows() {
  KmRuns r;
  memset(&r, 0, sizeof(r));
  r.all_one = 1;
  return r;
}

struct KmKeys {
  uint32_t nkeys;
  uint32_t key_col[HDK_HIP_MAX_JOIN_KEYS];
  uint32_t nullable[HDK_HIP_MAX_JOIN_KEYS];
  int64_t null_bits[HDK_HIP_MAX_JOIN_KEYS];
};

// gc_differs (column_segments.h) with the NULL test on the words it has loaded anyway: bit j of `differs` as there, bit j
// of `nulls`: this lane's row of item j holds a NULL in some component
HDK_DEV void km_differs_and_nulls(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, const KmKeys& keys, uint32_t r0,
                                  uint32_t lane, uint32_t& differs, uint32_t& nulls) {
  differs = 0;
  nulls = 0;
  for (uint32_t k = 0; k < keys.nkeys; ++k) {  // (wave-uniform: the description comes from scalar registers)
    const int64_t* col = cols + static_cast<uint64_t>(keys.key_col[k]) * capacity;
    int64_t a[kGcItems], b[kGcItems];
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
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
      nulls |= keys.nullable[k] && a[j] == keys.null_bits[k] ? 1u << j : 0u;
    }
  }
}

// the lanes 0 .. l of a 64-bit flag word
HDK_DEV uint64_t km_through(uint32_t l) { return (uint64_t(2) << l) - 1; }  // (l == 63: 0 - 1, every lane)

// sums[tile] = the summary of the tile's rows.  A wave walks its 16 items of 64 consecutive rows: the run that an item's
// first tail ends and the rows behind its last tail are wave-uniform arithmetic on the two ballots; every other tail lane
// weighs its own run, which lies inside the item, from the same ballots.
__global__ __launch_bounds__(kGcBlock) void hdk_key_runs(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n,
                                                          uint32_t ntiles, KmKeys keys, KmRuns* __restrict__ sums) {
  __shared__ KmRuns s_wave[kGcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t r0 = gc_row0(tile, wave, lane);
    uint32_t differs, nulls;
    km_differs_and_nulls(cols, capacity, n, keys, r0, lane, differs, nulls);
    const uint32_t tails = gc_tails_of(differs, n, r0);
    uint32_t open = 0;  // the weight of the rows since the last tail
    bool seen = false;  // a tail so far
    uint32_t lead = 0, best = 0, closed = 0, filed = 0;
    uint32_t my_best = 0, my_closed = 0;
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
      const bool tail = (tails >> j) & 1u;
      const uint64_t m = __builtin_amdgcn_ballot_w64(tail);
      const uint64_t v = __builtin_amdgcn_ballot_w64(r < n && !((nulls >> j) & 1u));
      filed += static_cast<uint32_t>(__popcll(v));
      if (m == 0) {
        open += static_cast<uint32_t>(__popcll(v));
        continue;
      }
      const uint32_t first = static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
      const uint32_t last = 63u - static_cast<uint32_t>(__clzll(static_cast<long long>(m)));
      const uint32_t w = open + static_cast<uint32_t>(__popcll(v & km_through(first)));
      if (!seen) {
        lead = w;
        seen = true;
      } else {
        best = w > best ? w : best;
        closed += w ? 1u : 0u;
      }
      open = static_cast<uint32_t>(__popcll(v & ~km_through(last)));
      if (tail && lane != first) {  // the run (previous tail, this lane]
        const uint64_t below = m & (km_through(lane) >> 1);
        const uint32_t prev = 63u - static_cast<uint32_t>(__clzll(static_cast<long long>(below)));
        const uint32_t mine = static_cast<uint32_t>(__popcll(v & km_through(lane) & ~km_through(prev)));
        my_best = mine > my_best ? mine : my_best;
        my_closed += mine ? 1u : 0u;
      }
    }
    my_best = static_cast<uint32_t>(km_wave_max(my_best));
    my_closed = static_cast<uint32_t>(km_wave_sum(my_closed));
    if (lane == 0) {
      KmRuns s;
      s.pad_[0] = s.pad_[1] = 0;
      s.all_one = seen ? 0u : 1u;
      s.lead = seen ? lead : open;
      s.trail = open;
      s.best = my_best > best ? my_best : best;
      s.closed = closed + my_closed;
      s.filed = filed;
      s_wave[wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      KmRuns t = s_wave[0];
#pragma unroll
      for (int w = 1; w < kGcWaves; ++w) {
        t = km_combine(t, s_wave[w]);
      }
      sums[tile] = t;
    }
    __syncthreads();
  }
}

// one block: thread t folds a contiguous stretch of the tile summaries, thread 0 the 256 results in order.  The last row
// is a tail, so nothing stays open: the leading run and the closed ones are all there is.
__global__ __launch_bounds__(kKmFoldBlock) void hdk_key_runs_fold(const KmRuns* __restrict__ sums, uint32_t ntiles,
                                                                   hdk_hip_key_multiplicity_result* __restrict__ result) {
  __shared__ KmRuns s[kKmFoldBlock];
  const uint32_t per = (ntiles + kKmFoldBlock - 1) / kKmFoldBlock;
  const uint64_t t0 = static_cast<uint64_t>(threadIdx.x) * per;
  const uint64_t t1 = t0 + per < ntiles ? t0 + per : ntiles;
  KmRuns acc = km_no_rows();
  for (uint64_t t = t0; t < t1; ++t) {
    acc = km_combine(acc, sums[t]);
  }
  s[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    KmRuns f = s[0];
    for (int t = 1; t < kKmFoldBlock; ++t) {
      f = km_combine(f, s[t]);
    }
    hdk_hip_key_multiplicity_result r;
    r.max_matches = f.lead > f.best ? f.lead : f.best;
    r.occupied = static_cast<uint64_t>(f.closed) + (f.lead ? 1u : 0u);
    r.rows_filed = f.filed;
    r.rows_out_of_range = 0;
    *result = r;
  }
}

static uint64_t km_tiles(uint64_t rows) { return (rows + kKmTile - 1) / kKmTile; }
// the rows of a column of the sorted temporary: columns start 256-byte aligned
static uint64_t km_sorted_capacity(uint64_t rows) { return (rows + 31) / 32 * 32; }

// the parts of the sorted route's workspace, in order: sorted columns | the sort's workspace | tile summaries
struct KmSortedParts {
  size_t sorted_bytes, sort_bytes, sums_bytes;
  size_t total() const { return sorted_bytes + sort_bytes + sums_bytes; }
};
static KmSortedParts km_sorted_parts(uint64_t num_rows, int32_t sort_cols, int32_t num_keys) {
  KmSortedParts p;
  p.sorted_bytes = align256(static_cast<size_t>(sort_cols) * km_sorted_capacity(num_rows) * 8);
  p.sort_bytes = align256(hdk_hip_sort_columns_workspace_bytes(num_rows, num_keys));
  p.sums_bytes = align256(km_tiles(num_rows) * sizeof(KmRuns));
  return p;
}

static size_t km_workspace_bytes(uint64_t num_rows, int32_t sort_cols, int32_t num_keys, int64_t entry_count) {
  if (num_rows == 0) return 0;
  if (entry_count > 0) {
    return align256(static_cast<size_t>(entry_count) * 4) + 2 * kKmGridMax * sizeof(KmPartial);
  }
  return km_sorted_parts(num_rows, sort_cols, num_keys).total();
}

}  // namespace hdk

using namespace hdk;

extern "C" size_t hdk_hip_key_multiplicity_workspace_bytes(uint64_t num_rows, const hdk_hip_multiplicity_key* keys, int32_t num_keys,
                                                           int64_t entry_count) {
  if (!keys || num_keys < 1 || num_keys > HDK_HIP_MAX_JOIN_KEYS || entry_count < 0 || (entry_count > 0 && num_keys != 1)) return 0;
  int32_t sort_cols = 0;
  for (int32_t i = 0; i < num_keys; ++i) {
    if (keys[i].col < 0) return 0;
    sort_cols = keys[i].col + 1 > sort_cols ? keys[i].col + 1 : sort_cols;
  }
  return km_workspace_bytes(num_rows, sort_cols, num_keys, entry_count);
}

extern "C" int32_t hdk_hip_key_multiplicity(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                                            const hdk_hip_multiplicity_key* keys, int32_t num_keys, int64_t entry_count,
                                            int64_t bucket, uint32_t flags, hdk_hip_key_multiplicity_result* result, void* workspace,
                                            size_t workspace_bytes, int32_t device_id, void* stream) {
  HDK_REQUIRE(keys && result && (cols || num_rows == 0),
              "hdk_hip_key_multiplicity: NULL argument (keys and result are required, and cols when there are rows)");
  HDK_REQUIRE(num_keys >= 1 && num_keys <= HDK_HIP_MAX_JOIN_KEYS, "hdk_hip_key_multiplicity: num_keys %d outside 1..%d", num_keys,
              HDK_HIP_MAX_JOIN_KEYS);
  int32_t sort_cols = 0;
  for (int32_t i = 0; i < num_keys; ++i) {
    HDK_REQUIRE(keys[i].col >= 0 && keys[i].col < num_cols, "hdk_hip_key_multiplicity: key %d names column %d of %d", i, keys[i].col,
                num_cols);
    sort_cols = keys[i].col + 1 > sort_cols ? keys[i].col + 1 : sort_cols;
  }
  HDK_REQUIRE(num_rows < (uint64_t(1) << 32), "hdk_hip_key_multiplicity: num_rows %llu does not fit 32-bit row indices",
              static_cast<unsigned long long>(num_rows));
  HDK_REQUIRE(num_rows <= capacity, "hdk_hip_key_multiplicity: num_rows %llu exceeds the capacity %llu",
              static_cast<unsigned long long>(num_rows), static_cast<unsigned long long>(capacity));
  HDK_REQUIRE(entry_count >= 0 && entry_count <= INT32_MAX,
              "hdk_hip_key_multiplicity: entry_count %lld outside 0..2^31 - 1 (0: the sorted route)", static_cast<long long>(entry_count));
  HDK_REQUIRE(entry_count == 0 || num_keys == 1,
              "hdk_hip_key_multiplicity: entry_count %lld with %d keys (a perfect table has one key; entry_count 0 sorts)",
              static_cast<long long>(entry_count), num_keys);
  HDK_REQUIRE(bucket >= 1, "hdk_hip_key_multiplicity: bucket %lld is not positive", static_cast<long long>(bucket));
  HDK_REQUIRE((flags & ~HDK_HIP_KEYS_NULLS_MATCH) == 0, "hdk_hip_key_multiplicity: unknown flags 0x%x", flags);
  const size_t need = km_workspace_bytes(num_rows, sort_cols, num_keys, entry_count);
  HDK_REQUIRE(!workspace || workspace_bytes >= need, "hdk_hip_key_multiplicity: workspace of %zu bytes, %zu needed", workspace_bytes,
              need);
  HDK_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "hdk_hip_key_multiplicity: workspace %p is not 8-byte aligned",
              workspace);
  HDK_REQUIRE(reinterpret_cast<uintptr_t>(result) % 8 == 0, "hdk_hip_key_multiplicity: result %p is not 8-byte aligned", result);
  {
    const MemBlock blk[] = {
        {"cols", reinterpret_cast<uintptr_t>(cols), num_rows ? static_cast<uint64_t>(num_cols) * capacity * 8 : 0},
        {"result", reinterpret_cast<uintptr_t>(result), sizeof(hdk_hip_key_multiplicity_result)},
        {"workspace", reinterpret_cast<uintptr_t>(workspace), workspace ? static_cast<uint64_t>(need) : 0},
    };
    const int32_t bad = require_disjoint("hdk_hip_key_multiplicity", blk, sizeof(blk) / sizeof(blk[0]));
    if (bad) return bad;
  }
  hipStream_t s;
  int32_t st = device_enter(device_id, stream, &s);
  if (st) return st;
  if (num_rows == 0) {
    HDK_HIP_CHECK(hipMemsetAsync(result, 0, sizeof(hdk_hip_key_multiplicity_result), s));
    return HDK_HIP_OK;
  }
  AsyncScratch mem(s);
  st = acquire_workspace(mem, &workspace, need);
  if (st) return st;
  char* ws = static_cast<char*>(workspace);
  const hdk_hip_device_properties* props = device_props(device_id);
  const uint32_t ntiles = static_cast<uint32_t>(km_tiles(num_rows));
  const unsigned row_grid = persistent_grid(props, ntiles) < kKmGridMax ? persistent_grid(props, ntiles) : kKmGridMax;

  if (entry_count > 0) {
    const hdk_hip_multiplicity_key& q = keys[0];
    const KmKey k = {static_cast<uint32_t>(q.col), q.nullable ? 1u : 0u, q.null_bits, q.min_val, q.max_val, q.translated_null};
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws);
    KmPartial* row_part = reinterpret_cast<KmPartial*>(ws + align256(static_cast<size_t>(entry_count) * 4));
    KmPartial* slot_part = row_part + kKmGridMax;
    HDK_HIP_CHECK(hipMemsetAsync(hist, 0, static_cast<size_t>(entry_count) * 4, s));
    const int64_t* col = cols + static_cast<uint64_t>(k.col) * capacity;
    const uint32_t nulls_match = (flags & HDK_HIP_KEYS_NULLS_MATCH) ? 1u : 0u;
    if (bucket > 1) {
      hipLaunchKernelGGL(hdk_key_histogram<true>, dim3(row_grid), dim3(kKmBlock), 0, s, col, num_rows, ntiles, k,
                         static_cast<uint64_t>(entry_count), static_cast<uint64_t>(bucket), nulls_match, hist, row_part);
    } else {
      hipLaunchKernelGGL(hdk_key_histogram<false>, dim3(row_grid), dim3(kKmBlock), 0, s, col, num_rows, ntiles, k,
                         static_cast<uint64_t>(entry_count), uint64_t(1), nulls_match, hist, row_part);
    }
    const uint64_t slot_blocks = (static_cast<uint64_t>(entry_count) + kKmTile - 1) / kKmTile;
    const unsigned slot_grid = persistent_grid(props, slot_blocks) < kKmGridMax ? persistent_grid(props, slot_blocks) : kKmGridMax;
    hipLaunchKernelGGL(hdk_key_histogram_reduce, dim3(slot_grid), dim3(kKmBlock), 0, s, hist, static_cast<uint64_t>(entry_count),
                       slot_part);
    hipLaunchKernelGGL(hdk_key_histogram_fold, dim3(1), dim3(kKmFoldBlock), 0, s, row_part, row_grid, slot_part, slot_grid, result);
    HDK_HIP_CHECK(hipGetLastError());
    return HDK_HIP_OK;
  }

  // the sorted route: rows with equal keys become adjacent.  The entries are not nullable: a NULL word sorts as the
  // value it is, which keeps equal tuples together; the run kernel gives their run the weight 0.
  const KmSortedParts parts = km_sorted_parts(num_rows, sort_cols, num_keys);
  int64_t* sorted = reinterpret_cast<int64_t*>(ws);
  void* sort_ws = ws + parts.sorted_bytes;
  KmRuns* sums = reinterpret_cast<KmRuns*>(ws + parts.sorted_bytes + parts.sort_bytes);
  const uint64_t sorted_capacity = km_sorted_capacity(num_rows);
  hdk_hip_order_entry order[HDK_HIP_MAX_JOIN_KEYS];
  KmKeys kk;
  memset(&kk, 0, sizeof(kk));
  memset(order, 0, sizeof(order));
  kk.nkeys = static_cast<uint32_t>(num_keys);
  for (int32_t i = 0; i < num_keys; ++i) {
    order[i].col = keys[i].col;
    kk.key_col[i] = static_cast<uint32_t>(keys[i].col);
    kk.nullable[i] = keys[i].nullable ? 1u : 0u;
    kk.null_bits[i] = keys[i].null_bits;
  }
  st = hdk_hip_sort_columns(cols, capacity, sort_cols, num_rows, order, num_keys, 0, 0, HDK_HIP_SORT_NO_SELECT, sorted, sorted_capacity,
                            nullptr, sort_ws, parts.sort_bytes, device_id, s);
  if (st) return st;
  hipLaunchKernelGGL(hdk_key_runs, dim3(row_grid), dim3(kGcBlock), 0, s, sorted, sorted_capacity, static_cast<uint32_t>(num_rows),
                     ntiles, kk, sums);
  hipLaunchKernelGGL(hdk_key_runs_fold, dim3(1), dim3(kKmFoldBlock), 0, s, sums, ntiles, result);
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
