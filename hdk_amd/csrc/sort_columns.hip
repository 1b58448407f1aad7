// sort_columns.hip -- ORDER BY / LIMIT / OFFSET over dense 8-byte result columns in HBM.
//
// Device form of ResultSet::sort for a result that lives on the device: doBaselineSort (omniscidb/QueryEngine/
// ResultSetSort.cpp:64-188, with ResultSetSortImpl.cu and TopKSort.cu behind it) and the comparator it restates,
// ResultSetComparator (ResultSetSort.cpp:329-480): per order entry NULLs by nulls_first, then (l < r) != is_desc on
// int64 or double values.  The input is what hdk_hip_columnarize_result wrote (result_columns.hip); the output is the
// same rows in order plus the permutation, the reference's permutation buffer.
//
// Every order entry becomes a 64-bit unsigned key whose unsigned order IS the comparator's order (sc_key), and the
// (key, row) pairs go through a stable LSD radix sort with 8-bit digits, last order entry first: stability makes the
// rounds lexicographic and leaves full ties in ascending row index.  Launches on one stream, ordered by nothing but the
// stream (no block ever waits for another block):
//   hdk_sort_build_keys   column (read through the current permutation from the second round on) -> keys, row indices
//                         of the first round, and the census: OR and OR-of-complement of all keys -> which digits are live
//   per LIVE digit        hdk_sort_hist (per-tile digit counts, digit-major) -> hdk_counts_scan<16> (one block, exclusive scan of
//                         256 x tiles counters) -> hdk_sort_scatter (stable ranks recomputed, pairs written to base + rank)
//   hdk_sort_gather       out_cols[t][r] = cols[t][perm[offset + r]], perm_out[r] = perm[offset + r]
// The host reads the 16-byte census back once per order entry (one stream synchronisation each) and launches only the
// live digits: COUNT(*) values below 2^24 cost 3 passes, a constant column none.
// Top-N (limit set, offset + limit <= num_rows / 8): MSD radix select on the FIRST entry's keys -- per live digit, from
// the top, hdk_sort_select_hist (digit counts of the keys that carry the prefix chosen so far, 8 bytes a row, read only)
// and hdk_sort_select_pick (one block: the bucket that holds the (offset+limit)-th key extends the prefix) -- then the
// rows whose key is <= that key are compacted in row order (count -> scan -> compact, as result_columns.hip does) and
// only they are sorted, by all entries.  Ties at the threshold key stay in, so the result is word for word the full sort's.
#include <string.h>

#include "column_primitives.h"
#include "host_common.h"

namespace hdk {

constexpr int kScBlock = kTileBlock;
constexpr int kScItems = 16;  // rows per thread and tile
constexpr int kScWaves = kScBlock / kWave;
constexpr uint32_t kScWaveSpan = kScItems * kWave;     // a wave owns 1 024 consecutive rows of its tile, ...
constexpr uint32_t kScTile = kScWaveSpan * kScWaves;   // ... a tile is 4 096 rows: order inside = (wave, item, lane)
constexpr int kScDigits = 256;
static_assert(kScBlock == kScDigits, "one thread per digit value");
constexpr ScanPer kScScanPer = SCAN_PER_16;  // counters per thread and trip of the scan

struct ScKeySpec {
  int64_t null_bits;
  uint64_t null_key;  // sc_order_bits(null_bits): the one value of the key space no non-NULL row can take
  uint32_t is_desc, nulls_first, is_fp, nullable;
};

struct ScSelect {
  uint64_t prefix;  // the digits chosen so far (and the digits all keys share), others 0
  uint64_t mask;    // which bits of `prefix` are decided
  uint64_t k;       // 1-based rank of the wanted key among the keys that carry the prefix
  uint64_t below;   // keys smaller than every key that carries the prefix
  uint64_t m;       // below + keys in the bucket chosen last: after the last pass, the keys <= the threshold key
};

// int64: sign flipped.  double: negatives inverted, others sign flipped (-0.0 < +0.0, NaNs beyond the infinities by
// bit pattern).  Descending: all bits inverted.
HDK_HOST_DEV uint64_t sc_order_bits(int64_t w, bool is_fp, bool desc) {
  uint64_t u = static_cast<uint64_t>(w);
  u = (is_fp && (u >> 63)) ? ~u : (u ^ (uint64_t(1) << 63));
  return desc ? ~u : u;
}

// NULLs and values are kept apart by rule: a nullable column cannot hold null_bits as a value, so the 2^64 - 1 possible
// values are moved one step over the hole that null_bits leaves -- towards 0 with NULLS LAST (~0 is then free for NULL),
// away from 0 with NULLS FIRST (0 is then free).  The move keeps the order.
HDK_DEV uint64_t sc_key(int64_t w, const ScKeySpec& k) {
  const uint64_t u = sc_order_bits(w, k.is_fp != 0, k.is_desc != 0);
  if (!k.nullable) {
    return u;
  }
  if (w == k.null_bits) {
    return k.nulls_first ? uint64_t(0) : ~uint64_t(0);
  }
  if (k.nulls_first) {
    return u < k.null_key ? u + 1 : u;
  }
  return u > k.null_key ? u - 1 : u;
}

// the valid lanes of this wave that hold the same digit (all 64 lanes call this together; the result of an invalid lane
// means nothing)
HDK_DEV uint64_t sc_match(uint32_t digit, bool valid) {
  uint64_t m = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1u;
    const uint64_t v = __builtin_amdgcn_ballot_w64(bit);
    m &= bit ? v : ~v;
  }
  return m;
}

HDK_DEV uint64_t sc_wave_or(uint64_t v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    v |= static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(v), d, kWave));
  }
  return v;
}

// first row of this thread in its tile; item j is at + j * kWave
HDK_DEV uint64_t sc_first_row(uint32_t tile) {
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  return static_cast<uint64_t>(tile) * kScTile + wave * kScWaveSpan + lane;
}

enum ScBuild : int { SC_IDENTITY = 0, SC_THROUGH_PERM = 1, SC_KEYS_ONLY = 2 };

// keys[i] = sc_key(col[row(i)]), row(i) = i (SC_IDENTITY, which also writes idx[i] = i; SC_KEYS_ONLY) or idx[i]
// (SC_THROUGH_PERM).  census[0] |= key, census[1] |= ~key over all rows.
template <int MODE>
__global__ __launch_bounds__(kScBlock) void hdk_sort_build_keys(const int64_t* __restrict__ col, uint64_t n, ScKeySpec spec,
                                                                 uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                                 unsigned long long* __restrict__ census) {
  __shared__ uint64_t s_or[kScWaves], s_nor[kScWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const uint64_t e0 = sc_first_row(blockIdx.x);
  int64_t word[kScItems];
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    // (a row past the end reads the last row instead, so that the loads of a tile are issued together)
    const uint64_t e = e0 + static_cast<uint32_t>(j) * kWave;
    const uint64_t ec = e < n ? e : n - 1;
    const uint64_t row = MODE == SC_THROUGH_PERM ? idx[ec] : ec;
    word[j] = col[row];
  }
  uint64_t o = 0, no = 0;
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const uint64_t e = e0 + static_cast<uint32_t>(j) * kWave;
    if (e < n) {
      const uint64_t k = sc_key(word[j], spec);
      keys[e] = k;
      if (MODE == SC_IDENTITY) {
        idx[e] = static_cast<uint32_t>(e);
      }
      o |= k;
      no |= ~k;
    }
  }
  o = sc_wave_or(o);
  no = sc_wave_or(no);
  if (lane == 0) {
    s_or[wave] = o;
    s_nor[wave] = no;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kScWaves; ++w) {
      o |= s_or[w];
      no |= s_nor[w];
    }
    // (OR only grows: a block that has nothing to add skips the atomic, and after the first few blocks most do)
    if ((__atomic_load_n(&census[0], __ATOMIC_RELAXED) | o) != __atomic_load_n(&census[0], __ATOMIC_RELAXED)) {
      atomicOr(&census[0], static_cast<unsigned long long>(o));
    }
    if ((__atomic_load_n(&census[1], __ATOMIC_RELAXED) | no) != __atomic_load_n(&census[1], __ATOMIC_RELAXED)) {
      atomicOr(&census[1], static_cast<unsigned long long>(no));
    }
  }
}

// counters[digit * ntiles + tile] = rows of the tile whose key has `digit` at `shift`
__global__ __launch_bounds__(kScBlock) void hdk_sort_hist(const uint64_t* __restrict__ keys, uint64_t n, uint32_t shift,
                                                           uint32_t ntiles, uint32_t* __restrict__ counters) {
  __shared__ uint32_t s_hist[kScDigits];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t e0 = sc_first_row(blockIdx.x);
  uint64_t key[kScItems];
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const uint64_t e = e0 + static_cast<uint32_t>(j) * kWave;
    key[j] = keys[e < n ? e : n - 1];
  }
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const bool valid = e0 + static_cast<uint32_t>(j) * kWave < n;
    const uint32_t digit = static_cast<uint32_t>(key[j] >> shift) & 255u;
    const uint64_t mask = sc_match(digit, valid);
    if (valid && lane_rank(mask) == 0) {  // the lowest lane of each digit adds for all of them
      atomicAdd(&s_hist[digit], static_cast<uint32_t>(__popcll(mask)));
    }
  }
  __syncthreads();
  counters[static_cast<size_t>(threadIdx.x) * ntiles + blockIdx.x] = s_hist[threadIdx.x];
}

// pair i of the tile goes to bases[digit * ntiles + tile] + (pairs of the tile before i with the same digit)
__global__ __launch_bounds__(kScBlock) void hdk_sort_scatter(const uint64_t* __restrict__ keys_in,
                                                              const uint32_t* __restrict__ idx_in, uint64_t n, uint32_t shift,
                                                              uint32_t ntiles, const uint32_t* __restrict__ bases,
                                                              uint64_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out) {
  __shared__ uint32_t s_cnt[kScWaves][kScDigits], s_base[kScWaves][kScDigits];
  const uint32_t wave = threadIdx.x / kWave;
#pragma unroll
  for (int w = 0; w < kScWaves; ++w) {
    s_cnt[w][threadIdx.x] = 0;
  }
  __syncthreads();
  const uint64_t e0 = sc_first_row(blockIdx.x);
  uint64_t key[kScItems];
  uint32_t row[kScItems], rank[kScItems];
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const uint64_t e = e0 + static_cast<uint32_t>(j) * kWave;
    const uint64_t ec = e < n ? e : n - 1;
    key[j] = keys_in[ec];
    row[j] = idx_in[ec];
  }
  // a wave walks its 1 024 rows in order and keeps its own running digit counts: no other wave touches s_cnt[wave], and
  // the LDS operations of one wave complete in order (the fences keep the compiler from moving them)
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const bool valid = e0 + static_cast<uint32_t>(j) * kWave < n;
    const uint32_t digit = static_cast<uint32_t>(key[j] >> shift) & 255u;
    const uint64_t mask = sc_match(digit, valid);
    const uint32_t before = s_cnt[wave][digit];
    const uint32_t r = lane_rank(mask);
    rank[j] = before + r;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (valid && r == 0) {
      s_cnt[wave][digit] = before + static_cast<uint32_t>(__popcll(mask));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  __syncthreads();
  {
    uint32_t run = bases[static_cast<size_t>(threadIdx.x) * ntiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kScWaves; ++w) {
      s_base[w][threadIdx.x] = run;
      run += s_cnt[w][threadIdx.x];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const bool valid = e0 + static_cast<uint32_t>(j) * kWave < n;
    const uint32_t digit = static_cast<uint32_t>(key[j] >> shift) & 255u;
    const uint64_t dst = static_cast<uint64_t>(s_base[wave][digit]) + rank[j];
    if (valid && dst < n) {
      keys_out[dst] = key[j];
      idx_out[dst] = row[j];
    }
  }
}

__global__ __launch_bounds__(kScDigits) void hdk_sort_select_init(ScSelect* __restrict__ sel, uint32_t* __restrict__ hist,
                                                                   uint64_t prefix, uint64_t mask, uint64_t k) {
  hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    sel->prefix = prefix;
    sel->mask = mask;
    sel->k = k;
    sel->below = 0;
    sel->m = 0;
  }
}

// hist[digit] += keys that carry the prefix and have `digit` at `shift`
__global__ __launch_bounds__(kScBlock) void hdk_sort_select_hist(const uint64_t* __restrict__ keys, uint64_t n, uint32_t shift,
                                                                  const ScSelect* __restrict__ sel, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_hist[kScDigits];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t prefix = sel->prefix, pmask = sel->mask;
  const uint64_t e0 = sc_first_row(blockIdx.x);
  uint64_t key[kScItems];
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const uint64_t e = e0 + static_cast<uint32_t>(j) * kWave;
    key[j] = __builtin_nontemporal_load(&keys[e < n ? e : n - 1]);
  }
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const bool valid = e0 + static_cast<uint32_t>(j) * kWave < n && (key[j] & pmask) == prefix;
    const uint32_t digit = static_cast<uint32_t>(key[j] >> shift) & 255u;
    const uint64_t mask = sc_match(digit, valid);
    if (valid && lane_rank(mask) == 0) {
      atomicAdd(&s_hist[digit], static_cast<uint32_t>(__popcll(mask)));
    }
  }
  __syncthreads();
  const uint32_t c = s_hist[threadIdx.x];
  if (c) {
    atomicAdd(&hist[threadIdx.x], c);
  }
}

// one block: the bucket that holds the k-th key of the prefix extends the prefix; the histogram is cleared for the next pass
__global__ __launch_bounds__(kScDigits) void hdk_sort_select_pick(ScSelect* __restrict__ sel, uint32_t* __restrict__ hist,
                                                                   uint32_t shift) {
  __shared__ uint32_t s_c[kScDigits];
  s_c[threadIdx.x] = hist[threadIdx.x];
  __syncthreads();
  hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    const uint64_t k = sel->k;
    uint64_t cum = 0;
    uint32_t d = 0;
    for (; d < kScDigits - 1; ++d) {
      if (cum + s_c[d] >= k) {
        break;
      }
      cum += s_c[d];
    }
    sel->prefix |= static_cast<uint64_t>(d) << shift;
    sel->mask |= uint64_t(255) << shift;
    sel->k = k - cum;
    sel->below += cum;
    sel->m = sel->below + s_c[d];
  }
}

// tile_counts[tile] = rows of the tile whose key is <= the threshold key
__global__ __launch_bounds__(kScBlock) void hdk_sort_select_count(const uint64_t* __restrict__ keys, uint64_t n,
                                                                   const ScSelect* __restrict__ sel,
                                                                   uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t s_wave[kScWaves];
  const uint64_t threshold = sel->prefix;
  const uint64_t e0 = sc_first_row(blockIdx.x);
  uint64_t key[kScItems];
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const uint64_t e = e0 + static_cast<uint32_t>(j) * kWave;
    key[j] = keys[e < n ? e : n - 1];
  }
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const bool f = e0 + static_cast<uint32_t>(j) * kWave < n && key[j] <= threshold;
    c += static_cast<uint32_t>(__popcll(__builtin_amdgcn_ballot_w64(f)));
  }
  block_store_tile_count<false>(s_wave, c, tile_counts + blockIdx.x);
}

// idx_out[rank] = row, for the rows whose key is <= the threshold key, in row order
__global__ __launch_bounds__(kScBlock) void hdk_sort_select_compact(const uint64_t* __restrict__ keys, uint64_t n,
                                                                     const ScSelect* __restrict__ sel,
                                                                     const uint32_t* __restrict__ tile_offs,
                                                                     uint32_t* __restrict__ idx_out, uint64_t capacity) {
  __shared__ uint32_t s_wave[kScWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const uint64_t threshold = sel->prefix;
  const uint64_t e0 = sc_first_row(blockIdx.x);
  uint64_t key[kScItems];
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const uint64_t e = e0 + static_cast<uint32_t>(j) * kWave;
    key[j] = keys[e < n ? e : n - 1];
  }
  uint32_t rank[kScItems];
  uint32_t flags = 0, run = 0;
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const bool f = e0 + static_cast<uint32_t>(j) * kWave < n && key[j] <= threshold;
    const uint64_t mask = __builtin_amdgcn_ballot_w64(f);
    rank[j] = run + lane_rank(mask);
    run += static_cast<uint32_t>(__popcll(mask));
    flags |= static_cast<uint32_t>(f) << j;
  }
  if (lane == 0) {
    s_wave[wave] = run;
  }
  __syncthreads();
  uint64_t base = tile_offs[blockIdx.x];
#pragma unroll
  for (int w = 0; w < kScWaves; ++w) {
    base += static_cast<uint32_t>(w) < wave ? s_wave[w] : 0;
  }
#pragma unroll
  for (int j = 0; j < kScItems; ++j) {
    const uint64_t dst = base + rank[j];
    if (((flags >> j) & 1u) && dst < capacity) {
      idx_out[dst] = static_cast<uint32_t>(e0 + static_cast<uint32_t>(j) * kWave);
    }
  }
}

// consecutive lanes write consecutive output rows of every column; the reads follow the permutation
__global__ __launch_bounds__(kScBlock) void hdk_sort_gather(const int64_t* __restrict__ cols, uint64_t capacity, int32_t num_cols,
                                                             const uint32_t* __restrict__ perm, uint64_t out_rows,
                                                             int64_t* __restrict__ out, uint64_t out_capacity,
                                                             uint32_t* __restrict__ perm_out) {
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kScBlock + threadIdx.x;
  if (r >= out_rows) {
    return;
  }
  const uint64_t row = perm[r];
  if (perm_out) {
    perm_out[r] = static_cast<uint32_t>(row);
  }
  for (int32_t t = 0; t < num_cols; ++t) {
    out[static_cast<uint64_t>(t) * out_capacity + r] = cols[static_cast<uint64_t>(t) * capacity + row];
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
static size_t sc_tiles(uint64_t n) { return static_cast<size_t>((n + kScTile - 1) / kScTile); }

// [census 16 B | select state | select histogram] [keys x2] [rows x2] [256 x tiles counters + 1]
constexpr size_t kScHeadBytes = 4096, kScSelOff = 64, kScSelHistOff = 1024;
static_assert(kScSelOff + sizeof(ScSelect) <= kScSelHistOff && kScSelHistOff + kScDigits * 4 <= kScHeadBytes, "header layout");

struct ScSpace {
  unsigned long long* census;
  ScSelect* sel;
  uint32_t* sel_hist;
  uint64_t* keys[2];
  uint32_t* idx[2];
  uint32_t* counters;
};

static size_t sc_carve(uint64_t n, void* base, ScSpace* sp) {
  int8_t* p = static_cast<int8_t*>(base);
  size_t off = kScHeadBytes;
  const size_t kb = align256(static_cast<size_t>(n) * 8), ib = align256(static_cast<size_t>(n) * 4);
  if (sp) {
    sp->census = reinterpret_cast<unsigned long long*>(p);
    sp->sel = reinterpret_cast<ScSelect*>(p + kScSelOff);
    sp->sel_hist = reinterpret_cast<uint32_t*>(p + kScSelHistOff);
    sp->keys[0] = reinterpret_cast<uint64_t*>(p + off);
    sp->keys[1] = reinterpret_cast<uint64_t*>(p + off + kb);
    sp->idx[0] = reinterpret_cast<uint32_t*>(p + off + 2 * kb);
    sp->idx[1] = reinterpret_cast<uint32_t*>(p + off + 2 * kb + ib);
    sp->counters = reinterpret_cast<uint32_t*>(p + off + 2 * kb + 2 * ib);
  }
  off += 2 * kb + 2 * ib;
  off += align256((sc_tiles(n) * kScDigits + 1) * sizeof(uint32_t));
  return off;
}

static ScKeySpec sc_spec(const hdk_hip_order_entry& e) {
  ScKeySpec k;
  k.null_bits = e.null_bits;
  k.null_key = sc_order_bits(e.null_bits, e.is_fp != 0, e.is_desc != 0);
  k.is_desc = e.is_desc != 0;
  k.nulls_first = e.nulls_first != 0;
  k.is_fp = e.is_fp != 0;
  k.nullable = e.nullable != 0;
  return k;
}

// the census of the keys just built: bits on which not all keys agree, and the bits they share (one synchronisation)
static int32_t sc_read_census(const ScSpace& sp, hipStream_t s, uint64_t* varying, uint64_t* common) {
  unsigned long long c[2];
  HDK_HIP_CHECK(hipMemcpyAsync(c, sp.census, sizeof(c), hipMemcpyDeviceToHost, s));
  HDK_HIP_CHECK(hipStreamSynchronize(s));
  *varying = c[0] & c[1];
  *common = c[0] & ~c[1];
  return HDK_HIP_OK;
}

template <int MODE>
static void sc_launch_build(const int64_t* col, uint64_t n, const ScKeySpec& spec, uint64_t* keys, uint32_t* idx,
                            unsigned long long* census, hipStream_t s) {
  hipLaunchKernelGGL(hdk_sort_build_keys<MODE>, dim3(static_cast<unsigned>(sc_tiles(n))), dim3(kScBlock), 0, s, col, n, spec, keys,
                     idx, census);
}

}  // namespace hdk

using namespace hdk;

extern "C" size_t hdk_hip_sort_columns_workspace_bytes(uint64_t num_rows, int32_t num_order) {
  (void)num_order;  // the rounds reuse the same pairs
  return sc_carve(num_rows, nullptr, nullptr);
}

extern "C" int32_t hdk_hip_sort_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                                        const hdk_hip_order_entry* order, int32_t num_order, uint64_t offset, uint64_t limit,
                                        uint32_t flags, int64_t* out_cols, uint64_t out_capacity, uint32_t* perm_out,
                                        void* workspace, size_t workspace_bytes, int32_t device_id, void* stream) {
  HDK_REQUIRE(cols && order && out_cols, "hdk_hip_sort_columns: NULL argument (cols, order and out_cols are required)");
  HDK_REQUIRE(num_cols >= 1, "hdk_hip_sort_columns: num_cols %d", num_cols);
  HDK_REQUIRE(num_order >= 1 && num_order <= HDK_HIP_MAX_ORDER_ENTRIES, "hdk_hip_sort_columns: num_order %d outside 1..%d",
              num_order, HDK_HIP_MAX_ORDER_ENTRIES);
  for (int32_t i = 0; i < num_order; ++i) {
    HDK_REQUIRE(order[i].col >= 0 && order[i].col < num_cols, "hdk_hip_sort_columns: order entry %d names column %d of %d", i,
                order[i].col, num_cols);
  }
  HDK_REQUIRE(num_rows < (uint64_t(1) << 32), "hdk_hip_sort_columns: num_rows %llu does not fit 32-bit row indices",
              static_cast<unsigned long long>(num_rows));
  HDK_REQUIRE(num_rows <= capacity, "hdk_hip_sort_columns: num_rows %llu exceeds the capacity %llu",
              static_cast<unsigned long long>(num_rows), static_cast<unsigned long long>(capacity));
  const uint64_t after = num_rows > offset ? num_rows - offset : 0;
  const uint64_t out_rows = limit && limit < after ? limit : after;
  HDK_REQUIRE(out_capacity >= out_rows, "hdk_hip_sort_columns: out_capacity %llu below the %llu output rows",
              static_cast<unsigned long long>(out_capacity), static_cast<unsigned long long>(out_rows));
  {
    // (perm_out and workspace are not checked: adding them would change behaviour and is a change of its own; a block
    // of zero bytes -- out_capacity 0, nothing to write -- overlaps nothing)
    const MemBlock blk[] = {
        {"cols", reinterpret_cast<uintptr_t>(cols), static_cast<uint64_t>(num_cols) * capacity * 8},
        {"out_cols", reinterpret_cast<uintptr_t>(out_cols), static_cast<uint64_t>(num_cols) * out_capacity * 8},
    };
    const int32_t bad = require_disjoint("hdk_hip_sort_columns", blk, 2);
    if (bad) return bad;
  }
  const size_t need = hdk_hip_sort_columns_workspace_bytes(num_rows, num_order);
  HDK_REQUIRE(!workspace || workspace_bytes >= need, "hdk_hip_sort_columns: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  if (num_rows == 0 || out_rows == 0) {
    return HDK_HIP_OK;
  }
  hipStream_t s;
  int32_t st = device_enter(device_id, stream, &s);
  if (st) return st;
  AsyncScratch mem(s);
  st = acquire_workspace(mem, &workspace, need);
  if (st) return st;
  ScSpace sp;
  sc_carve(num_rows, workspace, &sp);

  uint64_t m = num_rows;   // rows in the sort
  bool have_perm = false;  // idx[cur][0 .. m) already names the rows
  int cur = 0;
  const uint64_t want = offset + out_rows;  // the sort's first `want` rows are needed
  if (limit && !(flags & HDK_HIP_SORT_NO_SELECT) && want <= num_rows / 8) {
    const ScKeySpec spec = sc_spec(order[0]);
    HDK_HIP_CHECK(hipMemsetAsync(sp.census, 0, 16, s));
    sc_launch_build<SC_KEYS_ONLY>(cols + static_cast<uint64_t>(order[0].col) * capacity, num_rows, spec, sp.keys[1], nullptr,
                                  sp.census, s);
    uint64_t varying, common;
    st = sc_read_census(sp, s, &varying, &common);
    if (st) return st;
    if (varying) {  // (all first keys equal: nothing to select by)
      uint64_t dead = 0;
      for (int d = 0; d < 8; ++d) {
        if (!((varying >> (8 * d)) & 255u)) dead |= uint64_t(255) << (8 * d);
      }
      const dim3 grid(static_cast<unsigned>(sc_tiles(num_rows))), block(kScBlock);
      hipLaunchKernelGGL(hdk_sort_select_init, dim3(1), dim3(kScDigits), 0, s, sp.sel, sp.sel_hist, common & dead, dead, want);
      for (int d = 7; d >= 0; --d) {
        if ((dead >> (8 * d)) & 1u) continue;
        hipLaunchKernelGGL(hdk_sort_select_hist, grid, block, 0, s, sp.keys[1], num_rows, static_cast<uint32_t>(8 * d), sp.sel,
                           sp.sel_hist);
        hipLaunchKernelGGL(hdk_sort_select_pick, dim3(1), dim3(kScDigits), 0, s, sp.sel, sp.sel_hist, static_cast<uint32_t>(8 * d));
      }
      hipLaunchKernelGGL(hdk_sort_select_count, grid, block, 0, s, sp.keys[1], num_rows, sp.sel, sp.counters);
      launch_counts_scan(sp.counters, static_cast<uint32_t>(sc_tiles(num_rows)), kScScanPer, nullptr, s);
      ScSelect sel;
      HDK_HIP_CHECK(hipMemcpyAsync(&sel, sp.sel, sizeof(sel), hipMemcpyDeviceToHost, s));
      HDK_HIP_CHECK(hipStreamSynchronize(s));
      if (sel.m < want || sel.m > num_rows) {
        set_error("hdk_hip_sort_columns: top-N selection kept %llu of %llu rows for %llu wanted",
                  static_cast<unsigned long long>(sel.m), static_cast<unsigned long long>(num_rows),
                  static_cast<unsigned long long>(want));
        return HDK_HIP_ERR_RUNTIME;
      }
      m = sel.m;
      hipLaunchKernelGGL(hdk_sort_select_compact, grid, block, 0, s, sp.keys[1], num_rows, sp.sel, sp.counters, sp.idx[0], m);
      have_perm = true;
    }
  }

  const uint32_t mtiles = static_cast<uint32_t>(sc_tiles(m));
  const dim3 grid(mtiles), block(kScBlock);
  for (int32_t e = num_order - 1; e >= 0; --e) {
    const ScKeySpec spec = sc_spec(order[e]);
    const int64_t* col = cols + static_cast<uint64_t>(order[e].col) * capacity;
    HDK_HIP_CHECK(hipMemsetAsync(sp.census, 0, 16, s));
    if (have_perm) {
      sc_launch_build<SC_THROUGH_PERM>(col, m, spec, sp.keys[cur], sp.idx[cur], sp.census, s);
    } else {
      sc_launch_build<SC_IDENTITY>(col, m, spec, sp.keys[cur], sp.idx[cur], sp.census, s);
    }
    have_perm = true;
    uint64_t varying, common;
    st = sc_read_census(sp, s, &varying, &common);
    if (st) return st;
    for (int d = 0; d < 8; ++d) {
      if (!((varying >> (8 * d)) & 255u)) continue;  // all keys agree on this digit: no pass
      const uint32_t shift = static_cast<uint32_t>(8 * d);
      hipLaunchKernelGGL(hdk_sort_hist, grid, block, 0, s, sp.keys[cur], m, shift, mtiles, sp.counters);
      launch_counts_scan(sp.counters, mtiles * kScDigits, kScScanPer, nullptr, s);
      hipLaunchKernelGGL(hdk_sort_scatter, grid, block, 0, s, sp.keys[cur], sp.idx[cur], m, shift, mtiles, sp.counters,
                         sp.keys[cur ^ 1], sp.idx[cur ^ 1]);
      cur ^= 1;
    }
  }
  hipLaunchKernelGGL(hdk_sort_gather, dim3(static_cast<unsigned>((out_rows + kScBlock - 1) / kScBlock)), block, 0, s, cols, capacity,
                     num_cols, sp.idx[cur] + offset, out_rows, out_cols, out_capacity, perm_out);
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
