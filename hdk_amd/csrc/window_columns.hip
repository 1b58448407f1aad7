// window_columns.hip -- window functions over dense 8-byte result columns in HBM: one word per input row and output.
//
// Device form of the reference's window step over a materialised result (WindowFunctionContext, omniscidb/QueryEngine/
// WindowContext.cpp, WindowFunctionIR.cpp), over what hdk_hip_columnarize_result, hdk_hip_filter_columns,
// hdk_hip_sort_columns and hdk_hip_group_columns write.  It is group_columns.hip's segmented walk (column_segments.h)
// with two kinds of tails -- a PARTITION tail (a partition key word differs from the next row's, or the last row) and a
// PEER tail (a partition or order key word differs) -- that stores at every row instead of at every tail.
//
// Up to seven launches on one stream, ordered by nothing but the stream (no global atomics, no look-back, no flags):
//   hdk_window_count      persistent grid over tiles of kGcTile rows: the tile's partition tails and peer tails ->
//                         two counters per tile; per aggregate the tile's open suffix with respect to the partition tails
//                         (every frame starts at its partition's first row)
//   hdk_counts_scan<4>    twice (column_scan.hip): exclusive offsets of both counters in place
//   hdk_window_carry_scan one block per aggregate: column_segments.h's segmented exclusive scan of the open suffixes
//   hdk_window_directory  every tail stores its row index at its scanned rank: part_end[p], peer_end[q], and per
//                         partition the ordinal of its last peer group, part_lastq[p].  Row r of partition p and peer
//                         group q then has start = part_end[p - 1] + 1, end = part_end[p], pstart = peer_end[q - 1] + 1,
//                         pend = peer_end[q] and dense rank q - part_lastq[p - 1] (the rows before row 0 count as one
//                         partition and peer group that ends at row -1)
//   hdk_window_rows       per tile the tails again and p, q of every row (the tile's offsets plus ballot ranks); per
//                         output, the switch over its kind outside the item loop: the ranking kinds are arithmetic over
//                         the directory, LAG / LEAD / FIRST_VALUE / LAST_VALUE gathers through it, an aggregate the
//                         segmented inclusive scan -- per 64-row item a wave-level segmented scan, lane 63 carried to the
//                         next item, the waves chained through LDS, carry_in applied to the tile's first open partition
//                         -- whose value at row r is the ROWS frame's.  All 16 items of a lane stay in registers until the
//                         waves have exchanged what they end with
//   hdk_window_broadcast  only when an aggregate has a RANGE or PARTITION frame: out[r] = out[pend] or out[end].  The
//                         tail rows already hold their frame's value and are never written, so the pass works in place
//                         and all rows of a peer group or partition receive one word, bit for bit
// Traffic for n rows, k = kp + ko key columns, a aggregated columns, g gathered columns, w outputs, b of them broadcast:
// count 8nk (+ the suffix items of the aggregated columns), directory 8nk read + at most 12n written, rows
// 8n(k + a + g) read + 8nw written (+ the directory, at most 12n, through the caches), broadcast 8nk + 8nb read + 8nb
// written.
#include <string.h>

#include "column_segments.h"
#include "host_common.h"

namespace hdk {

struct WnKeys {
  uint32_t nkeys;
  uint32_t key_col[HDK_HIP_MAX_WINDOW_KEYS];
};

struct WnOut {
  GcOut g;  // g.op == GC_ID: not an aggregate
  uint32_t kind, frame;
  uint32_t avg, pad_;
  int64_t param;
};

struct WnDesc {
  WnKeys part, order;
  uint32_t nouts;
  WnOut out[HDK_HIP_MAX_WINDOW_OUTS];
};

struct WnDir {
  uint32_t* part_end;    // [p] last row of partition p
  uint32_t* part_lastq;  // [p] ordinal of the last peer group of partition p
  uint32_t* peer_end;    // [q] last row of peer group q
};

// the partition tails and the peer tails of this lane's 16 rows
HDK_DEV void wn_tails(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, const WnDesc& d, uint32_t r0, uint32_t lane,
                      uint32_t* ptails, uint32_t* qtails) {
  const uint32_t dp = gc_differs(cols, capacity, n, d.part, r0, lane);
  const uint32_t dq = gc_differs(cols, capacity, n, d.order, r0, lane);
  *ptails = gc_tails_of(dp, n, r0);
  *qtails = gc_tails_of(dp | dq, n, r0);
}

// sufv == NULL: no aggregates
__global__ __launch_bounds__(kGcBlock) void hdk_window_count(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, WnDesc d,
                                                              uint32_t ntiles, uint32_t* __restrict__ part_counts,
                                                              uint32_t* __restrict__ peer_counts, int64_t* __restrict__ sufv,
                                                              uint32_t* __restrict__ sufc) {
  __shared__ uint32_t s_wave[kGcWaves];
  __shared__ int64_t s_v[kGcWaves];
  __shared__ uint32_t s_c[kGcWaves], s_t[kGcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t r0 = gc_row0(tile, wave, lane);
    uint32_t ptails, qtails;
    wn_tails(cols, capacity, n, d, r0, lane, &ptails, &qtails);
    block_store_tile_count(s_wave, gc_count_tails(ptails), part_counts + tile);
    block_store_tile_count(s_wave, gc_count_tails(qtails), peer_counts + tile);
    if (!sufv) {
      continue;
    }
    for (uint32_t a = 0; a < d.nouts; ++a) {
      const GcOut o = d.out[a].g;
      const int64_t* col = cols + static_cast<uint64_t>(o.col) * capacity;
      int64_t* dv = sufv + static_cast<uint64_t>(a) * ntiles + tile;
      uint32_t* dc = sufc + static_cast<uint64_t>(a) * ntiles + tile;
#define HDK_GC_CASE(OP) \
  case OP: gc_open_suffix<OP>(col, n, o, r0, lane, wave, ptails, s_v, s_c, s_t, dv, dc); break;
      switch (o.op) {
        HDK_GC_AGG_CASES
        default: break;  // not an aggregate: no partial
      }
#undef HDK_GC_CASE
    }
  }
}

__global__ __launch_bounds__(kGcCarryBlock) void hdk_window_carry_scan(WnDesc d, uint32_t ntiles, const uint32_t* __restrict__ offs,
                                                                        int64_t* __restrict__ sufv, uint32_t* __restrict__ sufc) {
  const uint32_t a = blockIdx.x;
  int64_t* v = sufv + static_cast<uint64_t>(a) * ntiles;
  uint32_t* c = sufc + static_cast<uint64_t>(a) * ntiles;
#define HDK_GC_CASE(OP) \
  case OP: gc_carry_scan<OP>(ntiles, offs, v, c); break;
  switch (d.out[a].g.op) {
    HDK_GC_AGG_CASES
    default: break;
  }
#undef HDK_GC_CASE
}

// What the row passes know of a tile: the tails of this lane's rows and the directory slots of this wave's first tails.
struct WnTile {
  uint32_t r0, ptails, qtails;
  uint32_t pbase, qbase;
};

HDK_DEV WnTile wn_locate(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, const WnDesc& d, uint32_t tile, uint32_t lane,
                         uint32_t wave, const uint32_t* __restrict__ part_offs, const uint32_t* __restrict__ peer_offs,
                         uint32_t (&s_wave)[kGcWaves]) {
  WnTile t;
  t.r0 = gc_row0(tile, wave, lane);
  wn_tails(cols, capacity, n, d, t.r0, lane, &t.ptails, &t.qtails);
  // (a directory slot is a rank among at most n < 2^32 tails)
  t.pbase = static_cast<uint32_t>(gc_wave_base(s_wave, part_offs[tile], gc_count_tails(t.ptails), lane, wave));
  t.qbase = static_cast<uint32_t>(gc_wave_base(s_wave, peer_offs[tile], gc_count_tails(t.qtails), lane, wave));
  return t;
}

__global__ __launch_bounds__(kGcBlock) void hdk_window_directory(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n,
                                                                  WnDesc d, uint32_t ntiles, const uint32_t* __restrict__ part_offs,
                                                                  const uint32_t* __restrict__ peer_offs, WnDir dir) {
  __shared__ uint32_t s_wave[kGcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const WnTile t = wn_locate(cols, capacity, n, d, tile, lane, wave, part_offs, peer_offs, s_wave);
    uint32_t pb = t.pbase, qb = t.qbase;
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      const uint32_t r = t.r0 + static_cast<uint32_t>(j) * kWave;
      const uint64_t pm = gc_item_tails(t.ptails, j), qm = gc_item_tails(t.qtails, j);
      const uint32_t p = pb + lane_rank(pm), q = qb + lane_rank(qm);
      if ((t.qtails >> j) & 1u) {  // (a tail is a row below n: its ranks are below n)
        dir.peer_end[q] = r;
      }
      if ((t.ptails >> j) & 1u) {
        dir.part_end[p] = r;
        dir.part_lastq[p] = q;
      }
      pb += static_cast<uint32_t>(__popcll(pm));
      qb += static_cast<uint32_t>(__popcll(qm));
    }
  }
}

// the six ranking kinds: arithmetic over the directory
template <uint32_t KIND>
HDK_DEV void wn_rank(uint32_t n, const WnTile& t, uint32_t lane, const WnDir& dir, int64_t param, int64_t* __restrict__ dst) {
  uint32_t pb = t.pbase, qb = t.qbase;
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    const uint32_t r = t.r0 + static_cast<uint32_t>(j) * kWave;
    const uint64_t pm = gc_item_tails(t.ptails, j), qm = gc_item_tails(t.qtails, j);
    const uint32_t p = pb + lane_rank(pm), q = qb + lane_rank(qm);
    pb += static_cast<uint32_t>(__popcll(pm));
    qb += static_cast<uint32_t>(__popcll(qm));
    if (r < n) {
      const uint32_t start = p ? dir.part_end[p - 1] + 1u : 0u;
      int64_t w;
      if constexpr (KIND == HDK_WIN_ROW_NUMBER) {
        w = static_cast<int64_t>(r - start) + 1;
      } else if constexpr (KIND == HDK_WIN_RANK) {
        const uint32_t pstart = q ? dir.peer_end[q - 1] + 1u : 0u;
        w = static_cast<int64_t>(pstart - start) + 1;
      } else if constexpr (KIND == HDK_WIN_DENSE_RANK) {
        const uint32_t firstq = p ? dir.part_lastq[p - 1] + 1u : 0u;
        w = static_cast<int64_t>(q - firstq) + 1;
      } else if constexpr (KIND == HDK_WIN_PERCENT_RANK) {
        const uint32_t pstart = q ? dir.peer_end[q - 1] + 1u : 0u;
        const uint32_t last = dir.part_end[p] - start;  // size - 1
        w = double_to_bits(last == 0 ? 0.0 : static_cast<double>(pstart - start) / static_cast<double>(last));
      } else if constexpr (KIND == HDK_WIN_CUME_DIST) {
        const uint64_t size = static_cast<uint64_t>(dir.part_end[p] - start) + 1;
        const uint64_t upto = static_cast<uint64_t>(dir.peer_end[q] - start) + 1;
        w = double_to_bits(static_cast<double>(upto) / static_cast<double>(size));
      } else {  // HDK_WIN_NTILE: ceil(size / n) rows per tile; n >= size gives one row per tile
        const uint64_t size = static_cast<uint64_t>(dir.part_end[p] - start) + 1;
        const uint64_t nt = static_cast<uint64_t>(param);
        const uint32_t per = nt >= size ? 1u : static_cast<uint32_t>((size + nt - 1) / nt);
        w = static_cast<int64_t>((r - start) / per) + 1;
      }
      dst[r] = w;
    }
  }
}

// LAG, LEAD, FIRST_VALUE, LAST_VALUE: one word of `col` per row, found through the directory and copied unexamined
template <uint32_t KIND>
HDK_DEV void wn_gather(const int64_t* __restrict__ col, uint32_t n, const WnTile& t, uint32_t lane, const WnDir& dir, uint32_t frame,
                       int64_t param, int64_t null_bits, int64_t* __restrict__ dst) {
  uint32_t pb = t.pbase, qb = t.qbase;
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    const uint32_t r = t.r0 + static_cast<uint32_t>(j) * kWave;
    const uint64_t pm = gc_item_tails(t.ptails, j), qm = gc_item_tails(t.qtails, j);
    const uint32_t p = pb + lane_rank(pm), q = qb + lane_rank(qm);
    pb += static_cast<uint32_t>(__popcll(pm));
    qb += static_cast<uint32_t>(__popcll(qm));
    if (r < n) {
      const uint64_t k = static_cast<uint64_t>(param);
      int64_t w = null_bits;
      if constexpr (KIND == HDK_WIN_LAG) {
        const uint32_t start = p ? dir.part_end[p - 1] + 1u : 0u;
        if (k <= r - start) {
          w = col[r - static_cast<uint32_t>(k)];
        }
      } else if constexpr (KIND == HDK_WIN_LEAD) {
        if (k <= dir.part_end[p] - r) {
          w = col[r + static_cast<uint32_t>(k)];
        }
      } else if constexpr (KIND == HDK_WIN_FIRST_VALUE) {
        w = col[p ? dir.part_end[p - 1] + 1u : 0u];
      } else {  // HDK_WIN_LAST_VALUE
        w = col[frame == HDK_FRAME_ROWS ? r : frame == HDK_FRAME_RANGE ? dir.peer_end[q] : dir.part_end[p]];
      }
      dst[r] = w;
    }
  }
}

// One aggregate over one tile: at every row the value over the rows of its partition up to it (the ROWS frame).  Every
// wave runs its 16 items in row order with the partial of the partition that is open at the end of an item carried to the
// next (from lane 63, unless that lane is a tail).  The rows before the wave's first tail cannot be finished yet -- their
// partition may have begun in an earlier wave or tile --: they are marked pending and receive what enters the wave once
// the waves have exchanged what they end with.
template <uint32_t OP, bool AVG>
HDK_DEV void wn_scan(const int64_t* __restrict__ col, uint32_t n, const GcOut& o, uint32_t r0, uint32_t lane, uint32_t wave,
                     uint32_t tails, int64_t in_v, uint32_t in_c, int64_t (&s_v)[kGcWaves], uint32_t (&s_c)[kGcWaves],
                     uint32_t (&s_t)[kGcWaves], int64_t* __restrict__ dst) {
  int64_t x[kGcItems];
  uint32_t c[kGcItems];
  if constexpr (OP != GC_COUNT_STAR) {
#pragma unroll
    for (int j = 0; j < kGcItems; ++j) {
      const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
      x[j] = gc_load(col + (r < n ? r : n - 1));
    }
  }
  int64_t carry_v = gc_identity<OP>();  // of the partition that is open where item j begins (wave-uniform)
  uint32_t carry_c = 0;
  bool seen = false;     // a tail in an earlier item of this wave
  uint32_t pending = 0;  // bit j: this lane's row of item j lies before the wave's first tail, or is it
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
    bool has = r < n;
    if constexpr (OP != GC_COUNT_STAR) {
      has = has && !(o.nullable && x[j] == o.null_bits);
    }
    const uint64_t nn = __builtin_amdgcn_ballot_w64(has);
    const uint64_t mj = gc_item_tails(tails, j);
    const uint64_t below = mj & ((uint64_t(1) << lane) - 1);  // the tails before this lane
    const uint32_t s = below ? 64u - static_cast<uint32_t>(__clzll(static_cast<long long>(below))) : 0u;  // where this lane's partition starts
    int64_t xx = gc_identity<OP>();
    if constexpr (!gc_counts<OP>()) {
      xx = has ? x[j] : xx;
#pragma unroll
      for (int dd = 1; dd < kWave; dd <<= 1) {
        const int64_t up = gc_shfl_up(xx, dd);
        if (lane >= s + static_cast<uint32_t>(dd)) {
          xx = gc_combine<OP>(up, xx);
        }
      }
    }
    // the non-NULL words of lanes s .. lane
    uint32_t cc = static_cast<uint32_t>(__popcll(nn & (~uint64_t(0) >> (63u - lane)) & (~uint64_t(0) << s)));
    if (below == 0) {  // the partition reaches back into the item before
      xx = gc_combine<OP>(carry_v, xx);
      cc += carry_c;
      pending |= seen ? 0u : 1u << j;
    }
    x[j] = xx;
    c[j] = cc;
    const bool closed = (mj >> (kWave - 1)) & 1u;
    const int64_t last_v = gc_lane63(xx);
    const uint32_t last_c = __builtin_amdgcn_readlane(cc, kWave - 1);
    carry_v = closed ? gc_identity<OP>() : last_v;
    carry_c = closed ? 0u : last_c;
    seen = seen || mj != 0;
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
#pragma unroll
  for (int j = 0; j < kGcItems; ++j) {
    const uint32_t r = r0 + static_cast<uint32_t>(j) * kWave;
    const bool pend = (pending >> j) & 1u;
    const int64_t v = pend ? gc_combine<OP>(in_v, x[j]) : x[j];
    const uint32_t cnt = pend ? in_c + c[j] : c[j];
    if (r < n) {
      if constexpr (AVG) {  // (double)sum / (double)count, the reference's pair_to_double
        const double sum = OP == GC_SUM_F ? bits_to_double(v) : static_cast<double>(v);
        dst[r] = cnt ? double_to_bits(sum / static_cast<double>(cnt)) : HDK_NULL_DOUBLE_BITS;
      } else {
        dst[r] = gc_result<OP>(v, cnt, o.null_bits);
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kGcBlock) void hdk_window_rows(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n, WnDesc d,
                                                             uint32_t ntiles, const uint32_t* __restrict__ part_offs,
                                                             const uint32_t* __restrict__ peer_offs, WnDir dir,
                                                             const int64_t* __restrict__ carv, const uint32_t* __restrict__ carc,
                                                             int64_t* __restrict__ out, uint64_t out_capacity) {
  __shared__ uint32_t s_wave[kGcWaves];
  __shared__ int64_t s_v[kGcWaves];
  __shared__ uint32_t s_c[kGcWaves], s_t[kGcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const WnTile t = wn_locate(cols, capacity, n, d, tile, lane, wave, part_offs, peer_offs, s_wave);
    for (uint32_t a = 0; a < d.nouts; ++a) {
      const WnOut o = d.out[a];
      const int64_t* col = cols + static_cast<uint64_t>(o.g.col) * capacity;
      int64_t* dst = out + static_cast<uint64_t>(a) * out_capacity;
      if (o.g.op == GC_ID) {
#define HDK_WN_RANK(K) \
  case K: wn_rank<K>(n, t, lane, dir, o.param, dst); break;
#define HDK_WN_GATHER(K) \
  case K: wn_gather<K>(col, n, t, lane, dir, o.frame, o.param, o.g.null_bits, dst); break;
        switch (o.kind) {
          HDK_WN_RANK(HDK_WIN_ROW_NUMBER)
          HDK_WN_RANK(HDK_WIN_RANK)
          HDK_WN_RANK(HDK_WIN_DENSE_RANK)
          HDK_WN_RANK(HDK_WIN_PERCENT_RANK)
          HDK_WN_RANK(HDK_WIN_CUME_DIST)
          HDK_WN_RANK(HDK_WIN_NTILE)
          HDK_WN_GATHER(HDK_WIN_LAG)
          HDK_WN_GATHER(HDK_WIN_LEAD)
          HDK_WN_GATHER(HDK_WIN_FIRST_VALUE)
          HDK_WN_GATHER(HDK_WIN_LAST_VALUE)
          default: break;
        }
#undef HDK_WN_RANK
#undef HDK_WN_GATHER
        continue;
      }
      const int64_t in_v = carv[static_cast<uint64_t>(a) * ntiles + tile];
      const uint32_t in_c = carc[static_cast<uint64_t>(a) * ntiles + tile];
      if (o.avg) {
        if (o.g.op == GC_SUM_F) {
          wn_scan<GC_SUM_F, true>(col, n, o.g, t.r0, lane, wave, t.ptails, in_v, in_c, s_v, s_c, s_t, dst);
        } else {
          wn_scan<GC_SUM_I, true>(col, n, o.g, t.r0, lane, wave, t.ptails, in_v, in_c, s_v, s_c, s_t, dst);
        }
        continue;
      }
#define HDK_GC_CASE(OP) \
  case OP: wn_scan<OP, false>(col, n, o.g, t.r0, lane, wave, t.ptails, in_v, in_c, s_v, s_c, s_t, dst); break;
      switch (o.g.op) {
        HDK_GC_AGG_CASES
        default: break;
      }
#undef HDK_GC_CASE
    }
  }
}

// RANGE and PARTITION aggregates: every row takes the word of its peer group's or partition's last row, which holds the
// frame's value since hdk_window_rows and is not written here
__global__ __launch_bounds__(kGcBlock) void hdk_window_broadcast(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n,
                                                                  WnDesc d, uint32_t ntiles, const uint32_t* __restrict__ part_offs,
                                                                  const uint32_t* __restrict__ peer_offs, WnDir dir, int64_t* out,
                                                                  uint64_t out_capacity) {
  __shared__ uint32_t s_wave[kGcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const WnTile t = wn_locate(cols, capacity, n, d, tile, lane, wave, part_offs, peer_offs, s_wave);
    for (uint32_t a = 0; a < d.nouts; ++a) {
      const WnOut o = d.out[a];
      if (o.g.op == GC_ID || o.frame == HDK_FRAME_ROWS) {
        continue;
      }
      int64_t* dst = out + static_cast<uint64_t>(a) * out_capacity;
      const bool peers = o.frame == HDK_FRAME_RANGE;
      uint32_t pb = t.pbase, qb = t.qbase;
#pragma unroll
      for (int j = 0; j < kGcItems; ++j) {
        const uint32_t r = t.r0 + static_cast<uint32_t>(j) * kWave;
        const uint64_t pm = gc_item_tails(t.ptails, j), qm = gc_item_tails(t.qtails, j);
        const uint32_t p = pb + lane_rank(pm), q = qb + lane_rank(qm);
        pb += static_cast<uint32_t>(__popcll(pm));
        qb += static_cast<uint32_t>(__popcll(qm));
        if (r < n) {
          const uint32_t from = peers ? dir.peer_end[q] : dir.part_end[p];
          if (from != r) {
            dst[r] = dst[from];
          }
        }
      }
    }
  }
}

static size_t wn_tiles(uint64_t num_rows) { return static_cast<size_t>((num_rows + kGcTile - 1) / kGcTile); }
static size_t wn_counts_bytes(size_t ntiles) { return align256((ntiles + 1) * sizeof(uint32_t)); }
static size_t wn_values_bytes(size_t ntiles, int32_t num_outs) { return align256(ntiles * static_cast<size_t>(num_outs) * sizeof(int64_t)); }
static size_t wn_nonnull_bytes(size_t ntiles, int32_t num_outs) { return align256(ntiles * static_cast<size_t>(num_outs) * sizeof(uint32_t)); }
static size_t wn_dir_bytes(uint64_t num_rows) { return align256(static_cast<size_t>(num_rows) * sizeof(uint32_t)); }

static bool wn_is_aggregate(uint8_t kind) { return kind >= HDK_WIN_AVG && kind <= HDK_WIN_COUNT; }
static bool wn_is_ranking(uint8_t kind) { return kind <= HDK_WIN_NTILE; }

}  // namespace hdk

using namespace hdk;

// [partition counters + 1][peer counters + 1][num_outs x ntiles partial values][num_outs x ntiles non-NULL counts]
// [part_end: num_rows][part_lastq: num_rows][peer_end: num_rows]
extern "C" size_t hdk_hip_window_columns_workspace_bytes(uint64_t num_rows, int32_t num_outs) {
  const size_t ntiles = wn_tiles(num_rows);
  const int32_t outs = num_outs < 0 ? 0 : num_outs;
  return 2 * wn_counts_bytes(ntiles) + wn_values_bytes(ntiles, outs) + wn_nonnull_bytes(ntiles, outs) + 3 * wn_dir_bytes(num_rows);
}

extern "C" int32_t hdk_hip_window_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                                          const int32_t* part_cols, int32_t num_part, const int32_t* order_cols, int32_t num_order,
                                          const hdk_hip_window_out* outs, int32_t num_outs, int64_t* out_cols, uint64_t out_capacity,
                                          void* workspace, size_t workspace_bytes, int32_t device_id, void* stream) {
  HDK_REQUIRE(cols && outs && out_cols, "hdk_hip_window_columns: NULL argument (cols, outs and out_cols are required)");
  HDK_REQUIRE(num_cols >= 1, "hdk_hip_window_columns: num_cols %d", num_cols);
  HDK_REQUIRE(num_part >= 0 && num_part <= HDK_HIP_MAX_WINDOW_KEYS, "hdk_hip_window_columns: num_part %d outside 0..%d", num_part,
              HDK_HIP_MAX_WINDOW_KEYS);
  HDK_REQUIRE(num_order >= 0 && num_order <= HDK_HIP_MAX_WINDOW_KEYS, "hdk_hip_window_columns: num_order %d outside 0..%d", num_order,
              HDK_HIP_MAX_WINDOW_KEYS);
  HDK_REQUIRE(num_outs >= 1 && num_outs <= HDK_HIP_MAX_WINDOW_OUTS, "hdk_hip_window_columns: num_outs %d outside 1..%d", num_outs,
              HDK_HIP_MAX_WINDOW_OUTS);
  HDK_REQUIRE(part_cols || num_part == 0, "hdk_hip_window_columns: NULL part_cols with num_part %d", num_part);
  HDK_REQUIRE(order_cols || num_order == 0, "hdk_hip_window_columns: NULL order_cols with num_order %d", num_order);
  WnDesc d;
  memset(&d, 0, sizeof(d));
  d.part.nkeys = static_cast<uint32_t>(num_part);
  d.order.nkeys = static_cast<uint32_t>(num_order);
  d.nouts = static_cast<uint32_t>(num_outs);
  for (int32_t k = 0; k < num_part; ++k) {
    HDK_REQUIRE(part_cols[k] >= 0 && part_cols[k] < num_cols, "hdk_hip_window_columns: partition key %d names column %d of %d", k,
                part_cols[k], num_cols);
    d.part.key_col[k] = static_cast<uint32_t>(part_cols[k]);
  }
  for (int32_t k = 0; k < num_order; ++k) {
    HDK_REQUIRE(order_cols[k] >= 0 && order_cols[k] < num_cols, "hdk_hip_window_columns: order key %d names column %d of %d", k,
                order_cols[k], num_cols);
    d.order.key_col[k] = static_cast<uint32_t>(order_cols[k]);
  }
  bool aggregates = false, broadcast = false;
  for (int32_t i = 0; i < num_outs; ++i) {
    const hdk_hip_window_out& o = outs[i];
    HDK_REQUIRE(o.kind <= HDK_WIN_COUNT, "hdk_hip_window_columns: out %d has kind %d (0..%d)", i, static_cast<int>(o.kind),
                static_cast<int>(HDK_WIN_COUNT));
    HDK_REQUIRE(o.frame <= HDK_FRAME_PARTITION, "hdk_hip_window_columns: out %d has frame %d (ROWS, RANGE or PARTITION)", i,
                static_cast<int>(o.frame));
    const bool count_star = o.kind == HDK_WIN_COUNT && o.col < 0;
    const bool ranking = wn_is_ranking(o.kind);
    HDK_REQUIRE(ranking || count_star || (o.col >= 0 && o.col < num_cols), "hdk_hip_window_columns: out %d names column %d of %d", i,
                o.col, num_cols);
    HDK_REQUIRE(o.param >= 0, "hdk_hip_window_columns: out %d has param %lld (negative)", i, static_cast<long long>(o.param));
    HDK_REQUIRE(o.kind != HDK_WIN_NTILE || o.param >= 1, "hdk_hip_window_columns: out %d is an NTILE with param %lld (n >= 1)", i,
                static_cast<long long>(o.param));
    WnOut& w = d.out[i];
    w.g.col = ranking || count_star ? 0u : static_cast<uint32_t>(o.col);
    w.g.nullable = o.nullable ? 1u : 0u;
    w.g.null_bits = o.null_bits;
    w.g.op = GC_ID;
    w.kind = o.kind;
    w.frame = o.frame;
    w.param = o.param;
    if (o.kind == HDK_WIN_COUNT) {
      // (a column that cannot be NULL counts its rows: no load)
      w.g.op = count_star || !o.nullable ? GC_COUNT_STAR : GC_COUNT;
    } else if (o.kind == HDK_WIN_SUM || o.kind == HDK_WIN_AVG) {
      w.g.op = o.is_fp ? GC_SUM_F : GC_SUM_I;
      w.avg = o.kind == HDK_WIN_AVG;
    } else if (o.kind == HDK_WIN_MIN) {
      w.g.op = o.is_fp ? GC_MIN_F : GC_MIN_I;
    } else if (o.kind == HDK_WIN_MAX) {
      w.g.op = o.is_fp ? GC_MAX_F : GC_MAX_I;
    }
    if (wn_is_aggregate(o.kind)) {
      aggregates = true;
      broadcast = broadcast || o.frame != HDK_FRAME_ROWS;
    }
  }
  HDK_REQUIRE(num_rows < (uint64_t(1) << 32), "hdk_hip_window_columns: num_rows %llu does not fit 32-bit row indices",
              static_cast<unsigned long long>(num_rows));
  HDK_REQUIRE(num_rows <= capacity, "hdk_hip_window_columns: num_rows %llu exceeds the capacity %llu",
              static_cast<unsigned long long>(num_rows), static_cast<unsigned long long>(capacity));
  HDK_REQUIRE(out_capacity >= num_rows, "hdk_hip_window_columns: out_capacity %llu is below num_rows %llu",
              static_cast<unsigned long long>(out_capacity), static_cast<unsigned long long>(num_rows));
  const size_t need = hdk_hip_window_columns_workspace_bytes(num_rows, num_outs);
  HDK_REQUIRE(!workspace || workspace_bytes >= need, "hdk_hip_window_columns: workspace of %zu bytes, %zu needed", workspace_bytes,
              need);
  HDK_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "hdk_hip_window_columns: workspace %p is not 8-byte aligned",
              workspace);
  {
    const MemBlock blk[] = {
        {"cols", reinterpret_cast<uintptr_t>(cols), static_cast<uint64_t>(num_cols) * capacity * 8},
        {"out_cols", reinterpret_cast<uintptr_t>(out_cols), static_cast<uint64_t>(num_outs) * out_capacity * 8},
        {"workspace", reinterpret_cast<uintptr_t>(workspace), workspace ? static_cast<uint64_t>(need) : 0},
    };
    const int32_t bad = require_disjoint("hdk_hip_window_columns", blk, sizeof(blk) / sizeof(blk[0]));
    if (bad) return bad;
  }
  if (num_rows == 0) {
    return HDK_HIP_OK;
  }
  hipStream_t s;
  int32_t st = device_enter(device_id, stream, &s);
  if (st) return st;
  AsyncScratch mem(s);
  st = acquire_workspace(mem, &workspace, need);
  if (st) return st;
  const uint32_t n = static_cast<uint32_t>(num_rows);
  const uint32_t ntiles = static_cast<uint32_t>(wn_tiles(num_rows));
  int8_t* at = static_cast<int8_t*>(workspace);
  uint32_t* part_tiles = reinterpret_cast<uint32_t*>(at);
  at += wn_counts_bytes(ntiles);
  uint32_t* peer_tiles = reinterpret_cast<uint32_t*>(at);
  at += wn_counts_bytes(ntiles);
  int64_t* sufv = reinterpret_cast<int64_t*>(at);
  at += wn_values_bytes(ntiles, num_outs);
  uint32_t* sufc = reinterpret_cast<uint32_t*>(at);
  at += wn_nonnull_bytes(ntiles, num_outs);
  WnDir dir;
  dir.part_end = reinterpret_cast<uint32_t*>(at);
  at += wn_dir_bytes(num_rows);
  dir.part_lastq = reinterpret_cast<uint32_t*>(at);
  at += wn_dir_bytes(num_rows);
  dir.peer_end = reinterpret_cast<uint32_t*>(at);
  const dim3 grid(persistent_grid(device_props(device_id), ntiles)), block(kGcBlock);
  hipLaunchKernelGGL(hdk_window_count, grid, block, 0, s, cols, capacity, n, d, ntiles, part_tiles, peer_tiles,
                     aggregates ? sufv : nullptr, aggregates ? sufc : nullptr);
  launch_counts_scan(part_tiles, ntiles, kGcScanPer, nullptr, s);
  launch_counts_scan(peer_tiles, ntiles, kGcScanPer, nullptr, s);
  if (aggregates) {
    hipLaunchKernelGGL(hdk_window_carry_scan, dim3(static_cast<unsigned>(num_outs)), dim3(kGcCarryBlock), 0, s, d, ntiles, part_tiles,
                       sufv, sufc);
  }
  hipLaunchKernelGGL(hdk_window_directory, grid, block, 0, s, cols, capacity, n, d, ntiles, part_tiles, peer_tiles, dir);
  hipLaunchKernelGGL(hdk_window_rows, grid, block, 0, s, cols, capacity, n, d, ntiles, part_tiles, peer_tiles, dir, sufv, sufc,
                     out_cols, out_capacity);
  if (broadcast) {
    hipLaunchKernelGGL(hdk_window_broadcast, grid, block, 0, s, cols, capacity, n, d, ntiles, part_tiles, peer_tiles, dir, out_cols,
                       out_capacity);
  }
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
