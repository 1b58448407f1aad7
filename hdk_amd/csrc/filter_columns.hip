// filter_columns.hip -- HAVING over dense 8-byte result columns in HBM: the rows on which a predicate is TRUE, compacted.
//
// Device form of the reference's filter step over a temporary table (the previous step's ResultSet, materialised as
// ColumnarResults): the comparisons are DEF_CMP_NULLABLE* (omniscidb/QueryEngine/RuntimeFunctions.cpp:83-117: a NULL
// operand makes the comparison NULL), combined by logical_not / logical_and / logical_or (:355-384); a row is kept only
// when the whole predicate is TRUE.  The input is what hdk_hip_columnarize_result and hdk_hip_sort_columns write.
//
// Three launches on one stream, ordered by nothing but the stream (no block ever waits for another block):
//   hdk_filter_count    persistent grid over tiles of kFcTile rows: every leaf of every row into TRUE / NULL bit masks
//                       (bit j of a lane's mask = its j-th row of the tile), the postfix program over the masks -- no
//                       per-row control flow --, one pass bit per row (a 64-bit ballot word per wave-row, which lands at
//                       bits[row / 64]) and the tile's count -> workspace
//   hdk_counts_scan<4>  one block (column_scan.hip): exclusive scan of the tile counts in place, the total -> *row_count
//   hdk_filter_compact  per tile: a tile without a passing row is skipped unread; otherwise the tile's 64 ballot words,
//                       rank = tile offset + words before + mbcnt, and every column loaded only for passing rows and
//                       written at column + rank
// The leaves and the program travel as a POD kernel argument (FcDesc): the row loops read them from scalar registers.
// The host orders the leaves by their left-hand column (and renames them in the program), and the count pass keeps the
// left-hand column of the previous leaf in registers: `n > 100 AND n < 500` reads n once.  A right-hand COLUMN is loaded
// for its leaf.  Traffic: count 8n per column read + n/8; compact n/8 + 16 bytes per column and passing row.
#include <string.h>

#include "column_primitives.h"
#include "host_common.h"

namespace hdk {

constexpr int kFcBlock = kTileBlock;
constexpr int kFcItems = 16;  // rows per thread and tile
constexpr uint32_t kFcTile = kFcBlock * kFcItems;
constexpr int kFcWaves = kFcBlock / kWave;
constexpr int kFcWords = kFcItems * kFcWaves;  // ballot words of a tile, in row order: word j * kFcWaves + wave
static_assert(kFcWords == kWave, "one wave scans the ballot words of a tile");
static_assert(kFcItems <= 32, "a lane's rows are one 32-bit mask");
constexpr ScanPer kFcScanPer = SCAN_PER_4;  // tile counts per thread and trip of the scan
constexpr int kFcStack = HDK_HIP_MAX_HAVING_LEAVES;  // 16 ops hold at most 8 pushes beside their 7 binary operators

enum FcFlag : uint32_t {
  FC_RHS_COL = 1u,
  FC_CMP_FP = 2u,
  FC_LHS_FP = 4u,
  FC_LHS_NULLABLE = 8u,
  FC_RHS_FP = 16u,
  FC_RHS_NULLABLE = 32u
};

struct FcLeaf {
  uint32_t lhs_col, rhs_col;
  uint32_t cmp, flags;
  int64_t lhs_null, rhs_null;
  int64_t rhs_lit;
};

struct FcDesc {
  uint32_t nleaves, nprog;
  uint64_t prog[2];  // byte i of the program: (prog[i / 8] >> 8 * (i % 8)) & 255 -- shifts of scalars, no indexing
  FcLeaf leaf[HDK_HIP_MAX_HAVING_LEAVES];
};

// the columns are read once per pass: every load is non-temporal
HDK_DEV int64_t fc_load(const int64_t* p) { return nt_load<int64_t>(p, 0); }

HDK_DEV uint64_t fc_shfl64(uint64_t v, uint32_t src) {
  const uint32_t lo = __shfl(static_cast<uint32_t>(v), static_cast<int>(src), kWave);
  const uint32_t hi = __shfl(static_cast<uint32_t>(v >> 32), static_cast<int>(src), kWave);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// bit j: a[j] <cmp> b[j], as int64 or (FP) as doubles with the C operators
template <bool FP>
HDK_DEV uint32_t fc_compare(uint32_t cmp, const int64_t (&a)[kFcItems], const int64_t (&b)[kFcItems], bool a_fp, bool b_fp) {
  uint32_t m = 0;
#define HDK_FC_BITS(OP)                                                                       \
  _Pragma("unroll") for (int j = 0; j < kFcItems; ++j) {                                      \
    bool t;                                                                                   \
    if (FP) {                                                                                 \
      const double x = a_fp ? bits_to_double(a[j]) : static_cast<double>(a[j]);               \
      const double y = b_fp ? bits_to_double(b[j]) : static_cast<double>(b[j]);               \
      t = x OP y;                                                                             \
    } else {                                                                                  \
      t = a[j] OP b[j];                                                                       \
    }                                                                                         \
    m |= t ? 1u << j : 0u;                                                                    \
  }
  switch (cmp) {
    case HDK_CMP_EQ: HDK_FC_BITS(==) break;
    case HDK_CMP_NE: HDK_FC_BITS(!=) break;
    case HDK_CMP_LT: HDK_FC_BITS(<) break;
    case HDK_CMP_GT: HDK_FC_BITS(>) break;
    case HDK_CMP_LE: HDK_FC_BITS(<=) break;
    default: HDK_FC_BITS(>=) break;
  }
#undef HDK_FC_BITS
  return m;
}

// Row r of a tile belongs to thread r % kFcBlock, item r / kFcBlock: consecutive lanes read consecutive rows, and the
// ballot of item j in wave w covers rows [tile * kFcTile + (j * kFcWaves + w) * 64, + 64): word (tile * 64 + j * 4 + w) of
// `bits` is bits[row / 64].  (tile * kFcTile + 4095 never exceeds 2^32 - 1: tile < ceil(n / kFcTile), n < 2^32.)
__global__ __launch_bounds__(kFcBlock) void hdk_filter_count(const int64_t* __restrict__ cols, uint64_t capacity, uint32_t n,
                                                              FcDesc d, uint32_t ntiles, uint32_t* __restrict__ tile_counts,
                                                              uint64_t* __restrict__ bits) {
  __shared__ uint32_t s_wave[kFcWaves];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t r0 = tile * kFcTile + threadIdx.x;
    // leaf k: bit j = TRUE / NULL for this lane's j-th row
    uint32_t lt[HDK_HIP_MAX_HAVING_LEAVES], ln[HDK_HIP_MAX_HAVING_LEAVES];
#pragma unroll
    for (int k = 0; k < HDK_HIP_MAX_HAVING_LEAVES; ++k) {
      lt[k] = 0;
      ln[k] = 0;
    }
    int64_t a[kFcItems], b[kFcItems];
    uint32_t held = ~0u;  // the column in a[]
    for (uint32_t qi = 0; qi < d.nleaves; ++qi) {  // (wave-uniform: the leaf comes from scalar registers)
      const FcLeaf q = d.leaf[qi];
      if (q.lhs_col != held) {
        held = q.lhs_col;
        const int64_t* col = cols + static_cast<uint64_t>(held) * capacity;
#pragma unroll
        for (int j = 0; j < kFcItems; ++j) {
          // (a row past the end reads the last row instead, so that the loads of a tile are issued together)
          const uint32_t r = r0 + static_cast<uint32_t>(j) * kFcBlock;
          a[j] = fc_load(col + (r < n ? r : n - 1));
        }
      }
      uint32_t isnull = 0;
      if (q.flags & FC_RHS_COL) {
        const int64_t* col = cols + static_cast<uint64_t>(q.rhs_col) * capacity;
#pragma unroll
        for (int j = 0; j < kFcItems; ++j) {
          const uint32_t r = r0 + static_cast<uint32_t>(j) * kFcBlock;
          b[j] = fc_load(col + (r < n ? r : n - 1));
        }
        if (q.flags & FC_RHS_NULLABLE) {
#pragma unroll
          for (int j = 0; j < kFcItems; ++j) {
            isnull |= b[j] == q.rhs_null ? 1u << j : 0u;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < kFcItems; ++j) {
          b[j] = q.rhs_lit;
        }
      }
      if (q.flags & FC_LHS_NULLABLE) {
#pragma unroll
        for (int j = 0; j < kFcItems; ++j) {
          isnull |= a[j] == q.lhs_null ? 1u << j : 0u;
        }
      }
      const uint32_t t = (q.flags & FC_CMP_FP) ? fc_compare<true>(q.cmp, a, b, q.flags & FC_LHS_FP, q.flags & FC_RHS_FP)
                                               : fc_compare<false>(q.cmp, a, b, false, false);
#pragma unroll
      for (int k = 0; k < HDK_HIP_MAX_HAVING_LEAVES; ++k) {
        lt[k] = static_cast<uint32_t>(k) == qi ? t & ~isnull : lt[k];  // (a NULL operand: the comparison is NULL, not TRUE)
        ln[k] = static_cast<uint32_t>(k) == qi ? isnull : ln[k];
      }
    }
    // the value stack, st[0] the top: a wave-uniform program over per-lane masks
    uint32_t st[kFcStack], sn[kFcStack];
#pragma unroll
    for (int k = 0; k < kFcStack; ++k) {
      st[k] = 0;
      sn[k] = 0;
    }
    for (uint32_t i = 0; i < d.nprog; ++i) {
      const uint32_t op = static_cast<uint32_t>((i < 8 ? d.prog[0] : d.prog[1]) >> (8u * (i & 7u))) & 255u;
      if (op < HDK_F_AND) {
#pragma unroll
        for (int k = kFcStack - 1; k > 0; --k) {
          st[k] = st[k - 1];
          sn[k] = sn[k - 1];
        }
        uint32_t vt = lt[0], vn = ln[0];
#pragma unroll
        for (int k = 1; k < HDK_HIP_MAX_HAVING_LEAVES; ++k) {
          vt = op == static_cast<uint32_t>(k) ? lt[k] : vt;
          vn = op == static_cast<uint32_t>(k) ? ln[k] : vn;
        }
        st[0] = vt;
        sn[0] = vn;
      } else if (op == HDK_F_NOT) {
        st[0] = ~(st[0] | sn[0]);  // NULL stays NULL, TRUE <-> FALSE
      } else {
        uint32_t rt, rn;
        if (op == HDK_F_AND) {
          const uint32_t fa = ~(st[0] | sn[0]), fb = ~(st[1] | sn[1]);  // FALSE operands
          rt = st[0] & st[1];
          rn = ~(rt | fa | fb);
        } else {
          rt = st[0] | st[1];
          rn = ~rt & (sn[0] | sn[1]);
        }
        st[0] = rt;
        sn[0] = rn;
#pragma unroll
        for (int k = 1; k < kFcStack - 1; ++k) {
          st[k] = st[k + 1];
          sn[k] = sn[k + 1];
        }
      }
    }
    const uint32_t pass = st[0];
    uint32_t cnt = 0;  // of this wave
#pragma unroll
    for (int j = 0; j < kFcItems; ++j) {
      const uint32_t r = r0 + static_cast<uint32_t>(j) * kFcBlock;
      const uint64_t mask = __builtin_amdgcn_ballot_w64(r < n && ((pass >> j) & 1u));
      if (lane == 0) {
        bits[static_cast<uint64_t>(tile) * kFcWords + static_cast<uint32_t>(j) * kFcWaves + wave] = mask;
      }
      cnt += static_cast<uint32_t>(__popcll(mask));
    }
    block_store_tile_count(s_wave, cnt, tile_counts + tile);
  }
}

// (no ballot here: the pass bits come from the count pass; every wave scans the tile's 64 words for itself)
__global__ __launch_bounds__(kFcBlock) void hdk_filter_compact(const int64_t* __restrict__ cols, uint64_t capacity,
                                                                uint32_t num_cols, uint32_t ntiles,
                                                                const uint32_t* __restrict__ tile_offs,
                                                                const uint64_t* __restrict__ bits, int64_t* __restrict__ out,
                                                                uint64_t out_capacity, uint32_t* __restrict__ perm_out) {
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t first = tile_offs[tile];
    if (tile_offs[tile + 1] == first || first >= out_capacity) {
      continue;  // no passing row in this tile, or all of them past the capacity (block-uniform)
    }
    const uint64_t word = bits[static_cast<uint64_t>(tile) * kFcWords + lane];
    const uint32_t c = static_cast<uint32_t>(__popcll(word));
    const uint32_t excl = wave_inclusive_sum(c, lane) - c;
    const uint64_t r0 = static_cast<uint64_t>(tile) * kFcTile + threadIdx.x;
    uint32_t flags = 0;
    uint64_t rank[kFcItems];
#pragma unroll
    for (int j = 0; j < kFcItems; ++j) {
      const uint32_t w = static_cast<uint32_t>(j) * kFcWaves + wave;
      const uint64_t mask = fc_shfl64(word, w);
      const uint32_t before = __shfl(excl, static_cast<int>(w), kWave);
      rank[j] = static_cast<uint64_t>(first) + before + lane_rank(mask);
      const bool f = ((mask >> lane) & 1u) && rank[j] < out_capacity;
      flags |= static_cast<uint32_t>(f) << j;
    }
    if (perm_out) {
#pragma unroll
      for (int j = 0; j < kFcItems; ++j) {
        if ((flags >> j) & 1u) {
          perm_out[rank[j]] = static_cast<uint32_t>(r0 + static_cast<uint32_t>(j) * kFcBlock);
        }
      }
    }
    for (uint32_t t = 0; t < num_cols; ++t) {
      const int64_t* src = cols + static_cast<uint64_t>(t) * capacity;
      int64_t* dst = out + static_cast<uint64_t>(t) * out_capacity;
      int64_t v[kFcItems];
#pragma unroll
      for (int j = 0; j < kFcItems; ++j) {
        v[j] = 0;
        if ((flags >> j) & 1u) {
          v[j] = fc_load(src + r0 + static_cast<uint32_t>(j) * kFcBlock);
        }
      }
#pragma unroll
      for (int j = 0; j < kFcItems; ++j) {
        if ((flags >> j) & 1u) {
          dst[rank[j]] = v[j];
        }
      }
    }
  }
}

static size_t fc_tiles(uint64_t num_rows) { return static_cast<size_t>((num_rows + kFcTile - 1) / kFcTile); }
static size_t fc_counts_bytes(size_t ntiles) { return align256((ntiles + 1) * sizeof(uint32_t)); }

// the program is well formed: no underflow, no leaf beyond `num_leaves`, one value left
static const char* fc_check_program(const uint8_t* ops, int32_t num_ops, int32_t num_leaves) {
  int depth = 0;
  for (int32_t i = 0; i < num_ops; ++i) {
    const uint8_t op = ops[i];
    if (op < HDK_F_AND) {
      if (op >= num_leaves) return "names a leaf index >= num_leaves";
      ++depth;
    } else if (op == HDK_F_NOT) {
      if (depth < 1) return "underflows its stack";
    } else if (op == HDK_F_AND || op == HDK_F_OR) {
      if (depth < 2) return "underflows its stack";
      --depth;
    } else {
      return "holds an unknown op";
    }
  }
  return depth == 1 ? nullptr : "does not leave exactly one value (final stack depth != 1)";
}

}  // namespace hdk

using namespace hdk;

extern "C" size_t hdk_hip_filter_columns_workspace_bytes(uint64_t num_rows) {
  const size_t ntiles = fc_tiles(num_rows);
  return fc_counts_bytes(ntiles) + ntiles * kFcWords * sizeof(uint64_t);
}

extern "C" int32_t hdk_hip_filter_columns(const int64_t* cols, uint64_t capacity, int32_t num_cols, uint64_t num_rows,
                                          const hdk_hip_having_leaf* leaves, int32_t num_leaves, const uint8_t* ops,
                                          int32_t num_ops, int64_t* out_cols, uint64_t out_capacity, uint64_t* row_count,
                                          uint32_t* perm_out, void* workspace, size_t workspace_bytes, int32_t device_id,
                                          void* stream) {
  HDK_REQUIRE(cols && leaves && row_count, "hdk_hip_filter_columns: NULL argument (cols, leaves and row_count are required)");
  HDK_REQUIRE(num_cols >= 1, "hdk_hip_filter_columns: num_cols %d", num_cols);
  HDK_REQUIRE(num_leaves >= 1 && num_leaves <= HDK_HIP_MAX_HAVING_LEAVES, "hdk_hip_filter_columns: num_leaves %d outside 1..%d",
              num_leaves, HDK_HIP_MAX_HAVING_LEAVES);
  for (int32_t i = 0; i < num_leaves; ++i) {
    const hdk_hip_having_leaf& l = leaves[i];
    HDK_REQUIRE(l.lhs_col >= 0 && l.lhs_col < num_cols, "hdk_hip_filter_columns: leaf %d names column %d of %d (lhs)", i, l.lhs_col,
                num_cols);
    HDK_REQUIRE(!l.rhs_is_col || (l.rhs_col >= 0 && l.rhs_col < num_cols),
                "hdk_hip_filter_columns: leaf %d names column %d of %d (rhs)", i, l.rhs_col, num_cols);
    HDK_REQUIRE(l.cmp >= HDK_CMP_EQ && l.cmp <= HDK_CMP_GE, "hdk_hip_filter_columns: leaf %d has cmp %d outside hdk_hip_cmp", i,
                static_cast<int>(l.cmp));
  }
  HDK_REQUIRE(num_ops >= 0 && num_ops <= HDK_HIP_MAX_FILTER_OPS && (num_ops == 0 || ops),
              "hdk_hip_filter_columns: a program of %d ops (0..%d, with a non-NULL ops)", num_ops, HDK_HIP_MAX_FILTER_OPS);
  if (num_ops) {
    const char* why = fc_check_program(ops, num_ops, num_leaves);
    HDK_REQUIRE(!why, "hdk_hip_filter_columns: malformed program: it %s", why);
  }
  HDK_REQUIRE(num_rows < (uint64_t(1) << 32), "hdk_hip_filter_columns: num_rows %llu does not fit 32-bit row indices",
              static_cast<unsigned long long>(num_rows));
  HDK_REQUIRE(num_rows <= capacity, "hdk_hip_filter_columns: num_rows %llu exceeds the capacity %llu",
              static_cast<unsigned long long>(num_rows), static_cast<unsigned long long>(capacity));
  const size_t need = hdk_hip_filter_columns_workspace_bytes(num_rows);
  HDK_REQUIRE(!workspace || workspace_bytes >= need, "hdk_hip_filter_columns: workspace of %zu bytes, %zu needed", workspace_bytes,
              need);
  HDK_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "hdk_hip_filter_columns: workspace %p is not 8-byte aligned",
              workspace);
  {
    // every block the call reads or writes; a block nothing is written to or read from (out_capacity == 0, count only)
    // has no bytes and overlaps nothing
    const bool writes = out_cols && out_capacity;
    const MemBlock blk[] = {
        {"cols", reinterpret_cast<uintptr_t>(cols), static_cast<uint64_t>(num_cols) * capacity * 8},
        {"out_cols", reinterpret_cast<uintptr_t>(out_cols), writes ? static_cast<uint64_t>(num_cols) * out_capacity * 8 : 0},
        {"perm_out", reinterpret_cast<uintptr_t>(perm_out), writes && perm_out ? out_capacity * 4 : 0},
        {"row_count", reinterpret_cast<uintptr_t>(row_count), 8},
        {"workspace", reinterpret_cast<uintptr_t>(workspace), workspace ? static_cast<uint64_t>(need) : 0},
    };
    const int32_t bad = require_disjoint("hdk_hip_filter_columns", blk, sizeof(blk) / sizeof(blk[0]));
    if (bad) return bad;
  }
  hipStream_t s;
  int32_t st = device_enter(device_id, stream, &s);
  if (st) return st;
  if (num_rows == 0) {
    HDK_HIP_CHECK(hipMemsetAsync(row_count, 0, sizeof(uint64_t), s));
    return HDK_HIP_OK;
  }

  // leaves in the order of their left-hand columns (stable), the program renamed to match
  FcDesc d;
  memset(&d, 0, sizeof(d));
  int order[HDK_HIP_MAX_HAVING_LEAVES], where[HDK_HIP_MAX_HAVING_LEAVES];
  for (int i = 0; i < num_leaves; ++i) {
    int k = i;
    for (; k > 0 && leaves[order[k - 1]].lhs_col > leaves[i].lhs_col; --k) {
      order[k] = order[k - 1];
    }
    order[k] = i;
  }
  d.nleaves = static_cast<uint32_t>(num_leaves);
  for (int k = 0; k < num_leaves; ++k) {
    const hdk_hip_having_leaf& l = leaves[order[k]];
    where[order[k]] = k;
    FcLeaf& q = d.leaf[k];
    q.lhs_col = static_cast<uint32_t>(l.lhs_col);
    q.rhs_col = l.rhs_is_col ? static_cast<uint32_t>(l.rhs_col) : 0u;
    q.cmp = l.cmp;
    q.flags = (l.rhs_is_col ? FC_RHS_COL : 0u) | (l.cmp_fp ? FC_CMP_FP : 0u) | (l.lhs_is_fp ? FC_LHS_FP : 0u) |
              (l.lhs_nullable ? FC_LHS_NULLABLE : 0u) | (l.rhs_is_fp ? FC_RHS_FP : 0u) |
              (l.rhs_is_col && l.rhs_nullable ? FC_RHS_NULLABLE : 0u);  // (a literal is never NULL)
    q.lhs_null = l.lhs_null_bits;
    q.rhs_null = l.rhs_null_bits;
    q.rhs_lit = l.rhs_lit;
  }
  uint8_t prog[HDK_HIP_MAX_FILTER_OPS];
  int nprog = 0;
  if (num_ops) {
    for (; nprog < num_ops; ++nprog) {
      prog[nprog] = ops[nprog] < HDK_F_AND ? static_cast<uint8_t>(where[ops[nprog]]) : ops[nprog];
    }
  } else {  // the plain conjunction: 0 1 AND 2 AND ... (2 * num_leaves - 1 <= 15 ops)
    for (int k = 0; k < num_leaves; ++k) {
      prog[nprog++] = static_cast<uint8_t>(k);
      if (k) prog[nprog++] = HDK_F_AND;
    }
  }
  d.nprog = static_cast<uint32_t>(nprog);
  for (int i = 0; i < nprog; ++i) {
    d.prog[i / 8] |= static_cast<uint64_t>(prog[i]) << (8 * (i % 8));
  }

  AsyncScratch mem(s);
  st = acquire_workspace(mem, &workspace, need);
  if (st) return st;
  const uint32_t ntiles = static_cast<uint32_t>(fc_tiles(num_rows));
  uint32_t* tiles = static_cast<uint32_t*>(workspace);
  uint64_t* bits = reinterpret_cast<uint64_t*>(static_cast<int8_t*>(workspace) + fc_counts_bytes(ntiles));
  const dim3 grid(persistent_grid(device_props(device_id), ntiles)), block(kFcBlock);
  hipLaunchKernelGGL(hdk_filter_count, grid, block, 0, s, cols, capacity, static_cast<uint32_t>(num_rows), d, ntiles, tiles, bits);
  launch_counts_scan(tiles, ntiles, kFcScanPer, row_count, s);
  if (out_cols && out_capacity) {
    hipLaunchKernelGGL(hdk_filter_compact, grid, block, 0, s, cols, capacity, static_cast<uint32_t>(num_cols), ntiles, tiles, bits,
                       out_cols, out_capacity, perm_out);
  }
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;
}
