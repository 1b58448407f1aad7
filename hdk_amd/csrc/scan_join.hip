// scan_join.hip -- the join families of the LDS strategy (route.h: FAM_LDS_JOIN, FAM_BH_BEHIND) and the clustering pre-pass:
//   hdk_join_agg_direct                  (scan_join_direct.h)   BASELINE config 3's shape probed in row order, or over tuples that
//                                                               hdk_cluster_by_key (scan_cluster.h) scattered by key range
//   hdk_join_agg_sliced                  (scan_join_sliced.h)   the same shape probed out of LDS, slice by slice
//   hdk_join_agg_sliced2                 (scan_join_sliced2.h)  the star shapes around it: group key, filters, lists of aggregates;
//                                                               also behind a baseline-hash plan whose key the kernel can bound
// with their matchers and launchers.  Every rule the matchers and launchers share -- slice and cluster geometry, the carve of a
// pass's scratch memory, when slices pay, what the column statistics must promise -- is defined once, first.  scan_agg.hip
// routes the rest of the LDS strategy and keeps the interpreter that stays armed behind the sliced passes (host_match.h).
#include "host_match.h"
#include "scan_bh_decl.h"
#include "scan_bh_host.h"
#include "scan_cluster.h"
#include "scan_join_direct.h"
#include "scan_join_sliced.h"
#include "scan_join_sliced2.h"

namespace hdk {

// ---- what the slice passes share ----------------------------------------------------------------------------------------------
// Do key-range slices pay for their scatter pass?  Only with row counts, never under HDK_HIP_LAUNCH_NO_CLUSTER_PROBES, and the
// key offset must fit the tuple's 32 bits; HDK_HIP_LAUNCH_CLUSTER_PROBES takes them whatever the sizes (tests).
static bool slices_worth_it(const hdk_hip_kernel_options* ko, uint64_t range) {
  if (!ko || ko->total_rows == 0 || (ko->flags & HDK_HIP_LAUNCH_NO_CLUSTER_PROBES)) return false;
  if (range >= 0xFFFFFFFFull) return false;
  const bool forced = (ko->flags & HDK_HIP_LAUNCH_CLUSTER_PROBES) != 0;
  // worth it when a probe in row order costs a memory line: table beyond the 4 MB L2s and the 256 MB Infinity Cache's
  // comfortable share, enough rows to pay for the scatter pass
  return forced || (range * 16 >= (32ull << 20) && ko->total_rows >= (32ull << 20));
}

// sub-slab and overflow capacities of the scatter pass: `rows` rows over sa->nbins slices; false: beyond the 32-bit cursors
static bool slice_buffer_geometry(uint64_t rows, SliceArgs* sa) {
  const uint64_t nsub = static_cast<uint64_t>(sa->nbins) * kSliceXcds;
  sa->sub = ((rows / nsub) * 17 / 16 + 4096 + 15) & ~15ull;
  sa->cap_ovf = rows / 8 + 4096;
  return sa->sub <= 0xFFFFFFF0ull && sa->cap_ovf <= 0xFFFFFFF0ull;
}

// a payload word travels as an int32 with two values to spare (kSliceNoMatch, kSliceNull): the column statistics of the fused
// inner column must say so (a word no column of the plan reads: nothing to promise)
static bool payload_fits_32_bits(const hdk_hip_col* pay) {
  return !pay || (pay->has_stats && pay->min_val > static_cast<int64_t>(INT32_MIN) + 1 && pay->max_val <= static_cast<int64_t>(INT32_MAX));
}

// Can x ride as the int32 half of an 8-byte tuple?  When the statistics allow (a nullable column gives up INT32_MIN for its
// NULL) and a column that may hold NULLs has a sentinel.  In: sa->x_null32 = the targets' leaves name x's NULL (sa->x_null).
// Settles x_null32 / x_null_is_stale whatever the answer; what a caller does with a wide x is its own business.
static bool x_fits_narrow(const hdk_hip_col* xcol, SliceArgs* sa) {
  const bool x_has_nulls = !xcol || !xcol->has_stats || xcol->has_nulls;
  bool narrow = xcol && xcol->has_stats && xcol->min_val >= static_cast<int64_t>(INT32_MIN) + (x_has_nulls ? 1 : 0) &&
                xcol->max_val <= static_cast<int64_t>(INT32_MAX);
  if (!x_has_nulls) {
    // no NULLs announced: INT32_MIN is an ordinary value; a NULL showing up anyway (the leaf is nullable, x_null is set)
    // is caught as stale by the scatter pass
    sa->x_null_is_stale = sa->x_null32;
    sa->x_null32 = 0;
  } else if (!sa->x_null32) {
    narrow = false;  // NULLs possible but no sentinel known from the leaves
  }
  return narrow;
}

// Scratch of the scatter pass: [level-1 tuples of `tw` words | level-2 tuples | cursors of both levels, mode word, probe words],
// cursors cleared.  `l2`: the launch has a second scatter level (or may have: its pointers are set either way).  scratch.p =
// nullptr: no scratch memory -- the caller probes in row order.
static int32_t carve_slice_scratch(AsyncScratch& scratch, SliceArgs& sa, size_t tw, Slice2Args* l2, hipStream_t s) {
  const size_t nsub = static_cast<size_t>(sa.nbins) * kSliceXcds;
  const size_t b_tuples = align256((nsub * sa.sub + sa.cap_ovf) * tw * 8);
  const size_t b_tuples2 = l2 && l2->two_level ? align256(static_cast<size_t>(l2->nslices) * l2->cap2 * 8) : 0;
  const size_t n_fill1 = nsub * kSliceCursorStride + 8;
  const size_t n_fill2 = l2 && l2->two_level ? static_cast<size_t>(l2->nslices) * kSliceCursorStride : 0;
  const size_t b_fill = align256((n_fill1 + n_fill2) * sizeof(uint32_t));
  if (hipMallocAsync(&scratch.p, b_tuples + b_tuples2 + b_fill, s) != hipSuccess) {
    (void)hipGetLastError();
    scratch.p = nullptr;
    return HDK_HIP_OK;
  }
  int8_t* q = static_cast<int8_t*>(scratch.p);
  sa.tuples = reinterpret_cast<int64_t*>(q);
  sa.fill = reinterpret_cast<uint32_t*>(q + b_tuples + b_tuples2);
  sa.fill_ovf = sa.fill + nsub * kSliceCursorStride;
  sa.mode = sa.fill_ovf + 1;
  sa.probe = sa.mode + 1;
  if (l2) {
    l2->tuples2 = reinterpret_cast<int64_t*>(q + b_tuples);
    l2->fill2 = sa.fill + n_fill1;
  }
  HDK_HIP_CHECK(hipMemsetAsync(sa.fill, 0, b_fill, s));
  return HDK_HIP_OK;
}

// Raises the probe pass's dynamic-LDS limit where `lds` needs it and asks how many of its blocks a CU holds.  0: no block this
// large here -- the launch is handed back.
static int probe_blocks_per_cu(const void* kernel, size_t lds) {
  if (lds > 48 * 1024 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kSliceAggBlock, lds) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    return 0;
  }
  return per_cu;
}

// ---- hdk_cluster_by_key (scan_cluster.h): geometry, carve and launch, for the pre-pass and for the clustered direct route ----------
constexpr uint64_t kClusterSubSlabs = static_cast<uint64_t>(kClusterBins) * kClusterXcds;

static void cluster_geometry(uint64_t rows, uint64_t range, ClusterArgs* ca) {
  ca->key_range = range;
  ca->bin_mult = (static_cast<uint64_t>(kClusterBins) << 32) / range;  // floor: bin <= kClusterBins - 1 for every key in range
  ca->sub = ((rows / kClusterSubSlabs) * 17 / 16 + 4096 + 15) & ~15ull;
  ca->cap_ovf = rows;
}

// Scratch of the pass: out[] -- one array per column, or (AoS) one of ncols-word tuples -- then the cursors, cleared, then `extra`
// bytes for the caller at *q.  *q = nullptr: no scratch memory -- the launch probes in row order.
static int32_t cluster_scratch(ClusterArgs& ca, size_t extra, hipStream_t s, void** scratch, int8_t** q) {
  const size_t b_out = align256((kClusterSubSlabs * ca.sub + ca.cap_ovf) * (ca.aos ? ca.ncols : 1) * 8);
  const size_t b_fill = align256((kClusterSubSlabs * kClusterCursorStride + 4) * sizeof(uint32_t));
  const int nout = ca.aos ? 1 : ca.ncols;
  *q = nullptr;
  if (hipMallocAsync(scratch, nout * b_out + b_fill + extra, s) != hipSuccess) {
    (void)hipGetLastError();
    *scratch = nullptr;
    return HDK_HIP_OK;
  }
  *q = static_cast<int8_t*>(*scratch);
  for (int c = 0; c < nout; ++c, *q += b_out) ca.out[c] = reinterpret_cast<int64_t*>(*q);
  ca.fill = reinterpret_cast<uint32_t*>(*q);
  ca.fill_ovf = ca.fill + kClusterSubSlabs * kClusterCursorStride;
  *q += b_fill;
  HDK_HIP_CHECK(hipMemsetAsync(ca.fill, 0, b_fill, s));
  return HDK_HIP_OK;
}
static void launch_cluster_by_key(const ClusterArgs& ca, const hdk_hip_device_properties* props, hipStream_t s) {
  const size_t lds = static_cast<size_t>(kClusterTile) * ca.ncols * 8 + kClusterTile + 16;
  const unsigned grid = resident_grid(reinterpret_cast<const void*>(hdk_cluster_by_key), kClusterBlock, lds, props);
  hipLaunchKernelGGL(hdk_cluster_by_key, dim3(grid), dim3(kClusterBlock), lds, s, ca);
}

// ---- clustering pre-pass for join probes (scan_cluster.h) -----------------------------------------------------------
bool route_cluster_prepass(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, LaunchRoute* r) {
  ClusterArgs* ca = &r->pre_as<ClusterArgs>();
  if (!ko || ko->total_rows == 0 || (ko->flags & HDK_HIP_LAUNCH_NO_CLUSTER_PROBES)) return false;
  if (ko->flags & (HDK_HIP_LAUNCH_FORCE_SCALAR | HDK_HIP_LAUNCH_FORCE_GENERIC)) return false;
  if (p->num_joins != 1 || p->query_kind == HDK_Q_PROJECTION || needs_join_loops(p) || p->num_filter_ops) return false;
  const hdk_hip_join& jn = p->joins[0];
  if ((jn.kind != HDK_JOIN_ONE_TO_ONE && jn.kind != HDK_JOIN_ONE_TO_ONE_FUSED) || !join_type_inner_like(jn.type)) return false;
  if (jn.null_mode == HDK_JOIN_NULL_BITWISE || jn.bucket > 1) return false;  // (a NULL key that matches: not dropped)
  int kc;
  if (!plain_outer_col(p, jn.outer_key, &kc)) return false;
  if (jn.max_key < jn.min_key || static_cast<uint64_t>(jn.max_key - jn.min_key) >= 0xFFFFFFFFull) return false;
  const uint64_t range = static_cast<uint64_t>(jn.max_key - jn.min_key) + 1;
  // Only on request.  Measured on C3 (256 M rows, 10 M-key dimension, 160 MB fused table): pre-pass 2.2 ms + probes over
  // the clustered rows 4.2 ms against 5.0 ms for probes in row order -- the batched interpreter that consumes the rows
  // needs 3.1 ms even when the whole table sits in L2, so the locality cannot pay for the pre-pass until a specialised
  // consumer exists.
  if (!(ko->flags & HDK_HIP_LAUNCH_CLUSTER_PROBES)) return false;
  memset(ca, 0, sizeof(*ca));
  for (int i = 0; i < HDK_HIP_MAX_COLS; ++i) ca->outer_slot[i] = -1;
  // the join key first, then every other outer column of the plan: all of them 8 bytes wide
  ca->buf_idx[0] = p->cols[kc].buf_idx;
  ca->outer_slot[kc] = 0;
  ca->ncols = 1;
  for (int i = 0; i < p->num_cols; ++i) {
    const hdk_hip_col& c = p->cols[i];
    if (c.table < 0) continue;  // payload word of a fused table: no buffer
    if (c.table != 0) continue;
    if (c.width != 8 || (c.kind != HDK_COL_INT && c.kind != HDK_COL_DOUBLE)) return false;
    if (c.buf_idx != i) return false;  // (plan.py numbers them alike; the parameter builder relies on it)
    if (i == kc) continue;
    if (ca->ncols == kClusterMaxCols) return false;
    ca->buf_idx[ca->ncols] = c.buf_idx;
    ca->outer_slot[i] = ca->ncols++;
  }
  if (p->cols[kc].width != 8 || p->cols[kc].kind != HDK_COL_INT || p->cols[kc].buf_idx != kc) return false;
  ca->ncols_total = p->num_cols;
  ca->key_min = jn.min_key;
  cluster_geometry(ko->total_rows, range, ca);
  return true;
}

// runs the pre-pass and points `kp` at the permuted data; *scratch is freed (stream-ordered) by the caller after the scan.
// Out of scratch memory is not an error: the launch then simply probes in row order.
int32_t launch_cluster_prepass(LaunchRoute& r, KernParams* kp, const hdk_hip_device_properties* props, hipStream_t s, void** scratch) {
  ClusterArgs ca = r.pre_as<ClusterArgs>();
  const uint64_t nfr = kClusterSubSlabs + 1;
  const uint32_t ntab_max = 1 + HDK_HIP_MAX_JOINS;
  const size_t b_colptrs = align256(nfr * ca.ncols_total * sizeof(void*));
  const size_t b_fragptrs = align256(nfr * sizeof(void*));
  const size_t b_rows = align256(nfr * ntab_max * sizeof(int64_t));
  int8_t* q;
  const int32_t st = cluster_scratch(ca, b_colptrs + b_fragptrs + 2 * b_rows + 256, s, scratch, &q);
  if (st || !q) return st;
  ca.col_ptrs = reinterpret_cast<const int8_t**>(q); q += b_colptrs;
  ca.frag_ptrs = reinterpret_cast<const int8_t* const**>(q); q += b_fragptrs;
  ca.num_rows = reinterpret_cast<int64_t*>(q); q += b_rows;
  ca.frag_offs = reinterpret_cast<uint64_t*>(q); q += b_rows;
  ca.num_fragments = reinterpret_cast<uint64_t*>(q);
  ca.kp = *kp;
  launch_cluster_by_key(ca, props, s);
  hipLaunchKernelGGL(hdk_cluster_params, dim3(8), dim3(256), 0, s, ca);
  HDK_HIP_CHECK(hipGetLastError());
  kp->col_buffers = reinterpret_cast<const int8_t* const* const*>(ca.frag_ptrs);
  kp->num_fragments = ca.num_fragments;
  kp->num_rows = ca.num_rows;
  kp->frag_row_offsets = ca.frag_offs;
  return HDK_HIP_OK;
}

// ---- hdk_join_agg_direct (scan_join_direct.h): the matcher ------------------------------------------------------------
static bool jd_leaf_from(const hdk_hip_plan* p, const hdk_hip_leaf& l, int kc, int xc, JdLeaf* out) {
  out->nullable = l.nullable;
  out->null_val = l.null_val;
  out->ival = l.ival;
  if (l.kind == HDK_LEAF_INT) {
    out->kind = JD_LITERAL;
    out->nullable = 0;
    return true;
  }
  if (l.kind != HDK_LEAF_COL) return false;
  const hdk_hip_col& c = p->cols[l.col];
  if (c.table == 0 && l.col == xc && l.col != kc) {
    out->kind = JD_X;
    return true;
  }
  if (c.table == -1 && c.buf_idx == 1) {  // payload word 1 of join 0's fused entry
    out->kind = JD_PAYLOAD;
    return true;
  }
  return false;
}

static bool match_join_direct(const hdk_hip_plan* p, const LaunchShape& shape, JoinDirectArgs* ja) {
  if (shape.strategy != STRAT_LDS || p->query_kind != HDK_Q_NON_GROUPED || p->num_joins != 1 || p->num_quals ||
      p->num_filter_ops || p->num_targets > kJdMaxTargets) {
    return false;
  }
  if (shape.rep == 0 || (shape.rep & (shape.rep - 1))) return false;
  const hdk_hip_join& jn = p->joins[0];
  if (jn.kind != HDK_JOIN_ONE_TO_ONE_FUSED || jn.fused_stride != 2 || !join_type_inner_like(jn.type) || jn.bucket > 1 ||
      jn.null_mode == HDK_JOIN_NULL_BITWISE || jn.table_idx != 0) {
    return false;
  }
  int kc;
  if (!plain_outer_col(p, jn.outer_key, &kc) || p->cols[kc].width != 8 || p->cols[kc].kind != HDK_COL_INT) return false;
  int xc = -1;
  for (int i = 0; i < p->num_cols; ++i) {
    const hdk_hip_col& c = p->cols[i];
    if (c.table == 0) {
      if (i == kc) continue;
      if (xc >= 0 || c.width != 8 || c.kind != HDK_COL_INT) return false;  // one more outer column, 8-byte integer
      xc = i;
    } else if (!(c.table == -1 && c.buf_idx == 1)) {
      return false;  // an inner column read through the row id, or a second payload word
    }
  }
  memset(ja, 0, sizeof(*ja));
  WordLayout wl;
  make_word_layout(p, &wl);
  if (wl.wpe != static_cast<int>(shape.wpe)) return false;
  ja->wpe = wl.wpe;
  for (int w = 0; w < wl.wpe; ++w) ja->wop[w] = wl.wop[w];
  ja->rep = shape.rep;
  ja->key_buf_idx = p->cols[kc].buf_idx;
  ja->x_buf_idx = xc >= 0 ? p->cols[xc].buf_idx : -1;
  ja->min_key = jn.min_key;
  ja->max_key = jn.max_key;
  ja->key_null = jn.null_val;
  ja->key_nullable = jn.null_mode == HDK_JOIN_NULL_NULLABLE;
  ja->ntargets = p->num_targets;
  for (int t = 0; t < p->num_targets; ++t) {
    const hdk_hip_target& tg = p->targets[t];
    JdTarget& jt = ja->t[t];
    if (tg.agg == HDK_AGG_ID || tg.slot_width != 8 || tg.arg_is_fp) return false;
    if (tg.agg == HDK_AGG_AVG && tg.slot2_width != 8) return false;
    jt.has_arg = tg.has_arg;
    jt.vword = wl.vword[t];
    jt.nword = wl.nword[t];
    jt.wop = wl.vword[t] >= 0 ? wl.wop[wl.vword[t]] : WOP_ADD_U64;
    if (jt.wop != WOP_ADD_U64 && jt.wop != WOP_MIN_I64 && jt.wop != WOP_MAX_I64) return false;
    if (wl.nword[t] >= 0) ja->nword_mask |= 1u << wl.nword[t];
    if (!tg.has_arg) {
      if (tg.agg != HDK_AGG_COUNT) return false;
      continue;
    }
    const hdk_hip_expr& e = tg.arg;
    if (e.vclass != HDK_VC_INT || e.nsteps > 1 || !jd_leaf_from(p, e.leaf0, kc, xc, &jt.a) || jt.a.kind == JD_LITERAL) return false;
    jt.nsteps = e.nsteps;
    if (e.nsteps == 1) {
      const hdk_hip_step& st = e.steps[0];
      if ((st.op != HDK_OP_ADD && st.op != HDK_OP_SUB && st.op != HDK_OP_MUL) || st.out_class != HDK_VC_INT) return false;
      if (!jd_leaf_from(p, st.rhs, kc, xc, &jt.b)) return false;
      jt.op = st.op;
      jt.check_width = st.check_width;
      jt.step_null = st.null_out;
    }
    // what eval_target_arg tests: after a step the value is nullable with the step's NULL (eval_expr), else the leaf's
    jt.arg_null = e.null_val;
    jt.arg_nullable = e.nullable;
    jt.skip_null = tg.skip_null;
    jt.slot_null = tg.null_val;
  }
  return true;
}

// does the direct join kernel read key-range-clustered tuples?  `ca`: the pass that makes them (AoS: key, x)
static bool match_join_direct_clustered(const hdk_hip_plan* p, const JoinDirectArgs& ja, const hdk_hip_kernel_options* ko, ClusterArgs* ca) {
  if (!ko || ko->total_rows == 0 || (ko->flags & HDK_HIP_LAUNCH_NO_CLUSTER_PROBES)) return false;
  // Only on request.  Measured on C3 (256 M rows, 160 MB table): pre-pass 1.96 ms + probes over the clustered tuples
  // 3.19 ms (a quarter of them still miss L2: several key ranges are in flight at once) against 5.08 ms in row order --
  // no gain yet; with the table L2-resident this kernel needs 2.06 ms (the interpreter 3.09).
  const hdk_hip_join& jn = p->joins[0];
  if (!(ko->flags & HDK_HIP_LAUNCH_CLUSTER_PROBES) || static_cast<uint64_t>(jn.max_key - jn.min_key) >= 0xFFFFFFFFull) return false;
  memset(ca, 0, sizeof(*ca));
  ca->aos = 1;
  ca->ncols = ja.x_buf_idx >= 0 ? 2 : 1;
  ca->buf_idx[0] = ja.key_buf_idx;
  ca->buf_idx[1] = ja.x_buf_idx;
  ca->key_min = jn.min_key;
  cluster_geometry(ko->total_rows, static_cast<uint64_t>(jn.max_key - jn.min_key) + 1, ca);
  return true;
}

// ---- hdk_join_agg_sliced (scan_join_sliced.h): key-range slices of the join table probed out of LDS ----------------
// Taken by default for the hdk_join_agg_direct shape when the table is far larger than the caches and the column
// statistics let payload and key offset travel in 32 bits; HDK_HIP_LAUNCH_CLUSTER_PROBES takes it whatever the sizes
// (tests), HDK_HIP_LAUNCH_NO_CLUSTER_PROBES never.
static bool match_join_sliced(const hdk_hip_plan* p, const JoinDirectArgs& ja, const hdk_hip_kernel_options* ko, uint32_t grid,
                              SliceArgs* sa) {
  const hdk_hip_join& jn = p->joins[0];
  if (jn.max_key < jn.min_key) return false;
  const uint64_t range = static_cast<uint64_t>(jn.max_key - jn.min_key) + 1;
  if (!slices_worth_it(ko, range)) return false;
  uint32_t slice = static_cast<uint32_t>((range + kSliceMaxBins - 1) / kSliceMaxBins);
  if (slice < 64) slice = 64;
  if (slice > kSliceMaxEntries) return false;  // > 10.2 M keys: a slice no longer fits the LDS of a CU
  memset(sa, 0, sizeof(*sa));
  // payload: in 32 bits with two values to spare (column statistics of the fused inner column)
  const hdk_hip_col* pay = nullptr;
  const hdk_hip_col* xcol = nullptr;
  for (int i = 0; i < p->num_cols; ++i) {
    if (p->cols[i].table == -1 && p->cols[i].buf_idx == 1) pay = &p->cols[i];
    if (p->cols[i].table == 0 && p->cols[i].buf_idx == ja.x_buf_idx) xcol = &p->cols[i];
  }
  if (!payload_fits_32_bits(pay)) return false;
  sa->key_buf_idx = ja.key_buf_idx;
  sa->x_buf_idx = ja.x_buf_idx;
  sa->key_min = jn.min_key;
  sa->key_range = range;
  sa->key_nullable = ja.key_nullable;
  sa->key_null = ja.key_null;
  sa->slice = slice;
  magic_u32(slice, &sa->slice_magic, &sa->slice_shift);
  sa->nbins = static_cast<uint32_t>((range + slice - 1) / slice);
  // every block of the probe pass flushes into slab[blockIdx.x], and the workspace holds (and hdk_finalize folds) as many
  // slabs as the launch shape's grid -- which the caller may have made small (KernelOptions::gridDimX): one block per
  // slice at least, or the slices are not used
  if (sa->nbins > grid) return false;
  // the NULL sentinels of x and of the payload, as the targets' leaves name them
  for (int t = 0; t < ja.ntargets; ++t) {
    for (const JdLeaf* l : {&ja.t[t].a, &ja.t[t].b}) {
      if (!ja.t[t].has_arg) continue;
      if (l->kind == JD_X && l->nullable) sa->x_null = l->null_val, sa->x_null32 = 1;
      if (l->kind == JD_PAYLOAD && l->nullable) sa->pay_null = l->null_val, sa->pay_nullable = 1;
    }
  }
  // x: 32 bits when the statistics allow (a nullable column gives up INT32_MIN for its NULL), else 16-byte tuples
  sa->narrow = 1;
  if (ja.x_buf_idx >= 0) {
    if (!x_fits_narrow(xcol, sa) || hdk_sw(SW_SLICE_WIDE)) sa->narrow = 0;
  } else {
    sa->x_null32 = 0;
  }
  // the FAST form of the probe pass: ONE target, SUM(x + payload) in either order, into an ADD word
  if (ja.ntargets == 1 && ja.t[0].has_arg && ja.t[0].nsteps == 1 && ja.t[0].op == HDK_OP_ADD && ja.t[0].vword >= 0 &&
      ja.t[0].wop == WOP_ADD_U64 && !hdk_sw(SW_SLICE_GENERAL)) {
    const JdLeaf &la = ja.t[0].a, &lb = ja.t[0].b;
    const JdLeaf* lx = la.kind == JD_X ? &la : (lb.kind == JD_X ? &lb : nullptr);
    const JdLeaf* lp = la.kind == JD_PAYLOAD ? &la : (lb.kind == JD_PAYLOAD ? &lb : nullptr);
    if (lx && lp && lx != lp) {
      sa->fast = 1;
      sa->fast_x_nullable = lx->nullable;
      sa->fast_x_null = lx->null_val;
      sa->fast_p_nullable = lp->nullable;
      sa->fast_p_null = lp->null_val;
    }
  }
  return slice_buffer_geometry(ko->total_rows, sa);
}

static int32_t launch_sliced_kernels(SliceArgs& sa, const LaunchShape& shape, const hdk_hip_device_properties* props, hipStream_t s,
                                     bool* launched) {
  *launched = false;
  typedef void (*SliceKernel)(SliceArgs);
  const SliceKernel kagg_fn = sa.narrow ? (sa.fast ? hdk_join_agg_sliced<true, true> : hdk_join_agg_sliced<true, false>)
                                        : (sa.fast ? hdk_join_agg_sliced<false, true> : hdk_join_agg_sliced<false, false>);
  const SliceKernel ksc_fn = sa.narrow ? hdk_join_scatter_slices<true> : hdk_join_scatter_slices<false>;
  const void* kagg = reinterpret_cast<const void*>(kagg_fn);
  const size_t lds_agg = static_cast<size_t>(shape.wpe) * shape.rep * 8 + static_cast<size_t>(sa.slice) * 4;
  const int per_cu = probe_blocks_per_cu(kagg, lds_agg);
  if (per_cu < 1) return HDK_HIP_OK;  // no block this large here: probe in row order
  const int VR = sa.narrow ? 8 : 4, TW = sa.narrow ? 1 : 2;  // rows per lane and batch, words per tuple
  const size_t lds_sc = static_cast<size_t>(kSliceBlock) * VR * TW * 8 + static_cast<size_t>(kSliceBlock) * VR + 16;
  const unsigned g_sc = scatter_grid(reinterpret_cast<const void*>(ksc_fn), kSliceBlock, lds_sc, props, 2);
  uint32_t members = static_cast<uint32_t>(per_cu) * static_cast<uint32_t>(props->num_cu) / sa.nbins;
  if (members < 1) members = 1;
  if (sa.nbins * members > shape.grid) members = shape.grid / sa.nbins;  // slab[blockIdx.x] must exist (match_join_sliced: nbins <= grid)
  if (members < 1) return HDK_HIP_OK;
  hipLaunchKernelGGL(hdk_join_order_probe, dim3(256), dim3(256), 0, s, sa);
  hipLaunchKernelGGL(ksc_fn, dim3(g_sc), dim3(kSliceBlock), lds_sc, s, sa);
  hipLaunchKernelGGL(kagg_fn, dim3(sa.nbins * members), dim3(kSliceAggBlock), lds_agg, s, sa);
  HDK_HIP_CHECK(hipGetLastError());
  *launched = true;
  return HDK_HIP_OK;
}

// what the routes of hdk_join_agg_direct carry (sa: ROUTE_JOIN_SLICED only, ca: ROUTE_JOIN_DIRECT_CLUSTERED only)
struct JoinDirectRoute { JoinDirectArgs ja; SliceArgs sa; ClusterArgs ca; };

// (no scratch for the passes in front of the row-order kernel, or no block that large: it probes in row order, unarmed)
static int32_t launch_join_direct(LaunchRoute& r, const hdk_hip_device_properties* props, hipStream_t s) {
  const LaunchShape& shape = r.shape;
  JoinDirectArgs& ja = r.as<JoinDirectRoute>().ja;
  AsyncScratch scratch(s);
  if (r.kind == ROUTE_JOIN_SLICED) {
    // key-range slices probed out of LDS; the row-order kernel below stays armed for what the slices cannot carry
    SliceArgs& sa = r.as<JoinDirectRoute>().sa;
    int32_t st = carve_slice_scratch(scratch, sa, sa.narrow ? 1 : 2, nullptr, s);
    if (st) return st;
    if (scratch.p) {
      sa.kp = ja.kp;
      sa.jd = ja;
      sa.num_slabs = shape.grid;
      bool launched = false;
      st = launch_sliced_kernels(sa, shape, props, s, &launched);
      if (st) return st;
      if (launched) {
        ja.run_if = sa.mode;
      }
    }
  } else if (r.kind == ROUTE_JOIN_DIRECT_CLUSTERED) {
    ClusterArgs& ca = r.as<JoinDirectRoute>().ca;
    int8_t* q;
    const int32_t st = cluster_scratch(ca, 0, s, &scratch.p, &q);
    if (st) return st;
    if (q) {  // (else no scratch: probe in row order)
      ca.kp = ja.kp;
      launch_cluster_by_key(ca, props, s);
      ja.clustered = 1;
      ja.tw = ca.ncols;
      ja.tuples = ca.out[0];
      ja.fill = ca.fill;
      ja.fill_ovf = ca.fill_ovf;
      ja.sub = ca.sub;
      ja.cap_ovf = ca.cap_ovf;
    }
  }
  hipLaunchKernelGGL(hdk_join_agg_direct, dim3(shape.grid), dim3(kJdBlock), shape.lds_bytes, s, ja);
  HDK_HIP_CHECK(hipGetLastError());
  return HDK_HIP_OK;  // (`scratch` is freed here, stream-ordered after the kernels above)
}

// ---- the general sliced join (scan_join_sliced2.h): join + perfect-hash GROUP BY on the joined column / + filters / any
// list of integer aggregates over x and the payload, everything in 8-byte tuples ----------------------------------------
// leaf of an aggregate argument: 0 = x (the one other 8-byte outer column), 1 = the payload, 2 = an integer literal
// (`yc`: the outer column that rides in the tuple's spare bits, if any -- it reads like a third payload word, pidx 2)
static int s2_leaf_kind(const hdk_hip_plan* p, const hdk_hip_leaf& l, int kc, int* xc, int* pidx = nullptr, int yc = -1) {
  if (l.kind == HDK_LEAF_INT) return 2;
  if (l.kind != HDK_LEAF_COL) return -1;
  const hdk_hip_col& c = p->cols[l.col];
  if (c.table == -1 && (c.buf_idx == 1 || c.buf_idx == 2)) {
    if (pidx) *pidx = c.buf_idx - 1;
    return 1;
  }
  if (l.col == yc) {  // (match_join_sliced2 checked it: an integer column of the outer table, 8 or 4 bytes wide)
    if (pidx) *pidx = 2;
    return 1;
  }
  if (c.table != 0 || l.col == kc || c.width != 8 || c.kind != HDK_COL_INT) return -1;
  if (*xc >= 0 && *xc != l.col) return -1;  // one value column travels in the tuple
  *xc = l.col;
  return 0;
}

static bool match_join_sliced2(const hdk_hip_plan* p, const LaunchShape& shape, const hdk_hip_kernel_options* ko, Slice2Args* ga) {
  if (hdk_sw(SW_NO_SLICED2)) return false;
  if (shape.strategy != STRAT_LDS || p->num_joins != 1 || p->num_filter_ops || p->num_targets > HDK_HIP_MAX_TARGETS) return false;
  if (p->query_kind != HDK_Q_NON_GROUPED && p->query_kind != HDK_Q_PERFECT_HASH) return false;
  if (plan_reads_small_dates(p)) return false;
  const hdk_hip_join& jn = p->joins[0];
  if (jn.kind != HDK_JOIN_ONE_TO_ONE_FUSED || (jn.fused_stride != 2 && jn.fused_stride != 3) || !join_type_inner_like(jn.type) || jn.bucket > 1 ||
      jn.null_mode == HDK_JOIN_NULL_BITWISE || jn.table_idx != 0 || jn.max_key < jn.min_key) {
    return false;
  }
  int kc;
  if (!plain_outer_col(p, jn.outer_key, &kc) || p->cols[kc].width != 8 || p->cols[kc].kind != HDK_COL_INT) return false;
  const uint64_t range = static_cast<uint64_t>(jn.max_key - jn.min_key) + 1;
  if (!slices_worth_it(ko, range)) return false;
  memset(ga, 0, sizeof(*ga));
  SliceArgs& sa = ga->s;
  const int npay = jn.fused_stride - 1;
  const hdk_hip_col* pay[2] = {nullptr, nullptr};
  for (int i = 0; i < p->num_cols; ++i) {
    const hdk_hip_col& c = p->cols[i];
    if (c.table == -1 && c.buf_idx >= 1 && c.buf_idx <= npay) pay[c.buf_idx - 1] = &c;
    else if (c.table != 0) return false;  // an inner column read through the row id, or a third payload word
  }
  ga->npay = npay;
  // ---- a second outer column: y, in the bits of the tuple's low word the key offset leaves free ------------------------------
  // Which one: the group key's column when that is an outer column (GROUP BY fact.g ... WHERE dim.d < c); else, when the
  // aggregates read two outer columns, the one with the narrower statistics.  It must fit: codes 1 .. max - min + 1.
  uint32_t key_bits = 1;
  while (key_bits < 32 && (1ull << key_bits) < range) ++key_bits;
  auto y_fits = [&](int ci) {
    const hdk_hip_col& c = p->cols[ci];
    if (c.table != 0 || ci == kc || (c.width != 8 && c.width != 4) || c.kind != HDK_COL_INT || !c.has_stats || c.max_val < c.min_val) return false;
    if (c.min_val <= static_cast<int64_t>(INT32_MIN) + 2 || c.max_val > static_cast<int64_t>(INT32_MAX)) return false;
    return static_cast<uint64_t>(c.max_val - c.min_val) + 2 <= (1ull << (32 - key_bits));
  };
  int yc = -1;
  if (!hdk_sw(SW_S2_NO_Y)) {
    if (p->query_kind == HDK_Q_PERFECT_HASH && p->key_count == 1 && p->keys[0].leaf0.kind == HDK_LEAF_COL &&
        p->cols[p->keys[0].leaf0.col].table == 0) {
      yc = p->keys[0].leaf0.col;
      if (!y_fits(yc)) return false;
    } else {
      int oc[2] = {-1, -1}, noc = 0;
      auto note = [&](const hdk_hip_leaf& l) {
        if (l.kind != HDK_LEAF_COL || p->cols[l.col].table != 0 || l.col == kc) return true;
        for (int i = 0; i < noc; ++i) {
          if (oc[i] == l.col) return true;
        }
        if (noc == 2) return false;
        oc[noc++] = l.col;
        return true;
      };
      for (int t = 0; t < p->num_targets; ++t) {
        const hdk_hip_target& tg = p->targets[t];
        if (tg.agg == HDK_AGG_ID || !tg.has_arg) continue;
        if (!note(tg.arg.leaf0) || (tg.arg.nsteps >= 1 && !note(tg.arg.steps[0].rhs))) return false;
      }
      if (noc == 2) {
        const bool f0 = y_fits(oc[0]), f1 = y_fits(oc[1]);
        if (!f0 && !f1) return false;
        if (f0 && f1) {
          yc = (p->cols[oc[0]].max_val - p->cols[oc[0]].min_val) <= (p->cols[oc[1]].max_val - p->cols[oc[1]].min_val) ? oc[0] : oc[1];
        } else {
          yc = f0 ? oc[0] : oc[1];
        }
      }
    }
  }
  // ---- targets ----------------------------------------------------------------------------------------------------------
  WordLayout wl;
  make_word_layout(p, &wl);
  if (wl.wpe != static_cast<int>(shape.wpe)) return false;
  ga->wpe = wl.wpe;
  for (int w = 0; w < wl.wpe; ++w) ga->wop[w] = wl.wop[w];
  int xc = -1;
  int nt = 0;
  int64_t x_null = 0, p_null[3] = {0, 0, 0};  // ([2]: y)
  bool x_nullable = false, p_nullable[3] = {false, false, false};
  for (int t = 0; t < p->num_targets; ++t) {
    const hdk_hip_target& tg = p->targets[t];
    if (tg.agg == HDK_AGG_ID) {
      if (p->query_kind != HDK_Q_PERFECT_HASH || tg.key_idx != 0) return false;
      continue;  // hdk_finalize rebuilds a projected key from the entry index
    }
    if (tg.agg == HDK_AGG_SINGLE_VALUE || tg.arg_is_fp || tg.slot_width != 8) return false;
    if (tg.agg == HDK_AGG_AVG && tg.slot2_width != 8) return false;
    if (!tg.has_arg) {
      if (tg.agg != HDK_AGG_COUNT) return false;
      continue;  // COUNT(*): the row count word
    }
    if (wl.vword[t] < 0 && wl.nword[t] < 0) continue;  // COUNT(not-null expression): the row count too
    if (nt == kS2MaxTargets) return false;
    S2Target& st = ga->t[nt++];
    st.vword = wl.vword[t];
    st.nword = wl.nword[t];
    st.wop = wl.vword[t] >= 0 ? wl.wop[wl.vword[t]] : WOP_ADD_U64;
    if (st.wop != WOP_ADD_U64 && st.wop != WOP_MIN_I64 && st.wop != WOP_MAX_I64) return false;
    if (wl.nword[t] >= 0) ga->nword_mask |= 1u << wl.nword[t];
    const hdk_hip_expr& e = tg.arg;
    if (e.vclass != HDK_VC_INT || e.nsteps > 1) return false;
    int pi = 0;
    const int ka = s2_leaf_kind(p, e.leaf0, kc, &xc, &pi, yc);
    if (ka != 0 && ka != 1) return false;
    bool nullable = e.leaf0.nullable != 0;
    if (ka == 0 && e.leaf0.nullable) x_nullable = true, x_null = e.leaf0.null_val;
    if (ka == 1 && e.leaf0.nullable) p_nullable[pi] = true, p_null[pi] = e.leaf0.null_val;
    if (ka == 1) st.pidx = pi;
    st.null_if_x = ka == 0 && e.leaf0.nullable;
    st.null_if_p = ka == 1 && e.leaf0.nullable;
    if (e.nsteps == 0) {
      st.src = ka == 0 ? S2_X : S2_P;
    } else {
      const hdk_hip_step& sp = e.steps[0];
      if ((sp.op != HDK_OP_ADD && sp.op != HDK_OP_SUB && sp.op != HDK_OP_MUL) || sp.out_class != HDK_VC_INT) return false;
      if (sp.check_width != 0 && sp.check_width != 8) return false;  // (a 4-byte SQL type can overflow: the interpreter checks)
      int pj = 0;
      const int kb = s2_leaf_kind(p, sp.rhs, kc, &xc, &pj, yc);
      if (kb < 0) return false;
      if (kb == 2) {
        if (sp.rhs.ival <= -(int64_t(1) << 31) || sp.rhs.ival >= (int64_t(1) << 31)) return false;
        st.src = ka == 0 ? S2_X_OP_LIT : S2_P_OP_LIT;
        st.op = sp.op;
        st.lit = sp.rhs.ival;
      } else {
        if (kb == ka) return false;  // x op x, payload op payload
        nullable = nullable || sp.rhs.nullable;
        if (kb == 0 && sp.rhs.nullable) x_nullable = true, x_null = sp.rhs.null_val, st.null_if_x = 1;
        if (kb == 1) st.pidx = pj;
        if (kb == 1 && sp.rhs.nullable) p_nullable[pj] = true, p_null[pj] = sp.rhs.null_val, st.null_if_p = 1;
        if (sp.op == HDK_OP_ADD) st.src = S2_X_ADD_P;
        else if (sp.op == HDK_OP_MUL) st.src = S2_X_MUL_P;
        else st.src = ka == 0 ? S2_X_SUB_P : S2_P_SUB_X;
      }
    }
    // a NULL argument is skipped (and counted) -- the only reading of a NULL the kernel has; a plan that would AGGREGATE
    // the sentinel (nullable leaf, skip_null off) is the interpreter's
    if (nullable && !tg.skip_null) return false;
  }
  ga->ntargets = nt;
  // ---- filters: `outer column cmp literal` in pass 1, `payload cmp literal` in pass 2 ----------------------------------------
  {
    hdk_hip_plan outer_only;
    memset(&outer_only, 0, sizeof(outer_only));
    int nq = 0;
    for (int i = 0; i < p->num_quals; ++i) {
      const hdk_hip_qual& q = p->quals[i];
      if (q.lhs.nsteps == 0 && q.lhs.leaf0.kind == HDK_LEAF_COL && p->cols[q.lhs.leaf0.col].table == -1 &&
          p->cols[q.lhs.leaf0.col].buf_idx >= 1 && p->cols[q.lhs.leaf0.col].buf_idx <= npay) {
        if (q.rhs.kind != HDK_LEAF_INT || ga->npq == kS2MaxPayQuals) return false;
        const int qi = p->cols[q.lhs.leaf0.col].buf_idx - 1;
        if (q.lhs.leaf0.nullable) p_nullable[qi] = true, p_null[qi] = q.lhs.leaf0.null_val;
        ga->pq[ga->npq].pidx = qi;
        ga->pq[ga->npq].cmp = q.cmp;
        ga->pq[ga->npq].rhs = q.rhs.ival;
        ++ga->npq;
      } else {
        if (nq == kMaxPlainQuals) return false;
        outer_only.quals[nq++] = q;
      }
    }
    outer_only.num_quals = nq;
    outer_only.num_filter_ops = 0;
    outer_only.num_cols = p->num_cols;
    memcpy(outer_only.cols, p->cols, sizeof(p->cols));
    if (nq && !match_plain_quals(&outer_only, sa.q)) return false;
    sa.nquals = nq;
  }
  // ---- group key: the payload, or payload / literal; perfect hash without a bucket ----------------------------------------------
  ga->entry_count = shape.entry_count;
  if (p->query_kind == HDK_Q_PERFECT_HASH) {
    if (p->key_count != 1 || p->key_bucket[0] > 1) return false;
    const hdk_hip_expr& ke = p->keys[0];
    int dummy = -1, ki = 0;
    if (ke.nsteps > 1 || s2_leaf_kind(p, ke.leaf0, kc, &dummy, &ki, yc) != 1) return false;
    ga->key_pidx = ki;
    if (ke.leaf0.nullable) p_nullable[ki] = true, p_null[ki] = ke.leaf0.null_val;
    if (ke.nsteps == 1) {
      const hdk_hip_step& sp = ke.steps[0];
      if ((sp.op != HDK_OP_DIV && sp.op != HDK_OP_MOD) || sp.out_class != HDK_VC_INT || sp.rhs.kind != HDK_LEAF_INT || sp.rhs.ival < 1 ||
          sp.rhs.ival > INT32_MAX) {
        return false;
      }
      ga->key_div = static_cast<int32_t>(sp.rhs.ival);
      ga->key_mod = sp.op == HDK_OP_MOD;
      if (ga->key_div >= 2) magic_u32(static_cast<uint32_t>(ga->key_div), &ga->div_magic, &ga->div_shift);
    }
    ga->grouped = 1;
    ga->key_min = p->key_min[0];
    // eval_key: a NULL key takes the translated value when the layout has a slot for NULLs, else stays the NULL sentinel
    const int64_t null_key = (p->key_has_nulls[0] && ke.nullable) ? p->key_null_translated[0] : ke.null_val;
    ga->null_entry = static_cast<int64_t>(static_cast<uint64_t>(null_key) - static_cast<uint64_t>(p->key_min[0]));
  }
  // ---- the 8-byte tuple: payload and x inside 32 bits by the column statistics ------------------------------------------------------
  for (int j = 0; j < npay; ++j) {
    if (!payload_fits_32_bits(pay[j])) return false;
  }
  sa.key_buf_idx = p->cols[kc].buf_idx;
  sa.x_buf_idx = xc >= 0 ? p->cols[xc].buf_idx : -1;
  sa.key_min = jn.min_key;
  sa.key_range = range;
  sa.key_nullable = jn.null_mode == HDK_JOIN_NULL_NULLABLE;
  sa.key_null = jn.null_val;
  sa.pay_null = p_null[0];
  sa.pay_nullable = p_nullable[0];
  ga->pay_null1 = p_null[1];
  ga->pay_nullable1 = p_nullable[1];
  sa.narrow = 1;
  if (yc >= 0) {
    const hdk_hip_col& ycol = p->cols[yc];
    if (ycol.has_nulls && !p_nullable[2]) return false;  // NULLs possible but no sentinel known from the leaves
    sa.y_buf_idx = ycol.buf_idx;
    sa.y_width = ycol.width;
    sa.y_shift = key_bits;
    sa.y_min = ycol.min_val;
    sa.y_codes = static_cast<uint32_t>(ycol.max_val - ycol.min_val) + 2;
    sa.y_nullable = p_nullable[2];
    sa.y_null = p_null[2];
  }
  // two payload words in one LDS word when their statistics leave room (codes: word 0 two reserved, word 1 one)
  if (npay == 2 && pay[0] && pay[1] && !hdk_sw(SW_S2_NO_PACKED_PAIR)) {
    const uint64_t n0 = static_cast<uint64_t>(pay[0]->max_val - pay[0]->min_val) + 3, n1 = static_cast<uint64_t>(pay[1]->max_val - pay[1]->min_val) + 2;
    uint32_t b0 = 1, b1 = 1;
    while (b0 < 32 && (1ull << b0) < n0) ++b0;
    while (b1 < 32 && (1ull << b1) < n1) ++b1;
    if (pay[0]->max_val >= pay[0]->min_val && pay[1]->max_val >= pay[1]->min_val && b0 + b1 <= 32) {
      ga->packed = 1;
      ga->pk_bits0 = b0;
      ga->pk_codes0 = static_cast<uint32_t>(n0);  // codes in all (b0 <= 31: at most 2^31)
      ga->pk_codes1 = static_cast<uint32_t>(n1);
      ga->pk_min0 = pay[0]->min_val;
      ga->pk_min1 = pay[1]->min_val;
    }
  }
  if (xc >= 0) {
    sa.x_null = x_null;
    sa.x_null32 = x_nullable ? 1 : 0;
    if (!x_fits_narrow(&p->cols[xc], &sa)) return false;  // (no 16-byte tuples here)
  }
  // ---- geometry: slices whose payloads fit LDS next to the group table; <= 256 of them: one scatter level, else two ------------
  const uint64_t table_bytes1 = static_cast<uint64_t>(shape.entry_count) * wl.wpe * 8;
  if (table_bytes1 > kS2MaxTableBytes) return false;
  const uint64_t rows = ko->total_rows;
  uint32_t slice = static_cast<uint32_t>((range + kSliceMaxBins - 1) / kSliceMaxBins);
  if (slice < 64) slice = 64;
  const uint64_t kb4 = 4ull * (ga->packed ? 1 : npay);  // LDS bytes per key of a slice
  const bool one_level = static_cast<uint64_t>(slice) * kb4 + table_bytes1 <= kS2LdsBytes && !hdk_sw(SW_SLICE_TWO_LEVELS);
  auto pick_rep = [&](uint32_t keys) {
    uint32_t rep = 1;
    while (rep < 32 && static_cast<uint64_t>(keys) * kb4 + table_bytes1 * (rep * 2) <= kS2LdsBytes && table_bytes1 * (rep * 2) <= 16 * 1024) rep *= 2;
    return rep;
  };
  if (one_level) {
    ga->rep = pick_rep(slice);
    sa.slice = slice;
    magic_u32(slice, &sa.slice_magic, &sa.slice_shift);
    sa.nbins = static_cast<uint32_t>((range + slice - 1) / slice);
    ga->fslice = slice;
    ga->nslices = sa.nbins;
    ga->nsl_par = sa.nbins;
    if (sa.nbins > shape.grid) return false;  // one block (and one slab) per slice at least
  } else {
    // fine slices of <= 32 K keys (128 KB of LDS; less when the group table is big), `fpc` of them per coarse bin
    uint64_t fs = (kS2LdsBytes - table_bytes1) / kb4;
    if (fs > 32768) fs = 32768;
    fs &= ~static_cast<uint64_t>(63);
    if (fs < 1024) return false;
    if (const char* e = hdk_sw(SW_SLICE_FINE_KEYS)) fs = static_cast<uint64_t>(atoi(e)) & ~63ull;  // (tests: small tables, two levels)
    if (fs < 64) fs = 64;
    const uint64_t nslices = (range + fs - 1) / fs;
    const uint64_t fpc = (nslices + kSliceMaxBins - 1) / kSliceMaxBins;
    if (fpc > static_cast<uint64_t>(kSliceMaxBins) || fpc * fs > 0xFFFFFFFFull) return false;
    const uint64_t coarse = fpc * fs;
    ga->two_level = 1;
    ga->fpc = static_cast<uint32_t>(fpc);
    ga->fslice = static_cast<uint32_t>(fs);
    magic_u32(ga->fslice, &ga->fmagic, &ga->fshift);
    sa.slice = static_cast<uint32_t>(coarse);
    magic_u32(sa.slice, &sa.slice_magic, &sa.slice_shift);
    sa.nbins = static_cast<uint32_t>((range + coarse - 1) / coarse);
    ga->nslices = sa.nbins * ga->fpc;  // (the last coarse bin's slices past the key range stay empty)
    ga->rep = pick_rep(ga->fslice);
    ga->cap2 = ((rows / ((range + fs - 1) / fs)) * 17 / 16 + 2048 + 15) & ~15ull;
    if (ga->cap2 > 0xFFFFFFF0ull) return false;
    ga->nsl_par = ga->nslices < shape.grid ? ga->nslices : shape.grid;  // (launch_join_sliced2 lowers it to what is resident)
  }
  return slice_buffer_geometry(rows, &sa);
}

// `bh`: the launch belongs to a GroupByBaselineHash plan run through an internal dense table (launch_baseline_sliced_join):
// armed behind the passes is the open-addressing interpreter of that plan, and the slabs are folded into the open-addressing
// table by hdk_bh_fold_dense instead of hdk_finalize.
typedef void (*S2Kernel)(Slice2Args);
template <bool GROUPED, bool HASY>
static S2Kernel s2_agg_kernel_npay(int npay_form) {
  return npay_form == 3 ? hdk_join_agg_sliced2<GROUPED, 3, HASY> : (npay_form == 2 ? hdk_join_agg_sliced2<GROUPED, 2, HASY> : hdk_join_agg_sliced2<GROUPED, 1, HASY>);
}
static S2Kernel s2_agg_kernel(const Slice2Args& ga) {
  const int form = ga.packed ? 3 : (ga.npay == 2 ? 2 : 1);
  const bool y = ga.s.y_shift != 0;
  return ga.grouped ? (y ? s2_agg_kernel_npay<true, true>(form) : s2_agg_kernel_npay<true, false>(form))
                    : (y ? s2_agg_kernel_npay<false, true>(form) : s2_agg_kernel_npay<false, false>(form));
}
typedef void (*S2Scatter)(SliceArgs);
static S2Scatter s2_scatter_kernel(const SliceArgs& sa) {
  if (sa.y_shift && sa.y_width == 4) return sa.nquals ? hdk_join_scatter_slices<true, true, 4> : hdk_join_scatter_slices<true, false, 4>;
  if (sa.y_shift) return sa.nquals ? hdk_join_scatter_slices<true, true, 8> : hdk_join_scatter_slices<true, false, 8>;
  return sa.nquals ? hdk_join_scatter_slices<true, true, 0> : hdk_join_scatter_slices<true, false, 0>;
}

struct BhBehindSliced {
  BhGeom g;                  // the open-addressing interpreter's table, as its route was matched
  BhDenseFold fold;
};
static int32_t launch_join_sliced2(const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp, Slice2Args& ga,
                                   const LaunchShape& shape, int64_t* slabs, const hdk_hip_kernel_options* ko,
                                   const hdk_hip_device_properties* props, hipStream_t s, bool* launched, BhBehindSliced* bh = nullptr) {
  *launched = false;
  SliceArgs& sa = ga.s;
  const S2Kernel kagg_fn = s2_agg_kernel(ga);
  const size_t lds_agg = static_cast<size_t>(ga.entry_count) * ga.wpe * ga.rep * 8 + static_cast<size_t>(ga.fslice) * 4 * ((ga.npay == 2 && !ga.packed) ? 2 : 1);
  const int per_cu = probe_blocks_per_cu(reinterpret_cast<const void*>(kagg_fn), lds_agg);
  if (per_cu < 1) return HDK_HIP_OK;
  AsyncScratch scratch(s);
  int32_t st = carve_slice_scratch(scratch, sa, 1, &ga, s);
  if (st || !scratch.p) return st;  // (no scratch: the interpreter probes in row order)
  sa.kp = kp;
  sa.num_slabs = shape.grid;
  ga.slabs = slabs;
  ga.error_code = kp.error_code;
  constexpr int VR = 8;
  const size_t lds_sc = static_cast<size_t>(kSliceBlock) * VR * 8 + static_cast<size_t>(kSliceBlock) * VR + 16;
  const S2Scatter ksc_fn = s2_scatter_kernel(sa);
  const unsigned g_sc = scatter_grid(reinterpret_cast<const void*>(ksc_fn), kSliceBlock, lds_sc, props, 2);
  const uint32_t resident = static_cast<uint32_t>(per_cu) * static_cast<uint32_t>(props->num_cu);
  uint32_t members = 1;
  if (ga.two_level) {  // persistent blocks, each walking slices b, b + nsl_par, ...
    if (ga.nsl_par > resident) ga.nsl_par = resident;
    if (ga.nsl_par > shape.grid) ga.nsl_par = shape.grid;
  } else {
    members = resident / sa.nbins;
    if (members < 1) members = 1;
    if (sa.nbins * members > shape.grid) members = shape.grid / sa.nbins;
  }
  if (members < 1 || ga.nsl_par < 1) return HDK_HIP_OK;
  hipLaunchKernelGGL(hdk_join_order_probe, dim3(256), dim3(256), 0, s, sa);
  hipLaunchKernelGGL(ksc_fn, dim3(g_sc), dim3(kSliceBlock), lds_sc, s, sa);
  if (ga.two_level) {
    const size_t lds_l2 = static_cast<size_t>(kSliceBlock) * VR * 8 + static_cast<size_t>(kSliceBlock) * VR + 16;
    const uint32_t ncx = (sa.nbins + kSliceXcds - 1) / kSliceXcds;
    const uint32_t res2 = resident_grid(reinterpret_cast<const void*>(hdk_join_scatter_level2), kSliceBlock, lds_l2, props);
    uint32_t m2 = res2 / (ncx * kSliceXcds);
    if (m2 < 1) m2 = 1;
    hipLaunchKernelGGL(hdk_join_scatter_level2, dim3(ncx * kSliceXcds * m2), dim3(kSliceBlock), lds_l2, s, ga);
  }
  hipLaunchKernelGGL(kagg_fn, dim3(ga.nsl_par * members), dim3(kSliceAggBlock), lds_agg, s, ga);
  // armed behind the passes: the batched interpreter over the plan's own columns, in row order -- clustered input, stale
  // statistics, an overflow area that filled up
  if (bh) {
    st = launch_bh_vec_armed(bh->g, plan, d_plan, kp, props, s, sa.mode);
    if (st) return st;
    bh->fold.slabs = slabs;
    bh->fold.num_slabs = shape.grid;
    st = launch_bh_fold_dense(bh->fold, d_plan, kp, s);
  } else {
    st = launch_vec_armed(plan, d_plan, kp, slabs, shape, ko, s, sa.mode);
  }
  if (st) return st;
  *launched = true;
  return HDK_HIP_OK;  // (`scratch` is freed here, stream-ordered after the kernels above)
}

// ---- FAM_LDS_JOIN (route.h): the plans of the LDS strategy that the join kernels take ------------------------------------------------
// r->shape.grid is the grid of the interpreter that stays armed behind the sliced passes (route_scan_lds); `refused`: a sliced2
// launch that was handed back (no scratch / no block this large) goes to the kernels that probe in row order
bool route_lds_join(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, RouteSet refused,
                    LaunchRoute* r) {
  const LaunchShape& s = r->shape;
  JoinDirectArgs ja;
  SliceArgs sa;
  const bool direct = match_join_direct(p, s, &ja);
  const bool sliced = direct && match_join_sliced(p, ja, ko, s.grid, &sa);
  // (BASELINE config 3 itself, SUM(x + payload), keeps the compile-time form of its slices)
  const bool c3_itself = sliced && sa.fast && !hdk_sw(SW_SLICED2_ALWAYS);
  Slice2Args& ga = r->as<Slice2Args>();
  if (!c3_itself && match_join_sliced2(p, s, ko, &ga)) {
    r->kind = ga.two_level ? ROUTE_SLICED2_TWO_LEVELS : ROUTE_SLICED2;
    if (!route_refused(refused, r->kind)) return true;
  }
  if (!direct) return false;
  JoinDirectRoute& jd = r->as<JoinDirectRoute>();
  jd.ja = ja;
  if (sliced) jd.sa = sa;
  r->kind = sliced ? ROUTE_JOIN_SLICED : (match_join_direct_clustered(p, ja, ko, &jd.ca) ? ROUTE_JOIN_DIRECT_CLUSTERED : ROUTE_JOIN_DIRECT);
  return true;
}

int32_t launch_lds_join(LaunchRoute& r, const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp, int64_t* slabs,
                        const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, hipStream_t s, bool* launched) {
  *launched = true;
  if (r.kind == ROUTE_SLICED2 || r.kind == ROUTE_SLICED2_TWO_LEVELS) {
    return launch_join_sliced2(plan, d_plan, kp, r.as<Slice2Args>(), r.shape, slabs, ko, props, s, launched);
  }
  r.as<JoinDirectRoute>().ja.kp = kp;
  r.as<JoinDirectRoute>().ja.slabs = slabs;
  return launch_join_direct(r, props, s);
}

// ---- GroupByBaselineHash behind the sliced join (`GROUP BY dim.dval % 64`) -----------------------------------------
// The reference's planner has no range for a modulo (QE/ExpressionRange.cpp:391-419), so the OUTPUT is an open-addressing
// table -- but the kernel can bound the key itself: payload % m lies in (-m, m).  The plan runs as an INTERNAL perfect-hash
// plan over that range (the same scatter and LDS passes as C3g, a dense private group table beside every slice); the slabs
// are folded into the open-addressing table through the reference's probe sequence (scan_bh.hip: hdk_bh_fold_dense).
struct BhBehindSlicedRoute { BhBehindSliced bh; Slice2Args ga; LaunchShape inner_shape; };

// `r` holds the open-addressing interpreter's route (the armed fallback): it becomes this one when the plan has the shape
bool route_baseline_sliced_join(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props,
                                RouteSet refused, LaunchRoute* r) {
  if (p->query_kind != HDK_Q_BASELINE_HASH || p->num_joins != 1 || p->key_count != 1 || p->key_width != 8 || p->output_columnar) return false;
  if (!ko || (ko->flags & (HDK_HIP_LAUNCH_FORCE_GLOBAL_ATOMICS | HDK_HIP_LAUNCH_FORCE_PARTITIONED)) || launch_forces_generic(ko)) return false;
  const hdk_hip_expr& ke = p->keys[0];
  if (ke.nsteps != 1 || ke.leaf0.kind != HDK_LEAF_COL) return false;
  const hdk_hip_step& sp = ke.steps[0];
  if (sp.op != HDK_OP_MOD || sp.out_class != HDK_VC_INT || sp.rhs.kind != HDK_LEAF_INT || sp.rhs.ival < 1 || sp.rhs.ival > 4096) return false;
  const hdk_hip_col& kc = p->cols[ke.leaf0.col];
  const int64_t m = sp.rhs.ival;
  const bool nonneg = kc.has_stats && kc.min_val >= 0;
  const int64_t lo = nonneg ? 0 : -(m - 1), hi = m - 1;
  const bool has_null = ke.nullable != 0;
  hdk_hip_plan inner = *p;
  inner.query_kind = HDK_Q_PERFECT_HASH;
  inner.keyless = 0;
  inner.idx_target_as_key = -1;
  inner.key_min[0] = lo;
  inner.key_bucket[0] = 0;
  inner.key_card[0] = static_cast<uint32_t>(hi - lo + 1 + (has_null ? 1 : 0));
  inner.key_has_nulls[0] = has_null ? 1 : 0;
  inner.key_null_translated[0] = hi + 1;
  inner.entry_count = static_cast<uint32_t>(hi - lo + 1 + (has_null ? 1 : 0));
  LaunchShape shape = base_shape(&inner, ko, props);
  if (shape.strategy != STRAT_LDS) return false;
  if (!ko->grid_dim_x) shape.grid = interpreter_grid(&inner, ko, shape.lds_bytes, props);
  // (two views of the same bytes: the interpreter's geometry is copied out before the matcher writes over it, and put back
  // when this route does not take the plan)
  const BhGeom g = r->as<BhGeom>();
  BhBehindSlicedRoute& b = r->as<BhBehindSlicedRoute>();
  const RouteKind kind = match_join_sliced2(&inner, shape, ko, &b.ga) ? (b.ga.two_level ? ROUTE_BH_BEHIND_SLICED2_TWO_LEVELS : ROUTE_BH_BEHIND_SLICED2)
                                                                       : ROUTE_BH_VEC_JOIN;
  if (kind == ROUTE_BH_VEC_JOIN || route_refused(refused, kind)) {
    r->as<BhGeom>() = g;
    return false;
  }
  r->kind = kind;
  b.inner_shape = shape;
  b.bh.g = g;
  BhDenseFold* fold = &b.bh.fold;
  memset(fold, 0, sizeof(*fold));
  fold->entries = inner.entry_count;
  fold->out_entry_count = p->entry_count;
  fold->wpe = b.ga.wpe;
  for (int w = 0; w < b.ga.wpe; ++w) fold->wop[w] = b.ga.wop[w];
  fold->nword_mask = b.ga.nword_mask;
  fold->key_lo = lo;
  fold->null_entry = has_null ? static_cast<uint32_t>(hi + 1 - lo) : 0xFFFFFFFFu;
  fold->null_key = ke.null_val;
  return true;
}

int32_t launch_baseline_sliced_join(LaunchRoute& r, const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp,
                                    const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, hipStream_t s, bool* launched) {
  *launched = false;
  BhBehindSlicedRoute& b = r.as<BhBehindSlicedRoute>();
  const LaunchShape& shape = b.inner_shape;
  AsyncScratch slabs(s);
  if (hipMallocAsync(&slabs.p, static_cast<size_t>(shape.grid) * shape.slab_words * 8, s) != hipSuccess) {
    (void)hipGetLastError();
    slabs.p = nullptr;
    return HDK_HIP_OK;
  }
  return launch_join_sliced2(plan, d_plan, kp, b.ga, shape, static_cast<int64_t*>(slabs.p), ko, props, s, launched, &b.bh);
}

}  // namespace hdk
