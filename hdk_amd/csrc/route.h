// route.h -- the ONE routing decision of a launch (host only): route_launch (scan_agg.hip) turns (plan, kernel options, device
// properties) into a LaunchRoute; hdk_hip_launch launches it, hdk_hip_describe_launch prints its kernels, hdk_hip_workspace_size
// takes its shape.  A launcher that hands a launch back (no scratch memory, no block that large) gets its route REFUSED and the
// plan is routed again, so the fallback order is the routing order.
#pragma once
#include <type_traits>

#include "device_common.h"
#include "host_common.h"
#include "launch_common.h"

namespace hdk {

enum PrePass { PRE_NONE = 0, PRE_CLUSTER_BY_KEY };

// X(enumerator, family, pre-pass and kernels of the launch in order, armed fallbacks included).  The family, not the place in the
// list, says who launches a route and what surrounds it: LDS* fill slabs that hdk_finalize folds (scan_agg.hip; LDS_JOIN: scan_join.hip),
// BH* fold into the output table themselves (scan_bh_packed.hip, scan_bhm.hip, scan_bh.hip; BH_BEHIND: scan_join.hip), BASELINE: scan_baseline.hip.
#define HDK_ROUTE_LIST(X) \
  X(STREAM_DIRECT, LDS, "hdk_scan_agg_direct,hdk_finalize") \
  X(COLS, LDS, "hdk_scan_agg_cols,hdk_finalize") \
  X(JOIN_SLICED, LDS_JOIN, "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced,hdk_join_agg_direct,hdk_finalize") \
  X(SLICED2, LDS_JOIN, "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize") \
  X(SLICED2_TWO_LEVELS, LDS_JOIN, "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_scatter_level2,hdk_join_agg_sliced2,hdk_scan_agg_vec_join,hdk_finalize") \
  X(JOIN_DIRECT, LDS_JOIN, "hdk_join_agg_direct,hdk_finalize") \
  X(JOIN_DIRECT_CLUSTERED, LDS_JOIN, "hdk_cluster_by_key,hdk_join_agg_direct,hdk_finalize") \
  X(KEYS, LDS, "hdk_scan_agg_keys,hdk_finalize") \
  X(KEYS_VALUES, LDS, "hdk_scan_agg_keys_values,hdk_finalize") \
  X(VEC, LDS, "hdk_scan_agg_vec,hdk_finalize") \
  X(VEC_JOIN, LDS, "hdk_scan_agg_vec_join,hdk_finalize") \
  X(VEC_KEYED, LDS, "hdk_scan_agg_vec_keyed,hdk_finalize") \
  X(VEC_MANY, LDS, "hdk_scan_agg_vec_many,hdk_finalize") \
  X(GENERIC, LDS, "hdk_scan_agg_generic,hdk_finalize") \
  X(BH_PACKED, BH_PACKED, "hdk_scan_agg_bh_packed,hdk_bh_fold_slabs") \
  X(BH_PACKED_PLAIN, BH_PACKED, "hdk_scan_agg_bh_packed_plain,hdk_bh_fold_slabs") \
  X(BH_DENSE, BH_PACKED, "hdk_scan_agg_bh_dense,hdk_bh_fold_slabs") \
  X(BH_DENSE_PLAIN, BH_PACKED, "hdk_scan_agg_bh_dense_plain,hdk_bh_fold_slabs") \
  X(BHM, BHM, "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_bhm_fold") \
  X(BHM_PERFECT, BHM, "hdk_scan_agg_bhm,hdk_bhm_reduce_slabs,hdk_finalize") \
  X(BHM_PART, BHM, "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_bhm_fold")  /* (behind hdk_bhm_part_sample, _layout) */ \
  X(BHM_PART_PERFECT, BHM, "hdk_bhm_scatter,hdk_bhm_aggregate,hdk_bhm_reduce_slabs,hdk_finalize") \
  X(BH_DENSE_PART, BH_PACKED, "hdk_bh_dscatter,hdk_bh_daggregate") \
  X(BH_PARTITIONED, BH_PACKED, "hdk_bh_scatter,hdk_bh_aggregate") \
  X(BH_DIRECT, BH, "hdk_scan_agg_bh_direct") \
  X(BH_VEC, BH, "hdk_scan_agg_bh_vec") \
  X(BH_VEC_JOIN, BH, "hdk_scan_agg_bh_vec_join") \
  X(BH_BEHIND_SLICED2, BH_BEHIND, "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_agg_sliced2,hdk_scan_agg_bh_vec_join,hdk_bh_fold_dense") \
  X(BH_BEHIND_SLICED2_TWO_LEVELS, BH_BEHIND, "hdk_join_order_probe,hdk_join_scatter_slices,hdk_join_scatter_level2,hdk_join_agg_sliced2,hdk_scan_agg_bh_vec_join,hdk_bh_fold_dense") \
  X(RADIX_PARTITIONED, BASELINE, "hdk_part_scatter,hdk_part_scatter,hdk_part_aggregate,hdk_part_overflow,hdk_scan_agg_baseline_direct") \
  X(PERFECT_PARTITIONED, BASELINE, "hdk_pp_scatter,hdk_pp_scatter2,hdk_pp_aggregate,hdk_scan_agg_global") \
  X(BASELINE_DIRECT, BASELINE, "hdk_scan_agg_baseline_direct") \
  X(GLOBAL, BASELINE, "hdk_scan_agg_global") \
  X(PROJECT_FAST, PROJECT, "hdk_scan_project_count,hdk_scan_project_offsets,hdk_scan_project_dense,hdk_scan_project_direct") \
  X(PROJECT_FAST_ONE_PASS, PROJECT, "hdk_scan_project_stream,hdk_scan_project_count,hdk_scan_project_offsets,hdk_scan_project_dense,hdk_scan_project_direct") \
  X(PROJECT_SCALAR, PROJECT, "hdk_scan_project_scalar") \
  X(PROJECT_KEYED, PROJECT, "hdk_scan_project_keyed") \
  X(PROJECT_JOIN, PROJECT, "hdk_scan_project_join") \
  X(PROJECT, PROJECT, "hdk_scan_project")

enum RouteFamily { FAM_LDS, FAM_LDS_JOIN, FAM_BH_PACKED, FAM_BHM, FAM_BH, FAM_BH_BEHIND, FAM_BASELINE, FAM_PROJECT };
enum RouteKind {
#define HDK_ROUTE_ENUM(name, family, kernels) ROUTE_##name,
  HDK_ROUTE_LIST(HDK_ROUTE_ENUM)
#undef HDK_ROUTE_ENUM
      ROUTE_COUNT
};
struct RouteInfo { RouteFamily family; const char* kernels; };
inline const RouteInfo& route_info(RouteKind k) {
  static const RouteInfo info[ROUTE_COUNT] = {
#define HDK_ROUTE_INFO(name, family, kernels) {FAM_##family, kernels},
      HDK_ROUTE_LIST(HDK_ROUTE_INFO)
#undef HDK_ROUTE_INFO
  };
  return info[k];
}
inline RouteFamily route_family(RouteKind k) { return route_info(k).family; }
// routes whose launcher handed the launch back
typedef uint64_t RouteSet;
static_assert(ROUTE_COUNT <= 64, "RouteSet is one word");
inline bool route_refused(RouteSet refused, RouteKind k) { return (refused >> k) & 1; }

// the scan kernels of the LDS strategy: the caller folds their slabs with hdk_finalize
inline bool route_fills_slabs(RouteKind k) { return route_family(k) == FAM_LDS || route_family(k) == FAM_LDS_JOIN; }
// the open-addressing kernels of scan_bh*.hip: the readers of fused join tables among the routes beyond the LDS strategy
inline bool route_is_on_chip_bh(RouteKind k) { return route_family(k) >= FAM_BH_PACKED && route_family(k) <= FAM_BH_BEHIND; }
// a join that reads its outer rows as tuples of its own: no clustering pre-pass in front of it
inline bool route_clusters_its_own_input(RouteKind k) { return route_family(k) == FAM_LDS_JOIN || route_family(k) == FAM_BH_BEHIND; }

// A plain value: nothing on the heap, nothing kept between calls.
struct LaunchRoute {
  PrePass pre;
  RouteKind kind;
  LaunchShape shape;
  alignas(16) unsigned char args[12 * 1024];          // what the matcher that won filled in: as<ItsArgs>()
  alignas(16) unsigned char pre_args[2 * 1024];   // the pre-pass's

  template <class T, size_t N>
  static T& view(unsigned char (&bytes)[N]) {
    static_assert(sizeof(T) <= N && alignof(T) <= 16 && std::is_trivially_copyable<T>::value, "argument block of a route");
    return *reinterpret_cast<T*>(bytes);
  }
  template <class T> T& as() { return view<T>(args); }
  template <class T> T& pre_as() { return view<T>(pre_args); }
};

// ---- every family: route a plan (false: not this family's), launch a route (*launched = false: handed back) ------------------------
// scan_bhm.hip <- scan_bh_packed.hip (its packed forms first, its partitioned forms last) <- scan_bh.hip (then its own two)
bool route_bhm(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, RouteSet refused, LaunchRoute* r);
bool route_bh_packed(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, RouteSet refused, LaunchRoute* r);
bool route_bh(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, RouteSet refused, LaunchRoute* r);
int32_t launch_bhm(LaunchRoute& r, const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp, const hdk_hip_kernel_options* ko,
                   const hdk_hip_device_properties* props, hipStream_t s, bool* launched);
int32_t launch_bh_packed(LaunchRoute& r, const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp,
                         const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, hipStream_t s, bool* launched);
int32_t launch_bh(LaunchRoute& r, const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp, const hdk_hip_kernel_options* ko,
                  const hdk_hip_device_properties* props, hipStream_t s, bool* launched);
// scan_join.hip: the join kernels among the LDS strategy's plans (r->shape.grid: the interpreter's, which stays armed behind them);
// the clustering pre-pass in front of another route's join probes (fills r->pre_args; *scratch: freed by the caller after the scan)
bool route_lds_join(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, RouteSet refused,
                    LaunchRoute* r);
int32_t launch_lds_join(LaunchRoute& r, const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp, int64_t* slabs,
                        const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, hipStream_t s, bool* launched);
bool route_cluster_prepass(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, LaunchRoute* r);
int32_t launch_cluster_prepass(LaunchRoute& r, KernParams* kp, const hdk_hip_device_properties* props, hipStream_t s, void** scratch);
// ... and a baseline-hash plan with a bounded key behind the sliced join (an internal dense table + hdk_bh_fold_dense)
bool route_baseline_sliced_join(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props,
                                RouteSet refused, LaunchRoute* r);
int32_t launch_baseline_sliced_join(LaunchRoute& r, const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp,
                                    const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, hipStream_t s, bool* launched);
// scan_baseline.hip: STRAT_GLOBAL -- the routes above, the partitioned passes, the global-atomics kernels (always routes; sets
// the grid).  *init_output: HDK_HIP_LAUNCH_INIT_OUTPUT is still to do (fused into the radix passes' last, else the init kernel first)
void route_baseline(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, RouteSet refused,
                    LaunchRoute* r);
int32_t launch_baseline(LaunchRoute& r, const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp,
                        const hdk_hip_kernel_options* ko, bool* init_output, const hdk_hip_device_properties* props, hipStream_t s,
                        bool* launched);
// scan_project.hip: STRAT_PROJECT (always routes; sets the grid)
void route_project(const hdk_hip_plan* p, const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, LaunchRoute* r);
int32_t launch_project(LaunchRoute& r, const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp,
                       const hdk_hip_kernel_options* ko, const hdk_hip_device_properties* props, hipStream_t s);

}  // namespace hdk
