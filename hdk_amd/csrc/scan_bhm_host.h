// scan_bhm_host.h -- what the translation units around the multi-argument on-chip group-by (scan_bhm.hip; its route and
// launch: route.h) export to it.
#pragma once
#include "host_common.h"
#include "device_common.h"

namespace hdk {

// scan_agg.hip: hdk_finalize over slabs of the generic partial-aggregate words ([slab][entry][word], agg_common.h) that another
// strategy wrote; skip_if != nullptr: the kernel does nothing when *skip_if != 0
int32_t launch_finalize_slabs(const hdk_hip_plan* d_plan, const int64_t* slabs, int64_t** groupby_buf, uint32_t num_slabs,
                              uint32_t entry_count, const uint32_t* skip_if, hipStream_t s);

// scan_baseline.hip: the global-atomics kernel (the reference's own scheme, any plan) ARMED behind another strategy: it runs
// only when *run_if != 0
int32_t launch_scan_global_armed(const hdk_hip_plan* plan, const hdk_hip_plan* d_plan, const KernParams& kp,
                                 const hdk_hip_device_properties* props, hipStream_t s, const uint32_t* run_if);

}  // namespace hdk
