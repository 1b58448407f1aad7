// column_primitives.h -- the wave- and block-level steps that the count / scan / compact kernels share.
#pragma once
#include "device_common.h"

namespace hdk {

constexpr int kTileBlock = 256;  // threads of a block that counts one tile at a time
constexpr int kTileWaves = kTileBlock / kWave;

HDK_DEV uint32_t lane_rank(uint64_t mask) {  // set bits of `mask` below this lane
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// sum of `v` over lanes 0 .. lane of this wave (all 64 lanes call this together)
template <typename T>
HDK_DEV T wave_inclusive_sum(T v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const T up = __shfl_up(v, d, kWave);
    if (lane >= static_cast<uint32_t>(d)) v += up;
  }
  return v;
}

// for data that is read once per pass and is larger than the last-level cache
template <typename T>
HDK_DEV T nt_load(const void* base, size_t byte_off) {
  return __builtin_nontemporal_load(reinterpret_cast<const __attribute__((address_space(1))) T*>(
      reinterpret_cast<uintptr_t>(static_cast<const int8_t*>(base) + byte_off)));
}

// *dst = the sum of `wave_count` over the kTileWaves waves of the block (every thread calls this).  The trailing barrier
// lets a persistent block reuse s_wave for its next tile; a block that counts one tile only passes REUSE = false.
template <bool REUSE = true>
HDK_DEV void block_store_tile_count(uint32_t (&s_wave)[kTileWaves], uint32_t wave_count, uint32_t* dst) {
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_wave[threadIdx.x / kWave] = wave_count;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kTileWaves; ++w) {
      sum += s_wave[w];
    }
    *dst = sum;
  }
  if (REUSE) {
    __syncthreads();
  }
}

}  // namespace hdk
