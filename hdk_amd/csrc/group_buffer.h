// group_buffer.h -- reading a group-by output buffer on the device: where a slot lives and which entries are empty.
//
// The one definition of ResultSetStorage::isEmptyEntry[Columnar] (RS/ResultSetStorage.cpp:439-521) and of the slot
// addresses that the reductions (reduce.hip) and the columnar results (result_columns.hip) share.  Columnar offsets for
// an entry count other than the plan's come from columnar_slot_off (device_common.h).
#pragma once
#include "device_common.h"

namespace hdk {

constexpr int kMaxSlots = 2 * HDK_HIP_MAX_TARGETS;

struct SlotInit {
  int64_t v[kMaxSlots];
};

HDK_DEV int64_t read_slot(const int8_t* p, int w) {
  return w == 4 ? static_cast<int64_t>(*reinterpret_cast<const int32_t*>(p)) : *reinterpret_cast<const int64_t*>(p);
}

HDK_DEV void slot_ptrs(const hdk_hip_plan* p, int64_t* buf, uint32_t entry_count, uint32_t entry, int t,
                       int first_slot, int8_t** s1, int8_t** s2) {
  const hdk_hip_target& tg = p->targets[t];
  if (p->query_kind == HDK_Q_NON_GROUPED) {
    *s1 = reinterpret_cast<int8_t*>(buf + first_slot);
    *s2 = reinterpret_cast<int8_t*>(buf + first_slot + 1);
  } else if (p->output_columnar) {
    *s1 = reinterpret_cast<int8_t*>(buf) + columnar_slot_off(p, entry_count, first_slot) +
          static_cast<size_t>(entry) * tg.slot_width;
    *s2 = tg.agg == HDK_AGG_AVG ? reinterpret_cast<int8_t*>(buf) + columnar_slot_off(p, entry_count, first_slot + 1) +
                                      static_cast<size_t>(entry) * tg.slot2_width
                                : nullptr;
  } else {
    int8_t* row = reinterpret_cast<int8_t*>(buf + static_cast<size_t>(entry) * p->row_size_quad);
    *s1 = row + tg.slot_off;
    *s2 = row + tg.slot2_off;
  }
}

// ResultSetStorage::isEmptyEntry[Columnar] (RS/ResultSetStorage.cpp:439-521)
HDK_DEV bool is_empty_entry(const hdk_hip_plan* p, const int64_t* buf, uint32_t entry_count, uint32_t e,
                            const SlotInit& init) {
  if (p->query_kind == HDK_Q_NON_GROUPED) {
    return false;
  }
  if (p->keyless) {
    const int ks = p->idx_target_as_key;
    int s = 0;
    const int nt = p->num_targets;
    for (int t = 0; t < nt; ++t) {
      const hdk_hip_target& tg = p->targets[t];
      const int n = tg.agg == HDK_AGG_AVG ? 2 : 1;
      if (ks < s + n) {
        int8_t *s1, *s2;
        slot_ptrs(p, const_cast<int64_t*>(buf), entry_count, e, t, s, &s1, &s2);
        const bool second = ks != s;
        const int w = second ? tg.slot2_width : tg.slot_width;
        int64_t iv = init.v[0];
#pragma unroll
        for (int k = 1; k < kMaxSlots; ++k) {
          if (k == ks) iv = init.v[k];
        }
        if (w == 4) iv = static_cast<int32_t>(iv);
        return read_slot(second ? s2 : s1, w) == iv;
      }
      s += n;
    }
    return true;
  }
  if (p->output_columnar) {
    return buf[e] == HDK_EMPTY_KEY_64;
  }
  const int64_t* keys = buf + static_cast<size_t>(e) * p->row_size_quad;
  return p->key_width == 4 ? *reinterpret_cast<const int32_t*>(keys) == HDK_EMPTY_KEY_32
                           : *keys == HDK_EMPTY_KEY_64;
}

// is_empty_entry as a descriptor: WHERE the word that decides emptiness lives and WHAT it holds in an empty entry --
// entry e is empty when the `width`-byte word at  base + e * stride  (sign-extended) equals `empty`.  The host works
// it out once per call (hdk_hip_columnarize_result), so that a streaming kernel gets it in scalar registers and never
// reads the plan.  The rule is is_empty_entry's, case by case; group-by plans only.
struct EmptyProbe {
  uint64_t base;    // bytes from the buffer start
  uint32_t stride;  // bytes between entries
  uint32_t width;   // bytes of that word
  int64_t empty;
};

inline EmptyProbe empty_probe_of(const hdk_hip_plan* p, uint32_t entry_count, const int64_t* init_vals) {
  EmptyProbe pr = {0, 8, 8, HDK_EMPTY_KEY_64};  // columnar: the first key column
  const uint32_t row_bytes = p->row_size_quad * 8u;
  if (p->keyless) {
    const int ks = p->idx_target_as_key;
    int s = 0;
    for (int t = 0; t < p->num_targets; ++t) {
      const hdk_hip_target& tg = p->targets[t];
      const int n = tg.agg == HDK_AGG_AVG ? 2 : 1;
      if (ks < s + n) {
        const bool second = ks != s;
        const int w = second ? tg.slot2_width : tg.slot_width;
        // (read_slot knows 4- and 8-byte slots, the only ones a keyless plan has had so far; a narrower slot is
        // compared at its own width here, never read past its end)
        pr.width = (w == 1 || w == 2 || w == 4) ? static_cast<uint32_t>(w) : 8u;
        const int drop = 64 - 8 * static_cast<int>(pr.width);
        pr.empty = static_cast<int64_t>(static_cast<uint64_t>(init_vals[ks]) << drop) >> drop;
        if (p->output_columnar) {
          pr.base = columnar_slot_off(p, entry_count, ks);
          pr.stride = static_cast<uint32_t>(w);
        } else {
          pr.base = static_cast<uint64_t>(second ? tg.slot2_off : tg.slot_off);
          pr.stride = row_bytes;
        }
        return pr;
      }
      s += n;
    }
    return pr;  // (validate_plan_layout keeps idx_target_as_key inside the slots)
  }
  if (!p->output_columnar) {
    pr.stride = row_bytes;
    if (p->key_width == 4) {
      pr.width = 4;
      pr.empty = HDK_EMPTY_KEY_32;
    }
  }
  return pr;
}

HDK_DEV int64_t slot_init(const SlotInit& init, int idx) {
  int64_t iv = init.v[0];
#pragma unroll
  for (int k = 1; k < kMaxSlots; ++k) {
    if (k == idx) iv = init.v[k];
  }
  return iv;
}

inline void fill_slot_init(const hdk_hip_plan* plan, const int64_t* init_vals, SlotInit* init) {
  int nslots = 0;
  for (int t = 0; t < plan->num_targets; ++t) {
    nslots += plan->targets[t].agg == HDK_AGG_AVG ? 2 : 1;
  }
  for (int i = 0; i < kMaxSlots; ++i) {
    init->v[i] = i < nslots ? init_vals[i] : 0;
  }
}

}  // namespace hdk
