// key_multiplicity_args.cpp -- hdk_hip_key_multiplicity's host side under AddressSanitizer / UBSan: a stand-alone program
// (its own main, nothing loaded into an interpreter) that walks the argument checks and the workspace arithmetic of the
// call.  Every call here comes back before any device is touched: the pointers are made up and never dereferenced.
// scripts/sanitize_key_multiplicity.sh builds it against the host-sanitized variant of the library and runs it.
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "hdk_hip.h"

static int failures = 0;

#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, hdk_hip_last_error()); \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static hdk_hip_multiplicity_key key(int32_t col) {
  hdk_hip_multiplicity_key k;
  memset(&k, 0, sizeof(k));
  k.col = col;
  k.nullable = 1;
  k.null_bits = INT64_MIN;
  k.max_val = 99;
  k.translated_null = 100;
  return k;
}

struct Args {
  const int64_t* cols = reinterpret_cast<const int64_t*>(4096);
  uint64_t capacity = 100;
  int32_t num_cols = 3;
  uint64_t num_rows = 100;
  const hdk_hip_multiplicity_key* keys = nullptr;
  int32_t num_keys = 1;
  int64_t entry_count = 100;
  int64_t bucket = 1;
  uint32_t flags = 0;
  hdk_hip_key_multiplicity_result* result = reinterpret_cast<hdk_hip_key_multiplicity_result*>(1 << 20);
  void* workspace = nullptr;
  size_t workspace_bytes = 0;
  int32_t device_id = 0;
};

static int32_t call(const Args& a) {
  return hdk_hip_key_multiplicity(a.cols, a.capacity, a.num_cols, a.num_rows, a.keys, a.num_keys, a.entry_count, a.bucket, a.flags,
                                  a.result, a.workspace, a.workspace_bytes, a.device_id, nullptr);
}

static bool refused(const Args& a, const char* word) {
  return call(a) == HDK_HIP_ERR_INVALID_ARG && strstr(hdk_hip_last_error(), word) != nullptr;
}

int main() {
  hdk_hip_multiplicity_key keys[4] = {key(1), key(0), key(2), key(0)};
  Args ok;
  ok.keys = keys;
  {
    Args a = ok;
    a.cols = nullptr;
    EXPECT(refused(a, "NULL"));
    a = ok;
    a.keys = nullptr;
    EXPECT(refused(a, "NULL"));
    a = ok;
    a.result = nullptr;
    EXPECT(refused(a, "NULL"));
  }
  for (int32_t nk : {0, 4, -1}) {
    Args a = ok;
    a.num_keys = nk;
    a.entry_count = 0;
    EXPECT(refused(a, "num_keys"));
  }
  for (int32_t col : {3, -1}) {
    hdk_hip_multiplicity_key bad[2] = {key(0), key(col)};
    Args a = ok;
    a.keys = bad;
    a.num_keys = 2;
    a.entry_count = 0;
    EXPECT(refused(a, "names column"));
  }
  {
    Args a = ok;
    a.num_rows = uint64_t(1) << 32;
    a.capacity = uint64_t(1) << 33;
    EXPECT(refused(a, "32-bit"));
    a = ok;
    a.num_rows = 101;
    EXPECT(refused(a, "capacity"));
    a = ok;
    a.entry_count = -1;
    EXPECT(refused(a, "entry_count"));
    a.entry_count = int64_t(1) << 31;
    EXPECT(refused(a, "entry_count"));
    a = ok;
    a.num_keys = 2;
    EXPECT(refused(a, "entry_count"));
    a = ok;
    a.bucket = 0;
    EXPECT(refused(a, "bucket"));
    a.bucket = INT64_MIN;
    EXPECT(refused(a, "bucket"));
    a = ok;
    a.flags = 2;
    EXPECT(refused(a, "flags"));
    a = ok;
    a.result = reinterpret_cast<hdk_hip_key_multiplicity_result*>((1 << 20) + 4);
    EXPECT(refused(a, "aligned"));
    a.result = reinterpret_cast<hdk_hip_key_multiplicity_result*>(4096 + 16);
    EXPECT(refused(a, "overlap"));
  }
  // the workspace of both routes: too small, misaligned, overlapping the columns
  for (int route = 0; route < 2; ++route) {
    Args a = ok;
    if (route) {
      a.num_keys = 3;
      a.entry_count = 0;
    }
    const size_t need = hdk_hip_key_multiplicity_workspace_bytes(a.num_rows, a.keys, a.num_keys, a.entry_count);
    EXPECT(need > 0 && need % 256 == 0);
    a.workspace = reinterpret_cast<void*>(1 << 24);
    a.workspace_bytes = need - 1;
    EXPECT(refused(a, "needed"));
    a.workspace_bytes = need;
    a.workspace = reinterpret_cast<void*>((1 << 24) + 4);
    EXPECT(refused(a, "aligned"));
    a.workspace = reinterpret_cast<void*>(4096 + 1024);
    EXPECT(refused(a, "overlap"));
  }
  // the arithmetic at its ends: the largest table, the largest row count, what the call would refuse
  EXPECT(hdk_hip_key_multiplicity_workspace_bytes(1, keys, 1, INT32_MAX) == ((size_t(INT32_MAX) * 4 + 255) & ~size_t(255)) + 65536);
  EXPECT(hdk_hip_key_multiplicity_workspace_bytes((uint64_t(1) << 32) - 1, keys, 3, 0) > (uint64_t(1) << 32) * 8 * 3);
  EXPECT(hdk_hip_key_multiplicity_workspace_bytes(0, keys, 1, 100) == 0);
  EXPECT(hdk_hip_key_multiplicity_workspace_bytes(100, nullptr, 1, 100) == 0);
  EXPECT(hdk_hip_key_multiplicity_workspace_bytes(100, keys, 4, 0) == 0);
  EXPECT(hdk_hip_key_multiplicity_workspace_bytes(100, keys, 2, 7) == 0);
  EXPECT(hdk_hip_key_multiplicity_workspace_bytes(100, keys, 1, -1) == 0);
  // valid arguments on a device that does not exist: refused at the door of the device, after every check
  {
    Args a = ok;
    a.device_id = -1;
    EXPECT(refused(a, "device -1"));
    a.num_keys = 3;
    a.entry_count = 0;
    EXPECT(refused(a, "device -1"));
    a = ok;
    a.device_id = -1;
    a.cols = nullptr;
    a.num_rows = 0;
    a.capacity = 0;
    EXPECT(refused(a, "device -1"));
    a = ok;
    a.device_id = -1;
    a.entry_count = INT32_MAX;
    a.bucket = 86400;
    a.flags = HDK_HIP_KEYS_NULLS_MATCH;
    EXPECT(refused(a, "device -1"));
  }
  if (failures) {
    fprintf(stderr, "key_multiplicity_args: %d failures\n", failures);
    return 1;
  }
  printf("key_multiplicity_args: ok\n");
  return 0;
}
