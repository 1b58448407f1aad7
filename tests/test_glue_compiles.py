"""The HDK-side C++ bindings (hdk_amd/glue/) compile against the reference's own interface headers
where /root/reference exists (build container); skipped on the GPU box."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/omniscidb"


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present")
def test_hipmgr_glue_compiles_against_reference_gpumgr(tmp_path):
    src = tmp_path / "glue_check.cpp"
    src.write_text('#include "HipMgr.h"\n#include "HipRuntimeOnDevice.h"\n'
                   "// instantiates every override: HipMgr must not be abstract\n"
                   "GpuMgr* make() { return new hip_mgr::HipMgr(); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", REF, "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hdk_amd", "glue"), str(src)])


def test_public_header_is_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    src.write_text('#include "hdk_hip.h"\nint main(void) { return sizeof(hdk_hip_plan) > 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-pedantic", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_join_build_forwards_instantiate(tmp_path):
    """The templated *_on_device forwards instantiate with structs that carry the reference's member
    names (JoinColumn / JoinColumnTypeInfo / HashEntryInfo, HashJoinRuntime.h:43-57,100-124).  The real
    header pulls in Logger.h -> Boost, absent here, so the test declares same-shaped structs itself:
    this checks the templates, not the reference's layout."""
    src = tmp_path / "fwd_check.cpp"
    src.write_text('''
#include <cstddef>
#include <cstdint>
enum ColumnType { SmallDate = 0, Signed = 1, Unsigned = 2, Double = 3 };
struct JoinColumn { const int8_t* col_chunks_buff; size_t col_chunks_buff_sz; size_t num_chunks; size_t num_elems; size_t elem_sz; };
struct JoinColumnTypeInfo { size_t elem_sz; int64_t min_val; int64_t max_val; int64_t null_val; bool uses_bw_eq;
                            int64_t translated_null_val; ColumnType column_type; };
struct HashEntryInfo { size_t hash_entry_count; int64_t bucket_normalization; };
#include "HipRuntimeOnDevice.h"
void f(int8_t* b, int32_t* otm, int* err, const JoinColumn* jc, const JoinColumnTypeInfo* ti, HashEntryInfo hei) {
  hip_rt::init_hash_join_buff_on_device(otm, 10, -1, 0);
  hip_rt::fill_hash_join_buff_on_device(otm, -1, false, err, jc[0], ti[0], 0);
  hip_rt::fill_hash_join_buff_on_device_bucketized(otm, -1, false, err, jc[0], ti[0], 4, 0);
  hip_rt::fill_one_to_many_hash_table_on_device(otm, hei, -1, jc[0], ti[0], 0);
  hip_rt::init_baseline_hash_join_buff_on_device<8>(b, 100, 2, true, -1, 0);
  hip_rt::fill_baseline_hash_join_buff_on_device<8>(b, 100, -1, false, 2, true, err, jc, ti, 0);
  hip_rt::fill_one_to_many_baseline_hash_table_on_device<4>(otm, b, 100, -1, 2, jc, ti, 0);
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "hdk_amd", "glue"), str(src)])


def test_hipkernel_glue_compiles(tmp_path):
    """hdk_amd/glue/HipKernel.h against declarations shaped like the reference's QueryEngine/DeviceKernel.h:25-65
    (DeviceClock, KernelOptions, DeviceKernel) and CompilationContext.h:23-26.  The real headers pull in LLVM and
    Boost, absent here, so the test restates the four declarations: it checks that HipKernel overrides every pure
    virtual with the reference's signatures, not the reference's file."""
    src = tmp_path / "kernel_check.cpp"
    src.write_text('''
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>
class CompilationContext { public: virtual ~CompilationContext() {} };
class DeviceClock { public: virtual void start() = 0; virtual int stop() = 0; virtual ~DeviceClock() = default; };
struct KernelOptions { unsigned int gridDimX = 1, gridDimY = 1, gridDimZ = 1, blockDimX = 1, blockDimY = 1, blockDimZ = 1;
                       unsigned int sharedMemBytes = 0, literalsOffset = 0; bool hoistLiterals = true; };
class DeviceKernel {
 public:
  virtual void launch(const KernelOptions& ko, std::vector<int8_t*>& kernelParams) = 0;
  virtual void initializeDynamicWatchdog(bool could_interrupt, uint64_t cycle_budget, size_t time_limit) {}
  virtual void initializeRuntimeInterrupter() {}
  virtual std::unique_ptr<DeviceClock> make_clock() = 0;
  virtual ~DeviceKernel() = default;
};
#include "HipKernel.h"
struct Arena : hip_rt::HipWorkspaceAllocator { int8_t* alloc(size_t) override { return nullptr; } };
std::unique_ptr<DeviceKernel> make(const hip_rt::HipPlanContext* ctx, Arena* a) {
  return std::make_unique<hip_rt::HipKernel>(ctx, 0, a, 1000, true);   // not abstract: every pure virtual is overridden
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "hdk_amd", "glue"), str(src)])


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present")
def test_cpp_harness_compiles_against_the_reference_gpumgr():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-parameter", "-I", REF,
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hdk_amd", "glue"), "-I",
                           os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "harness.cpp")])


def test_cpp_harness_golden_is_what_the_generator_prints():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_cpp_harness_golden",
                                                  os.path.join(ROOT, "tests", "golden", "gen_cpp_harness_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = open(os.path.join(ROOT, "tests", "golden", "cpp_harness_output.txt")).read().strip().split("\n")
    assert mod.expected_lines() == want
    want_mg = open(os.path.join(ROOT, "tests", "golden", "cpp_multi_device_output.txt")).read().strip().split("\n")
    assert mod.multi_device_lines() == want_mg


@pytest.mark.skipif(not (os.path.isdir(REF) and os.path.exists("/opt/rocm/include/rccl/rccl.h")), reason="reference tree / RCCL headers not present")
def test_multi_device_merge_host_compiles_against_rccl():
    """hdk_amd/glue/HipReduce.h (ncclCommInitAll, ncclAllGather, grouped ncclSend / ncclRecv around the C ABI's reduce and
    tuple-exchange calls) and its harness compile against the image's rccl.h -- and link, so that every symbol it names
    exists in librccl / libamdhip64 / libhdk_hip (running it needs a GPU: tests/test_gpu_cpp_harness.py)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "--no-print-directory", "_ref/cpp/multi_device"])
    assert os.access(os.path.join(ROOT, "oracle", "_ref", "cpp", "multi_device"), os.X_OK)
