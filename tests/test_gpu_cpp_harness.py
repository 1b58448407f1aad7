"""The executed C++ binding: tests/cpp/harness.cpp drives HipMgr (over the reference's GpuMgr interface), make_plan
(from a QueryMemoryDescriptor-shaped object), the plan extractor (HipPlanExtractor.h over the stand-in hdk::ir tree:
taxi Q3, the C5 shape through the radix-partitioned passes, a filter projection, float accumulators), the *_on_device
forwards, hdk_hip_reduce_buffers and HipKernel::launch(ko, params) with the 12-pointer block -- no Python between
main() and the kernels.  Its output is compared with the committed golden
(tests/golden/cpp_harness_output.txt, computed with numpy by tests/golden/gen_cpp_harness_golden.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cpp_harness_output.txt")


@pytest.mark.gpu
def test_cpp_harness_matches_the_golden():
    # built by __graft_entry__.build() against the reference's own GpuMgr.h where that tree exists (oracle/Makefile, target
    # `cpp`); a machine without the tree runs the binary built there
    exe = os.path.join(ROOT, "oracle", "_ref", "cpp", "harness")
    assert os.path.exists(exe), "oracle/_ref/cpp/harness is missing: run __graft_entry__.build() where the reference tree exists"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = open(GOLDEN).read().split("\n")
    got = r.stdout.strip().split("\n")
    assert got == [w for w in want if w], r.stderr
    # the steps ran on the specialised kernels, not on an interpreter fallback
    err = r.stderr
    assert "c2: hdk_scan_agg_direct" in err and "q3: hdk_scan_agg_keys" in err, err
    assert "c5: hdk_part_scatter" in err and "projection: hdk_scan_project" in err and "floats: hdk_scan_agg_keys_values" in err, err


@pytest.mark.gpu
def test_cpp_multi_device_merge_matches_the_golden():
    """tests/cpp/multi_device.cpp: hdk_amd/glue/HipReduce.h -- ONE process, ncclCommInitAll over every device HipMgr reports,
    a host thread per device: ncclAllGather + hdk_hip_reduce_buffers for the perfect-hash partials, hdk_hip_scatter_to_owners
    -> grouped ncclSend / ncclRecv -> hdk_hip_aggregate_from_ranks for the open-addressing group-by.  The result does not
    depend on the number of devices (one here: a rank exchanging with itself, every kernel and both collectives run)."""
    exe = os.path.join(ROOT, "oracle", "_ref", "cpp", "multi_device")
    assert os.path.exists(exe), "oracle/_ref/cpp/multi_device is missing: run __graft_entry__.build() where the reference tree exists"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    want = [w for w in open(os.path.join(ROOT, "tests", "golden", "cpp_multi_device_output.txt")).read().split("\n") if w]
    got = [ln for ln in r.stdout.strip().split("\n") if ln.startswith("mg_")]  # (RCCL may print a banner of its own)
    assert got == want, r.stderr[-3000:]
    assert "multi_device: " in r.stderr and "owner(s)" in r.stderr
