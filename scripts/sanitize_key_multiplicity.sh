#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the HOST side of hdk_hip_key_multiplicity (argument checks, workspace
# arithmetic) with a stand-alone program: tests/cpp/key_multiplicity_args.cpp has its own main and is linked with the
# sanitizers' runtime, so nothing is preloaded and nothing is loaded into an interpreter.  It needs no device: every call
# it makes comes back before one is touched.  The library is the host-sanitized variant that scripts/run_sanitizers.sh
# builds too (device code is not instrumented).
# Usage: bash scripts/sanitize_key_multiplicity.sh      exit status 0 = no report
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
export ASAN_OPTIONS=detect_leaks=0:halt_on_error=1:abort_on_error=1
export UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1
make -C hdk_amd/csrc variant NAME=asan DEFS="-O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-gpu-sanitize" \
  LDEXTRA="-fsanitize=address,undefined -fno-gpu-sanitize" -j4 > /tmp/asan_build.log 2>&1 || { tail -20 /tmp/asan_build.log; exit 1; }
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -shared-libsan -Wall -Werror \
  -I include tests/cpp/key_multiplicity_args.cpp -L hdk_amd -lhdk_hip_asan -Wl,-rpath,"$ROOT/hdk_amd" \
  -Wl,-rpath,"$(dirname "$(/opt/rocm/lib/llvm/bin/clang -print-file-name=libclang_rt.asan-x86_64.so)")" -o "$OUT/key_multiplicity_args"
"$OUT/key_multiplicity_args"
echo "sanitizers: no report"
