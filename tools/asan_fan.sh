#!/bin/bash
# The fan exchange's host arithmetic under AddressSanitizer + UBSan (CPU only):
# tools/fan_host_check.cpp, a stand-alone program, linked with the host
# library's sources built the same way; then tools/stream_loop_check.cpp, the
# stream engines' loop, likewise stand-alone.  Nothing is loaded into python.
# Usage: tools/asan_fan.sh [build-dir]   (default: a fresh temporary directory)
set -e -o pipefail
cd "$(dirname "$0")/.."
d=${1:-$(mktemp -d)}
SAN="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
gcc $SAN -std=c11 -D_GNU_SOURCE -c mpi-perf_amd/host/mpx_host.c -o "$d/mpx_host.o"
g++ $SAN -std=c++17 -D__HIP_PLATFORM_AMD__ -I"${ROCM:-/opt/rocm}/include" -Impi-perf_amd/csrc -Impi-perf_amd/host \
    tools/fan_host_check.cpp "$d/mpx_host.o" -o "$d/fan_host_check"
ASAN_OPTIONS=detect_leaks=1 "$d/fan_host_check"
# the stream engines' one loop with its recording operations object, built the same way
g++ $SAN -std=c++17 -D__HIP_PLATFORM_AMD__ -I"${ROCM:-/opt/rocm}/include" -Impi-perf_amd/csrc \
    tools/stream_loop_check.cpp -o "$d/stream_loop_check"
ASAN_OPTIONS=detect_leaks=1 "$d/stream_loop_check"
