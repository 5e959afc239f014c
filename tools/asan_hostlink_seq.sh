#!/bin/bash
# The host link's sequenced CPU loop (mpi-perf_amd/csrc/mpx_hostlink.h:
# run_seq) under the host sanitizers (CPU only): tools/hostlink_seq_host_check.cpp,
# a stand-alone program in which a second CPU thread plays the GPU's side,
# built with AddressSanitizer + UBSan and once more with ThreadSanitizer, each
# run once.  Nothing is loaded into python.
# Usage: tools/asan_hostlink_seq.sh [build-dir]   (default: a fresh temporary directory)
set -e -o pipefail
cd "$(dirname "$0")/.."
d=${1:-$(mktemp -d)}
COMMON="-O1 -g -std=c++17 -fno-omit-frame-pointer -Impi-perf_amd/csrc -pthread"
g++ $COMMON -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/hostlink_seq_host_check.cpp -o "$d/hostlink_seq_host_check_asan"
ASAN_OPTIONS=detect_leaks=1 "$d/hostlink_seq_host_check_asan"
g++ $COMMON -fsanitize=thread tools/hostlink_seq_host_check.cpp -o "$d/hostlink_seq_host_check_tsan"
"$d/hostlink_seq_host_check_tsan"
