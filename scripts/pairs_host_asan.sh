#!/bin/bash
# The host side of the paired-end paths (lmat_reads_upload_pairs, the three forms of stream submit, their refusals, empty batches, the
# threaded bookkeeping) as a stand-alone program under AddressSanitizer + UBSan, without a GPU: the library's own host sources are
# linked against lmat_amd/csrc/hostcheck/ -- HIP calls on heap blocks of exactly the size asked for, and the pack / offset launchers
# making their kernels' reads and writes index for index -- so every copy and index is checked against the size of its buffer.
# Prints "pairs host paths: clean" and exits 0, or the sanitizer's report.
set -e
cd "$(dirname "$0")/../lmat_amd/csrc"
T=$(mktemp -d)
g++ -std=c++17 -O1 -g -w -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -ffp-contract=off \
    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I. -I../../include -o $T/pairs_host \
    hostcheck/pairs_host_main.cpp hostcheck/hip_stub.cpp hostcheck/launch_stub.cpp lmat_api.cpp taxonomy.cpp dbbuild.cpp nullmodel.cpp collective.cpp \
    -Wl,--unresolved-symbols=ignore-all -lz -lpthread -ldl
$T/pairs_host
rm -rf $T
