#!/bin/bash
# The host side of the device images (lmat_db_save_image / lmat_db_load_image of LMATIMG2, lmat_image_check: the header checks, the
# streaming through pinned buffers, the refusals that must leave the context as it was) as a stand-alone program under
# AddressSanitizer + UBSan, without a GPU: the library's own host sources are linked against lmat_amd/csrc/hostcheck/ -- HIP calls on
# heap blocks of exactly the size asked for -- so every copy and index is checked against the size of its buffer.
# Prints "image host paths: clean" and exits 0, or the sanitizer's report.
set -e
cd "$(dirname "$0")/../lmat_amd/csrc"
T=$(mktemp -d)
g++ -std=c++17 -O1 -g -w -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -ffp-contract=off \
    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I. -I../../include -o $T/image_host \
    hostcheck/image_host_main.cpp hostcheck/hip_stub.cpp hostcheck/launch_stub.cpp lmat_api.cpp taxonomy.cpp dbbuild.cpp nullmodel.cpp collective.cpp \
    -Wl,--unresolved-symbols=ignore-all -lz -lpthread -ldl
$T/image_host
rm -rf $T
