#!/bin/bash
# Runs csrc/gram_grad.hip's batched contraction on the HOST: internal.h here replaces the library's with a shim that runs a
# workgroup as 256 std::threads with a std::barrier for __syncthreads (workgroups one after another), under the host address
# sanitizer.  main.cpp compares B x N x Q x (contiguous / padded w with NaN padding and an odd batch stride) against plain loops
# at 1e-12.  It checks the indexing and the bounds of the kernel's source without a GPU; it says nothing about the compiled
# gfx950 code.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
out=$(mktemp -d)
sed 's/extern __shared__ __align__(16) unsigned char smem_raw\[\];/unsigned char *smem_raw = ::g_smem;/' \
    "$here/../../dp_gp_lvm_amd/csrc/gram_grad.hip" > "$out/gram_grad_emu.inc"
cp "$here/internal.h" "$here/main.cpp" "$out/"
g++ -std=c++20 -O1 -pthread -fsanitize=address -g "$out/main.cpp" -o "$out/emu"
"$out/emu"
