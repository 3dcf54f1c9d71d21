#!/bin/bash
# builds the attention harness attn_dev.bin
cd "$(dirname "$0")"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-value -I../../include -I../../item_alignment_amd/csrc attn_dev.hip -o attn_dev.bin
