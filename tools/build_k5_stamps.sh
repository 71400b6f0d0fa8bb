#!/bin/bash
# diagnostic build of the library with k_lookup_v5's phase stamps (see tools/k5_stamps.py); the normal objects must be built first
set -e
cd "$(dirname "$0")/../shrimp_amd/csrc"
mkdir -p /tmp/k5st
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-atomic-optimizer-strategy=None -DGM_TUNING -DK5_STAMPS $K5_EXTRA -c gm_lookup5.hip -o /tmp/k5st/gm_lookup5_st.o
# (every object of the normal build but gm_lookup5.o, whatever the Makefile's list has grown to)
hipcc --offload-arch=gfx950 -shared -o ../${K5_OUT:-libgm_k5stamps.so} $(ls build/*.o | grep -v '/gm_lookup5\.o$') /tmp/k5st/gm_lookup5_st.o -lz
