#!/bin/bash
# tools/build_variant.sh NAME [-DFLAG ...] : build dgl-ke_amd/variants/libkge_NAME.so for A/B runs
# (the sources are csrc/Makefile's SRCS: a variant library must export everything dglke_amd/_lib.py binds)
NAME=$1; shift
cd "$(dirname "$0")/../dgl-ke_amd" && mkdir -p variants build/var_$NAME
SRCS=$(sed -n 's/^SRCS *= *//p' csrc/Makefile)
[ -n "$SRCS" ] || { echo "no SRCS line in csrc/Makefile" >&2; exit 1; }
OBJS=
for s in $SRCS; do
  f=${s%.hip}; OBJS="$OBJS build/var_$NAME/$f.o"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-kernarg-preload-count=16 "$@" -c csrc/$s -o build/var_$NAME/$f.o &
done; wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS -o variants/libkge_$NAME.so && echo built variants/libkge_$NAME.so
