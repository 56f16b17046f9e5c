#!/bin/bash
# A second librwkv.so with ONE source built with extra flags (A/B runs on one box: tools/gpu_r5.sh ab):
#   tools/build_variant.sh lib_b ring_v6 -DR6_RT_STAMPS=1
#   tools/build_variant.sh lib_b prefill -DPF_EXP_STAMP
# ring_v6 is two translation units -- ring_v6.hip (the product kernels) and ring_v6_instr.hip (the instrumented ones, the same body included:
# every stamp is compiled there) -- so SRC = ring_v6 rebuilds both with the flags.
set -eu
cd "$(dirname "$0")/../rwkv.cpp_amd"
D=$1; SRC=$2; shift 2
mkdir -p build_$D $D
SRCS=$SRC
if [ $SRC = ring_v6 ]; then SRCS="ring_v6 ring_v6_instr"; fi
for s in $SRCS; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 "$@" -O3 -std=c++17 -ffp-contract=off -fPIC -DRWKV_SHARED -DRWKV_BUILD -fvisibility=hidden -I../include -Icsrc -Wall -Wno-unused-function -Wno-unused-variable -c csrc/$s.hip -o build_$D/$s.o &
done
wait
OBJS=$(for o in $(sed -n 's/^SRCS = //p' Makefile); do case " $SRCS " in *" $o "*) echo build_$D/$o.o;; *) echo build/$o.o;; esac; done)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--version-script=csrc/rwkv.map -o $D/librwkv.so $OBJS -ldl
ls -la $D/librwkv.so
