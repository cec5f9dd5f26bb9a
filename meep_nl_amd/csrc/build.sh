#!/bin/bash
# Build meep_nl_amd/libmnl.so for gfx950 (MI355X).  hipcc for the kernels,
# g++ for the host side (see mnl_host.cpp header for why): mnl_host.cpp (C-ABI), mnl_setup.cpp
# (grid, PML, materials, quadrature), mnl_sources.cpp (sources, get_field), mnl_fused.cpp
# (fused-tile planning), mnl_tb.cpp (pairs of steps), mnl_step.cpp (the step loop, NaN guard),
# mnl_tune.cpp (the tuner), mnl_dft.cpp (DFT monitors), mnl_io.cpp (checkpoints, slices, energy),
# mnl_stats.cpp (kernel statistics, the byte model), mnl_comm.cpp (RCCL / IPC).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT=${MNL_OUT:-"$HERE/../libmnl.so"}
ROCM=${ROCM_PATH:-/opt/rocm}
TMP=${MNL_OBJ:-"$HERE/_obj"}
mkdir -p "$TMP"
ARCH=${MNL_ARCH:-gfx950}
hipcc --offload-arch=$ARCH $MNL_KFLAGS -O3 -ffp-contract=off -fPIC -std=c++17 -Wall \
  -c "$HERE/mnl_kernels.hip" -o "$TMP/mnl_kernels.o"
CXXF="$MNL_KFLAGS -O2 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-result -D__HIP_PLATFORM_AMD__ -I$ROCM/include"
HOST_SRCS="mnl_host mnl_setup mnl_sources mnl_fused mnl_tb mnl_step mnl_tune mnl_dft mnl_io mnl_stats mnl_comm"
OBJS="$TMP/mnl_kernels.o"
for s in $HOST_SRCS; do
  g++ $CXXF -c "$HERE/$s.cpp" -o "$TMP/$s.o"
  OBJS="$OBJS $TMP/$s.o"
done
# Link with g++ so the host's complex arithmetic (__muldc3 / __divdc3 of
# std::complex) comes from libgcc as in the reference (and the oracle), not
# from clang's compiler-rt, whose complex division rounds differently.
g++ -shared -fPIC -o "$OUT" $OBJS \
  -L$ROCM/lib -lamdhip64 -lrccl -lrt -Wl,-rpath,$ROCM/lib
echo "built $OUT"
