#!/bin/bash
# Build meep_nl_amd/libmnl.so for gfx950 (MI355X).  hipcc for the kernel files: mnl_kernels.hip
# (what a step launches), mnl_kernels_setup.hip, mnl_kernels_dft.hip, mnl_kernels_io.hip.  g++
# for the host side (see mnl_host.cpp header for why): mnl_host.cpp (C-ABI), mnl_setup.cpp
# (grid, PML, materials, quadrature), mnl_sources.cpp (sources, get_field), mnl_fused.cpp
# (fused-tile planning), mnl_tb.cpp (pairs of steps), mnl_step.cpp (the step loop, NaN guard),
# mnl_tune.cpp (the tuner), mnl_dft.cpp (DFT monitors), mnl_probe.cpp (field probes, dft_norm),
# mnl_ldos.cpp (LDOS spectra), mnl_modes.cpp (mode coefficients), mnl_io.cpp (checkpoints, slices, energy),
# mnl_stats.cpp (kernel statistics, the byte model), mnl_comm.cpp (RCCL / IPC).
# All compiles run at once (at most MNL_JOBS, default 16), then one link.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT=${MNL_OUT:-"$HERE/../libmnl.so"}
ROCM=${ROCM_PATH:-/opt/rocm}
TMP=${MNL_OBJ:-"$HERE/_obj"}
mkdir -p "$TMP"
ARCH=${MNL_ARCH:-gfx950}
JOBS=${MNL_JOBS:-16}
CXXF="$MNL_KFLAGS -O2 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-result -D__HIP_PLATFORM_AMD__ -I$ROCM/include"
KERNEL_SRCS="mnl_kernels mnl_kernels_setup mnl_kernels_dft mnl_kernels_io"
HOST_SRCS="mnl_host mnl_setup mnl_sources mnl_fused mnl_tb mnl_step mnl_tune mnl_dft mnl_probe mnl_ldos mnl_modes mnl_io mnl_stats mnl_comm"
OBJS=""
PIDS=""
# set -e does not see a background job fail: every job's status is taken from wait on its pid
throttle() {
  while [ "$(jobs -rp | wc -l)" -ge "$JOBS" ]; do wait -n || true; done
}
for s in $KERNEL_SRCS; do  # the long compiles first
  throttle
  hipcc --offload-arch=$ARCH $MNL_KFLAGS -O3 -ffp-contract=off -fPIC -std=c++17 -Wall \
    -c "$HERE/$s.hip" -o "$TMP/$s.o" &
  PIDS="$PIDS $!"
  OBJS="$OBJS $TMP/$s.o"
done
for s in $HOST_SRCS; do
  throttle
  g++ $CXXF -c "$HERE/$s.cpp" -o "$TMP/$s.o" &
  PIDS="$PIDS $!"
  OBJS="$OBJS $TMP/$s.o"
done
FAILED=0
for p in $PIDS; do
  wait "$p" || FAILED=1
done
if [ "$FAILED" -ne 0 ]; then
  echo "build.sh: a compile failed" >&2
  exit 1
fi
# Link with g++ so the host's complex arithmetic (__muldc3 / __divdc3 of
# std::complex) comes from libgcc as in the reference (and the oracle), not
# from clang's compiler-rt, whose complex division rounds differently.
g++ -shared -fPIC -o "$OUT" $OBJS \
  -L$ROCM/lib -lamdhip64 -lrccl -lrt -Wl,-rpath,$ROCM/lib
echo "built $OUT"
