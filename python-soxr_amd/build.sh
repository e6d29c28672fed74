#!/bin/bash
# Build libhipsoxr.so (HIP kernels + C ABI) for gfx950, in-tree.  hipcc cross-compiles without a GPU.
#
# Two flag sets:
#   * everything on the canonical-order path (plan design, exact-engine kernels) is compiled with
#     -ffp-contract=off: every fused multiply-add there is written explicitly, so that host design
#     and device arithmetic are bit-identical to the oracle's;
#   * the frequency-domain engine (fft.hip) is a 1e-6-class path: contraction is allowed, and the
#     SLP vectoriser is off — on gfx950 v_pk_add_f32 / v_pk_mul_f32 cost exactly two scalar issues
#     (4.3 against 2.3 cycles per wave-instruction and SIMD), and v_pk_fma_f32 does two FMAs in the
#     4.4 cycles that two v_fmac_f32 take 8.0 for (profiles/r06_ab_experiments.txt §6): packing pays
#     for FMAs alone, and "vectorised" complex arithmetic otherwise only adds register shuffles
#     (measured: 5412 -> 3261 VALU issue slots per thread for the 2560/2352-point block; hand-packed
#     FMAs, -DFFT_FORCE_PK, gained nothing on these kernels either: §10 there).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
SRC="$HERE/csrc"
# HIPSOXR_VARIANT=<name>: an experiment build (with HIPSOXR_EXTRA_FLAGS) into _variants/<name>/ beside the product
# library, so that several builds made here travel to the GPU box in one snapshot (tools/with_variant.sh swaps one in).
OUTDIR="$HERE/soxr_amd"
OBJ="$HERE/_obj"   # (not build/: that name belongs to setuptools when a wheel is built from this directory)
if [ -n "$HIPSOXR_VARIANT" ]; then OUTDIR="$HERE/_variants/$HIPSOXR_VARIANT"; OBJ="$HERE/_obj/$HIPSOXR_VARIANT"; mkdir -p "$OUTDIR"; fi
OUT="$OUTDIR/libhipsoxr.so"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function -I$HERE/../include"
mkdir -p "$OBJ"
"$HIPCC" $COMMON -ffp-contract=off ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/plan.cpp" -o "$OBJ/plan.o" & P1=$!
"$HIPCC" $COMMON -ffp-contract=off ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/engine.cpp" -o "$OBJ/engine.o" & P2=$!
"$HIPCC" $COMMON -ffp-contract=off ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/kernels.hip" -o "$OBJ/kernels.o" & P3=$!
"$HIPCC" $COMMON -ffp-contract=off ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/soxr_abi.cpp" -o "$OBJ/soxr_abi.o" & P5=$!
# (adjoint.hip: the transposed operator of the exact engine — explicit fma chains, like kernels.hip)
"$HIPCC" $COMMON -ffp-contract=off ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/adjoint.hip" -o "$OBJ/adjoint.o" & P14=$!
# (adjoint_fft.hip: the adjoint on the frequency-domain engine — host code alone: the transposed plan, handed to fft.hip)
"$HIPCC" $COMMON -ffp-contract=off ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/adjoint_fft.hip" -o "$OBJ/adjoint_fft.o" & P19=$!
# (adjoint_auto.hip: HIPSOXR_KERNEL_ADJOINT_AUTO — host code alone: the decision, handed to the three adjoint launchers)
"$HIPCC" $COMMON -ffp-contract=off ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/adjoint_auto.hip" -o "$OBJ/adjoint_auto.o" & P20=$!
# (half.hip: the widening / narrowing passes of float16 / bfloat16 jobs no fused kernel takes — copies, no arithmetic)
"$HIPCC" $COMMON -ffp-contract=off ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/half.hip" -o "$OBJ/half.o" & P15=$!
# The A/B and timing-experiment switches (device.h `Switches`, everything but four product names) are read from the
# environment only by a build with -DHIPSOXR_DEBUG_SWITCHES.  The reader lives in kernels.hip alone, so the debug build is
# that one object compiled a second time and linked with the product's other objects: _variants/dbg/libhipsoxr.so
# (tests/test_gpu_switches.py, tests/test_gpu_launch_forms.py and tools/*.sh load it through HIPSOXR_LIBRARY).
P8=""
if [ -z "$HIPSOXR_VARIANT" ]; then
  "$HIPCC" $COMMON -ffp-contract=off ${HIPSOXR_EXTRA_FLAGS} -DHIPSOXR_DEBUG_SWITCHES -c "$SRC/kernels.hip" -o "$OBJ/kernels_dbg.o" & P8=$!
fi
# (fft.hip in nine translation units: see "Three translation units" there; 3 and 4 hold the integer-sample kernels, 5 the
#  float32-only block sizes of one-round jobs, 6 and 7 the float16 / bfloat16 kernels, 8 those of the one-round block sizes)
FFTFLAGS="${HIPSOXR_FFTFLAGS:--ffp-contract=fast -fno-slp-vectorize}"
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -DFFT_PART=0 -c "$SRC/fft.hip" -o "$OBJ/fft.o" & P4=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -DFFT_PART=1 -c "$SRC/fft.hip" -o "$OBJ/fft1.o" & P6=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -DFFT_PART=2 -c "$SRC/fft.hip" -o "$OBJ/fft2.o" & P7=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -DFFT_PART=3 -c "$SRC/fft.hip" -o "$OBJ/fft3.o" & P11=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -DFFT_PART=4 -c "$SRC/fft.hip" -o "$OBJ/fft4.o" & P12=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -DFFT_PART=5 -c "$SRC/fft.hip" -o "$OBJ/fft5.o" & P13=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -DFFT_PART=6 -c "$SRC/fft.hip" -o "$OBJ/fft6.o" & P16=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -DFFT_PART=7 -c "$SRC/fft.hip" -o "$OBJ/fft7.o" & P17=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -DFFT_PART=8 -c "$SRC/fft.hip" -o "$OBJ/fft8.o" & P18=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/twostage.hip" -o "$OBJ/twostage.o" & P9=$!
"$HIPCC" $COMMON $FFTFLAGS ${HIPSOXR_EXTRA_FLAGS} -c "$SRC/fftwave.hip" -o "$OBJ/fftwave.o" & P10=$!
wait $P1; wait $P2; wait $P3; wait $P4; wait $P5; wait $P6; wait $P7; wait $P9; wait $P10; wait $P11; wait $P12; wait $P13; wait $P14; wait $P15; wait $P16; wait $P17; wait $P18; wait $P19; wait $P20   # set -e: any failed compile aborts here
OBJS="$OBJ/plan.o $OBJ/engine.o $OBJ/kernels.o $OBJ/fft.o $OBJ/fft1.o $OBJ/fft2.o $OBJ/fft3.o $OBJ/fft4.o $OBJ/fft5.o $OBJ/fft6.o $OBJ/fft7.o $OBJ/fft8.o $OBJ/half.o $OBJ/twostage.o $OBJ/fftwave.o $OBJ/adjoint.o $OBJ/adjoint_fft.o $OBJ/adjoint_auto.o $OBJ/soxr_abi.o"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC $OBJS -o "$OUT"
# The same engine under libsoxr's name: what `find_library(SOXR_LIBRARY NAMES soxr)` of the
# reference's USE_SYSTEM_LIBSOXR build picks up (reference CMakeLists.txt:83-93).
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -Wl,-soname,libsoxr.so.0 $OBJS -o "$OUTDIR/libsoxr.so.0"
ln -sf libsoxr.so.0 "$OUTDIR/libsoxr.so"
if [ -n "$P8" ]; then
  wait $P8
  mkdir -p "$HERE/_variants/dbg"
  "$HIPCC" --offload-arch=gfx950 -shared -fPIC ${OBJS/kernels.o/kernels_dbg.o} -o "$HERE/_variants/dbg/libhipsoxr.so"
fi
echo "built $OUT (+ libsoxr.so.0)"
