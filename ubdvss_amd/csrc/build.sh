#!/bin/bash
# Builds libubd_hip.so (gfx950 only) in-tree next to the Python host package.
set -e
cd "$(dirname "$0")"
OUT=../libubd_hip.so
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function"
mkdir -p _obj
# fingerprint of the kernel sources, compiled into the library (ubd_build_id): the same digest bench.csrc_sha16() takes of the files
BUILD_ID=$(python3 - <<'PY'
import glob, hashlib, os
h = hashlib.sha256()
for f in sorted(glob.glob("*.hip") + glob.glob("*.h")):
    h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
print(h.hexdigest()[:16])
PY
)
UNITS="api forward fwd16 wino wino6 postprocess loss backward bwd32 bwd16 train comm raster resize warp photometric noise_alpha evaluate evaluate_pixels visualize epoch_stats multiscale"
pids=()
for f in $UNITS; do
  [ -f $f.hip ] || continue
  extra=""
  # OpenCV-exact float geometry: no FMA contraction in postprocess
  [ "$f" = "postprocess" ] && extra="-ffp-contract=off"
  # Pillow-exact float32 scan-line arithmetic: no FMA contraction
  [ "$f" = "raster" ] && extra="-ffp-contract=off"
  # the same scan-line arithmetic (raster_fill.h) and the fp32 denorm x * 127.5 + 127.5 as numpy rounds it: no FMA contraction
  [ "$f" = "visualize" ] && extra="-ffp-contract=off"
  # Pillow-exact double coefficient arithmetic of the bicubic resampler: no FMA contraction
  [ "$f" = "resize" ] && extra="-ffp-contract=off"
  # Pillow-exact double arithmetic of the generic transform and its bilinear filter: no FMA contraction
  [ "$f" = "warp" ] && extra="-ffp-contract=off"
  # fp32 Box-Muller of the noise mode, product and sum rounded separately as the numpy oracle does: no FMA contraction
  [ "$f" = "photometric" ] && extra="-ffp-contract=off"
  # exact fp64 cross products of the evaluation geometry (collinearity tests compare them with 0): no FMA contraction
  [ "$f" = "evaluate" ] && extra="-ffp-contract=off"
  # epoch sums acc + value * n with product and sum rounded separately, bit-equal to the host restatement: no FMA contraction
  [ "$f" = "epoch_stats" ] && extra="-ffp-contract=off"
  # the multi-scale mean: fp32 adds in level order and one IEEE division, bit-equal to the numpy oracle: no FMA contraction
  [ "$f" = "multiscale" ] && extra="-ffp-contract=off"
  # no SLP packing of adjacent fp32 adds into v_pk_add_f32: beside MFMAs the packed form issues slower than two scalar adds
  [ "$f" = "wino" ] && extra="$extra -fno-slp-vectorize"
  [ "$f" = "wino6" ] && extra="$extra -fno-slp-vectorize"
  stale=0
  for dep in $f.hip *.h ../../include/ubd.h; do [ "$dep" -nt _obj/$f.o ] && stale=1; done
  if [ "$f" = "api" ]; then   # carries the fingerprint of ALL kernel sources
    extra="$extra -DUBD_BUILD_ID=\"$BUILD_ID\""
    [ "$(cat _obj/api.build_id 2>/dev/null)" != "$BUILD_ID" ] && stale=1
  fi
  if [ ! -f _obj/$f.o ] || [ $stale = 1 ]; then
    # UBD_SAVE_TEMPS=1: the unit's gfx950 assembly beside its object, for tools/cmp_device_code.py.  A compile of its own:
    # -save-temps compiles the preprocessed text, where `#pragma unroll MACRO` (fwd16.hip) no longer finds its macro
    ( /opt/rocm/bin/hipcc $FLAGS $extra -c $f.hip -o _obj/$f.o
      [ -z "$UBD_SAVE_TEMPS" ] || /opt/rocm/bin/hipcc $FLAGS $extra -Wno-unused-command-line-argument --cuda-device-only -S $f.hip -o _obj/$f-hip-amdgcn-amd-amdhsa-gfx950.s ) &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
objs=""
for f in $UNITS; do [ -f _obj/$f.o ] && objs="$objs _obj/$f.o"; done
echo "$BUILD_ID" > _obj/api.build_id
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $objs -ldl
echo "built $OUT"
