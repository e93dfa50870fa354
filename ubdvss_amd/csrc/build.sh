#!/bin/bash
# Builds libubd_hip.so (gfx950 only) in-tree next to the Python host package -- and, from the same unit table, the two
# kinds of experiment library the tools load from tools/_ab/ (git-ignored scratch, never loaded by the package):
#   build.sh                                   the product: ../libubd_hip.so, objects in _obj/
#   build.sh diag                              diagnostic build: every unit with -DUBD_STAMPS (stamps.h) in an object directory
#                                              of its own -> tools/_ab/libubd_hip_diag.so.  DIAG_FLAGS: further flags for
#                                              every unit; DIAG_OUT: another file name; DIAG_FILES: compile only these units
#                                              in this run (the others are linked as an earlier run left them)
#   build.sh variant <name> <unit> <flags...>  the product objects with ONE unit rebuilt under extra flags -> tools/_ab/<name>.so
# Every mode compiles a unit only when its object is older than a source or was built with other flags, and compiles the
# same fingerprint into api (ubd_build_id).
set -e
cd "$(dirname "$0")"
MODE=${1:-product}
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function"
AB=../../tools/_ab
# fingerprint of the kernel sources, compiled into the library (ubd_build_id): the same digest bench.csrc_sha16() takes of the files
BUILD_ID=$(python3 - <<'PY'
import glob, hashlib, os
h = hashlib.sha256()
for f in sorted(glob.glob("*.hip") + glob.glob("*.h")):
    h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
print(h.hexdigest()[:16])
PY
)
UNITS="api forward fwd16 wino wino6 postprocess loss backward bwd32 bwd16 train comm raster resize warp extract decode decode_text decode_width decode_postal decode_matrix photometric noise_alpha evaluate evaluate_pixels visualize epoch_stats multiscale score"
unit_flags() {   # the flags a unit needs beside $FLAGS, in every mode
  case $1 in
    api) echo "-DUBD_BUILD_ID=\"$BUILD_ID\"" ;;           # carries the fingerprint of ALL kernel sources
    postprocess) echo "-ffp-contract=off" ;;              # OpenCV-exact float geometry: no FMA contraction in postprocess
    raster) echo "-ffp-contract=off" ;;                   # Pillow-exact float32 scan-line arithmetic: no FMA contraction
    visualize) echo "-ffp-contract=off" ;;                # the same scan-line arithmetic (raster_fill.h) and the fp32 denorm x * 127.5 + 127.5 as numpy rounds it: no FMA contraction
    resize) echo "-ffp-contract=off" ;;                   # Pillow-exact double coefficient arithmetic of the bicubic resampler: no FMA contraction
    warp) echo "-ffp-contract=off" ;;                     # Pillow-exact double arithmetic of the generic transform and its bilinear filter: no FMA contraction
    extract) echo "-ffp-contract=off" ;;                  # Pillow-exact double arithmetic of the QUAD transform and the bilinear filter it shares with warp: no FMA contraction
    photometric) echo "-ffp-contract=off" ;;              # fp32 Box-Muller of the noise mode, product and sum rounded separately as the numpy oracle does: no FMA contraction
    evaluate) echo "-ffp-contract=off" ;;                 # exact fp64 cross products of the evaluation geometry (collinearity tests compare them with 0): no FMA contraction
    epoch_stats) echo "-ffp-contract=off" ;;              # epoch sums acc + value * n with product and sum rounded separately, bit-equal to the host restatement: no FMA contraction
    multiscale) echo "-ffp-contract=off" ;;               # the multi-scale mean: fp32 adds in level order and one IEEE division, bit-equal to the numpy oracle: no FMA contraction
    score) echo "-ffp-contract=off" ;;                    # the scan-line arithmetic of raster_fill.h and the fixed fp32 sigmoid of the object scores (add, divide, product rounded separately): no FMA contraction
    wino|wino6) echo "-fno-slp-vectorize" ;;              # no SLP packing of adjacent fp32 adds into v_pk_add_f32: beside MFMAs the packed form issues slower than two scalar adds
  esac
}
pids=()
compile() {   # <unit> <object path without .o> <mode flags>: in the background, unless the object is up to date
  local f=$1 o=$2 flags="$FLAGS $(unit_flags $1) $3" stale=0
  for dep in $f.hip *.h ../../include/ubd.h; do [ "$dep" -nt $o.o ] && stale=1; done
  [ "$(cat $o.flags 2>/dev/null)" != "$flags" ] && stale=1
  [ $stale = 0 ] && return 0
  # UBD_SAVE_TEMPS=1: the unit's gfx950 assembly beside its object, for tools/cmp_device_code.py.  A compile of its own:
  # -save-temps compiles the preprocessed text, where `#pragma unroll MACRO` (fwd16.hip) no longer finds its macro
  ( rm -f $o.flags
    /opt/rocm/bin/hipcc $flags -c $f.hip -o $o.o
    [ -z "$UBD_SAVE_TEMPS" ] || /opt/rocm/bin/hipcc $flags -Wno-unused-command-line-argument --cuda-device-only -S $f.hip -o $(dirname $o)/$f-hip-amdgcn-amd-amdhsa-gfx950.s
    echo "$flags" > $o.flags ) &
  pids+=($!)
}
OBJ=_obj
mkdir -p $OBJ
case $MODE in
  product) OUT=../libubd_hip.so
    for f in $UNITS; do compile $f $OBJ/$f ""; done ;;
  diag) OBJ=$AB/_obj_diag; OUT=$AB/${DIAG_OUT:-libubd_hip_diag.so}
    mkdir -p $OBJ
    for f in ${DIAG_FILES:-$UNITS}; do compile $f $OBJ/$f "-DUBD_STAMPS $DIAG_FLAGS"; done ;;
  variant) NAME=$2; VUNIT=$3; shift 3; OUT=$AB/$NAME.so
    case " $UNITS " in *" $VUNIT "*) ;; *) echo "build.sh variant: no unit named $VUNIT" >&2; exit 2 ;; esac
    mkdir -p $AB/_obj_var
    for f in $UNITS; do [ $f = $VUNIT ] || compile $f $OBJ/$f ""; done
    compile $VUNIT $AB/_obj_var/$NAME "$*" ;;
  *) echo "build.sh: unknown mode $MODE (product, diag, variant)" >&2; exit 2 ;;
esac
for p in "${pids[@]}"; do wait $p; done
objs=""
for f in $UNITS; do
  if [ "$MODE" = variant ] && [ $f = $VUNIT ]; then objs="$objs $AB/_obj_var/$NAME.o"; else objs="$objs $OBJ/$f.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $objs -ldl
echo "built $OUT"
