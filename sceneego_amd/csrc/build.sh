#!/bin/bash
# Builds libsceneego_hip.so for gfx950 (cross-compiles without a GPU).
# Usage: build.sh [--devtools] [extra hipcc flags]
#   --devtools  builds ../libsceneego_hip_dev.so instead (tools/ load it through SCENEEGO_HIP_LIB) with -DSE_DEVTOOLS: the A/B kernel selector (se_debug_set_variant)
#               and the cycle-stamp hooks used by tools/.  The production library is built WITHOUT it.
# Objects live in _obj/<key>/ where <key> hashes the compiler version and the flag line, so objects of another compiler or
# another flag set are never reused; inside a key a source is rebuilt when it or any header is newer than its object.
set -euo pipefail
cd "$(dirname "$0")"
OUT=../libsceneego_hip.so
DEV=""
if [ "${1:-}" = "--devtools" ]; then DEV="-DSE_DEVTOOLS"; OUT=../libsceneego_hip_dev.so; shift; fi
FLAGS="-O3 $DEV --offload-arch=gfx950 -fPIC -std=c++17 -Wall -Wno-unused-function $*"
KEY=$( (hipcc --version 2>/dev/null; echo "$FLAGS") | sha256sum | cut -c1-12)
OBJ=_obj/$KEY
mkdir -p "$OBJ"
pids=()
newer() {  # source $1 or a header newer than object $2
  [ ! -f "$2" ] || [ "$1" -nt "$2" ] && return 0
  for i in *.h ../../include/sceneego_hip.h; do [ "$i" -nt "$2" ] && return 0; done
  return 1
}
OBJS=()
for f in voxelize gather softargmax joint_stats joint_modes volume_filter volume_viterbi volume_sample skeleton_prior skeleton_pose skeleton_sample conv2d_1x1 conv2d_3x3 deconv2d_k4s2 conv3d conv3d_pack conv3d_direct conv3d_small conv3d_tail conv3d_tiled conv3d_wino conv3d_wino2d conv3d_wino44pp conv3d_wino67 conv3d_fft7 conv3d_bf16 conv3d_bf16_tiled conv3d_split exr_piz exr_zip jpeg jpeg_enc png_enc render render_volume scene_probe scene_constraint scene_field; do
  [ -f $f.hip ] || { echo "build.sh: source $f.hip is missing" >&2; exit 1; }
  OBJS+=($OBJ/$f.o)
  extra=""
  [ "$f" = voxelize ] && extra="-ffp-contract=off"
  [ "$f" = render ] && extra="-ffp-contract=off"      # float64 in the order the header states: the splat is tested bit for bit
  [ "$f" = scene_probe ] && extra="-ffp-contract=off" # likewise: every value it writes is tested bit for bit
  [ "$f" = render_volume ] && extra="-ffp-contract=off" # likewise: the walk is compared with its float64 model pixel for pixel
  [ "$f" = scene_constraint ] && extra="-ffp-contract=off" # likewise: the free mask is tested bit for bit
  [ "$f" = scene_field ] && extra="-ffp-contract=off" # likewise: the sites and the distance transform are tested bit for bit
  [ "$f" = joint_modes ] && extra="-ffp-contract=off"   # likewise: the window sums are compared with their float64 model bit for bit
  [ "$f" = volume_viterbi ] && extra="-ffp-contract=off" # likewise: every score and back-pointer is compared with its float32 model bit for bit
  [ "$f" = volume_sample ] && extra="-ffp-contract=off"  # likewise: every drawn voxel is compared with its float64 model bit for bit
  [ "$f" = skeleton_pose ] && extra="-ffp-contract=off"  # likewise: every message and pose voxel is compared with its float32 model bit for bit
  [ "$f" = skeleton_sample ] && extra="-ffp-contract=off" # likewise: every drawn pose voxel is compared with its float64 model bit for bit
  # no SLP packing of float32 arithmetic into v_pk_*_f32: packed VALU beside an MFMA stream is an anti-lever (see commit() there)
  [ "$f" = conv3d_wino2d ] && extra="-fno-slp-vectorize"
  [ "$f" = conv3d_wino44pp ] && extra="-fno-slp-vectorize -Wno-inline-asm"      # -Wno-inline-asm: the "m0" clobber of the LDS-DMA asm (reserved register)
  [ "$f" = conv3d_wino67 ] && extra="-Wno-inline-asm"
  if newer $f.hip $OBJ/$f.o; then
    hipcc $FLAGS $extra -c $f.hip -o $OBJ/$f.o &
    pids+=($!)
  fi
done
# the F(4,7) 7^3 kernel: one object per input layout (each takes minutes to compile: 390 unrolled MFMAs under sched_group_barrier)
for v in 0 1; do
  OBJS+=($OBJ/conv3d_wino47_$v.o)
  if newer conv3d_wino47.hip $OBJ/conv3d_wino47_$v.o; then
    hipcc $FLAGS -DSE_K7F_PLANAR=$v -c conv3d_wino47.hip -o $OBJ/conv3d_wino47_$v.o &
    pids+=($!)
  fi
done
rc=0
for p in "${pids[@]:-}"; do [ -n "$p" ] && { wait $p || rc=1; }; done
[ $rc -eq 0 ] || { echo "build.sh: compilation failed" >&2; exit 1; }
# the kernels with hand-counted vmcnt waits around inline-assembly LDS-DMAs: no VGPR spill, no scratch, M0 written only
# by the asm - or the build fails (check_codeobj.py says why).  Attribution builds (extra flags) may spill: checked, not fatal, there.
for f in conv3d_wino44pp conv3d_wino67; do
  crc=0; python3 check_codeobj.py $OBJ/$f.o || crc=$?
  if [ $crc -eq 2 ]; then echo "build.sh: the code-object check of $f.hip could not run (tools / metadata, see above; SE_SKIP_CODEOBJ_CHECK=1 skips it)" >&2; exit 1; fi
  if [ $crc -ne 0 ]; then
    if [ -z "$*" ]; then echo "build.sh: $f.hip violates the conditions its hand-counted waits rely on" >&2; exit 1; fi
    echo "build.sh: (extra flags given: continuing)" >&2
  fi
done
# explicit object list: a stale object of a removed / renamed source in the same key directory is never linked
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT "${OBJS[@]}"
# the hash of the sources this binary was built from (sceneego_amd/_lib.py: built_fingerprint / source_fingerprint): counter records
# under profiles/ carry it, bench.py prints their traffic figure only for the binary they were taken on
python3 - "$OUT" <<'PY'
import hashlib, os, sys
here = os.getcwd()
h = hashlib.sha256()
files = sorted(os.path.join(here, f) for f in os.listdir(here) if f.endswith((".hip", ".h", ".sh")))
files.append(os.path.join(here, "..", "..", "include", "sceneego_hip.h"))
for p in files:
    h.update(os.path.basename(p).encode() + b"\0")
    h.update(open(p, "rb").read())
open(os.path.splitext(sys.argv[1])[0] + ".srchash", "w").write(h.hexdigest()[:16] + "\n")
PY
echo "built $(realpath $OUT) (objects: $OBJ)"
