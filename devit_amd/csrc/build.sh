#!/bin/bash
# Build libdevit_hip.so for gfx950 (cross-compiles without a GPU).
# Usage: build.sh [-f "extra hipcc flags"] [-b build_dir] [-o out.so] [-n] [outdir]
#        build.sh -g DIR      only generate the asm K loops (*_kloop.inc) into DIR
#   -f  extra compiler flags (a diagnostic variant: tools/build_variant.sh); give such a build its own -b and -o
#   -b  directory of the objects (default: csrc/build)
#   -o  the library to link (default: outdir/libdevit_hip.so, outdir = devit_amd/)
#   -n  skip the check_objects.py gate (stamped diagnostic builds may spill)
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
TOOLS="$HERE/../../tools"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
EXTRA="" BUILD="$HERE/build" LIB="" GATE=1 GEN_ONLY=""
while getopts "f:b:o:ng:" opt; do
  case $opt in
    f) EXTRA="$OPTARG" ;;
    b) BUILD="$OPTARG" ;;
    o) LIB="$OPTARG" ;;
    n) GATE=0 ;;
    g) GEN_ONLY="$OPTARG" ;;
    *) exit 2 ;;
  esac
done
shift $((OPTIND - 1))
LIB="${LIB:-${1:-$HERE/..}/libdevit_hip.so}"
case "$BUILD" in /*) ;; *) BUILD="$PWD/$BUILD" ;; esac
case "$LIB" in /*) ;; *) LIB="$PWD/$LIB" ;; esac
# -fvisibility=hidden: the library exports the C ABI of include/devit_hip.h (DEVIT_API) and nothing else
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -munsafe-fp-atomics -Wno-unused-result"
# one object per unit, the slowest to compile first (all are started at once)
UNITS="gemm_tile256 gemm_tile128 gemmfr gemm4 wgradfr attention elementwise optim dropout losses relation qkvce hid layernorm hsic gemm sgemm encoder shrink augment comm det api"

# The asm K loops of the four-wave and full-row GEMM kernels are GENERATED (tools/gen_gemm4.py, tools/gen_gemmfr.py document the register
# plans): made here, not committed (2 MB of text); tests/test_abi.py regenerates them and compares with what the library was built from.
# The generators' experiment switches (GEMM4_*, GEMMFR_* in the environment) are for their own command line: stripped here, every one.
generate() {   # generate gemm4|gemmfr DIR
  ( for v in $(compgen -e | grep -E '^(GEMM4|GEMMFR)_' || true); do unset "$v"; done
    python3 "$TOOLS/gen_$1.py" "$2/$1_kloop.inc" > /dev/null )
}
if [ -n "$GEN_ONLY" ]; then
  mkdir -p "$GEN_ONLY"
  for g in gemm4 gemmfr; do generate $g "$GEN_ONLY"; done
  exit 0
fi
for g in gemm4 gemmfr; do
  if [ ! -f "$HERE/${g}_kloop.inc" ] || [ "$TOOLS/gen_${g}.py" -nt "$HERE/${g}_kloop.inc" ]; then generate $g "$HERE"; fi
done

# a unit is rebuilt when its source, this script, any header or generated include of csrc/, or the public header is newer than its object,
# or when the build directory last held objects made with other flags ($BUILD/flags: tools/build_variant.sh NAME called again with another -D)
mkdir -p "$BUILD"
if [ ! -f "$BUILD/flags" ] || [ "$(cat "$BUILD/flags")" != "$FLAGS $EXTRA" ]; then echo "$FLAGS $EXTRA" > "$BUILD/flags"; fi
pids=()
for f in $UNITS; do
  stale=0
  for dep in "$BUILD/flags" "$HERE/$f.hip" "$HERE/build.sh" "$HERE"/*.h "$HERE"/*.inc "$HERE/../../include/devit_hip.h"; do
    if [ ! -f "$BUILD/$f.o" ] || [ "$dep" -nt "$BUILD/$f.o" ]; then stale=1; break; fi
  done
  if [ $stale = 1 ]; then
    $HIPCC $FLAGS $EXTRA -c "$HERE/$f.hip" -o "$BUILD/$f.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
# Build gates over the gfx950 code objects (check_objects.py: no spills / scratch anywhere; nothing but MFMAs writes AGPRs in the kernels whose
# asm K loops leave their accumulators there).  A missing LLVM tool fails the build: a gate that cannot run is not a pass.
if [ $GATE = 1 ]; then python3 "$HERE/check_objects.py" "$BUILD" $UNITS; fi
( cd "$BUILD" && $HIPCC --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden -o "$LIB" $(for f in $UNITS; do echo $f.o; done) -ldl )
echo "built $LIB"
