#!/bin/bash
# build a diagnostic variant of the library: tools/build_variant.sh NAME "-DFLAG ..."  -> tools/_diag/libdevit_NAME.so
# (csrc/build.sh with extra flags, objects in csrc/build_NAME; no check_objects.py gate: stamped builds may spill)
set -e
NAME=$1; EXTRA=$2
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "$ROOT/tools/_diag"
"$ROOT/devit_amd/csrc/build.sh" -n -f "$EXTRA" -b "$ROOT/devit_amd/csrc/build_$NAME" -o "$ROOT/tools/_diag/libdevit_$NAME.so"
echo built variant $NAME
