#!/bin/bash
# Timing-only variants of the LBS tile kernel: tools/libk2b_<name>.so (git-ignored; they travel to the GPU box).
# The diagnostics themselves live in tools/lbs_diag.h (hooks the shipped kernel leaves empty).
# The definitions also reach k2b_api_model.hip.  The other objects come from the Makefile (make print-objs).
# usage: tools/build_lbs_variants.sh name:"-DFLAGS" ...     e.g.  nostore:"-DK2B_TILE_DIAG=1" chunk4:"-DK2B_TILE_CHUNK=4"
set -e
cd "$(dirname "$0")/../keypoints2body_amd/csrc"
make -s -j8
DIAG="$(cd ../../tools && pwd)/lbs_diag.h"
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -ffp-contract=fast -fno-slp-vectorize -DK2B_LBS_DIAG_HEADER=\"$DIAG\""
for spec in "$@"; do
  name="${spec%%:*}"; defs="${spec#*:}"
  # (-DK2B_LBS_STREAM=0 is a switch of k2b_api_model.hip: that object is rebuilt with the same definitions)
  objs=""
  for o in $(make -s print-objs); do
    case $o in
      k2b_api_model.o|k2b_lbs_stream.o|k2b_lbs.o)
        /opt/rocm/bin/hipcc $FLAGS $defs -c ${o%.o}.hip -o /tmp/${o%.o}_$name.o
        o=/tmp/${o%.o}_$name.o ;;
    esac
    objs="$objs $o"
  done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/libk2b_$name.so $objs
  echo "built tools/libk2b_$name.so ($defs)"
done
