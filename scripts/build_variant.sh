#!/bin/bash
# A/B builds of libic_amd.so with extra -D flags: scripts/build_variant.sh <name> "<flags>" -> ab_libs/libic_amd_<name>.so
# (git-ignored through *.so; delete ab_libs/ when the experiment is over).  Used with
# ICAMD_ALLOW_LIB_OVERRIDE=1 ICAMD_LIB_PATH=$PWD/ab_libs/libic_amd_<name>.so (scripts/ab_bench.sh).
# The Makefile builds it -- one list of translation units, one set of flags: command-line variables override its assignments.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; FLAGS=$2
M=$R/image-compression_amd
O=$R/ab_libs/obj_$NAME
LIB=$R/ab_libs/libic_amd_$NAME.so
mkdir -p "$R/ab_libs"
HIPFLAGS=$(make -s -C "$M" --eval='print-hipflags: ; @echo $(HIPFLAGS)' print-hipflags)
make -j"${MAX_JOBS:-8}" -C "$M" OBJDIR="$O" LIB="$LIB" HIPFLAGS="$HIPFLAGS $FLAGS" "$LIB"
rm -rf "$O"
echo "built ab_libs/libic_amd_$NAME.so"
