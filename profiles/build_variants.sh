#!/bin/bash
# Build libcloudsc2_hip variants with different -D switches into build/variants/ (git-ignored, but shipped to the GPU box) (dev tool).
#   bash profiles/build_variants.sh name1 "" name2 "-DCS2_AD_DIAG=1" ...
# Every file is compiled with the Makefile's own flags for it (cloudsc2_ad: -fno-slp-vectorize), plus the variant's switches.
set -e
SRC=gt4py_dwarf_p_cloudsc2_tl_ad_amd/csrc
OUT=$PWD/build/variants
mkdir -p $OUT
while [ $# -gt 1 ]; do
  name=$1; flags=$2; shift 2
  d=$(mktemp -d)
  for f in capi nl tl ad aux; do
    cmd=$(make --no-print-directory -n -B -C $SRC cloudsc2_$f.o | grep -- " -c ")
    (cd $SRC && ${cmd% -o *} $flags -o $d/$f.o) &
  done
  wait
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $d/*.o -o $OUT/lib_$name.so
  rm -rf $d
  echo built $OUT/lib_$name.so
done
