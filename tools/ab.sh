#!/bin/bash
# Same-box A/B of library variants (development aid): bash tools/ab.sh "<python args...>" var1 var2 ... ; variants are _ab/<var>.so
# (and _ab/<var>_dev.so where the development library has to match: it reads the product's structs)
# Alternates the variants ROUNDS times so that clock drift of the box shows up as spread, not as a difference.
CMD="$1"; shift
LIB=halo-accumulation_amd/libhalo_hip.so
DEV=halo-accumulation_amd/libhalo_hip_dev.so
cp $LIB /tmp/keep.so; cp $DEV /tmp/keep_dev.so
for r in 1 2 3; do
  for v in "$@"; do
    cp _ab/$v.so $LIB; [ -e _ab/${v}_dev.so ] && cp _ab/${v}_dev.so $DEV
    echo -n "$v: "; timeout -k 10 200 python $CMD 2>/dev/null | tail -n 1
  done
done
cp /tmp/keep.so $LIB; cp /tmp/keep_dev.so $DEV
