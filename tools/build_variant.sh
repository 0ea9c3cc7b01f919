#!/bin/bash
# Build a variant of the library with extra compile flags: tools/build_variant.sh <name> "<flags>"
# -> blockcg_amd/_build/libblockcg_hip_<name>.so  (select with BCG_LIB or tools/ab_bench.sh)
# Through the Makefile (EXTRA = the flags, OUT = a directory of the variant's own), so the variant links every object
# of the default build and the flags reach every source file.
set -e
name=$1; flags=$2
cd "$(dirname "$0")/../blockcg_amd/csrc"
make -j16 OUT=../_build/variant_$name EXTRA="$flags" ../_build/variant_$name/libblockcg_hip.so
cp -f ../_build/variant_$name/libblockcg_hip.so ../_build/libblockcg_hip_$name.so
echo built $name
