#!/bin/bash
# probe builds of the attention translation units (ATTN_SRCS of csrc/Makefile): tools/probe/libv_<name>.so
#   usage: build_attn_variants.sh name "-DFLAG ..." [name "-DFLAG ..."] ...
# Built by csrc/Makefile itself, so a variant differs from the shipped library by its -D flags only.  One compile at a
# time per variant, the variants in parallel; objects under tools/probe/build/<name>/.
set -e
cd "$(dirname "$0")"
out=$(pwd)
while [ $# -gt 0 ]; do
  name=$1; flags=$2; shift 2
  make -s -C ../../glue-factory_amd/csrc EXTRA="$flags" O="$out/build/$name/" LIB="$out/libv_$name.so" SRCS='$(ATTN_SRCS)' &
done
wait
