#!/bin/bash
# probe builds of the whole library with the Sinkhorn translation units (SINKHORN_SRCS of csrc/Makefile) compiled under
# extra flags: tools/probe/libs_<name>.so
#   usage: build_sk_variants.sh name "-DSKR_ABL=4" [name "-DFLAG ..."] ...
# Built by csrc/Makefile itself, so a variant differs from the shipped library by its -D flags only (knobs: SKR_ABL,
# SKR_SAME_XCD_SCOPE, SK_CHUNK_MB, SKF_RPW_V, SKF_PF_V).  The other objects are the shipped ones, brought up to date first.
# The variants build in parallel; objects under tools/probe/build/<name>/.
set -e
cd "$(dirname "$0")"
out=$(pwd)
csrc=../../glue-factory_amd/csrc
make -s -C $csrc
others=$(cd $csrc && ls *.o | grep -v '^sinkhorn' | tr '\n' ' ')
while [ $# -gt 0 ]; do
  name=$1; flags=$2; shift 2
  make -s -C $csrc EXTRA="$flags" O="$out/build/$name/" LIB="$out/libs_$name.so" SRCS='$(SINKHORN_SRCS)' LDADD="$others" &
done
wait
