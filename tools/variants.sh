#!/bin/bash
# Build variants of libhakai_hip.so with extra compile definitions for hakai_element.hip, for A/B
# timing in one process tree (HAKAI_LIB=<path> selects the library, hakai/_abi.py):
#   tools/variants.sh name1 "-DFOO" name2 "-DBAR -DBAZ" ...   -> hakai-fem_amd/lib/variants/<name>.so
# The flags and the objects are the Makefile's (its `variant` target): the element kernels compiled
# with the definitions added, linked with every other object of the product build.
set -e
cd "$(dirname "$0")/../hakai-fem_amd"
make -s -j8 >/dev/null
pids=()
while [ $# -ge 2 ]; do
  make -s variant NAME="$1" DEFS="$2" & pids+=($!)
  shift 2
done
for p in "${pids[@]}"; do wait "$p"; done
ls -la lib/variants
