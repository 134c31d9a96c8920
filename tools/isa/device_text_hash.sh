#!/bin/bash
# sha256 of the gfx950 code object's .text and of its notes (registers, scratch, LDS per kernel) for each libbpp_hip.so named:
# a host-only change leaves both as they were (the hash of the whole code object moves either way).  No GPU needed.
set -e
LLVM=${LLVM_BIN:-/opt/rocm/lib/llvm/bin}
for LIB in "${@:-$(dirname "$0")/../../bulletproofs-plus_amd/libbpp_hip.so}"; do
  TMP=$(mktemp -d)
  "$LLVM/llvm-objcopy" --dump-section .hip_fatbin="$TMP/fat.bin" "$LIB"
  "$LLVM/clang-offload-bundler" --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$TMP/fat.bin" --output="$TMP/co.o" --unbundle
  "$LLVM/llvm-objcopy" --dump-section .text="$TMP/text.bin" "$TMP/co.o"
  echo "$LIB"
  echo "  .text  $(sha256sum < "$TMP/text.bin" | cut -d' ' -f1)"
  echo "  notes  $("$LLVM/llvm-readelf" --notes "$TMP/co.o" | sha256sum | cut -d' ' -f1)"
  rm -rf "$TMP"
done
