#!/bin/bash
# Is the gfx950 device code of csrc files the same as at a git revision?  CPU only (hipcc).
#   tools/isa_same.sh REV FILE... [-- EXTRA_FLAGS...]     e.g.  tools/isa_same.sh HEAD~1 fold.hip -- -DCRDT_STAMPS
# Compiles each FILE of go-crdt-playground_amd/csrc from REV and from the working tree with the
# product flags to device assembly and compares the two byte by byte.  -fuse-cuid=none: without it
# two compiles of one source differ in the random __hip_cuid_* symbol.
set -eu
cd "$(dirname "$0")/.."
rev=$1; shift
files=(); while [ $# -gt 0 ] && [ "$1" != -- ]; do files+=("$1"); shift; done
[ $# -gt 0 ] && shift
dir=go-crdt-playground_amd/csrc
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/old" "$tmp/new"
git archive "$rev" "$dir" include | tar -x -C "$tmp/old"
flags="--offload-arch=${ARCH:-gfx950} -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -x hip --cuda-device-only -fuse-cuid=none -S"
rc=0
for f in "${files[@]}"; do
  ${HIPCC:-/opt/rocm/bin/hipcc} $flags "$@" "$tmp/old/$dir/$f" -o "$tmp/old/$f.s" &
  ${HIPCC:-/opt/rocm/bin/hipcc} $flags "$@" "$dir/$f" -o "$tmp/new/$f.s"
  wait $!
  if cmp -s "$tmp/old/$f.s" "$tmp/new/$f.s"; then echo "$f: identical ($(wc -l < "$tmp/new/$f.s") lines)"
  else echo "$f: DIFFERS"; diff "$tmp/old/$f.s" "$tmp/new/$f.s" | head -20; rc=1; fi
done
exit $rc
