#!/bin/bash
# Compiles every .hip file of a tree to gfx950 device assembly with the Makefile's own HIPFLAGS and writes the
# normalised .s files plus their sha256 sums (SUMS) to a directory. Two trees generate the same device code
# exactly when their SUMS files are equal:
#   tools/device_asm_sums.sh <commit | directory with vision.cpp_amd/csrc and include> <outdir>
#   tools/device_asm_sums.sh HEAD /tmp/parent && tools/device_asm_sums.sh . /tmp/branch && diff /tmp/parent/SUMS /tmp/branch/SUMS
# Normalised: lines with the __hip_cuid_<hash> symbol are dropped (it hashes the source text; four lines per file).
set -e
tree=$1; out=$2
root=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$out"; out=$(cd "$out" && pwd)
tmp=
if [ ! -d "$tree" ]; then
    tmp=$(mktemp -d)
    git -C "$root" archive "$tree" vision.cpp_amd/csrc include | tar -x -C "$tmp"
    tree=$tmp
fi
csrc=$(cd "$tree/vision.cpp_amd/csrc" && pwd)
cc=$(make -s -C "$csrc" --eval 'print-cc: ; @echo $(HIPCC) $(HIPFLAGS)' print-cc)
cd "$csrc"
printf '%s\n' *.hip | xargs -P "${JOBS:-8}" -I{} bash -o pipefail -c \
    "$cc --cuda-device-only -S {} -o - | grep -v __hip_cuid_ > '$out'/\$(basename {} .hip).s"
(cd "$out" && sha256sum *.s > SUMS && cat SUMS)
[ -z "$tmp" ] || rm -rf "$tmp"
