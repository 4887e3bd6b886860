#!/bin/bash
# Developer tool, no GPU: is the device code of a sweep unit the same text as at another revision?
#
#   tools/asm_equal.sh <parent-rev> <unit>...        unit = psa_rk4_single_pump_f32 | psa_rk4_comb_f32 | psa_rk4_f32 | ...
#
# Builds the device assembly of csrc/<unit>.hip twice, from the working tree and from <parent-rev> (git archive into a
# scratch directory), with the flags csrc/Makefile gives the sweep units, drops what names the build and not the code
# (comment lines, .file / .ident / .loc, the __hip_cuid_* symbol) and compares the rest byte for byte.  align_encodings.py and
# the assembler are deterministic on that text, so "identical" here means the same code object.  Prints one line per unit and
# the per-kernel register figures where they differ; the exit status is the number of units that differ.
# WORK=<dir> keeps the scratch directory (and reuses the parent's assembly found there); EXTRA="-D..." reaches both builds.
set -u
[ $# -ge 2 ] || { echo "usage: $0 <parent-rev> <unit>..." >&2; exit 64; }
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PKG=psa-simulation-ode-rk-mvp-dispersion_amd
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${ARCH:-gfx950}
REV=$1; shift
if [ -n "${WORK:-}" ]; then mkdir -p "$WORK"; else WORK=$(mktemp -d); trap 'rm -rf "$WORK"' EXIT; fi
SHA=$(git -C "$ROOT" rev-parse --short "$REV") || exit 64
P=$WORK/parent-$SHA
if [ ! -d "$P/$PKG/csrc" ]; then
    mkdir -p "$P" && git -C "$ROOT" archive "$REV" include "$PKG/csrc" | tar -x -C "$P" || exit 64
fi

device_asm() {   # <tree> <unit> <out>
    ( cd "$1/$PKG/csrc" && $HIPCC -O3 -std=c++17 --offload-arch=$ARCH -I../../include -I. -Wall -Wno-unused-function -Wno-unused-command-line-argument ${EXTRA:-} \
        -mllvm -amdgpu-sched-strategy=max-ilp -mllvm -align-all-blocks=3 -S --cuda-device-only "$2.hip" -o "$3.raw" ) || return 1
    grep -v -E '^[[:space:]]*;|^[[:space:]]*\.(file|ident|loc)[[:space:]]|__hip_cuid_' "$3.raw" > "$3"
}
figures() {      # per kernel: name, VGPRs, scratch bytes, occupancy as the compiler reports them
    awk '/^[A-Za-z_][A-Za-z0-9_]*:/ {name=$1}
         /^; NumVgprs:/ {v=$3} /^; ScratchSize:/ {s=$3} /^; Occupancy:/ {print name, "vgpr", v, "scratch", s, "waves/SIMD", $3}' "$1"
}

differ=0
for U in "$@"; do
    [ -s "$P/$U.s" ] || device_asm "$P" "$U" "$P/$U.s" || { echo "$U: parent build failed"; differ=$((differ + 1)); continue; }
    device_asm "$ROOT" "$U" "$WORK/$U.s" || { echo "$U: build failed"; differ=$((differ + 1)); continue; }
    if cmp -s "$P/$U.s" "$WORK/$U.s"; then
        echo "$U: identical to $SHA ($(wc -l < "$WORK/$U.s") lines of device code)"
    else
        differ=$((differ + 1))
        echo "$U: DIFFERS from $SHA: $(diff "$P/$U.s" "$WORK/$U.s" | grep -c '^[<>]') differing lines"
        figures "$P/$U.s.raw" > "$WORK/$U.parent.fig"; figures "$WORK/$U.s.raw" > "$WORK/$U.head.fig"
        diff "$WORK/$U.parent.fig" "$WORK/$U.head.fig" | grep '^[<>]' | sed 's/^</  parent:/; s/^>/  head:  /'
    fi
done
exit $differ
