#!/bin/bash
# Host-side AddressSanitizer + UBSan build of psa_capi.hip (the kernels' objects are the ordinary build's: run `make` in csrc
# first) and one run of tests/c/chain_args_client.c against it: every chain entry point with invalid arguments and with
# n_points = 0.  Every call ends in validation, so this needs no GPU.  Usage: bash tools/chain_host_sanitize.sh
set -euo pipefail
cd "$(dirname "$0")/.."
SRC=psa-simulation-ode-rk-mvp-dispersion_amd/csrc
OUT=${TMPDIR:-/tmp}/psa_chain_san
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$OUT"
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer"
OBJS=$(ls $SRC/*.o | grep -v psa_capi.o)
$HIPCC -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Iinclude -I$SRC $SAN -c $SRC/psa_capi.hip -o $OUT/psa_capi.o
$HIPCC -shared -fPIC --offload-arch=gfx950 $SAN -o $OUT/libpsa_hip.so $OBJS $OUT/psa_capi.o
$HIPCC -x c -std=c99 -Wall -Iinclude $SAN tests/c/chain_args_client.c -o $OUT/chain_args_client -L$OUT -lpsa_hip -Wl,-rpath,$OUT -lm
export ASAN_OPTIONS=detect_leaks=0:protect_shadow_gap=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1
echo "== host ASan + UBSan build of psa_capi.hip: the chain entry points' argument rules"
$OUT/chain_args_client
echo "== host sanitizers: no report"
