#!/bin/bash
# Builds tools/asan_user_wave.c with the host layer and the CPU restatement under AddressSanitizer + UndefinedBehaviorSanitizer (the flags of
# `make -C oracle asan`) and runs it: CPU only, a stand-alone program.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
HOST="$ROOT/hpgmg_amd/csrc/host"
OUT="$ROOT/tools/asan_user_wave"
${CC:-gcc} -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -fopenmp -ffp-contract=off -std=gnu99 -Wall \
  -Wno-unknown-pragmas -I"$ROOT/include" -I"$ROOT/oracle" -o "$OUT" \
  "$ROOT/oracle/operators_cpu.c" "$HOST/level.c" "$HOST/mg.c" "$HOST/solvers.c" "$HOST/driver.c" "$HOST/config.c" "$ROOT/tools/asan_user_wave.c" -lm
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 OMP_NUM_THREADS=2 "$OUT"
