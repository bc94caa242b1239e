#!/bin/bash
# Host-only build of libfilm_hip, plain or with a sanitizer: every .cpp translation unit of csrc/ (planner, lane analysis, weight packer,
# tune cache, bundle reader, metrics entry point, executor bookkeeping - by wildcard, like the Makefile: a hand-kept list once left a unit
# out) by g++ + abort()ing stubs for what lives in the .hip units.  For plan-only handles (device = -1), no GPU.
#   tools/sanitize/build_host.sh none|address|thread|undefined [outdir=/tmp/film_san_<kind>[_extra]]    -> <outdir>/libfilm_hip_<kind>.so
#   none: no -fsanitize, a plain host library (tools/plan_digest.py).  FILM_EXTRA_FAMILIES=1 in the environment: the flavour that
#   can also select the opt-in kernel families (-DFILM_EXTRA_FAMILIES=1, as film_hip/build.py passes it).
# Run the CPU suites on it:
#   FILM_NO_TORCH=1 FILM_HIP_LIB=<so> LD_PRELOAD="$(g++ -print-file-name=lib{a,t,ub}san.so) $(g++ -print-file-name=libstdc++.so.6)" \
#     [ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 | TSAN_OPTIONS=halt_on_error=1] python -m pytest tests/test_host_threads_cpu.py ...
# (libstdc++ in LD_PRELOAD: the sanitizer's __cxa_throw interceptor must find the real one at process start; python does not link it)
set -e
KIND=${1:?none|address|thread|undefined}
R=$(cd "$(dirname "$0")/../.." && pwd)
EXTRA=
case "${FILM_EXTRA_FAMILIES:-0}" in ''|0) ;; *) EXTRA=1 ;; esac
OUT=${2:-/tmp/film_san_$KIND${EXTRA:+_extra}}
mkdir -p "$OUT"
SAN="-fsanitize=$KIND -fno-omit-frame-pointer"
[ "$KIND" = none ] && SAN=
FL="-std=c++17 -O1 -g $SAN -fPIC -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include ${EXTRA:+-DFILM_EXTRA_FAMILIES=1}"
pids=
objs=
for src in "$R"/frame-interpolation_amd/csrc/*.cpp "$R/tools/sanitize/launch_stubs.cpp"; do
  obj="$OUT/$(basename "$src" .cpp).o"
  g++ $FL -DFILM_SRC_ID="\"$KIND\"" -c "$src" -o "$obj" &
  pids="$pids $!"
  objs="$objs $obj"
done
for p in $pids; do wait "$p"; done
g++ -shared -fPIC $SAN -o "$OUT/libfilm_hip_$KIND.so" $objs -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
echo "$OUT/libfilm_hip_$KIND.so"
