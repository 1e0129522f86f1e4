#!/bin/bash
# Build a second liblfd_hip.so with extra -D flags for same-session A/B timing:
#   tools/ab_build.sh scratch/alt/liblfd_hip_x.so -DSOME_VARIANT
#   python bench.py ...; LFD_HIP_LIB=$PWD/scratch/alt/liblfd_hip_x.so python bench.py ...
# (run-to-run differences between GPU boxes are 5-20 %: only numbers from one session are comparable)
# The source list, FLAGS and the per-file flags (FLAGS_<file>) are csrc/Makefile's own, expanded by make (the extra flags go in
# as its EXTRA), so that without extra flags this builds the shipped library.
set -e
OUT=$(realpath -m "$1"); shift
cd "$(dirname "$0")/../lfd-a-light-and-fast-detector_amd/csrc"
B=$(mktemp -d)
for f in $(sed -n 's/^SRCS *= *//p' Makefile | sed 's/\.hip//g'); do
  flags=$(make -s --no-print-directory --eval "ab-flags: ; @echo \$(FLAGS) \$(FLAGS_$f)" ab-flags EXTRA="$*")
  /opt/rocm/bin/hipcc $flags -c $f.hip -o $B/$f.o &
done
wait
mkdir -p "$(dirname "$OUT")"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" $B/*.o -Wl,-rpath,/opt/rocm/lib -Wl,-soname,liblfd_hip.so
rm -rf $B; ls -la "$OUT"
