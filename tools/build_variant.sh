#!/bin/bash
# A/B builds of ONE source file with extra -D flags, linked against the stock objects of the other files (run `python -m tubedetr_amd.build` first):
#   tools/build_variant.sh <tag> <file.hip> "-DFOO=1 ..."  ->  tubedetr_amd/lib/libtubedetr_hip_<tag>.so   (select with TD_HIP_LIB=<path>)
# The source list and the compile flags are those of tubedetr_amd/build.py (SOURCES, FLAGS).
set -e
cd "$(dirname "$0")/.."
tag=$1; src=$2; defs=$3
L=tubedetr_amd/lib
base=${src%.*}
flags=$(python -c "from tubedetr_amd.build import FLAGS; print(' '.join(FLAGS))")
names=$(python -c "import os; from tubedetr_amd.build import SOURCES; print(' '.join(os.path.splitext(s)[0] for s in SOURCES))")
case "$src" in *.cpp) lang="-x hip" ;; *) lang="" ;; esac
/opt/rocm/bin/hipcc $flags $lang $defs -c tubedetr_amd/csrc/$src -o $L/${base}_$tag.o
objs=""
for o in $names; do
  if [ "$o" == "$base" ]; then objs="$objs $L/${base}_$tag.o"; else objs="$objs $L/$o.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $L/libtubedetr_hip_$tag.so $objs
echo $L/libtubedetr_hip_$tag.so
