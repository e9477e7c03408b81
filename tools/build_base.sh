#!/bin/bash
# Build libwtprune.so from a git revision (default HEAD) into tools/ab/libwtprune_base.so, for
# same-box A/B runs against the working tree (tools/gpu_ab.sh).  tools/ab/ travels to the GPU
# box (.so files are git-ignored, not gpurun-ignored).
set -e
REV=${1:-HEAD}
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
mkdir -p $T/w/csrc $T/include $R/tools/ab
for f in $(git -C $R ls-tree --name-only $REV wavelettransforms_amd/csrc/); do git -C $R show $REV:$f > $T/w/csrc/$(basename $f); done
for f in $(git -C $R ls-tree --name-only $REV include/); do git -C $R show $REV:$f > $T/include/$(basename $f); done
# every translation unit of that revision (its *.hip files), with the working tree's build line
python3 $R/wavelettransforms_amd/build.py --csrc $T/w/csrc --out $R/tools/ab/libwtprune_base.so
rm -rf $T
echo "built tools/ab/libwtprune_base.so from $REV"
