#!/bin/bash
# (container side) builds libsbwtgpu of an earlier commit into sbwt_amd/lib/<name>.so, for same-box A/B runs with
# tools/ab_libs5.sh (the .so travels to the GPU box with the snapshot; it is git-ignored):
#   tools/build_rev_lib.sh <git revision> <name>          e.g.  tools/build_rev_lib.sh 888bb2b lib_r4
set -eu
REV=$1; NAME=$2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=$(mktemp -d /tmp/sbwt_rev_XXXX)
git -C "$ROOT" worktree add -f "$W" "$REV" > /dev/null
# (compiler, flags and sources are those of the revision's own build driver, read as a file: its package is not imported)
CMD=$(cd "$W" && python -c "import runpy, sys; print(' '.join(runpy.run_path('sbwt_amd/build.py')['_hipcc_cmd'](sys.argv[1])))" "$ROOT/sbwt_amd/lib/$NAME.so")
$CMD
git -C "$ROOT" worktree remove --force "$W"
echo "built $ROOT/sbwt_amd/lib/$NAME.so from $REV"
