#!/bin/bash
# Build librtzig.so from a git revision into ab/<name>.so (for in-process A/B, tools/ab_libs.py).
#   tools/build_variant.sh <rev|WORKTREE> <name>
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=$1; NAME=$2
mkdir -p "$ROOT/ab"
if [ "$REV" = "WORKTREE" ]; then
  # EXTRA: extra compiler flags for ablation builds (e.g. -DRTZIG_RUV_TRIPS=2): the Makefile's own
  # object list and flags, on a copy of the sources so the in-tree build stays as it is
  if [ -n "$EXTRA" ]; then
    B=/tmp/rtab_$NAME; rm -rf "$B"; mkdir -p "$B/pkg/csrc" "$B/include"
    cp "$ROOT"/raytracing-with-zig_amd/csrc/{Makefile,*.hip,*.cpp,*.h,*.hpp} "$B/pkg/csrc/"
    cp "$ROOT/include/rt.h" "$B/include/"
    make -s -j"${JOBS:-8}" -C "$B/pkg/csrc" EXTRA="$EXTRA" ../librtzig.so >/dev/null
    cp "$B/pkg/librtzig.so" "$ROOT/ab/$NAME.so"
    echo "ab/$NAME.so"; exit 0
  fi
  make -s -C "$ROOT/raytracing-with-zig_amd/csrc" >/dev/null
  cp "$ROOT/raytracing-with-zig_amd/librtzig.so" "$ROOT/ab/$NAME.so"
else
  WT=/tmp/rtwt_$NAME
  rm -rf "$WT"; git -C "$ROOT" worktree prune
  git -C "$ROOT" worktree add -f "$WT" "$REV" >/dev/null 2>&1
  make -s -C "$WT/raytracing-with-zig_amd/csrc" >/dev/null
  cp "$WT/raytracing-with-zig_amd/librtzig.so" "$ROOT/ab/$NAME.so"
  git -C "$ROOT" worktree remove --force "$WT"
fi
echo "ab/$NAME.so"
