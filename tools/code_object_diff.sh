#!/bin/bash
# Is the device code of this tree the device code of another checkout, byte for byte?  Every device source of the Makefile's DEV_SRC and every shard of
# nrs_render_rows.hip is compiled to its bare code object (--cuda-device-only -c) in both trees with THIS tree's Makefile flags, and the two objects are compared.
# One line per object: name, size, identical | DIFFERS; exit status 1 on any difference.  For move-only refactors of the headers (profiles/header_split.md).
# usage: tools/code_object_diff.sh <parent-checkout>
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
PARENT="$(cd "${1:?usage: tools/code_object_diff.sh <parent-checkout>}" && pwd)"
CSRC=nerfshop_amd/csrc
ask() { make -s -C "$ROOT/$CSRC" --eval "print-it: ; @echo \$($1)" print-it; }
COMPILE="$(ask COMPILE)"; SHARDS="$(ask SHARDS)"; ROW_SHARDS="$(ask ROW_SHARDS)"
TMP=$(mktemp -d /tmp/code_object_diff.XXXXXX)
trap 'rm -rf "$TMP"' EXIT
mkdir "$TMP/new" "$TMP/old"
# one line per compile: tree, output, source and its defines
for side in new old; do
	tree="$ROOT"; [ $side == old ] && tree="$PARENT"
	for src in $(ask DEV_SRC); do echo "$tree/$CSRC $TMP/$side/${src%.hip} $src"; done
	for k in $SHARDS; do echo "$tree/$CSRC $TMP/$side/nrs_render_rows_$k nrs_render_rows.hip -DNRS_ROW_SHARDS=$ROW_SHARDS -DNRS_ROW_SHARD=$k"; done
done > "$TMP/jobs"
JOBS=$(nproc); [ "$JOBS" -gt 16 ] && JOBS=16
# (-fuse-cuid=none: hipcc otherwise names a symbol of every code object after a hash of the source's PATH, and two checkouts never share one)
xargs -P "$JOBS" -L 1 sh -c 'cd "$0" && out="$1" && shift && exec '"$COMPILE"' --cuda-device-only -fuse-cuid=none -c "$@" -o "$out"' < "$TMP/jobs"
status=0
for new in "$TMP"/new/*; do
	name=$(basename "$new")
	if cmp -s "$new" "$TMP/old/$name"; then verdict=identical; else verdict=DIFFERS; status=1; fi
	printf '%-26s %9d B  %s\n' "$name" "$(stat -c %s "$new")" "$verdict"
done
exit $status
