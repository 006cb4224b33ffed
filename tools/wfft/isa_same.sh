#!/bin/bash
# Do two revisions compile csrc/wfft.hip to the same gfx950 device code?  No GPU needed.
# usage: tools/wfft/isa_same.sh REV_A REV_B      (run inside the repository)
# Exports csrc/ and include/ of each revision, compiles wfft.hip device-only to assembly with the
# Makefile's flags, drops the lines that carry __hip_cuid_<hash> (a hash of the source text) and
# compares the rest byte by byte: prints both sha256 sums and IDENTICAL, or the kernel in which the
# first difference stands.  Exit status 0 only when identical.
set -euo pipefail
[ $# -eq 2 ] || { echo "usage: $0 REV_A REV_B" >&2; exit 2; }
ROOT=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CSRC=transport_analysis_amd/csrc
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
assemble() {  # revision, tag
    mkdir "$TMP/$2"
    git -C "$ROOT" archive "$1" $CSRC include | tar -x -C "$TMP/$2"
    FLAGS=$(sed -n 's/^CXXFLAGS ?= //p' "$TMP/$2/$CSRC/Makefile" | sed 's/\$(ARCH)/gfx950/')
    (cd "$TMP/$2/$CSRC" && $HIPCC $FLAGS -w --cuda-device-only -S wfft.hip -o - | grep -v __hip_cuid_ > "$TMP/$2.s")
}
assemble "$1" a &
assemble "$2" b &
wait %1
wait %2
echo "$(sha256sum < "$TMP/a.s" | cut -d' ' -f1)  $1  ($(wc -l < "$TMP/a.s") lines)"
echo "$(sha256sum < "$TMP/b.s" | cut -d' ' -f1)  $2  ($(wc -l < "$TMP/b.s") lines)"
if cmp -s "$TMP/a.s" "$TMP/b.s"; then echo IDENTICAL; exit 0; fi
LINE=$(cmp "$TMP/a.s" "$TMP/b.s" | sed 's/.* line //')
echo "DIFFERENT: first at line $LINE, in $(head -n "$LINE" "$TMP/a.s" | grep -E '^[A-Za-z_][A-Za-z0-9_$.]*:' | tail -1)"
exit 1
