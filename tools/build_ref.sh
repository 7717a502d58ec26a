#!/bin/bash
# Builds the engine library of a git revision as redrock_old_amd/librr_serdes_<name>.so (A/B timing
# against the working tree on the same GPU box; diagnostics only): the revision's csrc/ and
# include/ extracted under build/ref_<name>/src and built there by the revision's own Makefile
# (make -j$MAX_JOBS, 8 by default).  The revision's Makefile must know VARIANT=; one from before
# that builds librr_serdes.so instead, and the script stops with a message.
# (Knob variants of the working tree: make -C redrock_old_amd/csrc VARIANT=<name> EXTRA="-D...")
# usage: tools/build_ref.sh <rev> <name> ["-DEXTRA ..."]
set -e
rev=$1; name=$2; flags=$3
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root/build/ref_$name/src
rm -rf "$src"; mkdir -p "$src/redrock_old_amd/csrc" "$src/include"
for f in $(git -C "$root" ls-tree --name-only "$rev" redrock_old_amd/csrc/ include/); do
  git -C "$root" show "$rev:$f" > "$src/$f"
done
make -j"${MAX_JOBS:-8}" -C "$src/redrock_old_amd/csrc" VARIANT="$name" EXTRA="$flags" >/dev/null
lib=$src/redrock_old_amd/librr_serdes_$name.so
[ -f "$lib" ] || { echo "$rev's Makefile built no librr_serdes_$name.so (no VARIANT= support?)" >&2; exit 1; }
cp "$lib" "$root/redrock_old_amd/"
echo "built librr_serdes_$name.so from $rev"
