#!/bin/bash
# SHA-256 of each translation unit's gfx950 device assembly, compiled with the library's flags, less what follows the source
# text and not the code (comment lines, .file, .ident, the __hip_cuid_ symbol).  Equal hashes = equal device code.
# SRC=<dir> hashes another revision's sources: git archive REV grand_plus_amd/csrc | tar -x -C <tmp>, SRC=<tmp>/grand_plus_amd/csrc
# (they compile against THIS tree's include/; for a revision whose public headers differ, archive the whole tree and run its own copy)
cd "$(dirname "$0")/.."
for u in $(python -c 'import __graft_entry__ as g; print(*g.LIB_UNITS)'); do
  python -c 'import sys, subprocess, __graft_entry__ as g
r = subprocess.run(g.hipcc_command(sys.argv[1], ["--cuda-device-only", "-S"], src_dir=sys.argv[2], units=(sys.argv[3],), link=()), capture_output=True, text=True)
sys.exit(r.stderr if r.returncode else 0)' \
    /tmp/asm_$$.s "$(realpath "${SRC:-grand_plus_amd/csrc}")" "$u" || exit 1
  echo "$(grep -vE '^\s*(;|//|\.file|\.ident)|__hip_cuid_' /tmp/asm_$$.s | sha256sum | cut -c1-64)  $u"
done
rm -f /tmp/asm_$$.s
