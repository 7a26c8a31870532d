#!/bin/bash
# One more build of the product library under another name, for A/B runs on ONE box (tools/ab_libs.sh):
#   tools/build_variant.sh <name> [extra hipcc flags, e.g. -DGP_SK_TIMING]     -> grand_plus_amd/libgrandplus_<name>.so
# With GP_SRC=<dir> the sources come from that directory (e.g. an older revision exported with `git show`).
# Flags and translation units are those of __graft_entry__.hipcc_command.  Run from the repository root.
NAME=$1; shift
python -c 'import os, sys, __graft_entry__ as g
g._run(g.hipcc_command(os.path.join(g.PKG, "libgrandplus_%s.so" % sys.argv[1]), sys.argv[2:],
                       os.path.abspath(os.environ.get("GP_SRC") or g.CSRC)))' "$NAME" "$@"
