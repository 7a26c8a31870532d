#!/bin/bash
# Register / scratch usage of the GFPush kernels for the current sources (EXTRA adds compiler flags).
cd "$(dirname "$0")/.."
python -c 'import sys, __graft_entry__ as g
g._run(g.hipcc_command(sys.argv[1], sys.argv[2:] + ["-c", "-Rpass-analysis=kernel-resource-usage"], units=("gfpush.hip",), link=()))' \
  /tmp/regs_$$.o $EXTRA 2>&1 | \
  grep -E "Function Name|VGPRs:|ScratchSize|VGPRs Spill|SGPRs Spill" | sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//' | paste - - - - - | grep gfpush_kernel
rm -f /tmp/regs_$$.o
