#!/bin/bash
# Register / scratch usage of the GFPush kernels for the current sources (EXTRA adds compiler flags).
# UNIT=mlp_infer.hip KERNEL=mlp_infer tools/regs.sh reports another translation unit's kernels.
cd "$(dirname "$0")/.."
python -c 'import sys, __graft_entry__ as g
g._run(g.hipcc_command(sys.argv[1], sys.argv[3:] + ["-c", "-Rpass-analysis=kernel-resource-usage"], units=(sys.argv[2],), link=()))' \
  /tmp/regs_$$.o "${UNIT:-gfpush.hip}" $EXTRA 2>&1 | \
  grep -E "Function Name|VGPRs:|ScratchSize|VGPRs Spill|SGPRs Spill" | sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//' | paste - - - - - | grep "${KERNEL:-gfpush_kernel}"
rm -f /tmp/regs_$$.o
