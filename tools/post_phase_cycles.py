"""Per-batch cycles of the post work's phases from a batch dump (SHDPE_DEBUG=1
SHDPE_DUMP_BATCHES=<file>, the format tools/batch_cost.py reads): the
predecessor pass (dbg 6), the label walks (dbg 2) and the row writer (dbg 7
minus dbg 2: labels + writer, less the walks), in Mcycles per batch, with the
relax (dbg 5) beside them.  The counters are in units of 1,024 cycles.

usage: python tools/post_phase_cycles.py <dump file>
"""
import sys

import numpy as np

if __name__ != "__main__" or len(sys.argv) != 2:
    sys.exit(__doc__)
b = open(sys.argv[1], "rb").read()
nB, LB = (int(x) for x in np.frombuffer(b[:8], np.int32))
o = 8 + 4 * nB * LB
dbg = np.frombuffer(b[o:o + 4 * nB * 16], np.int32).reshape(nB, 16).astype(np.float64)
phase = {
    "relax": dbg[:, 5],
    "predecessor pass": dbg[:, 6],
    "label walks": dbg[:, 2],
    "row writer": dbg[:, 7] - dbg[:, 2],
    "tie export": dbg[:, 11],
}
print(f"batches {nB} lanes {LB}")
for k, v in phase.items():
    v = v * 1024 / 1e6
    print(f"{k:18s} mean {v.mean():8.3f}  min {v.min():8.3f}  max {v.max():8.3f}  sum {v.sum():10.1f}  Mcycles")
