"""A/B of the sparse heads launch at the bench shapes (B 64, 128 x 128 map, K 100 centres with six heads, 1700 peaks with one head):
the three paths of h3d_heads_sparse_lists interleaved in one process, HIP events around each launch (tests/heads_sparse_op.py holds the op)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from heads_sparse_op import CENTRE, DEV, PATHS, PEAK, Op

B, S, K, PK, REPS, WARM = 64, 128, 100, 1700, 30, 5
op = Op("bf16", B, S, S, 64)
rs = np.random.RandomState(0)
inds = torch.from_numpy(rs.randint(0, S * S, (B, K))).to(DEV)
peaks = torch.from_numpy(rs.randint(0, S * S, (B, PK))).to(DEV)
lists = [(inds, CENTRE), (peaks, PEAK)]
for path in PATHS:                     # the bits first
    op.check(op.sparse(path, *lists), lists, path)
print("bits equal to the dense launch on all paths", flush=True)
arr = op.list_array(lists)
for nlists, tag in ((2, "both lists"), (1, "centre list only")):
    us = {path: [] for path in PATHS}
    for _ in range(REPS):
        for path in PATHS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            op.launch(path, arr, nlists)
            e1.record()
            e1.synchronize()
            us[path].append(e0.elapsed_time(e1) * 1e3)
    for path, v in us.items():
        v = sorted(v[WARM:])
        print("%s  %-10s min %.1f  median %.1f  max %.1f us" % (tag, path, v[0], v[len(v) // 2], v[-1]), flush=True)
