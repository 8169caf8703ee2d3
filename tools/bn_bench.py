"""Time h3d_batch_norm_forward (training, + ReLU) and h3d_batch_norm_backward (training, + ReLU; grad_x, grad_gamma, grad_beta) on DLA-34's
BatchNorm shapes at a 512x512 input and the per-GPU shard B = 8.  CALL time: HIP events around `--reps` back-to-back calls after `--warmup`
calls, median of `--rounds` rounds (tools/pool_up_backward_bench.py's method), so launch gaps between the operator's own kernels count.
Bytes by the kernels' own account (csrc/bn.hip), every map N C 4 bytes:
    forward  = 3 reads of x (sum; centred squares; apply) + 1 write of y                                         = 4 maps
    backward = 2 reads each of grad_y, y, x (the sums; grad_x) + 1 write of grad_x                               = 7 maps
(the per-channel vectors and the partial-sum slots are left out: below 1 % of a map).  Beside each rate: the fp32 float4 copy rate of the
microarchitecture guide (6.29 TB/s) and, where profiles/pool_up_backward.json has the same map, maxpool2_bwd_kernel's rate -- the
project's own memory-bound kernel in this layout.  Maps of 2-34 MB stay in the 256 MB Infinity Cache between the calls, so rates above
the HBM copy rate are cache rates; no pass mark is attached.

    python tools/bn_bench.py [--out profiles/bn.json]
"""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import h3d_amd  # noqa: F401
from h3d_amd import bn

# (C, H = W of the map): stem / level0, level1 ... level5, then the DeformConvs of DLAUp / IDAUp
SHAPES = [(16, 512), (32, 256), (64, 128), (128, 64), (256, 32), (512, 16), (256, 16), (128, 32), (128, 16), (64, 64), (64, 32), (64, 16)]
COPY_TBPS = 6.29

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="profiles/bn.json")
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / args.reps)
    return {"ms": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts))}


pool = {}
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "pool_up_backward.json")
if os.path.exists(path):
    for r in json.load(open(path))["shapes"]:
        if r["op"] == "maxpool":
            pool[(r["C"], r["H"])] = r["backward_GBps"]

gen = torch.Generator().manual_seed(0)
rnd = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1).to(dev)
B = args.batch
rows = []
for C, H in SHAPES:
    xv, gv = rnd(B, H, H, C), rnd(B, H, H, C)
    w, b, rm, rv = rnd(C) + 1.5, rnd(C), torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y, mean, var, invstd = bn._forward_nhwc(xv, w, b, None, None, None, rm, rv, True, True, 0.1, 1e-5)
    fwd = timed(lambda: bn._forward_nhwc(xv, w, b, None, None, None, rm, rv, True, True, 0.1, 1e-5))
    bwd = timed(lambda: bn._backward_nhwc(xv, y, gv, w, mean, invstd, True, True, (True, False, True, True)))
    one = B * H * H * C * 4
    chunk, slots = bn.plan(B, C, H, H)
    row = {"C": C, "H": H, "W": H, "B": B, "map_MB": one / 1e6, "chunk": chunk, "slots": slots, "forward": fwd, "backward": bwd,
           "forward_bytes": 4 * one, "backward_bytes": 7 * one, "forward_GBps": 4 * one / fwd["ms"] / 1e6,
           "backward_GBps": 7 * one / bwd["ms"] / 1e6, "copy_GBps_guide": COPY_TBPS * 1e3, "maxpool2_bwd_GBps_same_map": pool.get((C, H))}
    rows.append(row)
    print(json.dumps(row), flush=True)
res = {"device": torch.cuda.get_device_name(0), "batch": B, "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds,
       "what": "call time (events around back-to-back calls, output allocation included); training mode, ReLU, no residual",
       "byte_model": "forward 3 reads of x + 1 write of y; backward 2 reads each of grad_y, y, x + 1 write of grad_x", "shapes": rows}
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
