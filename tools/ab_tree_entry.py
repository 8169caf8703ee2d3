"""Profiling aid: the fused Tree entries (Plan.FLAGS fold_tree_entry, H3D_OPF_TREE_ENTRY) against the three launches they replace, per level,
in one process: the bench plan's op array is timed launch by launch (h3d_run_ops_timed) with the flags set and cleared, alternating.  Level 2's
conv1 runs on csrc/conv2.hip in such a plan and on csrc/conv.hip in the default one: its three launches are timed both ways.

    python tools/ab_tree_entry.py [--batch 64] [--dtype bf16] [--reps 5]
"""
import argparse, ctypes, sys, numpy as np, torch
sys.path.insert(0, ".")
import h3d_amd
from h3d_amd import _lib, arch, synth
from h3d_amd.detector import MultiPoseDetector, Opt

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
opt = Opt(input_h=512, input_w=512, smpl=True, dtype=args.dtype)
sd = synth.synth_state_dict(arch.state_dict_shapes(opt.heads, True), seed=0, gain=1.25, offset_scale=0.5)
det = MultiPoseDetector(opt, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, device=dev)
x = torch.from_numpy(synth.synth_image_batch(args.batch, 512, 512)).to(dev)
det.run(x); torch.cuda.synchronize()
plan = det.model.engine(dev).plan(args.batch, 512, 512)
n = len(plan.ops)
ms = (ctypes.c_float * n)()
FLAGS = _lib.OPF_TREE_ENTRY | _lib.OPF_TREE_ENTRY_PRIVATE_POOL
pools = [i for i, op in enumerate(plan.ops) if op.kind == _lib.OP_MAXPOOL and op.reserved & _lib.OPF_TREE_ENTRY]
flagged = [i for i, op in enumerate(plan.ops) if op.reserved & _lib.OPF_TREE_ENTRY and op.kind in (_lib.OP_MAXPOOL, _lib.OP_CONV, _lib.OP_CONV_STREAM)]
assert flagged == [j for i in pools for j in (i, i + 1, i + 2)], flagged
word = {i: plan.ops[i].reserved for i in flagged}
# level 2's conv1 as the default plan lowers it: csrc/conv.hip on the [rows][9][Cin] pack
l2 = [i + 2 for i in pools if plan.ops[i].Cin == 32]
conv_hip = None
if l2:
    wp, bp, cout, cin, k, rows = plan.pw.conv("base.level2.tree1.conv1.weight", None, "base.level2.tree1.bn1")
    conv_hip = _lib.H3dOp.from_buffer_copy(plan.ops[l2[0]])
    conv_hip.kind, conv_hip.w, conv_hip.bias, conv_hip.wrows, conv_hip.reserved = _lib.OP_CONV, wp.data_ptr(), bp.data_ptr(), rows, 0
    conv2_op = _lib.H3dOp.from_buffer_copy(plan.ops[l2[0]])
modes = ["fused", "three"] + (["three, conv.hip"] if l2 else [])
runs = {m: [] for m in modes}
for rep in range(args.reps + 1):
    for m in modes:
        for i in flagged:
            plan.op_array[i].reserved = word[i] if m == "fused" else word[i] & ~FLAGS
        if l2:
            plan.op_array[l2[0]] = conv_hip if m == "three, conv.hip" else conv2_op
            plan.op_array[l2[0]].reserved = 0 if m == "three, conv.hip" else word[l2[0]] if m == "fused" else word[l2[0]] & ~FLAGS
        _lib.check(_lib.lib().h3d_run_ops_timed(plan.op_array, n, _lib.stream_ptr(), ms), "timed")
        if rep:
            runs[m].append(np.frombuffer(ms, dtype=np.float32, count=n).copy())
for i in flagged:
    plan.op_array[i].reserved = word[i]
if l2:
    plan.op_array[l2[0]] = conv2_op
med = {k: np.median(np.stack(v), axis=0) for k, v in runs.items()}
print("level (Cin -> Cout @ Ho)      pool   project     conv1   = three    fused    saved   [ms, median of %d]" % args.reps)
tot = [0.0, 0.0]
for i in pools:
    op = plan.ops[i + 2]
    a, f = med["three"][i:i + 3], med["fused"][i:i + 3]
    assert f[1] == 0.0 and f[2] == 0.0, f
    if op.Cin == 32:
        c = med["three, conv.hip"][i:i + 3]
        print("%4d -> %4d @ %3d  conv.hip  %8.4f  %8.4f  %8.4f  %8.4f %8.4f %8.4f   (the default plan's three launches)" % (
            op.Cin, op.Cout, op.Ho, c[0], c[1], c[2], c.sum(), f[0], c.sum() - f[0]))
        tot[0] += c.sum(); tot[1] += f[0]
        print("%4d -> %4d @ %3d  conv2     %8.4f  %8.4f  %8.4f  %8.4f %8.4f %8.4f" % (op.Cin, op.Cout, op.Ho, a[0], a[1], a[2], a.sum(), f[0], a.sum() - f[0]))
        continue
    tot[0] += a.sum(); tot[1] += f[0]
    print("%4d -> %4d @ %3d            %8.4f  %8.4f  %8.4f  %8.4f %8.4f %8.4f" % (op.Cin, op.Cout, op.Ho, a[0], a[1], a[2], a.sum(), f[0], a.sum() - f[0]))
print("all flagged levels: %.4f -> %.4f ms; whole plan (sum of launches): %.4f -> %.4f ms" % (
    tot[0], tot[1], med["three, conv.hip" if l2 else "three"].sum(), med["fused"].sum()))
