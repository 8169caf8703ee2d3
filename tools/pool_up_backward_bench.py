"""Time h3d_maxpool2_backward and h3d_upsample_backward on DLA-34's pool and up-sample shapes at a 512x512 input and the per-GPU shard
B=8, each against the `f32` forward op of the same shape (H3D_OP_MAXPOOL / H3D_OP_UPADD through h3d_run_ops) from a build of the PARENT
commit's library given on the command line (same ABI number required), never from the code under test.  HIP events around `--reps`
back-to-back calls after `--warmup` calls; median of `--rounds` rounds (tools/conv_backward_bench.py's method).
Expectation from the bytes moved: pool backward = 9/5 of its forward; up backward, grad_x alone,
= (f^2 + 2) / (2 f^2 + 1) of its forward, plus the grad_w pass.

    python tools/pool_up_backward_bench.py exp/lib_parent.so [--out profiles/pool_up_backward.json]
"""
import argparse, ctypes, json, sys
import numpy as np, torch
sys.path.insert(0, ".")
import h3d_amd  # noqa: F401
from h3d_amd import _lib

# Tree.downsample of level2..5 (models/model.py:201): (C, H of the input)
POOLS = [(32, 256), (64, 128), (128, 64), (256, 32)]
# IDAUp's up_k (arch.ida_specs): (C, f, H of the input); the last one is the f = 8 the operator also takes (no dla34 layer has it)
UPS = [(256, 2, 16), (128, 2, 32), (64, 2, 64), (64, 4, 32), (64, 8, 16)]

ap = argparse.ArgumentParser()
ap.add_argument("baseline")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="profiles/pool_up_backward.json")
args = ap.parse_args()
dev = torch.device("cuda:0")
L = _lib.lib()
P = ctypes.CDLL(args.baseline)
P.h3d_abi_version.restype = ctypes.c_int
if P.h3d_abi_version() != _lib.ABI_VERSION:
    raise SystemExit("%s: ABI %d, this tree binds ABI %d" % (args.baseline, P.h3d_abi_version(), _lib.ABI_VERSION))
if hasattr(P, "h3d_upsample_backward"):
    raise SystemExit("%s already has h3d_upsample_backward: the baseline must be a build of the parent commit" % args.baseline)
P.h3d_run_ops.argtypes = _lib.SIGNATURES["h3d_run_ops"]
P.h3d_run_ops.restype = ctypes.c_int


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
    return {"ms": float(np.median(ts)), "ms_min": float(min(ts))}


def run_op(op):
    arr = (_lib.H3dOp * 1)(op)

    def f():
        rc = P.h3d_run_ops(arr, 1, _lib.stream_ptr())
        assert rc == 0, rc
    return f


gen = torch.Generator().manual_seed(0)
rnd = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1).to(dev)
B = args.batch
rows = []
for C, H in POOLS:
    x, gy = rnd(B, H, H, C), rnd(B, H // 2, H // 2, C)
    y, gx = torch.empty_like(gy), torch.empty_like(x)
    op = _lib.H3dOp()
    op.kind, op.dtype, op.in_, op.out = _lib.OP_MAXPOOL, _lib.H3D_F32, x.data_ptr(), y.data_ptr()
    op.B, op.H, op.W, op.Cin, op.in_cs, op.Ho, op.Wo, op.Cout, op.out_cs = B, H, H, C, C, H // 2, H // 2, C, C
    op.ksize, op.stride, op.out_mode = 2, 2, _lib.OUT_NHWC

    def bwd():
        rc = L.h3d_maxpool2_backward(_lib.ptr(x), C, _lib.ptr(gy), C, _lib.ptr(gx), C, B, C, H, H, _lib.stream_ptr())
        assert rc == 0, rc
    row = {"op": "maxpool", "C": C, "H": H, "W": H, "B": B, "forward_f32": timed(run_op(op)), "backward": timed(bwd)}
    row["ratio_backward_to_forward"] = row["backward"]["ms"] / row["forward_f32"]["ms"]
    row["expected_ratio"] = 9 / 5
    row["backward_GBps"] = 9 * gy.numel() * 4 / row["backward"]["ms"] / 1e6
    rows.append(row)
    print("pool %4d @%3d  fwd %7.4f  bwd %7.4f  ratio %5.2f (expected 1.80)" % (C, H, row["forward_f32"]["ms"], row["backward"]["ms"],
                                                                               row["ratio_backward_to_forward"]), flush=True)
for C, f, H in UPS:
    k = 2 * f
    x, w, skip, gy = rnd(B, H, H, C), rnd(k * k, C), rnd(B, H * f, H * f, C), rnd(B, H * f, H * f, C)
    y, gx, gw = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(w)
    op = _lib.H3dOp()
    op.kind, op.dtype = _lib.OP_UPADD, _lib.H3D_F32
    op.in_, op.in2, op.w, op.out = x.data_ptr(), skip.data_ptr(), w.data_ptr(), y.data_ptr()
    op.B, op.H, op.W, op.Cin, op.in_cs, op.in2_cs, op.Ho, op.Wo, op.Cout, op.out_cs = B, H, H, C, C, C, H * f, H * f, C, C
    op.ksize, op.stride, op.out_mode = k, f, _lib.OUT_NHWC
    n = ctypes.c_size_t(0)
    _lib.check(L.h3d_upsample_backward_workspace_bytes(B, C, H, H, f, ctypes.byref(n)), "ws")
    ws = torch.empty(max(n.value, 256), dtype=torch.uint8, device=dev)

    def bwd(want_x=True, want_w=True):
        rc = L.h3d_upsample_backward(_lib.ptr(x), C, _lib.ptr(w), _lib.ptr(gy), C, _lib.ptr(gx) if want_x else None, C, _lib.ptr(gw) if want_w else None,
                                     B, C, H, H, f, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        assert rc == 0, rc
    row = {"op": "upadd", "C": C, "f": f, "H": H, "W": H, "B": B, "workspace_bytes": int(n.value), "forward_f32": timed(run_op(op)),
           "backward": timed(bwd), "backward_grad_x_only": timed(lambda: bwd(True, False)), "backward_grad_w_only": timed(lambda: bwd(False, True))}
    fw = row["forward_f32"]["ms"]
    row["ratio_backward_to_forward"] = row["backward"]["ms"] / fw
    row["ratio_grad_x_only_to_forward"] = row["backward_grad_x_only"]["ms"] / fw
    row["expected_ratio_grad_x_only"] = (f * f + 2) / (2 * f * f + 1)
    rows.append(row)
    print("up f%d %4d @%3d  fwd %7.4f  bwd %7.4f (gx %7.4f, gw %7.4f)  gx / fwd %5.2f (expected %.2f)  all / fwd %5.2f" % (
        f, C, H, fw, row["backward"]["ms"], row["backward_grad_x_only"]["ms"], row["backward_grad_w_only"]["ms"],
        row["ratio_grad_x_only_to_forward"], row["expected_ratio_grad_x_only"], row["ratio_backward_to_forward"]), flush=True)
res = {"device": torch.cuda.get_device_name(0), "batch": B, "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds,
       "baseline": "library built from the parent commit: H3D_OP_MAXPOOL / H3D_OP_UPADD f32 forward of the same shape", "shapes": rows}
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
