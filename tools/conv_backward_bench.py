"""Time h3d_conv2d_backward (all four gradients, ReLU gate and residual on) on the distinct conv shapes of DLA-34's base network at a
512x512 input and the per-GPU shard B=8, against two baselines from a build of the PARENT commit's library given on the command line
(loaded as tools/ab_lib.py does: same ABI number required), never from the code under test:
  (a) the `f32` plan's forward conv of the same shape: H3D_OP_CONV through the baseline's h3d_run_ops (the 7x7 stem has no such op);
  (b) for the 3x3 stride-1 shapes, the baseline's h3d_dcn_v2_backward at zero offsets and a unit mask: the only route to these
      gradients before this operator.
HIP events around `--reps` back-to-back calls after `--warmup` calls; median of `--rounds` rounds; the shader clock is read right after
each series.  Expectation from the operation count: backward <= 3 x (a).

    python tools/conv_backward_bench.py exp/lib_parent.so [--out profiles/conv_backward.json]
"""
import argparse, ctypes, json, re, subprocess, sys
import numpy as np, torch
sys.path.insert(0, ".")
import h3d_amd  # noqa: F401
from h3d_amd import _lib

# (k, stride, Cin, Cout, H of the input) of the base network (models/model.py:225-300): stem, level0/1, the BasicBlocks, `project` and Root
SHAPES = [(7, 1, 3, 16, 512), (3, 1, 16, 16, 512), (3, 2, 16, 32, 512), (3, 2, 32, 64, 256), (3, 1, 64, 64, 128), (1, 1, 32, 64, 128),
          (1, 1, 128, 64, 128), (3, 2, 64, 128, 128), (3, 1, 128, 128, 64), (1, 1, 64, 128, 64), (1, 1, 256, 128, 64), (1, 1, 448, 128, 64),
          (3, 2, 128, 256, 64), (3, 1, 256, 256, 32), (1, 1, 128, 256, 32), (1, 1, 512, 256, 32), (1, 1, 896, 256, 32),
          (3, 2, 256, 512, 32), (3, 1, 512, 512, 16), (1, 1, 256, 512, 16), (1, 1, 1280, 512, 16)]

ap = argparse.ArgumentParser()
ap.add_argument("baseline")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="profiles/conv_backward.json")
ap.add_argument("--only", type=int, default=-1, help="index into SHAPES: time that shape's backward alone (for a kernel trace)")
args = ap.parse_args()
dev = torch.device("cuda:0")
L = _lib.lib()
P = ctypes.CDLL(args.baseline)
P.h3d_abi_version.restype = ctypes.c_int
if P.h3d_abi_version() != _lib.ABI_VERSION:
    raise SystemExit("%s: ABI %d, this tree binds ABI %d" % (args.baseline, P.h3d_abi_version(), _lib.ABI_VERSION))
if hasattr(P, "h3d_conv2d_backward"):
    raise SystemExit("%s already has h3d_conv2d_backward: the baseline must be a build of the parent commit" % args.baseline)
for n in ("h3d_run_ops", "h3d_dcn_v2_backward", "h3d_dcn_v2_backward_workspace_bytes"):
    getattr(P, n).argtypes = _lib.SIGNATURES[n]
    getattr(P, n).restype = ctypes.c_int


def sclk_mhz():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


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
    return {"ms": float(np.median(ts)), "ms_min": float(min(ts)), "sclk_mhz_after": sclk_mhz()}


rows = []
gen = torch.Generator().manual_seed(0)
for idx, (k, s, C, Co, H) in enumerate(SHAPES):
    if args.only >= 0 and idx != args.only:
        continue
    B, W, p = args.batch, H, k // 2
    Ho = (H + 2 * p - k) // s + 1
    cs = (C + 3) // 4 * 4
    x = (torch.rand(B, H, W, cs, generator=gen) * 2 - 1).to(dev)                   # NHWC, channel stride a multiple of 4
    w = ((torch.rand(Co, C, k, k, generator=gen) * 2 - 1) * (1.5 / (k * k * C) ** 0.5)).to(dev)
    b = ((torch.rand(Co, generator=gen) * 2 - 1) * 0.1).to(dev)
    res = (torch.rand(B, Ho, Ho, Co, generator=gen) * 2 - 1).to(dev)
    gy = (torch.rand(B, Ho, Ho, Co, generator=gen) * 2 - 1).to(dev)
    geo = (B, C, H, W, Co, k, k, s, s, p, p, 1, 1)
    y = torch.empty(B, Ho, Ho, Co, device=dev)
    row = {"k": k, "stride": s, "Cin": C, "Cout": Co, "H": H, "W": W, "B": B, "matrix_core": bool(k != 7)}
    fwd = None
    if k != 7:
        rows128 = (Co + 127) // 128 * 128
        wp = torch.zeros(rows128, k * k, C, device=dev)
        wp[:Co] = w.permute(0, 2, 3, 1).reshape(Co, k * k, C)
        bp = torch.zeros(rows128, device=dev)
        bp[:Co] = b
        op = _lib.H3dOp()
        op.kind, op.dtype = _lib.OP_CONV, _lib.H3D_F32
        op.in_, op.in2, op.w, op.bias, op.out = x.data_ptr(), res.data_ptr(), wp.data_ptr(), bp.data_ptr(), y.data_ptr()
        op.B, op.H, op.W, op.Cin, op.in_cs, op.in2_cs = B, H, W, C, cs, Co
        op.Ho, op.Wo, op.Cout, op.out_cs = Ho, Ho, Co, Co
        op.ksize, op.stride, op.relu, op.out_mode, op.wrows = k, s, 1, _lib.OUT_NHWC, rows128
        arr = (_lib.H3dOp * 1)(op)

        def fwd():
            rc = P.h3d_run_ops(arr, 1, _lib.stream_ptr())
            assert rc == 0, rc
        fwd()                                           # y: the saved output the backward gates on
    else:
        y.copy_(torch.rand(B, Ho, Ho, Co, generator=gen).to(dev) - 0.5)
    torch.cuda.synchronize()
    flags = _lib.CONV_BWD_RELU
    n = ctypes.c_size_t(0)
    _lib.check(L.h3d_conv2d_backward_workspace_bytes(*geo, flags, ctypes.byref(n)), "ws")
    ws = torch.empty(max(n.value, 256), dtype=torch.uint8, device=dev)
    gx, gres, gw, gb = torch.empty(B, H, W, C, device=dev), torch.empty_like(gy), torch.empty_like(w), torch.empty_like(b)

    def bwd():
        rc = L.h3d_conv2d_backward(_lib.ptr(x), cs, _lib.ptr(w), _lib.ptr(y), Co, _lib.ptr(gy), Co, _lib.ptr(gx), _lib.ptr(gres), _lib.ptr(gw),
                                   _lib.ptr(gb), *geo, flags, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        assert rc == 0, rc
    if fwd is not None and args.only < 0:
        row["forward_f32"] = timed(fwd)
    row["backward"] = timed(bwd)
    row["workspace_bytes"] = int(n.value)
    if k == 3 and s == 1 and args.only < 0:
        # (b) today's route: the DeformConv backward of the parent build at zero offsets and a unit mask, NCHW tensors, its five outputs
        xn = x[..., :C].permute(0, 3, 1, 2).contiguous()
        gn = gy.permute(0, 3, 1, 2).contiguous()
        off, m = torch.zeros(B, 18, H, W, device=dev), torch.ones(B, 9, H, W, device=dev)
        dgeo = (B, C, H, W, Co, 3, 3, 1, 1, 1, 1, 1, 1, 1)
        nd = ctypes.c_size_t(0)
        rc = P.h3d_dcn_v2_backward_workspace_bytes(*dgeo, ctypes.byref(nd))
        assert rc == 0, rc
        wsd = torch.empty(max(nd.value, 256), dtype=torch.uint8, device=dev)
        outs = [torch.empty_like(t) for t in (xn, off, m, w, b)]

        def dcn():
            rc = P.h3d_dcn_v2_backward(*[_lib.ptr(t) for t in (xn, w, b, off, m, gn)], *[_lib.ptr(t) for t in outs], *dgeo, _lib.ptr(wsd), nd.value,
                                       _lib.stream_ptr())
            assert rc == 0, rc
        row["dcn_v2_backward_zero_offsets"] = timed(dcn)
        del xn, gn, off, m, wsd, outs
    f = row.get("forward_f32", {}).get("ms")
    d = row.get("dcn_v2_backward_zero_offsets", {}).get("ms")
    row["ratio_backward_to_forward"] = row["backward"]["ms"] / f if f else None
    row["speedup_over_dcn_route"] = d / row["backward"]["ms"] if d else None
    rows.append(row)
    print("%dx%d s%d %4d -> %4d @%3d  fwd %s  bwd %8.3f  ratio %s  dcn route %s" % (
        k, k, s, C, Co, H, "%8.3f" % f if f else "       -", row["backward"]["ms"], "%5.2f" % row["ratio_backward_to_forward"] if f else "    -",
        "%8.3f" % d if d else "-"), flush=True)
if args.only >= 0:
    sys.exit(0)
with_f = [r for r in rows if r.get("forward_f32")]
sa, sb = sum(r["forward_f32"]["ms"] for r in with_f), sum(r["backward"]["ms"] for r in with_f)
res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds,
       "baseline": "library built from the parent commit: (a) H3D_OP_CONV f32 forward, (b) h3d_dcn_v2_backward at zero offsets / unit mask",
       "sum_forward_f32_ms": sa, "sum_backward_ms_of_the_same_shapes": sb, "ratio_backward_to_forward": sb / sa, "shapes": rows}
print(json.dumps({k: v for k, v in res.items() if k != "shapes"}))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
