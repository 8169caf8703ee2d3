"""Time dcn_v2_backward on the 16 DeformConv shapes of the DLA-34 network (512x512 input) at the per-GPU shard B=8:
(a) the forward operator's exact-fp32 fast path (H3D_DCN_F32_MFMA) from a BASELINE build of the library given on the command line
    (loaded as tools/ab_lib.py does: same ABI number required), (b) h3d_dcn_v2_backward (matrix-core kernels),
(c) h3d_dcn_v2_backward_general.  HIP events around `--reps` back-to-back calls after `--warmup` calls; median of `--rounds` rounds.

    python tools/dcn_backward_bench.py exp/lib_parent.so [--out profiles/dcn_backward.json]
"""
import argparse, ctypes, json, sys
import numpy as np, torch
sys.path.insert(0, ".")
import h3d_amd  # noqa: F401
from h3d_amd import _lib

# (Cin, Cout, H) of the 16 DeformConv layers of dla_34 + DLAUp / IDAUp at 512x512: proj and node of every IDAUp step
SHAPES = [(512, 256, 16), (256, 256, 32), (256, 128, 32), (128, 128, 64), (128, 64, 64), (64, 64, 128),
          (256, 128, 32), (128, 128, 64), (128, 64, 64), (64, 64, 128), (128, 64, 64), (64, 64, 128),
          (128, 64, 64), (64, 64, 128), (256, 64, 32), (64, 64, 128)]

ap = argparse.ArgumentParser()
ap.add_argument("baseline")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="profiles/dcn_backward.json")
ap.add_argument("--skip-general", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
L = _lib.lib()
P = ctypes.CDLL(args.baseline)
P.h3d_abi_version.restype = ctypes.c_int
if P.h3d_abi_version() != _lib.ABI_VERSION:
    raise SystemExit("%s: ABI %d, this tree binds ABI %d" % (args.baseline, P.h3d_abi_version(), _lib.ABI_VERSION))
for n in ("h3d_dcn_v2_pack_weights", "h3d_dcn_v2_forward_packed"):
    getattr(P, n).argtypes = _lib.SIGNATURES[n]
    getattr(P, n).restype = ctypes.c_int
for n in ("h3d_dcn_v2_packed_weight_bytes", "h3d_dcn_v2_packed_workspace_bytes"):
    getattr(P, n).argtypes = [ctypes.c_int] * (3 if "weight" in n else 5)
    getattr(P, n).restype = ctypes.c_size_t


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
    return float(np.median(ts))


rows = []
gen = torch.Generator().manual_seed(0)
for (C, Co, H) in SHAPES:
    B, W = args.batch, H
    x = (torch.rand(B, C, H, W, generator=gen) * 2 - 1).to(dev)
    w = ((torch.rand(Co, C, 3, 3, generator=gen) * 2 - 1) * (1.5 / (9 * C) ** 0.5)).to(dev)
    b = torch.zeros(Co, device=dev)
    off = ((torch.rand(B, 18, H, W, generator=gen) * 2 - 1) * 1.5).to(dev)
    m = torch.rand(B, 9, H, W, generator=gen).to(dev)
    go = (torch.rand(B, Co, H, W, generator=gen) * 2 - 1).to(dev)
    out = torch.empty(B, Co, H, W, device=dev)
    packed = torch.empty(P.h3d_dcn_v2_packed_weight_bytes(Co, C, _lib.H3D_F32), dtype=torch.uint8, device=dev)
    _lib.check(P.h3d_dcn_v2_pack_weights(_lib.ptr(w), _lib.ptr(b), Co, C, _lib.H3D_F32, _lib.ptr(packed), _lib.stream_ptr()), "pack")
    nfw = P.h3d_dcn_v2_packed_workspace_bytes(B, C, H, W, 0)
    wsf = torch.empty(nfw, dtype=torch.uint8, device=dev)

    def fwd():
        rc = P.h3d_dcn_v2_forward_packed(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(off), _lib.ptr(m), _lib.ptr(out), B, C, H, W, Co, _lib.H3D_F32,
                                         _lib.DCN_F32_MFMA, _lib.ptr(wsf), nfw, _lib.stream_ptr())
        assert rc == 0, rc
    geo = (B, C, H, W, Co, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    n = ctypes.c_size_t(0)
    _lib.check(L.h3d_dcn_v2_backward_workspace_bytes(*geo, ctypes.byref(n)), "ws")
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
    outs = [torch.empty_like(t) for t in (x, off, m, w, b)]

    def bwd(fn):
        def run():
            rc = fn(*[_lib.ptr(t) for t in (x, w, b, off, m, go)], *[_lib.ptr(t) for t in outs], *geo, _lib.ptr(ws), n.value, _lib.stream_ptr())
            assert rc == 0, rc
        return run
    ta, tb = timed(fwd), timed(bwd(L.h3d_dcn_v2_backward))
    tc = None if args.skip_general else timed(bwd(L.h3d_dcn_v2_backward_general))
    rows.append({"Cin": C, "Cout": Co, "H": H, "W": W, "B": B, "forward_f32_ms": ta, "backward_ms": tb, "backward_general_ms": tc,
                 "workspace_bytes": int(n.value)})
    print("%4d -> %4d @%3d  fwd %8.3f  bwd %8.3f  general %s  ratio %.2f" % (C, Co, H, ta, tb, "%8.3f" % tc if tc else "-", tb / ta), flush=True)
sa, sb = sum(r["forward_f32_ms"] for r in rows), sum(r["backward_ms"] for r in rows)
res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds,
       "sum_forward_f32_ms": sa, "sum_backward_ms": sb, "ratio_backward_to_forward": sb / sa,
       "sum_backward_general_ms": None if args.skip_general else sum(r["backward_general_ms"] for r in rows), "shapes": rows}
print(json.dumps({k: v for k, v in res.items() if k != "shapes"}))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
