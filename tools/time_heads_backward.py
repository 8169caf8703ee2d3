#!/usr/bin/env python
"""Times the heads backward against the heads forward (reported, not gated):
    python tools/time_heads_backward.py [--out profiles/heads_backward.json] [--batch 8] [--parent-lib exp/lib_parent.so]
At B = 8, 128 x 128, head_conv 256, the multi_pose head set (hm 1, wh 2, hps 34, reg 2, hm_hp 17, hp_offset 2):
    backward            one h3d_heads_backward call, all gradients of all heads + grad_feat
    backward_no_feat    the same without grad_feat
    forward_f32         the `f32`-plan heads launches (H3D_OP_HEADS, one per group of equal width) -- through the library given with
                        --parent-lib (a build of the parent commit, as tools/ab_lib.py loads one) when present, the in-tree one otherwise
Each series: 3 warm-up calls, then rounds of back-to-back calls between device events, the median round divided by the calls per round;
the shader clock is read after each series.  Expectation from the operation count: backward <= 4 x forward."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}


def sclk_mhz():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def series(fn, calls=4, rounds=7, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "sclk_mhz_after": sclk_mhz()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads_backward.json"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--head-conv", type=int, default=256)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "exp", "lib_parent.so"))
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    from h3d_amd import _lib, heads
    dev = torch.device("cuda:0")
    B, S, hc = args.batch, args.size, args.head_conv
    g = torch.Generator().manual_seed(0)
    feat = torch.randn(B, S, S, 64, generator=g).to(dev)
    params = {h: tuple(t.to(dev) for t in ((torch.rand(hc, 64, 3, 3, generator=g) * 2 - 1) / 24.0, (torch.rand(hc, generator=g) * 2 - 1) / 24.0,
                                            (torch.rand(c, hc, 1, 1, generator=g) * 2 - 1) / 16.0, torch.zeros(c))) for h, c in HEADS.items()}
    gz = {h: torch.randn(B, c, S, S, generator=g).to(dev) for h, c in HEADS.items()}
    spec = [(p[0], p[1], p[2].reshape(p[2].shape[0], -1), gz[h], (True,) * 4) for h, p in params.items()]
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "height": S, "width": S, "head_conv": hc, "heads": HEADS,
           "sclk_mhz_before": sclk_mhz()}
    res["backward"] = series(lambda: heads.heads_backward(feat, spec, want_feat=True))
    res["backward_no_feat"] = series(lambda: heads.heads_backward(feat, spec, want_feat=False))
    # the forward: pack once, then time the launches alone
    L = _lib.lib()
    res["forward_library"] = "in-tree"
    if os.path.exists(args.parent_lib):
        P = ctypes.CDLL(args.parent_lib)
        P.h3d_abi_version.restype = ctypes.c_int
        if P.h3d_abi_version() != _lib.ABI_VERSION:
            raise SystemExit("%s: ABI %d, this tree binds ABI %d" % (args.parent_lib, P.h3d_abi_version(), _lib.ABI_VERSION))
        P.h3d_run_ops.argtypes, P.h3d_run_ops.restype = L.h3d_run_ops.argtypes, ctypes.c_int
        L, res["forward_library"] = P, os.path.relpath(args.parent_lib, ROOT)
    arr, outs, keep = heads.heads_ops(feat, params)
    res["forward_f32"] = series(lambda: _lib.check(L.h3d_run_ops(arr, len(arr), _lib.stream_ptr()), "h3d_run_ops"))
    res["backward_over_forward"] = res["backward"]["median_ms"] / res["forward_f32"]["median_ms"]
    res["backward_no_feat_over_forward"] = res["backward_no_feat"]["median_ms"] / res["forward_f32"]["median_ms"]
    res["target_backward_over_forward"] = 4.0
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
