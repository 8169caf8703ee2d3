#!/usr/bin/env python
"""Times one Adam step over the head parameters of the multi_pose task plus the pose / shape heads at head_conv 256 (reported, not gated):
    python tools/time_adam.py [--out profiles/adam_step.json] [--head-conv 256]
Series, each CALLS steps issued back to back between two device events, 3 warm-up rounds, the median of ROUNDS rounds, the shader clock
read right after each series:
    h3d            optim.Adam.step(): Python descriptor fill + one h3d_adam_step launch (csrc/optim.hip)
    h3d_launch     the h3d_adam_step call alone over descriptors filled once (what the kernel and its launch cost)
    torch_foreach  torch.optim.Adam(foreach=True).step() on tensors of the same shapes
    torch_fused    torch.optim.Adam(fused=True).step()
The torch series are the yardsticks.  Traffic: 28 bytes per element (p, g, m, v read; p, m, v written)."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2, "pose": 72, "shape": 10}
CALLS, ROUNDS = 50, 9
HBM_BYTES_PER_S = 8.0e12


def sclk_mhz():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def series(fn, warm=3):
    for _ in range(warm):
        for _ in range(CALLS):
            fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / CALLS)
    return {"us": float(np.median(ts)), "us_min": float(min(ts)), "sclk_mhz_after": sclk_mhz()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_step.json"))
    ap.add_argument("--head-conv", type=int, default=256)
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    from h3d_amd import _lib, optim
    assert torch.cuda.is_available(), "time_adam.py measures on the GPU only"
    dev = torch.device("cuda:0")
    hc = args.head_conv
    shapes = []
    for c in HEADS.values():
        shapes += [(hc, 64, 3, 3), (hc,), (c, hc, 1, 1), (c,)]
    g = torch.Generator().manual_seed(0)

    def params():
        ps = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i)).to(dev)) for i, s in enumerate(shapes)]
        for i, p in enumerate(ps):
            p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(dev)
        return ps
    elements = sum(int(np.prod(s)) for s in shapes)
    moved = 28 * elements
    ours_p, launch_p, foreach_p, fused_p = params(), params(), params(), params()
    ours = optim.Adam(ours_p, lr=1.25e-4)
    foreach = torch.optim.Adam(foreach_p, lr=1.25e-4, foreach=True)
    fused = torch.optim.Adam(fused_p, lr=1.25e-4, fused=True)
    # the bare call: descriptors of a step-1 state, filled once
    ms, vs = [torch.zeros_like(p) for p in launch_p], [torch.zeros_like(p) for p in launch_p]
    descs = (_lib.H3dAdamTensor * len(launch_p))()
    for d, p, m, v in zip(descs, launch_p, ms, vs):
        optim.fill(d, p, p.grad, m, v, optim.scalars(1.25e-4, 0.9, 0.999, 1e-8, 0.0, 1))
    L, st, n = _lib.lib(), _lib.stream_ptr(), len(launch_p)

    def bare():
        rc = L.h3d_adam_step(descs, n, st)
        assert rc == 0, L.h3d_last_error()
    runs = {"h3d": ours.step, "h3d_launch": bare, "torch_foreach": foreach.step, "torch_fused": fused.step}
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "head_conv": hc, "tensors": len(shapes), "elements": elements,
              "bytes_moved": moved, "launches_per_step": -(-len(shapes) // _lib.ADAM_CAPACITY), "calls_per_round": CALLS, "rounds": ROUNDS,
              "series": {}}
    for name, fn in runs.items():
        r = series(fn)
        r["GBps"] = moved / r["us"] / 1e3
        r["share_of_hbm_rate"] = moved / (r["us"] * 1e-6) / HBM_BYTES_PER_S
        result["series"][name] = r
        print(name, json.dumps(r))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
