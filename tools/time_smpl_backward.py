#!/usr/bin/env python
"""Times the SMPL backward against the forward and against torch autograd of the torch restatement (reported, not gated):
    python tools/time_smpl_backward.py [--out profiles/smpl_backward.json] [--persons 64 512 6400]
Per person count on the full 6890-vertex synthetic model: `smpl.lbs_backward` with both upstreams, `smpl.lbs` forward (gen3x), and the
fp32 torch-autograd backward of tests/smpl_grad_ref.lbs on the same device tensors.  Each series: 5 warm-up calls, then the median of 20
timed calls between device events; the shader clock is read before and after and written next to the numbers."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def sclk_mhz():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def median_ms(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smpl_backward.json"))
    ap.add_argument("--persons", type=int, nargs="+", default=[64, 512, 6400])
    ap.add_argument("--torch-max-persons", type=int, default=6400, help="skip the torch series above this person count (it keeps [P,6890,12] intermediates)")
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    import smpl_grad_ref as G
    from h3d_amd import smpl
    dev = torch.device("cuda:0")
    model = smpl.SMPLModel.synthetic(seed=0)
    mt = G.model_tensors(model.numpy_dict(), torch.float32, dev)
    res = {"device": torch.cuda.get_device_name(0), "sclk_mhz_before": sclk_mhz(), "vertices": 6890, "series": []}
    for P in args.persons:
        rs = np.random.RandomState(P)
        b = torch.from_numpy(rs.randn(P, 10).astype(np.float32)).to(dev)
        t = torch.from_numpy((rs.randn(P, 72) * 0.3).astype(np.float32)).to(dev)
        gv, gj = torch.randn(P, 6890, 3, device=dev), torch.randn(P, 24, 3, device=dev)
        row = {"persons": P}
        row["backward_ms"], row["backward_min_ms"] = median_ms(lambda: smpl.lbs_backward(model, b, t, gv, gj))
        row["forward_gen3x_ms"], row["forward_gen3x_min_ms"] = median_ms(lambda: smpl.lbs(model, b, t, return_joints=True, kernel="gen3x"))
        row["backward_over_forward"] = row["backward_ms"] / row["forward_gen3x_ms"]
        if P <= args.torch_max_persons:
            bb, tt = b.clone().requires_grad_(True), t.clone().requires_grad_(True)
            verts, joints, _, _ = G.lbs(bb, tt, mt, torch.float32)
            loss = (verts * gv).sum() + (joints * gj).sum()
            row["torch_backward_ms"], _ = median_ms(lambda: torch.autograd.grad(loss, (bb, tt), retain_graph=True), warm=2, reps=5)
            row["fused_over_torch"] = row["backward_ms"] / row["torch_backward_ms"]
            del verts, joints, loss
        else:
            row["torch_backward_ms"] = None
        print(json.dumps(row), flush=True)
        res["series"].append(row)
    res["sclk_mhz_after"] = sclk_mhz()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
