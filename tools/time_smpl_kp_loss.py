#!/usr/bin/env python
"""Times forward + backward of the SMPL keypoint reprojection loss at B = 8, max_objs = 32, V = 6890, K = 17 for NV = 0 and NV = 8
(reported, not gated):
    python tools/time_smpl_kp_loss.py [--out profiles/smpl_kp_loss.json] [--nv 0,8]
(one NV at a time under `rocprofv3 --kernel-trace --stats -- python tools/time_smpl_kp_loss.py --nv 8` gives the four kernels' device times)
Series, each CALLS forward + backward pairs issued back to back between two device events on the current stream, 3 warm-up rounds, the
median of ROUNDS rounds, the shader clock read right after each series:
    h3d        smpl_loss.smpl_keypoint_loss(...).backward(): autograd + two launches forward, two backward (csrc/smpl_loss.hip)
    h3d_calls  keypoint_loss_forward + keypoint_loss_backward without autograd (what the four launches and their Python cost)
    torch      the same loss in torch ops on the same device, tensors and stream: an index_select of the NV vertices per keypoint, the
               whole-map permute + gather of the three camera channels, about twenty elementwise launches, and autograd's dense
               [P,V,3] scatter for grad_verts
The gradients go to joints, verts (NV > 0) and cam_map in all three."""
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

B, MAX_OBJS, V, K, H, W = 8, 32, 6890, 17, 128, 128
CALLS, ROUNDS = 50, 9


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


def torch_loss(joints, verts, cam_map, ind, hps, mask, jw, vi, vw, n):
    """The definition in torch ops (tests/smpl_kp_loss_ref.kp_loss without the out-of-range rule: every index here is on the map)."""
    Bn, HW = cam_map.shape[0], cam_map.shape[2] * cam_map.shape[3]
    P, Kn = joints.shape[0], jw.shape[0]
    kp3d = torch.einsum("kj,pjc->pkc", jw, joints)
    if vi is not None:
        g = verts.index_select(1, vi.reshape(-1)).reshape(P, Kn, vi.shape[1], 3)
        kp3d = kp3d + (vw[None, :, :, None] * g).sum(2)
    idx = ind[:, :n]
    cam = cam_map.reshape(Bn, 3, HW).permute(0, 2, 1).contiguous().gather(1, idx[:, :, None].expand(Bn, n, 3)).reshape(P, 3)
    pred = cam[:, 0, None, None] * kp3d[..., :2] + cam[:, None, 1:3]
    m = mask[:, :n].reshape(P, Kn, 2)
    return (m * (pred - hps[:, :n].reshape(P, Kn, 2)).abs()).sum() / (m.sum() + 1e-4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smpl_kp_loss.json"))
    ap.add_argument("--nv", default="0,8", help="the NV values to time")
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    from h3d_amd import smpl_loss
    assert torch.cuda.is_available(), "time_smpl_kp_loss.py measures on the GPU only"
    dev = torch.device("cuda:0")
    n, P = MAX_OBJS, B * MAX_OBJS
    rs = np.random.RandomState(0)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)
    joints, verts = f(rs.randn(P, 24, 3) * 0.4), f(rs.randn(P, V, 3) * 0.4)
    cam = rs.randn(B, 3, H * W)
    cam[:, 0] = 4.0 + 8.0 * rs.rand(B, H * W)
    cam_map = f(cam.reshape(B, 3, H, W))
    ind = torch.from_numpy(np.stack([rs.permutation(H * W)[:MAX_OBJS] for _ in range(B)]).astype(np.int64)).to(dev)
    hps = f(rs.randn(B, MAX_OBJS, 2 * K) * 3.0)
    mask_u8 = torch.from_numpy((rs.rand(B, MAX_OBJS, 2 * K) < 0.7).astype(np.uint8)).to(dev)
    mask_f = mask_u8.float()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "max_objs": MAX_OBJS, "P": P, "V": V, "K": K,
              "map": [H, W], "calls_per_round": CALLS, "rounds": ROUNDS, "series": {}}
    for NV in [int(x) for x in args.nv.split(",")]:
        reg = smpl_loss.KeypointRegressor.synthetic(K, V, NV, seed=0)
        d = reg.device(dev)
        j, v, c = joints.clone().requires_grad_(True), verts.clone().requires_grad_(True), cam_map.clone().requires_grad_(True)
        vin = v if NV else None
        one = torch.ones((), device=dev)

        def h3d():
            j.grad = v.grad = c.grad = None
            smpl_loss.smpl_keypoint_loss(j, vin, c, ind, hps, mask_u8, reg, n).backward()

        def h3d_calls():
            stats, kp3d, pred, a = smpl_loss.keypoint_loss_forward(joints, verts if NV else None, cam_map, ind, hps, mask_u8, reg, n)
            smpl_loss.keypoint_loss_backward(a, stats, kp3d, pred, one)

        def torch_run():
            j.grad = v.grad = c.grad = None
            torch_loss(j, vin, c, ind, hps, mask_f, d["joint_w"], d["vert_idx"].long() if NV else None, d["vert_w"] if NV else None, n).backward()
        # the two agree before they are timed
        h3d()
        ours = [t.grad.clone() for t in (j, c)] + ([v.grad.clone()] if NV else [])
        torch_run()
        theirs = [t.grad for t in (j, c)] + ([v.grad] if NV else [])
        for a, b in zip(ours, theirs):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-12, "the fused loss and the torch restatement disagree"
        for name, fn in (("h3d", h3d), ("h3d_calls", h3d_calls), ("torch", torch_run)):
            r = series(fn)
            result["series"]["NV%d/%s" % (NV, name)] = r
            print("NV%d" % NV, name, json.dumps(r))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
