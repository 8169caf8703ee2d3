#!/usr/bin/env python
"""Times forward + backward of the SMPL 3D supervision loss (rotation, shape and 3D-joint terms) at B = 8, max_objs = 32, 128 x 128 maps
(reported, not gated):
    python tools/time_smpl_sup_loss.py [--out profiles/smpl_sup_loss.json]
(under `rocprofv3 --kernel-trace --stats -- python tools/time_smpl_sup_loss.py` the four kernels' device times)
Series, each CALLS forward + backward pairs issued back to back between two device events on the current stream, 3 warm-up rounds, the
median of ROUNDS rounds:
    h3d        smpl_sup.smpl_supervised_loss(...) and backward(): autograd + two launches forward, two backward (csrc/smpl_sup.hip)
    h3d_calls  supervised_loss_forward + supervised_loss_backward without autograd (what the four launches and their Python cost)
    labels     smpl_sup.smpl_targets_raw on device tensors: the one launch of the label transform (flipped and rotated images)
    torch      the same loss in torch ops on the same device, tensors and stream: the whole-map gathers of the 72 + 10 channels, Rodrigues
               in about thirty elementwise launches, and autograd's dense scatter back into the maps
The gradients go to pose_map, shape_map and joints in all three loss series."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, MAX_OBJS, H, W = 8, 32, 128, 128
CALLS, ROUNDS = 50, 9


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
    return {"us": float(np.median(ts)), "us_min": float(min(ts))}


def rodrigues(theta):
    e = theta + 1e-8
    angle = torch.sqrt((e * e).sum(-1, keepdim=True))
    d = theta / angle
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(theta.shape[:-1] + (3, 3))
    return torch.eye(3, device=theta.device) + torch.sin(angle)[..., None] * K + (1 - torch.cos(angle))[..., None] * (K @ K)


def gather(fmap, idx):
    Bn, C = fmap.shape[:2]
    return fmap.reshape(Bn, C, -1).gather(2, idx[:, None, :].expand(Bn, C, idx.shape[1])).permute(0, 2, 1)


def torch_loss(pose_map, shape_map, ind, joints, lab, n):
    """The definition in torch ops (tests/smpl_sup_ref.sup_loss without the out-of-range and NaN rules: every index here is on the map and
    every label finite)."""
    Bn = pose_map.shape[0]
    idx = ind[:, :n]
    R = rodrigues(gather(pose_map, idx).reshape(Bn, n, 24, 3)).reshape(Bn, n, 24, 9)
    wp, ws, wj = lab["smpl_pose_w"][:, :n], lab["smpl_shape_w"][:, :n], lab["smpl_joints_w"][:, :n]
    l_pose = (wp * ((R - lab["smpl_rotmat"][:, :n]) ** 2).sum(-1)).sum() / (9.0 * wp.sum() + 1e-4)
    l_shape = (ws * ((gather(shape_map, idx) - lab["smpl_shape"][:, :n]) ** 2).sum(-1)).sum() / (10.0 * ws.sum() + 1e-4)
    J, Jl = joints.reshape(Bn, n, 24, 3), lab["smpl_joints"][:, :n]
    d = (J - 0.5 * (J[:, :, 1:2] + J[:, :, 2:3])) - (Jl - 0.5 * (Jl[:, :, 1:2] + Jl[:, :, 2:3]))
    l_j = (wj * (d ** 2).sum(-1)).sum() / (3.0 * wj.sum() + 1e-4)
    return l_pose, l_shape, l_j


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smpl_sup_loss.json"))
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    from h3d_amd import smpl_sup
    assert torch.cuda.is_available(), "time_smpl_sup_loss.py measures on the GPU only"
    dev = torch.device("cuda:0")
    n, P = MAX_OBJS, B * MAX_OBJS
    rs = np.random.RandomState(0)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)
    pose_map, shape_map = f(rs.randn(B, 72, H, W) * 0.5), f(rs.randn(B, 10, H, W))
    joints = f(rs.randn(P, 24, 3) * 0.4)
    ind = torch.from_numpy(np.stack([rs.permutation(H * W)[:MAX_OBJS] for _ in range(B)]).astype(np.int64)).to(dev)
    # the labels through the label kernel: every row valid, half the images mirrored, all rotated
    raw = (f(rs.randn(B, MAX_OBJS, 72) * 0.5), f(rs.randn(B, MAX_OBJS, 10)), f(rs.randn(B, MAX_OBJS, 24, 3) * 0.4),
           torch.ones(B, MAX_OBJS, device=dev), f(0.25 + rs.rand(B, MAX_OBJS, 24)), f(0.25 + rs.rand(B, MAX_OBJS, 24)))
    num = torch.full((B,), MAX_OBJS, dtype=torch.int32, device=dev)
    reg_mask = torch.ones(B, MAX_OBJS, dtype=torch.uint8, device=dev)
    flipped = torch.tensor([b & 1 for b in range(B)], dtype=torch.int32, device=dev)
    r = np.deg2rad(np.linspace(-30, 30, B))
    rot2 = torch.from_numpy(np.stack([np.stack([np.cos(r), np.sin(r)], -1), np.stack([-np.sin(r), np.cos(r)], -1)], -2)).to(dev)
    lab = smpl_sup.smpl_targets_raw(raw[0], raw[1], raw[2], raw[3], raw[4], raw[5], num, reg_mask, flipped, rot2, MAX_OBJS)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "max_objs": MAX_OBJS, "P": P, "map": [H, W],
              "calls_per_round": CALLS, "rounds": ROUNDS, "series": {}}
    p, s, j = pose_map.clone().requires_grad_(True), shape_map.clone().requires_grad_(True), joints.clone().requires_grad_(True)
    go = torch.ones(3, device=dev)

    def h3d():
        p.grad = s.grad = j.grad = None
        a, b, c = smpl_sup.smpl_supervised_loss(p, s, ind, j, lab, n)
        (a + b + c).backward()

    def h3d_calls():
        stats, a = smpl_sup.supervised_loss_forward(pose_map, shape_map, ind, joints, lab, n)
        smpl_sup.supervised_loss_backward(a, stats, go)

    def labels():
        smpl_sup.smpl_targets_raw(raw[0], raw[1], raw[2], raw[3], raw[4], raw[5], num, reg_mask, flipped, rot2, MAX_OBJS, out=lab)

    def torch_run():
        p.grad = s.grad = j.grad = None
        a, b, c = torch_loss(p, s, ind, j, lab, n)
        (a + b + c).backward()
    # the two agree before they are timed
    h3d()
    ours = [t.grad.clone() for t in (p, s, j)]
    torch_run()
    for a, b in zip(ours, (p.grad, s.grad, j.grad)):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-12, "the fused loss and the torch restatement disagree"
    for name, fn in (("h3d", h3d), ("h3d_calls", h3d_calls), ("labels", labels), ("torch", torch_run)):
        result["series"][name] = series(fn)
        print(name, json.dumps(result["series"][name]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
