#!/usr/bin/env python
"""Times the mesh rasteriser (csrc/render.hip) on SMPL-sized bodies (reported in DESIGN.md section 23, not gated):
    python tools/time_render.py [--out profiles/render.json] [--sizes 8x32,64x100]
    rocprofv3 --kernel-trace --stats -- python tools/time_render.py --profile --sizes 64x100     (device time per kernel, a run of its own)
Workload: render.capsule_mesh(82, 84) bodies (6890 vertices, 13 776 faces: SMPL's counts), each turned at random, about 40 map pixels
high (s = 44 on a body 0.9 long), at random centres of 128 x 128 maps, up = 4 (512 x 512 targets), depth offset focal / s.
Series, each CALLS calls issued back to back between two device events on the current stream, 2 warm-up rounds, the median of ROUNDS
rounds, the shader clock read right after each series:
    rasterize        render.rasterize: one memset, render_raster_kernel, render_resolve_kernel<true, false>
    rasterize+shade  the same plus render.shade over a frame: render_resolve_kernel<false, true>
    lbs              smpl.lbs on the synthetic 6890-vertex body for the same P: the stage that produces the vertices (context)
and two variants of `rasterize` that tell what bounds the raster kernel:
    rasterize/cull_back  H3D_RENDER_CULL_BACK: the same staging, face loop and coverage tests, half the covered pixels (a closed body)
    rasterize/up1        up = 1: the same staging and face loop on a target of 1/16 of the pixels (nearly every face misses every centre)"""
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

H = W = 128
UP, ROUNDS = 4, 9


def sclk_mhz():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def series(fn, calls, warm=2):
    for _ in range(warm):
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    return {"us": float(np.median(ts)), "us_min": float(min(ts)), "us_max": float(max(ts)), "calls": calls, "sclk_mhz_after": sclk_mhz()}


def rotations(P, rs):
    q = rs.randn(P, 4)
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)


def workload(B, n, dev, seed=0):
    from h3d_amd import render
    rs = np.random.RandomState(seed)
    v, f = render.capsule_mesh(82, 84)
    P = B * n
    R = torch.from_numpy(rotations(P, rs).astype(np.float32)).to(dev)
    verts = torch.einsum("pij,vj->pvi", R, torch.from_numpy(v).to(dev)).contiguous()
    cam = rs.randn(B, 3, H * W).astype(np.float32)
    cam[:, 0] = 40.0 / 0.9 * rs.uniform(0.9, 1.1, (B, H * W))
    cam[:, 1:] = rs.uniform(-0.5, 0.5, (B, 2, H * W))
    ind = np.stack([rs.permutation(H * W)[:n] for _ in range(B)]).astype(np.int64)
    frames = torch.from_numpy(rs.randint(0, 256, (B, UP * H, UP * W, 3)).astype(np.uint8)).to(dev)
    return verts, f, torch.from_numpy(cam.reshape(B, 3, H, W)).to(dev), torch.from_numpy(ind).to(dev), frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    ap.add_argument("--sizes", default="8x32,64x100", help="B x n, comma separated")
    ap.add_argument("--profile", action="store_true", help="three calls of rasterize + shade per size and nothing else (for rocprofv3)")
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    from h3d_amd import render, smpl
    assert torch.cuda.is_available(), "time_render.py measures on the GPU only"
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "map": [H, W], "up": UP, "V": 6890, "F": 13776,
              "rounds": ROUNDS, "series": {}}
    body = smpl.SMPLModel.synthetic()
    for size in args.sizes.split(","):
        B, n = (int(t) for t in size.split("x"))
        P = B * n
        verts, f, cam, ind, frames = workload(B, n, dev)
        r = render.MeshRenderer(f, up=UP)
        faces, colour = r._on(dev, B, n)
        s = cam[:, 0].reshape(B, H * W).gather(1, ind)
        dz = torch.full_like(s, float(UP * W)) / s

        def rasterize():
            return render.rasterize(verts, faces, cam, ind, n, UP, dz=dz)

        def both():
            keys = rasterize()[2]
            return render.shade(keys, verts, faces, image=frames, colour=colour, alpha=r.alpha, ambient=r.ambient)

        fid = rasterize()[0]
        torch.cuda.synchronize()
        covered = float((fid >= 0).float().mean())
        seen = int(torch.unique(torch.div(fid[0][fid[0] >= 0], len(f), rounding_mode="floor")).numel())
        if args.profile:
            for _ in range(3):
                both()
            torch.cuda.synchronize()
            continue
        calls = max(3, min(50, 6400 // P))
        result["series"]["%s/workload" % size] = {"P": P, "covered_fraction": covered, "people_seen_in_image_0": seen}
        betas = torch.from_numpy(np.random.RandomState(1).randn(P, 10).astype(np.float32)).to(dev)
        thetas = torch.from_numpy((np.random.RandomState(2).randn(P, 72) * 0.3).astype(np.float32)).to(dev)
        dz1 = torch.full_like(s, float(W)) / s
        variants = (("rasterize/cull_back", lambda: render.rasterize(verts, faces, cam, ind, n, UP, dz=dz, flags=render.CULL_BACK)),
                    ("rasterize/up1", lambda: render.rasterize(verts, faces, cam, ind, n, 1, dz=dz1)))
        for name, fn in (("rasterize", rasterize), ("rasterize+shade", both), ("lbs", lambda: smpl.lbs(body, betas, thetas))) + variants:
            res = series(fn, calls)
            result["series"]["%s/%s" % (size, name)] = res
            print(size, name, json.dumps(res))
        del verts, frames
        torch.cuda.empty_cache()
    if not args.profile:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
