#!/usr/bin/env python
"""Times the training-target launches (csrc/targets.hip) at the workload's shape (reported, not gated):
    python tools/time_targets.py [--out profiles/targets.json] [--batch 64] [--res 128] [--persons 4 32]
Per person count: h3d_multi_pose_targets with every output (objects + render launch), the same call without the two maps (the objects
launch alone; the render launch is NOT timed by itself: its figure is the difference of the two series), a `fill_` of a tensor of the bytes the call writes (the box's fill rate, measured in
the same run), and the numpy restatement of tests/targets_ref.py on one CPU core per image.  The device series are 50 calls issued back
to back through ctypes between two device events (the launches are shorter than a Python-level call), 3 warm-up rounds, the median of
10 rounds.  The objects-only series is a launch of a few microseconds issued from Python: it may be bound by the launch rate rather than
by the kernel, so it is an upper bound of the kernel's time.  The shader clock is read right after each full-call series (the clock the
card held under that load; a reading in front of the run is an idle clock and says nothing) and written next to the numbers."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CALLS = 50


def sclk_mhz():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def per_call_us(fn, warm=3, rounds=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / CALLS)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--persons", type=int, nargs="+", default=[4, 32])
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    import targets_ref as R
    from h3d_amd import _lib, targets
    assert torch.cuda.is_available(), "time_targets.py measures on the GPU only"
    dev = torch.device("cuda:0")
    B, res, J, N = args.batch, args.res, 17, 32
    L = _lib.lib()
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "res": res, "calls_per_round": CALLS, "series": []}
    c = np.tile(np.array([320.0, 240.0], np.float32), (B, 1))
    trans = targets.target_transforms(c, np.full(B, 640.0), None, res, res)
    for persons in args.persons:
        scenes = [R.scene(1000 * persons + b, persons, M=N, quarter=False, vis_p=1.0) for b in range(B)]
        boxes, kps = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
        d = {"boxes": torch.from_numpy(boxes).to(dev), "kps": torch.from_numpy(kps).to(dev), "num": torch.full((B,), persons, dtype=torch.int32, device=dev),
             "trans": trans.to(dev)}
        o = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in targets.pose_output_specs(B, N, J, res, res).items()}
        ws = targets._workspace(B, N, J, dev)
        p, st = _lib.ptr, _lib.stream_ptr()
        order = ("hm", "hm_hp", "wh", "reg", "ind", "reg_mask", "hps", "hps_mask", "hp_offset", "hp_ind", "hp_mask", "gt_det", "gt_count")

        def call(maps):
            outs = [p(o[k]) if (maps or k not in ("hm", "hm_hp")) else p(None) for k in order]
            rc = L.h3d_multi_pose_targets(p(d["boxes"]), p(d["kps"]), p(d["num"]), p(d["trans"]), None, None, None, None, 0, B, N, J, res, res, N,
                                          *outs, 0, p(ws), ws.numel(), st)
            assert rc == 0, L.h3d_last_error()
        written = sum(t.numel() * t.element_size() for t in o.values())
        fill = torch.empty(written // 4, dtype=torch.float32, device=dev)
        both, both_min = per_call_us(lambda: call(True))
        sclk = sclk_mhz()
        objs, objs_min = per_call_us(lambda: call(False))
        fill_us, fill_min = per_call_us(lambda: fill.fill_(0.0))
        splats = int(o["hp_mask"].sum()) + int(o["gt_count"].sum())
        t0 = time.perf_counter()
        nimg = min(B, 8)
        for b in range(nimg):
            R.multi_pose_image(boxes[b], kps[b], persons, trans[b].numpy(), out_h=res, out_w=res, max_objs=N)
        cpu_ms = (time.perf_counter() - t0) / nimg * 1e3
        out["series"].append({"persons": persons, "splats": splats, "bytes_written": written, "both_launches_us": both, "both_launches_us_min": both_min,
                              "objects_launch_us": objs, "objects_launch_us_min": objs_min, "render_launch_us_by_difference": both - objs, "sclk_mhz_after_series": sclk,
                              "fill_us": fill_us, "fill_us_min": fill_min, "fill_GBps": written / fill_us / 1e3,
                              "render_over_fill": (both - objs) / fill_us, "images_per_s": B / both * 1e6,
                              "cpu_restatement_ms_per_image_one_core": cpu_ms})
        print(json.dumps(out["series"][-1]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
