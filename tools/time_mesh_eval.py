#!/usr/bin/env python
"""Times the 3D evaluation's joint call (n = 24, weights and roots) and vertex call (n = 6890, rooted by the joints) at P = 64 and 800
pairs, and the means over the pairs (reported, not gated: the evaluation is not on the detector's path):
    python tools/time_mesh_eval.py [--out profiles/mesh_eval.json] [--pairs 64,800]
Series, each CALLS calls issued back to back between two device events on the current stream, 3 warm-up rounds, the median of ROUNDS
rounds, the shader clock read right after each series:
    joints    mesh_eval.pointset_errors on [P,24,3]       one launch of pointset_errors_kernel, P workgroups (csrc/mesh_eval.hip)
    verts     mesh_eval.pointset_errors on [P,6890,3]     the same kernel: three passes over 2 x 82 KB per pair
    means     mesh_eval.metric_means on [P,2]             one wave
    mirror    mesh_eval.evaluate_numpy on the host for the same joint and vertex calls (one run each, wall clock; for information)
The device results equal the mirror's bit for bit before anything is timed."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

V, J = 6890, 24
CALLS, ROUNDS = 20, 9


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_eval.json"))
    ap.add_argument("--pairs", default="64,800", help="the numbers of pairs to time")
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    from h3d_amd import mesh_eval
    assert torch.cuda.is_available(), "time_mesh_eval.py measures on the GPU only"
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "V": V, "J": J, "calls_per_round": CALLS, "rounds": ROUNDS,
              "series": {}}
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)
    for P in [int(x) for x in args.pairs.split(",")]:
        rs = np.random.RandomState(P)
        pj, pv = (rs.randn(P, J, 3) * 0.3).astype(np.float32), (rs.randn(P, V, 3) * 0.3).astype(np.float32)
        gj, gv = (pj * 1.1 + rs.randn(P, J, 3) * 0.02).astype(np.float32), (pv * 1.1 + rs.randn(P, V, 3) * 0.02).astype(np.float32)
        w = (rs.rand(P, J) < 0.9).astype(np.uint8)
        idx = np.arange(P, dtype=np.int32)
        d = {k: torch.from_numpy(a).to(dev) for k, a in dict(pj=pj, pv=pv, gj=gj, gv=gv, w=w, idx=idx).items()}
        joints = lambda: mesh_eval.pointset_errors(d["pj"], d["gj"], d["idx"], d["idx"], d["w"], d["pj"], d["gj"], (1, 2))
        verts = lambda: mesh_eval.pointset_errors(d["pv"], d["gv"], d["idx"], d["idx"], None, d["pj"], d["gj"], (1, 2))
        ej, cj, _ = joints()
        ev, cv, _ = verts()
        means = lambda: mesh_eval.metric_means(ej, cj)
        host = {}
        for name, call, got in (("joints", lambda: mesh_eval.evaluate_numpy(pj, gj, idx, idx, w, pj, gj, (1, 2)), (ej, cj)),
                                ("verts", lambda: mesh_eval.evaluate_numpy(pv, gv, idx, idx, None, pj, gj, (1, 2)), (ev, cv))):
            t0 = time.perf_counter()
            want = call()
            host[name] = (time.perf_counter() - t0) * 1e6
            assert np.array_equal(bits(got[0].cpu().numpy()), bits(want[0])) and np.array_equal(got[1].cpu().numpy(), want[1]), \
                "the kernel and the mirror disagree"
        for name, fn in (("joints", joints), ("verts", verts), ("means", means)):
            r = series(fn)
            if name in host:
                r["mirror_us"] = host[name]
            result["series"]["P%d/%s" % (P, name)] = r
            print("P%d" % P, name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
