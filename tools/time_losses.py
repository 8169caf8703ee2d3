"""Timing aid: h3d_amd.losses.loss_multi_pose (csrc/loss.hip: every term in one partial-sum launch + one finish) against the torch
composition of tests/losses_ref.py run in fp32 on the same GPU -- the reference's formulation, and the only baseline there is (the
library had no loss before).  Workload shape: B = 64, 128 x 128 maps, the six multi_pose terms, M = 32.  HIP events after a warm-up;
forward (under no_grad, the validation case) and forward + backward; kernels per call counted by torch.profiler; achieved bytes/s of the
focal pass (one read of logits and gt, one write of pred) against the 6.29 TB/s measured copy rate.
Writes one JSON record to profiles/losses.json (argument: another path)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import h3d_amd  # noqa: F401,E402
import losses_ref as R  # noqa: E402
from h3d_amd import losses  # noqa: E402
from h3d_amd.detector import Opt  # noqa: E402

dev = torch.device("cuda:0")
COPY_RATE = 6.29e12
B, H, W, M = 64, 128, 128, 32


def timed(fn, warm=5, iters=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / iters


def kernels(fn):
    """Device kernels one call launches (None when the profiler is not available)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower())
    except Exception as e:       # noqa: BLE001
        print("profiler unavailable: %r" % (e,))
        return None


if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "losses.json")
    output, batch = R.multi_pose_inputs(0, B, H, W, M)
    o = {k: v.to(dev) for k, v in output.items()}
    b = {k: v.to(dev) for k, v in batch.items()}
    og = {k: v.clone().requires_grad_(True) for k, v in o.items()}
    mod = losses.loss_multi_pose(Opt())

    def hip_fwd():
        with torch.no_grad():
            return mod([dict(o)], b)[0]

    def torch_fwd():
        with torch.no_grad():
            return R.multi_pose(o, b)[0]

    def hip_fb():
        for v in og.values():
            v.grad = None
        mod([dict(og)], b)[0].backward()

    def torch_fb():
        for v in og.values():
            v.grad = None
        R.multi_pose(og, b)[0].backward()

    focal_terms = [losses.focal_term(o["hm"], b["hm"], from_logits=True), losses.focal_term(o["hm_hp"], b["hm_hp"], from_logits=True)]

    def hip_focal():
        return losses.forward_terms(focal_terms)

    lh, lt = float(hip_fwd()), float(torch_fwd())
    rec = {"shape": {"B": B, "H": H, "W": W, "M": M, "terms": 6}, "loss_hip": lh, "loss_torch_fp32": lt, "rel_diff": abs(lh - lt) / abs(lt)}
    rec["fwd_us"] = {"hip": timed(hip_fwd), "torch": timed(torch_fwd)}
    rec["fwd_bwd_us"] = {"hip": timed(hip_fb), "torch": timed(torch_fb)}
    rec["kernels_fwd"] = {"hip": kernels(hip_fwd), "torch": kernels(torch_fwd)}
    rec["kernels_fwd_bwd"] = {"hip": kernels(hip_fb), "torch": kernels(torch_fb)}
    n = o["hm"].numel() + o["hm_hp"].numel()
    t = timed(hip_focal)
    rec["focal_pass"] = {"elements": n, "bytes": 12 * n, "us": t, "bytes_per_s": 12 * n / (t * 1e-6), "of_copy_rate": 12 * n / (t * 1e-6) / COPY_RATE,
                         "note": "both focal terms with the pred store, partial + finish launches and the host call included"}
    rec["speedup"] = {"fwd": rec["fwd_us"]["torch"] / rec["fwd_us"]["hip"], "fwd_bwd": rec["fwd_bwd_us"]["torch"] / rec["fwd_bwd_us"]["hip"]}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
