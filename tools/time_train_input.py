#!/usr/bin/env python
"""Times the training-input launches (csrc/augment.hip) at the workload's shape (reported, not gated):
    python tools/time_train_input.py [--out profiles/train_input.json] [--batch 64] [--src 480 640] [--res 512]
Series, each CALLS calls issued back to back through ctypes between two device events, 3 warm-up rounds, the median of 10 rounds:
    colour      h3d_train_input with colour augmentation: train_warp_kernel + train_colour_kernel (the two launches together; their split
                comes from a kernel trace, e.g. rocprofv3 --kernel-trace --stats -- python tools/time_train_input.py)
    plain       the same call with H3D_TRAIN_INPUT_NO_COLOR_AUG: train_plain_kernel alone
    pre_process h3d_preprocess (the val branch, untouched by this path) on the same frames
The parameters are draw_params' under fixed seeds (random crop, rotation up to +-60 degrees, mirror).  Bytes moved per call: the source
frames (an upper bound of what the warp reads: a crop reads part of its frame, and neighbouring pixels share their 2 x 2 taps through
the caches), the dword-per-pixel intermediate written by launch 1 and read by launch 2, the fp32 output.  The share of the HBM rate is
those bytes over the time against 8 TB/s."""
import argparse
import ctypes
import json
import os
import random
import sys
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CALLS = 20
HBM_BYTES_PER_S = 8.0e12


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_input.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--src", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    ap.add_argument("--res", type=int, default=512)
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    from h3d_amd import _lib, preprocess, train_input
    assert torch.cuda.is_available(), "time_train_input.py measures on the GPU only"
    dev = torch.device("cuda:0")
    B, (h, w), res = args.batch, args.src, args.res
    L = _lib.lib()
    frames = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (B, h, w, 3)).astype(np.uint8)).to(dev)
    np.random.seed(0), random.seed(0)
    params = train_input.draw_params([(h, w)] * B, NS(aug_rot=0.5, rotate=30.0, flip=0.5), "multi_pose", data_rng=np.random.RandomState(123))
    buf, where = train_input._source(frames)
    desc = train_input.descriptors(where, params, res, res)
    desc_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(dev)
    mean_t, std_t = train_input._mean_std(train_input.MEAN, train_input.STD, dev)
    out = torch.empty(B, 3, res, res, dtype=torch.float32, device=dev)
    ws = _lib.workspace(L.h3d_train_input_workspace_bytes, B, res, res, 0, device=dev)
    p, st = _lib.ptr, _lib.stream_ptr()

    def call(options):
        rc = L.h3d_train_input(p(buf), buf.numel(), ctypes.c_void_p(desc.ctypes.data), p(desc_dev), B, p(mean_t), p(std_t), res, res, options,
                               p(ws), ws.numel(), p(out), None, st)
        assert rc == 0, L.h3d_last_error()

    n = res * res
    src_bytes, mid_bytes, out_bytes = B * h * w * 3, B * n * 4, B * 3 * n * 4
    moved = {"colour": src_bytes + 2 * mid_bytes + out_bytes, "plain": src_bytes + out_bytes, "pre_process": src_bytes + out_bytes}
    series = {"colour": lambda: call(0), "plain": lambda: call(_lib.TRAIN_INPUT_NO_COLOR_AUG)}
    series["pre_process"] = lambda: preprocess.pre_process(frames, input_res=res)
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "src": [h, w], "res": res, "calls_per_round": CALLS,
              "bytes": {"source_read_upper_bound": src_bytes, "intermediate_written": mid_bytes, "intermediate_read": mid_bytes, "fp32_written": out_bytes},
              "series": {}}
    for name, fn in series.items():
        med, best = per_call_us(fn)
        result["series"][name] = {"us": med, "us_min": best, "bytes_moved": moved[name], "GBps": moved[name] / med / 1e3,
                                  "share_of_hbm_rate": moved[name] / (med * 1e-6) / HBM_BYTES_PER_S, "images_per_s": B / med * 1e6}
        print(name, json.dumps(result["series"][name]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
