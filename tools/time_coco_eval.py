#!/usr/bin/env python
"""Times the COCO evaluation on a val2017-sized synthetic set (reported, not gated):
    python tools/time_coco_eval.py [--out profiles/coco_eval.json] [--images 5000] [--dets 100] [--max-gt 20] [--mirror-images 200]
For keypoints and bbox, each series CALLS calls issued back to back between two device events, 2 warm-up rounds, the median of ROUNDS:
    match        coco_eval.match without the public matrix: one h3d_coco_match launch (csrc/eval.hip) and its output allocations
    sort         coco_eval.sort_detections: the two stable torch sorts, bincount and cumsum
    accumulate   the h3d_coco_accumulate call alone (two launches) on a sorted order made once
    evaluate     coco_eval.evaluate end to end, the read-back of precision / recall and the host summary included (wall clock)
and once, on this machine's CPU, coco_eval.evaluate_numpy on the first --mirror-images images of the same data: the only other path.
Traffic: the bytes each kernel has to read and write once (for accumulate: per row, 17 bytes per position of its class' segment),
against the HBM rate."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CALLS, ROUNDS = 5, 7
HBM_BYTES_PER_S = 8.0e12


def workload(N, D, G, kp, seed=0):
    """-> (results [N,D,39 | 6] float32, GroundTruth): 1 .. G ground truths per image, three detections in four are jittered copies."""
    from h3d_amd import coco_eval as C
    rs = np.random.RandomState(seed)
    num = rs.randint(1, G + 1, N).astype(np.int32)
    wh = np.exp(rs.uniform(np.log(8.0), np.log(300.0), (N, G, 2)))
    xy = rs.uniform(0, 500, (N, G, 2))
    boxes = np.round(np.concatenate([xy, wh], -1), 2)
    area = np.round(boxes[..., 2] * boxes[..., 3] * rs.uniform(0.4, 0.9, (N, G)), 3)
    crowd = rs.rand(N, G) < 0.05
    v = rs.randint(0, 3, (N, G, 17)) * (rs.rand(N, G, 1) > 0.1)
    pts = np.round(boxes[..., None, :2] + rs.uniform(0, 1, (N, G, 17, 2)) * boxes[..., None, 2:], 0)
    kps = np.concatenate([pts * (v[..., None] > 0), v[..., None]], -1)
    pick = (rs.rand(N, D) * num[:, None]).astype(np.int64)
    b = np.take_along_axis(boxes, pick[..., None], 1)
    corners = np.concatenate([b[..., :2], b[..., :2] + b[..., 2:]], -1) + rs.uniform(0, 0.25, (N, D, 1)) * rs.uniform(-1, 1, (N, D, 4)) * np.tile(b[..., 2:], 2)
    stray = rs.rand(N, D) < 0.25
    sxy, swh = rs.uniform(0, 500, (N, D, 2)), np.exp(rs.uniform(np.log(8.0), np.log(300.0), (N, D, 2)))
    corners = np.where(stray[..., None], np.concatenate([sxy, sxy + swh], -1), corners)
    res = np.zeros((N, D, 39 if kp else 6), np.float32)
    res[..., :4], res[..., 4] = corners, rs.uniform(0.02, 1.0, (N, D))
    if kp:
        base = np.take_along_axis(pts, pick[..., None, None], 1) + 0.05 * np.sqrt(np.take_along_axis(area, pick, 1))[..., None, None] * rs.randn(N, D, 17, 2)
        res[..., 5:] = np.where(stray[..., None, None], corners[..., None, :2] + rs.uniform(0, 1, (N, D, 17, 2)) * swh[..., None, :], base).reshape(N, D, 34)
    return res, C.GroundTruth(boxes, kps if kp else None, area, crowd, None, num, 1)


def series(fn, warm=2):
    for _ in range(warm):
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


def traffic(r, moved):
    r["bytes_moved"] = int(moved)
    r["GBps"] = moved / r["us"] / 1e3
    r["share_of_hbm_rate"] = moved / (r["us"] * 1e-6) / HBM_BYTES_PER_S
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval.json"))
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--max-gt", type=int, default=20)
    ap.add_argument("--mirror-images", type=int, default=200)
    args = ap.parse_args()
    import h3d_amd  # noqa: F401
    from h3d_amd import _lib, coco_eval as C
    assert torch.cuda.is_available(), "time_coco_eval.py measures on the GPU only"
    dev = torch.device("cuda:0")
    N, D, G = args.images, args.dets, args.max_gt
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "images": N, "dets_per_image": D, "max_gt_per_image": G,
              "calls_per_round": CALLS, "rounds": ROUNDS, "mirror_images": args.mirror_images, "types": {}}
    L = _lib.lib()
    for iou_type in ("keypoints", "bbox"):
        kp = iou_type == "keypoints"
        res, gt = workload(N, D, G, kp)
        rng, max_dets = C._params(iou_type)
        A, T, M, R, K, W = len(rng), len(C.IOU_THRS), len(max_dets), len(C.REC_THRS), 1, res.shape[2]
        dres = torch.from_numpy(res).to(dev)
        out = {}
        m = C.match(dres, gt, iou_type, want_ious=False)
        moved = N * D * W * 4 + N * G * ((4 + 1 + (51 if kp else 0)) * 8 + 1 + 4) + N * D * ((6 + (34 if kp else 0)) * 8 + 4) + N * A * T * D * 5 + N * A * G
        out["match"] = traffic(series(lambda: C.match(dres, gt, iou_type, want_ious=False)), moved)
        out["sort"] = series(lambda: C.sort_detections(m, K))
        order, seg = C.sort_detections(m, K)
        g = gt.to(dev)
        ws = _lib.workspace(L.h3d_coco_accumulate_workspace_bytes, K, A, device=dev)
        precision = torch.empty(T, R, K, A, M, dtype=torch.float64, device=dev)
        recall = torch.empty(T, K, A, M, dtype=torch.float64, device=dev)
        md = (ctypes.c_int32 * M)(*[int(v) for v in max_dets])
        rec = C._constants(dev, iou_type)[3]

        def acc():
            _lib.check(L.h3d_coco_accumulate(_lib.ptr(order), _lib.ptr(seg), _lib.ptr(m["dt_rank"]), _lib.ptr(m["dt_match"]), _lib.ptr(m["dt_ignore"]),
                                             _lib.ptr(m["gt_ignore"]), _lib.ptr(g["cls"]), _lib.ptr(g["num"]), N, D, G, K, A, T, md, M, _lib.ptr(rec), R,
                                             _lib.ptr(precision), _lib.ptr(recall), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "h3d_coco_accumulate")
        rows = K * A * M * T
        out["accumulate"] = traffic(series(acc), rows * N * D * 17 + K * A * N * G * 5 + (rows * R + rows) * 8)
        out["accumulate"]["rows"] = rows
        ts = []
        for _ in range(2 + ROUNDS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = C.evaluate(dres, gt, iou_type)
            ts.append((time.perf_counter() - t0) * 1e6)
        out["evaluate"] = {"us": float(np.median(ts[2:])), "us_min": float(min(ts[2:])), "wall_clock": True}
        out["stats"] = [float(s) for s in ev.stats]
        n = min(args.mirror_images, N)
        t0 = time.perf_counter()
        mirror = C.evaluate_numpy(res[:n], gt.subset(n), iou_type)
        out["numpy_mirror"] = {"images": n, "us": (time.perf_counter() - t0) * 1e6, "cpus": os.cpu_count(), "stats": [float(s) for s in mirror.stats]}
        sub = C.evaluate(dres[:n].contiguous(), gt.subset(n), iou_type)
        out["numpy_mirror"]["device_stats_equal"] = bool(np.array_equal(sub.stats, mirror.stats))
        result["types"][iou_type] = out
        print(iou_type, json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
