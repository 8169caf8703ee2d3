"""One trainer.NetworkTrainer.train_step (the whole DLA-34 under autograd, folded BatchNorm) against one trainer.HeadsTrainer.train_step
(the heads on the frozen backbone) on a synthetic multi_pose batch at 512x512, B = 8: wall time (HIP events around `--reps` steps after
`--warmup` steps, median of `--rounds` rounds) and the peak of torch's device allocator over a step.

    python tools/time_train_step.py [--bn batch] [--out profiles/train_step.json]

--bn batch adds the same step with training-mode BatchNorm (NetworkTrainer(bn="batch"), h3d_amd/bn.py) under "NetworkTrainer_bn_batch",
measured in the same process right after the frozen step.
"""
import argparse, json, os, random, sys
from types import SimpleNamespace as NS
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import h3d_amd  # noqa: F401
from h3d_amd import arch, model, synth, train_input, trainer

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--plain", action="store_true", help="not_use_dcn")
ap.add_argument("--bn", choices=("frozen", "batch"), default="frozen", help="batch: also time NetworkTrainer(bn='batch')")
ap.add_argument("--out", default="profiles/train_step.json")
args = ap.parse_args()
dev = torch.device("cuda:0")
HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}
opt = NS(task="multi_pose", lr=1.25e-4, lr_step=[90, 120], num_iters=-1, input_res=args.res, output_res=args.res // 4, not_rand_crop=False,
         aug_rot=0.0, rotate=0.0, flip=0.5, no_color_aug=False)


def make_net():
    net = model.dla_net(HEADS, head_conv=256, not_use_dcn=args.plain, dtype="f32")
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, not args.plain, 256), seed=0, gain=1.25)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.to(dev)


rs = np.random.RandomState(13)
imgs = [torch.from_numpy(rs.randint(0, 256, (480, 640, 3)).astype(np.uint8)).to(dev) for _ in range(args.batch)]


def scene(seed, n=4, J=17, img_w=640, img_h=480, min_size=60.0, max_size=300.0):
    """n people in a 640 x 480 frame: boxes xywh [n,4] and keypoints [n,J,3] in and a little around their box, multiples of 1/4."""
    r = np.random.RandomState(seed)
    boxes, kps = np.zeros((n, 4), np.float32), np.zeros((n, J, 3), np.float32)
    for k in range(n):
        w, h = r.uniform(min_size, max_size, 2)
        x, y = r.uniform(-0.1 * img_w, img_w - 0.5 * w), r.uniform(-0.1 * img_h, img_h - 0.5 * h)
        boxes[k] = np.round(np.array([x, y, w, h]) * 4) / 4
        kps[k, :, 0] = np.round(r.uniform(x - 0.1 * w, x + 1.1 * w, J) * 4) / 4
        kps[k, :, 1] = np.round(r.uniform(y - 0.1 * h, y + 1.1 * h, J) * 4) / 4
        kps[k, :, 2] = (r.uniform(size=J) < 0.7) * r.randint(1, 3, J)
    return boxes, kps


scenes = [scene(20 + b) for b in range(args.batch)]
np.random.seed(17), random.seed(17)
batch = train_input.multi_pose_train_batch(imgs, np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes]), [4] * args.batch, opt,
                                           data_rng=np.random.RandomState(123))


def measure(cls, **kw):
    tr = cls(opt, make_net(), **kw)
    for _ in range(args.warmup):
        tr.train_step(dict(batch))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    ts = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            _, loss, _ = tr.train_step(dict(batch))
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / args.reps)
    n = sum(p.numel() for p in tr.heads.parameters())
    return {"ms": float(np.median(ts)), "ms_min": float(min(ts)), "peak_MiB": torch.cuda.max_memory_allocated(dev) / 2 ** 20,
            "resident_before_MiB": before / 2 ** 20, "parameters": n, "loss": float(loss.detach())}


res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "res": args.res, "dcn": not args.plain,
       "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds}
for name, cls in (("HeadsTrainer", trainer.HeadsTrainer), ("NetworkTrainer", trainer.NetworkTrainer)):
    res[name] = measure(cls)
    print(name, json.dumps(res[name]), flush=True)
    torch.cuda.empty_cache()
if args.bn == "batch":
    res["NetworkTrainer_bn_batch"] = measure(trainer.NetworkTrainer, bn="batch")
    print("NetworkTrainer_bn_batch", json.dumps(res["NetworkTrainer_bn_batch"]), flush=True)
    torch.cuda.empty_cache()
    res["ratio_ms_batch_over_frozen"] = res["NetworkTrainer_bn_batch"]["ms"] / res["NetworkTrainer"]["ms"]
# what the graph of one image keeps for its backward: distinct storages handed to save_for_backward during one forward
seen = {}


def pack(t):
    if t.is_cuda:
        seen[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
    return t


tm = trainer.NetworkTrainer(opt, make_net()).heads
with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
    out = tm(batch["input"][:1])
params = {p.untyped_storage().data_ptr() for p in tm.parameters()}
res["saved_for_backward_MiB_per_image"] = sum(n for ptr, n in seen.items() if ptr not in params) / 2 ** 20
print("saved for backward per image: %.1f MiB" % res["saved_for_backward_MiB_per_image"], flush=True)
del out, tm
res["ratio_ms"] = res["NetworkTrainer"]["ms"] / res["HeadsTrainer"]["ms"]
print(json.dumps({"ratio_ms": res["ratio_ms"]}))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
