"""DeformConv calibration and timing tooling of an engine (`DLAEngine` keeps thin methods of the same names): the far-sample counts of
csrc/dcn3.hip's tile variants on a calibration batch, the rule that chooses a variant per layer from them, and the stopwatch the
rule's constants were fitted against (tools/fit_dcn_rule.py)."""
import ctypes

import torch

from . import _lib
from ._lib import H3dOp
from .plan import DCN_F16IN
from .weights import LOWP

DCN_VARIANTS = {"narrow": 0, "slots512": _lib.OPF_DCN_STREAM_SLOTS512, "wide": _lib.OPF_DCN_STREAM_WIDE_MARGIN}      # h3d_op.reserved bits read by csrc/dcn3.hip's launcher

# Cost model of the three tile variants, in units of "one tile of the `narrow` variant that stays within its slots"
# (fitted once from round 3's timing table; tools/fit_dcn_rule.py prints model vs stopwatch per layer):
#   a tile with more far samples than slots re-runs them in pass 2 (offset conv recomputed + serialised global
#   gathers): it costs ~3.2x a normal tile; the 512-slot variant is 2 % slower on a tile that does not need it and pays
#   an exposed load latency per stage for a second fill round; the wide margin stages 40 % more apron: 5 % slower.
#   tail: a launch ends with its slowest workgroup -- on a grid of few rounds (workgroups / resident workgroups) ONE overflowing
#   tile delays the end by a good part of a tile time, whatever the share of such tiles (measured, round 4: 256 -> 256 @32x32
#   at batch 64, two rounds, 0.4 % of the tiles over their slots: 0.166 ms narrow vs 0.144 with 512 slots; 256 -> 64 @32x32,
#   half a round, 7 % of the wide variant's tiles over: 0.108 ms wide vs 0.075 with 512 slots).
DCN_RULE = {"pass2": 2.2, "slots512": 0.02, "round2": 0.30, "wide": 0.05, "tail": 0.30, "min_gain": 0.03}


def dcn_far_samples(eng, images):
    """Per fused DeformConv layer of the plan for `images`' shape: the kernel's own count of samples per 16x16 tile
    whose corners leave the apron (`h3d_dcn_far_samples`), for the margin-2 apron and for the wide one.
    -> {layer: {"narrow": int32 tensor [tiles], "wide": int32 tensor [tiles]}}.  Runs the plan once (one stream, so
    every layer's input buffer holds real activations), then phase A + geometry of every DeformConv twice."""
    _lib.require_cuda(images)
    if eng.pw.dtype not in LOWP:
        raise RuntimeError("dcn_far_samples: the fused DeformConv variants exist for bf16 / f16 plans")
    B, _, H, W = images.shape
    out = {}
    with torch.cuda.device(eng.device):
        streams, eng.streams = eng.streams, 1          # (_forward_split runs sub-plans: plan(B, H, W) would be left untouched)
        try:
            eng.forward(images)
        finally:
            eng.streams = streams
        plan = eng.plan(B, H, W)
        for p, i in plan.dcn_layers:
            src = plan.ops[i]
            if src.Cin % 32 or src.reserved & _lib.OPF_DCN_STREAM_NO_SLOTS:
                continue
            tiles = B * (-(-src.H // 16)) * (-(-src.W // 16))
            rec = {}
            for name in ("narrow", "wide"):
                op = H3dOp()
                ctypes.memmove(ctypes.byref(op), ctypes.byref(src), ctypes.sizeof(H3dOp))
                op.reserved = DCN_VARIANTS[name] | (src.reserved & DCN_F16IN)
                cnt = torch.empty(tiles, dtype=torch.int32, device=eng.device)
                _lib.check(_lib.lib().h3d_dcn_far_samples(ctypes.byref(op), cnt.data_ptr(), _lib.stream_ptr()), "h3d_dcn_far_samples")
                rec[name] = cnt
            out[p] = rec
        torch.cuda.synchronize()
    return out


def calibrate_dcn_margins(eng, images, rule=None):
    """Choose per fused DeformConv layer among the three tile variants of csrc/dcn3.hip:
      narrow    margin-2 apron, 256 patch slots per tile   (default; fastest while almost no tile overflows)
      slots512  margin-2 packed apron, 512 slots in two rounds per stage
      wide      margin-4 packed apron, 256 slots
    by a RULE on what the kernels themselves count on a calibration batch (`dcn_far_samples`: per tile, the samples
    that leave the apron) -- a deterministic function of (weights, images): two processes make the same choice and
    therefore return the same bits (round 3 timed the variants with HIP events, and where two of them were within 3 %
    the choice, and with it the accumulation order of overflowing tiles, differed from run to run).  Cost per layer in
    units of a normal tile (DCN_RULE): narrow = 1 + pass2 * P(n > 256); slots512 = 1 + c + round2 * P(256 < n <= 512) +
    pass2 * P(n > 512); wide = 1 + c' + pass2 * P(n_wide > 256); a layer leaves `narrow` only for a variant cheaper by
    `min_gain`.  Returns {layer: {"cost": {variant: x}, "tiles_over_256": f, ...}}; the choice lands in `pw.dcn_variant`
    and plans built before the call are dropped."""
    rule = dict(DCN_RULE, **(rule or {}))
    with torch.cuda.device(eng.device):
        eng.pw.dcn_variant = {}
        eng.plans.clear()
        stats = dcn_far_samples(eng, images)
    report = {}
    for p, rec in stats.items():
        n2, n4 = rec["narrow"].float(), rec["wide"].float()
        f256 = float((n2 > 256).float().mean())
        f512 = float((n2 > 512).float().mean())
        w256 = float((n4 > 256).float().mean())
        rounds = _dcn_rounds(eng, p, n2.numel())

        def over(f):                                    # cost of the tiles that run pass 2: their share, or the launch's tail
            return max(rule["pass2"] * f, min(rule["pass2"], rule["tail"] / rounds) if f > 0 else 0.0)
        cost = {"narrow": 1.0 + over(f256),
                "slots512": 1.0 + rule["slots512"] + rule["round2"] * (f256 - f512) + over(f512),
                "wide": 1.0 + rule["wide"] + over(w256)}
        best = min(("narrow", "slots512", "wide"), key=lambda k: (cost[k], k != "narrow"))
        if best != "narrow" and cost[best] < (1.0 - rule["min_gain"]) * cost["narrow"]:
            eng.pw.dcn_variant[p] = DCN_VARIANTS[best]
        else:
            best = "narrow"
        report[p] = {"choice": best, "cost": {k: round(v, 4) for k, v in cost.items()}, "tiles_over_256": round(f256, 5),
                     "tiles_over_512": round(f512, 5), "tiles_over_256_wide": round(w256, 5), "rounds": round(rounds, 3),
                     "far_samples_per_tile": round(float(n2.mean()), 2)}
    eng.plans.clear()
    return report


def _dcn_rounds(eng, p, tiles):
    """Workgroups of DeformConv layer `p` per resident workgroup of the device (csrc/dcn3.hip's launcher: <= 64-channel
    workgroups, two per CU; 128-channel ones, one per CU, unless that grid would leave CUs idle)."""
    cout = int(eng.pw.sd[p + ".conv.weight"].shape[0])
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    if cout <= 64:
        groups, per_cu = 1, 2
    elif tiles * (-(-cout // 128)) < 192:
        groups, per_cu = -(-cout // 64), 2
    else:
        groups, per_cu = -(-cout // 128), 1
    return max(tiles * groups / float(cus * per_cu), 1e-3)


def time_dcn_variants(eng, images, reps=3):
    """Stopwatch counterpart of `calibrate_dcn_margins` (what round 3 used to CHOOSE; now only the yardstick the rule's
    constants are fitted against, tools/fit_dcn_rule.py): every fused DeformConv op of the plan timed `reps` times per
    variant with HIP events (`h3d_run_ops_timed`), median.  Changes nothing.  -> {layer: {variant: ms}}."""
    _lib.require_cuda(images)
    if eng.pw.dtype not in LOWP:
        raise RuntimeError("time_dcn_variants: the fused DeformConv variants exist for bf16 / f16 plans")
    B, _, H, W = images.shape
    with torch.cuda.device(eng.device):
        streams, eng.streams = eng.streams, 1
        try:
            eng.forward(images)
        finally:
            eng.streams = streams
        plan = eng.plan(B, H, W)
        n = len(plan.ops)
        ms = (ctypes.c_float * n)()
        layers = [(p, i) for p, i in plan.dcn_layers if plan.ops[i].Cin % 32 == 0 and not plan.ops[i].reserved & _lib.OPF_DCN_STREAM_NO_SLOTS]
        saved = [plan.op_array[i].reserved for _, i in layers]
        times = {p: {} for p, _ in layers}
        for name, bits in DCN_VARIANTS.items():
            for (_, i), v in zip(layers, saved):
                plan.op_array[i].reserved = bits | (v & DCN_F16IN)
            runs = []
            for _ in range(reps + 1):                       # (first run of a variant: code-object load, dropped)
                _lib.check(_lib.lib().h3d_run_ops_timed(plan.op_array, n, _lib.stream_ptr(), ms), "h3d_run_ops_timed")
                runs.append([ms[i] for _, i in layers])
            runs = list(zip(*runs[1:]))                    # per layer: its `reps` durations
            for (p, _), r in zip(layers, runs):
                times[p][name] = float(sorted(r)[len(r) // 2])
        for (_, i), v in zip(layers, saved):
            plan.op_array[i].reserved = v
        torch.cuda.synchronize()
    return times


def _tiles_over_slots(om, margin, slots):
    """Share of 16x16 tiles of an offset/mask map [B,h,w,>=18] (channel 2t = dh, 2t+1 = dw of tap t) with more than `slots`
    samples whose bilinear corners leave the tile's apron of the given margin -- the test of csrc/dcn3.hip, on the device."""
    Bn, h, w = om.shape[0], om.shape[1], om.shape[2]
    dev = om.device
    ys = torch.arange(h, device=dev, dtype=torch.float32).view(1, h, 1)
    xs = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, w)
    y0, x0 = ys - ys % 16 - 1 - margin, xs - xs % 16 - 1 - margin
    HH = 18 + 2 * margin
    miss = torch.zeros(Bn, h, w, device=dev)
    for t in range(9):
        ti, tj = divmod(t, 3)
        h_im, w_im = ys - 1 + ti + om[..., 2 * t], xs - 1 + tj + om[..., 2 * t + 1]
        inside = (h_im > -1) & (w_im > -1) & (h_im < h) & (w_im < w)
        ry, rx = torch.floor(h_im) - y0, torch.floor(w_im) - x0
        ok = (ry >= 0) & (ry + 1 < HH) & (rx >= 0) & (rx + 1 < HH)
        miss += (inside & ~ok).float()
    th, tw = -(-h // 16), -(-w // 16)
    pad = torch.zeros(Bn, th * 16, tw * 16, device=dev)
    pad[:, :h, :w] = miss
    per_tile = pad.view(Bn, th, 16, tw, 16).sum(dim=(2, 4))
    return (per_tile > slots).float().mean()
