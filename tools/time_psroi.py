"""Timing aid: deformable PS-ROI pooling forward (csrc/psroi.hip) with HIP events after a warm-up, against the same op written in
torch (sample grid -> F.grid_sample(bilinear, border, align_corners=True) -> validity mask -> mean).  Prints us per call and
samples/s (R * C * P^2 * spp^2 bilinear samples per call), and the largest difference between the two results.

--backward: the backward (csrc/psroi_bwd.hip) on the same shapes and modes, against torch autograd through the same composition
(backward pass alone, the graph kept).  Two rows per case: grad_input combined per workgroup in LDS where the geometry allows (the
default) and every contribution its own global atomic (`direct`).  Atomic bytes/s: 4 bytes per global float atomic -- for the direct
form one per valid sample corner and channel, for the combined form one per pixel a roi touches and channel (an upper bound: a tile
pixel whose sum is exactly zero is skipped, a roi whose box is too large or too sparsely sampled falls back to the direct form)."""
import argparse
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
import h3d_amd  # noqa: F401,E402
from h3d_amd import dcn_v2  # noqa: E402

dev = torch.device("cuda:0")


def rand_rois(g, R, B, img):
    x = torch.rand(R, generator=g) * img
    y = torch.rand(R, generator=g) * img
    w = 16 + torch.rand(R, generator=g) * img / 4
    h = 16 + torch.rand(R, generator=g) * img / 4
    return torch.stack([torch.randint(0, B, (R,), generator=g).float(), x, y, x + w, y + h], 1)


def atomic_counts(inp, rois, offset, scale, P, spp, tstd):
    """(valid sample corners, pixels touched) summed over the rois, per channel."""
    B, C, H, W = inp.shape
    R = rois.shape[0]
    rnd = lambda v: torch.sign(v) * torch.floor(v.abs() + 0.5)
    sw, sh = rnd(rois[:, 1]) * scale - 0.5, rnd(rois[:, 2]) * scale - 0.5
    rw = ((rnd(rois[:, 3]) + 1) * scale - 0.5 - sw).clamp_min(0.1)
    rh = ((rnd(rois[:, 4]) + 1) * scale - 0.5 - sh).clamp_min(0.1)
    p = torch.arange(P, device=inp.device, dtype=torch.float32)
    s = torch.arange(spp, device=inp.device, dtype=torch.float32)
    tx = offset[:, 0] * tstd if offset is not None else torch.zeros(R, P, P, device=inp.device)
    ty = offset[:, 1] * tstd if offset is not None else torch.zeros(R, P, P, device=inp.device)
    w = (p.view(1, 1, P) * (rw / P).view(R, 1, 1) + sw.view(R, 1, 1) + tx * rw.view(R, 1, 1)).view(R, P, 1, P, 1) \
        + s.view(1, 1, 1, 1, spp) * (rw / P / spp).view(R, 1, 1, 1, 1)
    h = (p.view(1, P, 1) * (rh / P).view(R, 1, 1) + sh.view(R, 1, 1) + ty * rh.view(R, 1, 1)).view(R, P, 1, P, 1) \
        + s.view(1, 1, spp, 1, 1) * (rh / P / spp).view(R, 1, 1, 1, 1)
    w, h = torch.broadcast_tensors(w, h)
    valid = (w >= -0.5) & (w <= W - 0.5) & (h >= -0.5) & (h <= H - 0.5)
    w, h = w.clamp(0, W - 1), h.clamp(0, H - 1)
    x0, y0 = w.floor().long(), h.floor().long()
    fx, fy = (w > x0).long(), (h > y0).long()
    corners = int(((1 + fx) * (1 + fy))[valid].sum())
    touched = torch.zeros(R, H * W + W + 2, dtype=torch.bool, device=inp.device)
    r = torch.arange(R, device=inp.device).view(R, 1, 1, 1, 1).expand_as(x0)
    for dy in (0, 1):
        for dx in (0, 1):
            m = valid & ((fx >= dx) & (fy >= dy))
            touched[r[m], ((y0 + dy) * W + x0 + dx)[m]] = True
    return corners, int(touched.sum())


def torch_psroi(inp, rois, offset, scale, P, spp, tstd, mask=None):
    """The op in torch (one class, part_size == P): [R, C, P, P]."""
    B, C, H, W = inp.shape
    R = rois.shape[0]
    rnd = lambda v: torch.sign(v) * torch.floor(v.abs() + 0.5)
    sw, sh = rnd(rois[:, 1]) * scale - 0.5, rnd(rois[:, 2]) * scale - 0.5
    rw = ((rnd(rois[:, 3]) + 1) * scale - 0.5 - sw).clamp_min(0.1)
    rh = ((rnd(rois[:, 4]) + 1) * scale - 0.5 - sh).clamp_min(0.1)
    p = torch.arange(P, device=inp.device, dtype=torch.float32)
    s = torch.arange(spp, device=inp.device, dtype=torch.float32)
    tx = offset[:, 0] * tstd if offset is not None else torch.zeros(R, P, P, device=inp.device)
    ty = offset[:, 1] * tstd if offset is not None else torch.zeros(R, P, P, device=inp.device)
    # [R, ph, ih, pw, iw]
    w = (p.view(1, 1, P) * (rw / P).view(R, 1, 1) + sw.view(R, 1, 1) + tx * rw.view(R, 1, 1)).view(R, P, 1, P, 1) \
        + s.view(1, 1, 1, 1, spp) * (rw / P / spp).view(R, 1, 1, 1, 1)
    h = (p.view(1, P, 1) * (rh / P).view(R, 1, 1) + sh.view(R, 1, 1) + ty * rh.view(R, 1, 1)).view(R, P, 1, P, 1) \
        + s.view(1, 1, spp, 1, 1) * (rh / P / spp).view(R, 1, 1, 1, 1)
    w, h = torch.broadcast_tensors(w, h)
    valid = ((w >= -0.5) & (w <= W - 0.5) & (h >= -0.5) & (h <= H - 0.5)).float()
    grid = torch.stack([w.clamp(0, W - 1) / max(W - 1, 1) * 2 - 1, h.clamp(0, H - 1) / max(H - 1, 1) * 2 - 1], -1)
    out = torch.zeros(R, C, P, P, device=inp.device)
    b = rois[:, 0].long()
    for i in range(B):
        sel = (b == i).nonzero().flatten()
        if sel.numel() == 0:
            continue
        n = sel.numel()
        v = F.grid_sample(inp[i:i + 1], grid[sel].reshape(1, n * P * spp, P * spp, 2), mode="bilinear", padding_mode="border",
                          align_corners=True).view(C, n, P, spp, P, spp)
        m = valid[sel].view(1, n, P, spp, P, spp)
        cnt = m.sum((3, 5))
        o = ((v * m).sum((3, 5)) / cnt.clamp_min(1)).permute(1, 0, 2, 3)
        out[sel] = o
    if mask is not None:
        out = out * torch.sigmoid(mask)
    return out


def timed(fn, warm=5, iters=20):
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


SHAPES = [  # name, B, C, H, R, spatial_scale
    ("reference example", 2, 32, 64, 20, 1 / 4),
    ("R-FCN head R300", 2, 256, 64, 300, 1 / 16),
    ("R-FCN head R2000", 2, 256, 64, 2000, 1 / 16),
    ("B8 128^2 R1000", 8, 256, 128, 1000, 1 / 16),
]
P, SPP, TSTD = 7, 4, 0.1

def backward_table(g):
    print("%-20s %-9s %-9s %11s %12s %13s %11s %9s %10s" % ("shape", "mode", "path", "HIP us", "Gsamples/s", "atomic GB/s", "torch us", "speed-up",
                                                          "max|diff|"))
    for name, B, C, H, R, scale in SHAPES:
        inp = torch.randn(B, C, H, H, generator=g).to(dev)
        rois = rand_rois(g, R, B, H / scale).to(dev)
        om = (torch.randn(R, 3, P, P, generator=g) * 0.5).to(dev)
        off = om[:, :2].contiguous()
        go = torch.randn(R, C, P, P, generator=g).to(dev)
        samples = R * C * P * P * SPP * SPP
        with torch.no_grad():
            _, cnt0 = dcn_v2.dcn_v2_psroi_pooling_forward(inp, rois, inp.new(), 1, scale, C, 1, P, P, SPP, TSTD)
            _, cnt1 = dcn_v2.dcn_v2_psroi_pooling_forward(inp, rois, off, 0, scale, C, 1, P, P, SPP, TSTD)
        for mode in ("no_trans", "trans", "masked"):
            x = inp.clone().requires_grad_(True)
            o = None if mode == "no_trans" else om.clone().requires_grad_(True)
            out = torch_psroi(x, rois, None if o is None else o[:, :2], scale, P, SPP, TSTD, o[:, 2:] if mode == "masked" else None)
            leaves = [x] if o is None else [x, o]
            ref = lambda: torch.autograd.grad(out, leaves, go, retain_graph=True)
            corners, touched = atomic_counts(inp, rois, None if o is None else off, scale, P, SPP, TSTD)
            for path, direct in (("combined", False), ("direct", True)):
                if mode == "no_trans":
                    hip = lambda: dcn_v2._dcn_v2_psroi_pooling_backward(go, inp, rois, inp.new(), cnt0, 1, scale, C, 1, P, P, SPP, TSTD,
                                                                        need=(True, False), direct=direct)
                elif mode == "trans":
                    hip = lambda: dcn_v2._dcn_v2_psroi_pooling_backward(go, inp, rois, off, cnt1, 0, scale, C, 1, P, P, SPP, TSTD, direct=direct)
                else:
                    hip = lambda: dcn_v2._dcn_pooling_modulated_backward(go, inp, rois, om, scale, P, C, 1, P, SPP, TSTD, direct=direct)
                got, want = hip(), ref()
                diff = (got[0] - want[0]).abs().max().item()
                if mode == "trans":
                    diff = max(diff, (got[1] - want[1][:, :2]).abs().max().item())
                elif mode == "masked":
                    diff = max(diff, (got[1] - want[1]).abs().max().item())
                th, tt = timed(hip), timed(ref)
                abytes = 4.0 * C * (corners if direct else touched)
                print("%-20s %-9s %-9s %11.1f %12.1f %13.1f %11.1f %8.1fx %10.2e" % (name, mode, path, th, samples / th / 1e3, abytes / th / 1e3, tt,
                                                                                 tt / th, diff))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--backward", action="store_true", help="time the backward instead of the forward")
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    if args.backward:
        backward_table(g)
        sys.exit(0)
    print("%-20s %-9s %11s %12s %11s %9s %10s" % ("shape", "mode", "HIP us", "Gsamples/s", "torch us", "speed-up", "max|diff|"))
    with torch.no_grad():
        for name, B, C, H, R, scale in SHAPES:
            inp = torch.randn(B, C, H, H, generator=g).to(dev)
            rois = rand_rois(g, R, B, H / scale).to(dev)
            om = (torch.randn(R, 3, P, P, generator=g) * 0.5).to(dev)
            off = om[:, :2].contiguous()
            samples = R * C * P * P * SPP * SPP
            modes = [
                ("no_trans", lambda: dcn_v2.dcn_v2_psroi_pooling_forward(inp, rois, inp.new(), 1, scale, C, 1, P, P, SPP, TSTD)[0],
                 lambda: torch_psroi(inp, rois, None, scale, P, SPP, TSTD)),
                ("trans", lambda: dcn_v2.dcn_v2_psroi_pooling_forward(inp, rois, off, 0, scale, C, 1, P, P, SPP, TSTD)[0],
                 lambda: torch_psroi(inp, rois, off, scale, P, SPP, TSTD)),
                ("masked", lambda: dcn_v2._dcn_pooling_modulated(inp, rois, om, scale, P, C, 1, P, SPP, TSTD),
                 lambda: torch_psroi(inp, rois, om[:, :2], scale, P, SPP, TSTD, om[:, 2:])),
            ]
            for mode, hip, ref in modes:
                diff = (hip() - ref()).abs().max().item()
                th, tt = timed(hip), timed(ref)
                print("%-20s %-9s %11.1f %12.1f %11.1f %8.1fx %10.2e" % (name, mode, th, samples / th / 1e3, tt, tt / th, diff))
