"""Timing aid: deformable PS-ROI pooling forward (csrc/psroi.hip) with HIP events after a warm-up, against the same op written in
torch (sample grid -> F.grid_sample(bilinear, border, align_corners=True) -> validity mask -> mean).  Prints us per call and
samples/s (R * C * P^2 * spp^2 bilinear samples per call), and the largest difference between the two results."""
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

if __name__ == "__main__":
    g = torch.Generator().manual_seed(0)
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
