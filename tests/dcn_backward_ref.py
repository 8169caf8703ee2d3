"""TEST INFRASTRUCTURE ONLY -- the oracle of dcn_v2_backward: torch autograd over oracle/dcn.py's `dcn_v2_forward` (written in
differentiable torch ops: floor, gather, where), in fp64 for the value and in fp32 for the yardstick of the comparison; plus the case
builders shared by tests/test_oracle_dcn_backward.py and tests/test_gpu_dcn_backward.py."""
import torch

from oracle import dcn as odcn

NAMES = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


def out_size(H, W, k, s, p, d):
    return (H + 2 * p - (d * (k[0] - 1) + 1)) // s + 1, (W + 2 * p - (d * (k[1] - 1) + 1)) // s + 1


def forward(x, w, b, off, m, k, s, p, d, dg):
    return odcn.dcn_v2_forward(x, w, b, off, m, k[0], k[1], s, s, p, p, d, d, dg)


def oracle_grads(x, w, b, off, m, go, k, s, p, d, dg, dtype=torch.float64):
    """(grad_input, grad_offset, grad_mask, grad_weight, grad_bias) of sum(forward * go), all operands cast to `dtype` on the CPU."""
    leaves = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in (x, off, m, w, b)]
    out = forward(leaves[0], leaves[3], leaves[4], leaves[1], leaves[2], k, s, p, d, dg)
    return torch.autograd.grad(out, leaves, go.detach().cpu().to(dtype))


def make_offsets(gen, B, dg, k, Ho, Wo, int_range=4, outside=0.0, far=100.0, fraction=True):
    """Offsets = integer part in [-int_range, int_range] + fraction in [0.05, 0.95] (no sampling position within 0.05 of an integer: the
    unperturbed positions are integers), a share `outside` of the entries pushed `far` away (past the gate); fraction=False: integers."""
    shape = (B, 2 * dg * k[0] * k[1], Ho, Wo)
    off = torch.randint(-int_range, int_range + 1, shape, generator=gen).float()
    if fraction:
        off = off + (0.05 + 0.9 * torch.rand(shape, generator=gen))
    if outside > 0:
        push = torch.rand(shape, generator=gen) < outside
        sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
        off = torch.where(push, off + sign * far, off)
    return off


def make_case(seed, B, C, Co, H, W, k=(3, 3), s=1, p=1, d=1, dg=1, int_range=4, outside=0.1, fraction=True):
    gen = torch.Generator().manual_seed(seed)
    Ho, Wo = out_size(H, W, k, s, p, d)
    x = torch.rand(B, C, H, W, generator=gen) * 2 - 1
    w = (torch.rand(Co, C, k[0], k[1], generator=gen) * 2 - 1) * (1.5 / (C * k[0] * k[1]) ** 0.5)
    b = torch.rand(Co, generator=gen) * 2 - 1
    off = make_offsets(gen, B, dg, k, Ho, Wo, int_range, outside, far=float(H + W + 8), fraction=fraction)
    m = torch.rand(B, dg * k[0] * k[1], Ho, Wo, generator=gen)
    go = torch.rand(B, Co, Ho, Wo, generator=gen) * 2 - 1
    return x, w, b, off, m, go


def bounds(x, w, b, off, m, go, k, s, p, d, dg):
    """Per gradient tensor: (g64, e32) with e32 = max |g32 - g64|, the error of the SAME autograd run of the oracle in float32."""
    g64 = oracle_grads(x, w, b, off, m, go, k, s, p, d, dg, torch.float64)
    g32 = oracle_grads(x, w, b, off, m, go, k, s, p, d, dg, torch.float32)
    return g64, [float((a.double() - r).abs().max()) for a, r in zip(g32, g64)]


def check(name, got, g64, e32, factor=4.0):
    """The rule of the comparison: max |g - g64| <= factor * e32 + 1e-7 * max |g64|, per tensor; returns the observed ratios."""
    ratios = {}
    fails = []
    for nm, g, r, e in zip(NAMES, got, g64, e32):
        if g is None:
            continue
        err = float((g.detach().cpu().double() - r).abs().max())
        limit = factor * e + 1e-7 * float(r.abs().max())
        ratios[nm] = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s: err %.3g e32 %.3g ratio %.3g limit %.3g max|g64| %.3g" % (name, nm, err, e, ratios[nm], limit, float(r.abs().max())))
        if not err <= limit:
            fails.append((nm, err, limit))
    assert not fails, (name, fails)
    return ratios
