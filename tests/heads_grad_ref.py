"""Yardstick of the heads backward (csrc/heads_bwd.hip): the heads restated in torch -- F.conv2d(padding=1) -> relu -> F.conv2d, the
reference's nn.Conv2d modules (models/model.py:451-464, 485-489) -- differentiated by torch autograd on the CPU.

The ReLU gate: a pre-activation within rounding distance of 0 may be gated differently by two correct summation orders, which changes
a gradient by a whole term.  The generated cases are GRIDDED so that this cannot happen: y in multiples of 2^-4 in [-2, 2], W1 in
multiples of 2^-6 in [-1, 1], b1 in ODD multiples of 2^-11 in (-1, 1).  Every partial sum of pre = conv3x3(y, W1) + b1 is then a
multiple of 2^-11 below 2^11 (576 products of at most 2 + 1): exact in fp32 in any order, and never 0.  gz, W2 and b2 are ordinary random
floats, so rounding is exercised in all four gradient contractions.  One extra case is ungridded (`make_random_case`): its seed is
searched on the CPU until min |pre64| >= 1e-3 max |pre64|."""
import functools

import torch
import torch.nn.functional as F

NAMES = ("grad_feat", "grad_w1", "grad_b1", "grad_w2", "grad_b2")
SPLIT_PIXELS = 512       # the split length csrc/heads_bwd.hip states (HB_SPLIT_PIXELS): B*H*W <= 512 is one split, 513 is two


def pre_act(y, w1, b1):
    return F.conv2d(y, w1, b1, padding=1)


def forward(y, w1, b1, w2, b2):
    """y [B,Cin,H,W], w1 [hc,Cin,3,3], b1 [hc], w2 [C,hc], b2 [C] -> z [B,C,H,W]"""
    return F.conv2d(torch.relu(pre_act(y, w1, b1)), w2.reshape(w2.shape[0], w2.shape[1], 1, 1), b2)


def grads(y, w1, b1, w2, b2, gz, dtype=torch.float64):
    """(grad_feat, grad_w1, grad_b1, grad_w2, grad_b2) of sum(forward * gz), all operands cast to `dtype` on the CPU."""
    leaves = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in (y, w1, b1, w2, b2)]
    return torch.autograd.grad(forward(*leaves), leaves, gz.detach().cpu().to(dtype))


def make_case(seed, B, H, W, hc, C, cin=64):
    """Gridded (y, w1, b1, w2, b2, gz), float32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(-32, 33, (B, cin, H, W), generator=g).float() / 16.0
    w1 = torch.randint(-64, 65, (hc, cin, 3, 3), generator=g).float() / 64.0
    b1 = (2 * torch.randint(-1024, 1024, (hc,), generator=g) + 1).float() / 2048.0
    w2 = torch.randn(C, hc, generator=g) * 0.1
    b2 = torch.randn(C, generator=g)
    gz = torch.randn(B, C, H, W, generator=g)
    return y, w1, b1, w2, b2, gz


def make_random_case(seed=0, B=1, H=4, W=4, hc=64, C=3, tries=2000):
    """Ungridded random data whose gate has a margin: the first seed from `seed` on with min |pre64| >= 1e-3 max |pre64| (a bounded
    search on the CPU; the margin is asserted by the caller too)."""
    for s in range(seed, seed + tries):
        g = torch.Generator().manual_seed(s)
        y = torch.randn(B, 64, H, W, generator=g)
        w1 = torch.randn(hc, 64, 3, 3, generator=g) * 0.05
        b1 = torch.randn(hc, generator=g) * 0.1
        p = pre_act(y.double(), w1.double(), b1.double()).abs()
        if float(p.min()) >= 1e-3 * float(p.max()):
            w2 = torch.randn(C, hc, generator=g) * 0.1
            return y, w1, b1, w2, torch.randn(C, generator=g), torch.randn(B, C, H, W, generator=g)
    raise AssertionError("no seed with a gate margin in %d tries" % tries)


def gate_margin(case):
    p = pre_act(case[0].double(), case[1].double(), case[2].double()).abs()
    return float(p.min()), float(p.max())


# name -> (seed, B, H, W, head_conv, C): the smallest shapes at which tiling (4 x 32 pixel tiles), halo and split edges can go wrong
_SHAPES = ((1, 5, 7), (2, 9, 33), (1, 17, 40))
CASES = {}
for _i, _c in enumerate((1, 2, 3, 34, 72, 96)):
    CASES["c%d_hc64" % _c] = (100 + _i, *_SHAPES[_i % 3], 64, _c)
    CASES["c%d_hc256" % _c] = (200 + _i, *_SHAPES[(_i + 1) % 3], 256, _c)
CASES["split_512"] = (300, 1, 16, 32, 64, 3)         # exactly one split
CASES["split_513"] = (301, 1, 19, 27, 64, 3)         # one pixel over: two splits
CASES["split_511"] = (302, 1, 7, 73, 64, 34)
MODEL_CASES = {"model_c1": (400, 1, 128, 128, 256, 1), "model_c34": (401, 1, 128, 128, 256, 34)}


@functools.lru_cache(maxsize=None)
def case(name):
    return make_case(*(CASES.get(name) or MODEL_CASES[name]))


@functools.lru_cache(maxsize=None)
def bounds(name):
    """(g64, e32) of a named case: e32 = max |g32 - g64| per tensor, the error of the SAME autograd run in float32.  Computed once."""
    return bounds_of(case(name))


def bounds_of(c):
    g64 = grads(*c, dtype=torch.float64)
    g32 = grads(*c, dtype=torch.float32)
    return g64, [float((a.double() - r).abs().max()) for a, r in zip(g32, g64)]


def check(name, got, g64, e32, factor=4.0):
    """The rule of every comparison: max |g - g64| <= factor * e32 + 1e-7 * max |g64|, per tensor; returns the observed ratios.
    `got` follows NAMES; grad_feat may come as [B,64,H,W] (any strides); None entries are skipped."""
    ratios, fails = {}, []
    for nm, g, r, e in zip(NAMES, got, g64, e32):
        if g is None:
            continue
        g = g.detach().cpu().double().reshape(r.shape)
        err = float((g - r).abs().max())
        limit = factor * e + 1e-7 * float(r.abs().max())
        ratios[nm] = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s: err %.3g e32 %.3g ratio %.3g limit %.3g max|g64| %.3g" % (name, nm, err, e, ratios[nm], limit, float(r.abs().max())))
        if not err <= limit:
            fails.append((nm, err, limit))
    assert not fails, (name, fails)
    return ratios
