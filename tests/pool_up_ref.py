"""TEST INFRASTRUCTURE: the yardstick of the max-pool and up-sample + add backward (include/h3d.h section 2d) -- F.max_pool2d(x, 2, 2)
and F.conv_transpose2d(x, w, stride=f, padding=f//2, groups=C) + skip under torch autograd on the CPU, in float64 and float32 -- a numpy
restatement of the header's formulas, and the cases of tests/test_oracle_pool_up.py / tests/test_gpu_pool_up.py."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

TILE = {2: 8, 4: 4, 8: 2}            # csrc/pool_up_bwd.hip UpBwd<f>::TH = TW: input pixels a side of a workgroup's tile


# ---- max-pool ------------------------------------------------------------------------------------------------------------------------------
def pool_yardstick(x, gy, dtype=torch.float64):
    """-> (y, grad_x) of F.max_pool2d(x, 2, 2) on the CPU in `dtype`."""
    xx = x.to(dtype).clone().requires_grad_(True)
    y = F.max_pool2d(xx, 2, 2)
    if y.numel():
        y.backward(gy.to(dtype))
    return y.detach(), xx.grad if xx.grad is not None else torch.zeros_like(xx)


def pool_numpy(x, gy):
    """The header's rule with plain loops: the gradient goes to the first element of the window, in the order (0,0), (0,1), (1,0), (1,1),
    that equals the window's maximum; everything else, the odd last row / column included, is 0."""
    x, gy = np.asarray(x), np.asarray(gy)
    B, C, H, W = x.shape
    gx = np.zeros_like(x)
    y = np.zeros((B, C, H // 2, W // 2), x.dtype)
    for oy in range(H // 2):
        for ox in range(W // 2):
            win = np.stack([x[:, :, 2 * oy + j // 2, 2 * ox + j % 2] for j in range(4)], -1)         # [B,C,4]
            m = win.max(-1)
            at = (win == m[..., None]).argmax(-1)               # the first maximum
            y[:, :, oy, ox] = m
            for j in range(4):
                gx[:, :, 2 * oy + j // 2, 2 * ox + j % 2] = np.where(at == j, gy[:, :, oy, ox], 0)
    return y, gx


def pool_case(shape, seed, ties=True):
    """x from {-1, 0, 1, 2} (most windows tie) or random floats; grad_y random integers in [-8, 8] without zeros."""
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    x = torch.randint(-1, 3, shape, generator=g).float() if ties else torch.randn(shape, generator=g)
    gy = torch.randint(1, 9, (B, C, H // 2, W // 2), generator=g).float() * (torch.randint(0, 2, (B, C, H // 2, W // 2), generator=g) * 2 - 1).float()
    return x, gy


# ---- up-sample + add -------------------------------------------------------------------------------------------------------------------------
def fill_up_weights(C, f):
    """models/model.py:334-343 (fill_up_weights): the bilinear kernel, exact dyadics for f = 2, 4, 8 (unit 1 / (2f)^2)."""
    k = 2 * f
    ff = math.ceil(k / 2)
    c = (2 * ff - 1 - ff % 2) / (2.0 * ff)
    w = torch.zeros(C, 1, k, k, dtype=torch.float64)
    for i in range(k):
        for j in range(k):
            w[:, 0, i, j] = (1 - math.fabs(i / ff - c)) * (1 - math.fabs(j / ff - c))
    return w


def up_yardstick(x, w, skip, gy, f, dtype=torch.float64):
    """-> (y, grad_x, grad_w, grad_skip) of conv_transpose2d(x, w, stride=f, padding=f//2, groups=C) + skip on the CPU in `dtype`."""
    xx, ww, ss = [t.to(dtype).clone().requires_grad_(True) for t in (x, w, skip)]
    y = F.conv_transpose2d(xx, ww, None, stride=f, padding=f // 2, groups=x.shape[1]) + ss
    y.backward(gy.to(dtype))
    return y.detach(), xx.grad, ww.grad, ss.grad


def up_numpy(x, w, gy, f):
    """The header's two formulas, tap by tap (float64): -> (grad_x [B,C,H,W], grad_w [C,1,2f,2f])."""
    x, w, gy = [np.asarray(t, np.float64) for t in (x, w, gy)]
    B, C, H, W = x.shape
    k, p = 2 * f, f // 2
    gx, gw = np.zeros_like(x), np.zeros_like(w)
    for ki in range(k):
        for kj in range(k):
            for iy in range(H):
                oy = iy * f - p + ki
                if not 0 <= oy < H * f:
                    continue
                for ix in range(W):
                    ox = ix * f - p + kj
                    if not 0 <= ox < W * f:
                        continue
                    gx[:, :, iy, ix] += w[None, :, 0, ki, kj] * gy[:, :, oy, ox]
                    gw[:, 0, ki, kj] += (x[:, :, iy, ix] * gy[:, :, oy, ox]).sum(0)
    return gx, gw


# name -> (B, C, H, W, f, channel stride or None)
UP_CASES = {}
for _f in (2, 4, 8):
    _t = TILE[_f]
    UP_CASES.update({
        "f%d_1x4x1x1" % _f: (1, 4, 1, 1, _f, None),
        "f%d_2x8x3x5" % _f: (2, 8, 3, 5, _f, None),
        "f%d_1x64x4x4" % _f: (1, 64, 4, 4, _f, None),
        "f%d_c20_cs24" % _f: (1, 20, 3, 2, _f, 24),
        "f%d_tile_h-1_w+1" % _f: (1, 4, _t - 1, _t + 1, _f, None),
        "f%d_tile_h_w" % _f: (1, 4, _t, _t, _f, None),
        "f%d_tile_h+1_w-1" % _f: (1, 4, _t + 1, max(_t - 1, 1), _f, None),
    })
# more than 64 workgroup slots: the grad_w partials meet in G = 2 chains (f = 8: 65 tiles, 33 rows -> one zeroed slot; f = 2: 5 x 16 tiles)
UP_CASES["f8_chains_65"] = (1, 4, 10, 26, 8, None)
UP_CASES["f2_chains_80"] = (5, 4, 32, 32, 2, None)
LATTICE_CASES = tuple(n for n in UP_CASES if "c20" not in n)


class UpCase:
    def __init__(self, name, lattice=False):
        self.name = name
        self.B, self.C, self.H, self.W, self.f, self.cs = UP_CASES[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)) + (1000 if lattice else 0))
        B, C, H, W, f = self.B, self.C, self.H, self.W, self.f
        if lattice:
            draw = lambda *s: torch.randint(-8, 9, s, generator=g).double()
            self.w = fill_up_weights(C, f)
        else:
            draw = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()
            self.w = (torch.randn(C, 1, 2 * f, 2 * f, generator=g, dtype=torch.float64) / (2 * f)).float().double()
        self.x, self.skip, self.gy = draw(B, C, H, W), draw(B, C, H * f, W * f), draw(B, C, H * f, W * f)

    def run(self, dtype):
        return up_yardstick(self.x, self.w, self.skip, self.gy, self.f, dtype)


@functools.lru_cache(maxsize=None)
def up_case(name, lattice=False):
    return UpCase(name, lattice)


NAMES = ("y", "grad_x", "grad_w", "grad_skip")


@functools.lru_cache(maxsize=None)
def up_bounds(name):
    """-> (float64 results, e32 per tensor = max |float32 run - float64 run| of the yardstick itself)."""
    c = up_case(name)
    r64, r32 = c.run(torch.float64), c.run(torch.float32)
    return r64, tuple(float((a.double() - b).abs().max()) for a, b in zip(r32, r64))


def check(what, got, ref64, e32):
    """The project's rule per tensor: max |g - g64| <= 4 e32 + 1e-7 max |g64|.  -> the largest err / e32 seen."""
    err = float((got.detach().cpu().double() - ref64).abs().max())
    limit = 4 * e32 + 1e-7 * float(ref64.abs().max())
    print("%s: err %.3g e32 %.3g limit %.3g (err / e32 %.2f)" % (what, err, e32, limit, err / e32 if e32 else float("nan")))
    assert err <= limit, what
    return err / e32 if e32 else 0.0


def lattice_abs_sums(c):
    """The sums of the absolute values of every output's terms, in units of the output's grid: below 2^24 no order of summation rounds."""
    a = UpCase.__new__(UpCase)
    a.f, a.x, a.w, a.skip, a.gy = c.f, c.x.abs(), c.w.abs(), c.skip.abs(), c.gy.abs()
    y, gx, gw, _ = up_yardstick(a.x, a.w, a.skip, a.gy, a.f)
    unit = float((2 * c.f) ** 2)
    return {"y": float(y.max()) * unit, "grad_x": float(gx.max()) * unit, "grad_w": float(gw.max())}
