"""Yardstick of the convolution backward (csrc/conv_bwd.hip): y = act(F.conv2d(x, W, b) (+ res)) -- the reference's convs are nn.Conv2d
modules, so this IS the reference -- differentiated by torch autograd on the CPU, in float64 and in float32.

The ReLU gate: a pre-activation within rounding distance of 0 may be gated differently by two correct summation orders, which changes
a gradient by a whole term.  The gated cases are GRIDDED so that this cannot happen: x and res in multiples of 2^-4 in [-2, 2], W in
multiples of 2^-6 in [-1, 1], b in ODD multiples of 2^-11 in (-1, 1).  Every partial sum of pre = conv2d(x, W) + b + res is then a
multiple of 2^-11 and, as long as taps * C * 2 + 3 < 2^13 (`pre_bound`, asserted per case by the CPU test), below 2^13: exact in fp32
in any order, and never 0.  grad_y is ordinary random floats, so rounding is exercised in every gradient contraction.  One extra case
is ungridded (`make_random_case`): its seed is searched on the CPU until min |pre64| >= 1e-3 max |pre64|."""
import functools

import torch
import torch.nn.functional as F

NAMES = ("grad_x", "grad_res", "grad_weight", "grad_bias")
SPLIT_PIXELS = 512       # the split length csrc/conv_bwd.hip states (CB_SPLIT_PIXELS): B*Ho*Wo <= 512 is one split, 513 is two


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_size(H, W, k, stride, padding, dilation):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(k), _pair(stride), _pair(padding), _pair(dilation)
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def pre_act(x, w, b, res, stride, padding, dilation):
    p = F.conv2d(x, w, b, stride, padding, dilation)
    return p if res is None else p + res


def forward(x, w, b, res, stride, padding, dilation, relu):
    p = pre_act(x, w, b, res, stride, padding, dilation)
    return torch.relu(p) if relu else p


class Case:
    """x, w, b, res (or None), gy: float32 on the CPU; the geometry; relu."""

    def __init__(self, x, w, b, res, gy, stride, padding, dilation, relu):
        self.x, self.w, self.b, self.res, self.gy = x, w, b, res, gy
        self.stride, self.padding, self.dilation, self.relu = _pair(stride), _pair(padding), _pair(dilation), relu

    def y(self, dtype=torch.float32):
        c = lambda t: None if t is None else t.to(dtype)
        return forward(c(self.x), c(self.w), c(self.b), c(self.res), self.stride, self.padding, self.dilation, self.relu)

    def pre(self, dtype=torch.float64):
        c = lambda t: None if t is None else t.to(dtype)
        return pre_act(c(self.x), c(self.w), c(self.b), c(self.res), self.stride, self.padding, self.dilation)

    def pre_bound(self):
        """An upper bound of every partial sum of the pre-activation of a gridded case."""
        return self.w.shape[1] * self.w.shape[2] * self.w.shape[3] * 2 + 3


def grads(c, dtype=torch.float64):
    """(grad_x, grad_res or None, grad_weight, grad_bias) of sum(forward * gy), all operands cast to `dtype` on the CPU."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (c.x, c.w, c.b)]
    res = None if c.res is None else c.res.detach().to(dtype).clone().requires_grad_(True)
    y = forward(leaves[0], leaves[1], leaves[2], res, c.stride, c.padding, c.dilation, c.relu)
    g = torch.autograd.grad(y, leaves + ([] if res is None else [res]), c.gy.to(dtype))
    return g[0], (None if res is None else g[3]), g[1], g[2]


def make_case(seed, B, H, W, C, Cout, k=3, stride=1, padding=1, dilation=1, res=False, relu=False, int_gy=False):
    """Gridded (see the module docstring).  int_gy: grad_y is integers in [-8, 8] instead of random floats -- with the gridded x, w, b and
    res every gradient is then a sum of multiples of 2^-6 (grad_x), 2^-4 (grad_weight) or 1 (grad_res, grad_bias) far below 2^24 of them:
    exact in fp32 in any split order, so the kernels are compared with torch.equal (`INT_GY_CASES`)."""
    g = torch.Generator().manual_seed(seed)
    kh, kw = _pair(k)
    Ho, Wo = out_size(H, W, k, stride, padding, dilation)
    x = torch.randint(-32, 33, (B, C, H, W), generator=g).float() / 16.0
    w = torch.randint(-64, 65, (Cout, C, kh, kw), generator=g).float() / 64.0
    b = (2 * torch.randint(-1024, 1024, (Cout,), generator=g) + 1).float() / 2048.0
    r = torch.randint(-32, 33, (B, Cout, Ho, Wo), generator=g).float() / 16.0 if res else None
    gy = torch.randint(-8, 9, (B, Cout, Ho, Wo), generator=g).float() if int_gy else torch.randn(B, Cout, Ho, Wo, generator=g)
    return Case(x, w, b, r, gy, stride, padding, dilation, relu)


def make_random_case(seed=0, B=1, H=6, W=7, C=16, Cout=16, tries=4000):
    """Ungridded random data (3x3 s1 p1, residual, ReLU) whose gate has a margin: the first seed from `seed` on with
    min |pre64| >= 1e-3 max |pre64| (a bounded search on the CPU; the margin is asserted by the caller too)."""
    for s in range(seed, seed + tries):
        g = torch.Generator().manual_seed(s)
        x = torch.randn(B, C, H, W, generator=g)
        w = torch.randn(Cout, C, 3, 3, generator=g) * 0.1
        b = torch.randn(Cout, generator=g) * 0.1
        r = torch.randn(B, Cout, H, W, generator=g)
        c = Case(x, w, b, r, torch.randn(B, Cout, H, W, generator=g), 1, 1, 1, True)
        p = c.pre().abs()
        if float(p.min()) >= 1e-3 * float(p.max()):
            return c
    raise AssertionError("no seed with a gate margin in %d tries" % tries)


# name -> make_case arguments.  The smallest shapes at which tiling (4 x 32 pixel tiles, 64 / 32 channel tiles, 64-channel chunks), halo,
# parity and split edges can go wrong.
_SHAPES = ((1, 5, 7), (2, 9, 33), (1, 17, 40))
_CHANNELS = ((16, 16), (16, 32), (48, 80), (32, 144), (128, 64))
CASES = {}
_seed = 1000
for _s in _SHAPES:
    for _c, _co in _CHANNELS:
        for _res in (False, True):
            for _relu in (False, True):
                _seed += 1
                CASES["s1_%dx%dx%d_%dto%d%s%s" % (*_s, _c, _co, "_res" if _res else "", "_relu" if _relu else "")] = dict(
                    seed=_seed, B=_s[0], H=_s[1], W=_s[2], C=_c, Cout=_co, res=_res, relu=_relu)
for _h, _w in ((8, 10), (7, 10), (8, 9), (7, 9)):
    for _c, _co in ((16, 32), (48, 80)):
        _seed += 1
        CASES["s2_%dx%d_%dto%d" % (_h, _w, _c, _co)] = dict(seed=_seed, B=2, H=_h, W=_w, C=_c, Cout=_co, stride=2, res=True, relu=True)
CASES["k1_80to48"] = dict(seed=1201, B=2, H=9, W=33, C=80, Cout=48, k=1, padding=0, res=True, relu=True)
CASES["k1_448to64"] = dict(seed=1202, B=1, H=5, W=7, C=448, Cout=64, k=1, padding=0, res=False, relu=True)
CASES["split_511"] = dict(seed=1301, B=1, H=7, W=73, C=16, Cout=32, res=True, relu=True)           # one pixel short of a split
CASES["split_512"] = dict(seed=1302, B=1, H=16, W=32, C=16, Cout=32, res=True, relu=True)          # exactly one split
CASES["split_513"] = dict(seed=1303, B=1, H=19, W=27, C=16, Cout=32, res=True, relu=True)          # one pixel over: two splits
CASES["model_64to64"] = dict(seed=1401, B=1, H=128, W=128, C=64, Cout=64, res=True, relu=True)
MFMA_CASES = tuple(CASES)
GENERAL_CASES = {
    "g_stem7x7": dict(seed=1501, B=1, H=11, W=13, C=3, Cout=16, k=7, padding=3, relu=True),
    "g_3x3_d2": dict(seed=1502, B=2, H=9, W=11, C=8, Cout=12, dilation=2, padding=2, res=True, relu=True),
    "g_3x3_p0": dict(seed=1503, B=1, H=9, W=11, C=16, Cout=16, padding=0, relu=False),
    "g_1x1_s2": dict(seed=1504, B=2, H=9, W=10, C=16, Cout=32, k=1, stride=2, padding=0, res=True, relu=True),
    "g_5x3": dict(seed=1505, B=2, H=11, W=9, C=5, Cout=7, k=(5, 3), stride=(2, 1), padding=(2, 0), res=True, relu=True),
}
CASES.update(GENERAL_CASES)
# the matrix-core configurations `_general` is also run on
GENERAL_ON_MFMA = ("s1_2x9x33_48to80_res_relu", "s2_7x9_48to80")


# the cases that also run with an integer grad_y, bit for bit against the float64 autograd result
INT_GY_CASES = ("s1_2x9x33_48to80_res_relu", "s1_1x17x40_32to144_res_relu", "s2_7x9_48to80", "s2_8x10_16to32", "k1_448to64", "split_513",
                "model_64to64", "g_stem7x7", "g_5x3")


@functools.lru_cache(maxsize=None)
def case(name):
    return make_case(**CASES[name])


@functools.lru_cache(maxsize=None)
def int_gy_case(name):
    return make_case(int_gy=True, **CASES[name])


@functools.lru_cache(maxsize=None)
def int_gy_exact(name):
    """(grad_x, grad_res or None, grad_weight, grad_bias) of `int_gy_case(name)` from float64 autograd, cast to float32 (no rounding
    happens: tests/test_oracle_conv_backward.py asserts that float32 autograd gives the same bits).  Computed once."""
    return tuple(None if t is None else t.float() for t in grads(int_gy_case(name), torch.float64))


@functools.lru_cache(maxsize=None)
def bounds(name):
    """(g64, e32) of a named case: e32 = max |g32 - g64| per tensor, the error of the SAME autograd run in float32.  Computed once."""
    return bounds_of(case(name))


def bounds_of(c):
    g64 = grads(c, torch.float64)
    g32 = grads(c, torch.float32)
    return g64, [None if r is None else float((a.double() - r).abs().max()) for a, r in zip(g32, g64)]


def check(name, got, g64, e32, factor=4.0):
    """The rule of every comparison: max |g - g64| <= factor * e32 + 1e-7 * max |g64|, per tensor; returns the observed ratios.
    `got` follows NAMES; None entries (and tensors the yardstick does not have) are skipped."""
    ratios, fails = {}, []
    for nm, g, r, e in zip(NAMES, got, g64, e32):
        if g is None or r is None:
            continue
        g = g.detach().cpu().double()
        assert g.shape == r.shape, (name, nm, g.shape, r.shape)
        err = float((g - r).abs().max())
        limit = factor * e + 1e-7 * float(r.abs().max())
        ratios[nm] = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s: err %.3g e32 %.3g ratio %.3g limit %.3g max|g64| %.3g" % (name, nm, err, e, ratios[nm], limit, float(r.abs().max())))
        if not err <= limit:
            fails.append((nm, err, limit))
    assert not fails, (name, fails)
    return ratios


# ---- the operator restated on NHWC arrays the way csrc/conv_bwd.hip defines it (gather form), for the known answers on the CPU ----------
def gather_grads(c):
    """grad_x / grad_res / grad_weight / grad_bias from the definitions of include/h3d.h section 2c in float64, with plain loops over the taps
    (no autograd, no F.conv2d backward): gg = gy * [y > 0]; grad_x in gather form; grad_W as a pixel contraction."""
    x, w, gy = c.x.double(), c.w.double(), c.gy.double()
    gg = gy * (c.y(torch.float64) > 0) if c.relu else gy
    B, C, H, W = x.shape
    Cout, _, kh, kw = w.shape
    (sh, sw), (ph, pw), (dh, dw) = c.stride, c.padding, c.dilation
    Ho, Wo = gg.shape[2:]
    gx = torch.zeros_like(x)
    gw = torch.zeros_like(w)
    xp = F.pad(x, (pw, pw, ph, ph))
    gxp = torch.zeros_like(xp)
    for ty in range(kh):
        for tx in range(kw):
            ys, xs = ty * dh, tx * dw
            win = xp[:, :, ys:ys + (Ho - 1) * sh + 1:sh, xs:xs + (Wo - 1) * sw + 1:sw]            # x[c, px*s + t*d - p]
            gw[:, :, ty, tx] = torch.einsum("bohw,bchw->oc", gg, win)
            gxp[:, :, ys:ys + (Ho - 1) * sh + 1:sh, xs:xs + (Wo - 1) * sw + 1:sw] += torch.einsum("oc,bohw->bchw", w[:, :, ty, tx], gg)
    gx = gxp[:, :, ph:ph + H, pw:pw + W]
    return gx, (gg if c.res is not None else None), gw, gg.sum((0, 2, 3))


def known_answer_cases():
    """(what, Case, check(grads: grad_x, grad_res, grad_weight, grad_bias as float64 cpu tensors)): answers that do not depend on the yardstick,
    checked on the CPU for the restatement and on the GPU for the kernels."""
    g = torch.Generator().manual_seed(5)
    out = []
    # a 1x1 identity filter: grad_x == grad_y exactly
    eye = torch.eye(16).reshape(16, 16, 1, 1)
    c = Case(torch.randn(2, 16, 5, 7, generator=g), eye, torch.zeros(16), None, torch.randn(2, 16, 5, 7, generator=g), 1, 0, 1, False)
    out.append(("identity", c, lambda gr, c=c: torch.equal(gr[0], c.gy.double())))
    # grad_b is the plain sum of grad_y (integers: exact in any order)
    gy = torch.randint(-8, 9, (2, 32, 9, 11), generator=g).float()
    c = Case(torch.randn(2, 16, 9, 11, generator=g), torch.randn(32, 16, 3, 3, generator=g), torch.zeros(32), None, gy, 1, 1, 1, False)
    out.append(("bias_sum", c, lambda gr, c=c: torch.equal(gr[3], c.gy.double().sum((0, 2, 3)))))
    # a one-hot image: grad_W[o, c0, ty, tx] = grad_y[o, y0 + 1 - ty, x0 + 1 - tx], zero for the other input channels
    x = torch.zeros(1, 16, 6, 8)
    x[0, 3, 2, 5] = 1.0
    c = Case(x, torch.randn(16, 16, 3, 3, generator=g), torch.zeros(16), None, torch.randn(1, 16, 6, 8, generator=g), 1, 1, 1, False)

    def one_hot(gr, c=c):
        want = torch.zeros(16, 16, 3, 3, dtype=torch.float64)
        for ty in range(3):
            for tx in range(3):
                want[:, 3, ty, tx] = c.gy[0, :, 2 + 1 - ty, 5 + 1 - tx].double()
        return torch.equal(gr[2], want)
    out.append(("one_hot", c, one_hot))
    # 1x1 stride 2: the input pixels with an odd coordinate meet no tap; grad_x is exactly 0 there
    c = Case(torch.randn(2, 16, 7, 8, generator=g), torch.randn(32, 16, 1, 1, generator=g), torch.zeros(32), None,
               torch.randn(2, 32, 4, 4, generator=g), 2, 0, 1, False)

    def unreached(gr):
        gx = gr[0].clone()
        ok = float(gx[:, :, ::2, ::2].abs().min()) > 0
        gx[:, :, ::2, ::2] = 0
        return ok and float(gx.abs().max()) == 0.0
    out.append(("stride2_unreached", c, unreached))
    # 3x3 stride 2 pad 0 on an even side: the last row and column meet no tap either
    c = Case(torch.randn(1, 16, 8, 8, generator=g), torch.randn(16, 16, 3, 3, generator=g), torch.zeros(16), None,
               torch.randn(1, 16, 3, 3, generator=g), 2, 0, 1, False)
    out.append(("stride2_last_row", c, lambda gr: float(gr[0][:, :, 7, :].abs().max()) == 0.0 and float(gr[0][:, :, :, 7].abs().max()) == 0.0
                and float(gr[0][:, :, :7, :7].abs().min()) > 0))
    return out


def make_block_state_dict(cin, cout, seed, prefix="level2.tree1."):
    """A reference BasicBlock's state_dict entries with BatchNorm statistics away from the identity."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, ci in ((1, cin), (2, cout)):
        sd["%sconv%d.weight" % (prefix, i)] = torch.randn(cout, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        sd["%sbn%d.weight" % (prefix, i)] = torch.rand(cout, generator=g) + 0.5
        sd["%sbn%d.bias" % (prefix, i)] = torch.randn(cout, generator=g) * 0.1
        sd["%sbn%d.running_mean" % (prefix, i)] = torch.randn(cout, generator=g) * 0.1
        sd["%sbn%d.running_var" % (prefix, i)] = torch.rand(cout, generator=g) + 0.5
        sd["%sbn%d.num_batches_tracked" % (prefix, i)] = torch.tensor(7)
    return sd
