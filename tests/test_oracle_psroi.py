"""CPU: pin the PS-ROI pooling restatement (tests/psroi_ref.py) without trusting it -- closed forms on inputs that bilinear
interpolation reproduces exactly, identities between its arguments, the reference's own setup (DCNv2/test.py:100-131) with each
roi's mean computed by hand -- and the C ABI's argument checks, which run without a GPU."""
import ctypes
import math

import numpy as np
import pytest

import h3d_amd  # noqa: F401
from h3d_amd import _lib
from psroi_ref import psroi_pool, round_half_away

f32 = np.float32


def _ramp(B, C, H, W, coef):
    """channel c of every image: f(y, x) = a*x + b*y + c (coef[c] = (a, b, c))."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    img = np.stack([a * x + b * y + c0 for a, b, c0 in coef])
    return np.broadcast_to(img, (B, C, H, W)).astype(f32)


def _round_away(v):
    return math.copysign(math.floor(abs(v) + 0.5), v)


def _ramp_expected(roi, coef, H, W, scale, P, spp, rnd=_round_away):
    """Closed form, float64, written from the contract: the mean of f over the valid, clamped sample points of every bin."""
    x1, y1, x2, y2 = (rnd(float(v)) for v in roi[1:])
    sw, sh = x1 * scale - 0.5, y1 * scale - 0.5
    rw = max((x2 + 1) * scale - 0.5 - sw, 0.1)
    rh = max((y2 + 1) * scale - 0.5 - sh, 0.1)
    out = np.zeros((len(coef), P, P))
    cnt = np.zeros((P, P))
    for ph in range(P):
        for pw in range(P):
            pts = []
            for ih in range(spp):
                for iw in range(spp):
                    w = sw + pw * rw / P + iw * rw / P / spp
                    h = sh + ph * rh / P + ih * rh / P / spp
                    if w < -0.5 or w > W - 0.5 or h < -0.5 or h > H - 0.5:
                        continue
                    pts.append((min(max(h, 0), H - 1), min(max(w, 0), W - 1)))
            cnt[ph, pw] = len(pts)
            for c, (a, b, c0) in enumerate(coef):
                out[c, ph, pw] = np.mean([a * x + b * y + c0 for y, x in pts]) if pts else 0.0
    return out, cnt


RAMP_COEF = [(0.75, -0.5, 3.0), (-2.0, 1.25, -7.0)]
RAMP_ROIS = {
    "integer": [0, 2, 3, 9, 8],
    "fractional": [0, 1.3, 2.7, 7.2, 9.6],
    "half_integer": [0, 2.5, 3.5, 8.5, 6.5],
    "negative_half": [0, -1.5, 0.5, 4.5, 3.5],
    "partly_outside": [0, -6, -4, 5, 20],
    "outside": [0, 40, 40, 50, 50],
}


@pytest.mark.parametrize("name", sorted(RAMP_ROIS))
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_linear_ramp_closed_form(name, scale):
    H, W, P, spp = 12, 16, 4, 2
    inp = _ramp(1, 2, H, W, RAMP_COEF)
    roi = np.array([RAMP_ROIS[name]], f32)
    out, cnt = psroi_pool(inp, roi, None, 1, scale, 2, 1, P, P, spp, 0.0)
    exp, ecnt = _ramp_expected(roi[0], RAMP_COEF, H, W, scale, P, spp)
    np.testing.assert_array_equal(cnt[0, 0], ecnt)
    np.testing.assert_allclose(out[0], exp, atol=1e-4, rtol=0)
    if name == "outside":
        assert not cnt.any() and not out.any()
    if name == "partly_outside":
        assert 0 < cnt.sum() < cnt.size * spp * spp
    if "half" in name:
        # the half-integer corners are where round-half-to-even (np.round) would pick another box
        alt, _ = _ramp_expected(roi[0], RAMP_COEF, H, W, scale, P, spp, rnd=lambda v: float(np.round(v)))
        assert np.abs(alt - exp).max() > 0.1


def test_round_half_away_from_zero():
    v = np.array([2.5, -2.5, 0.5, -0.5, 1.49999994, 0.49999997, 3.0, -7.7], f32)
    np.testing.assert_array_equal(round_half_away(v), np.array([3, -3, 1, -1, 1, 0, 3, -8], f32))


def _rand_rois(rng, R, B, H, W, scale):
    x = rng.uniform(-10, W / scale + 10, (R, 2))
    y = rng.uniform(-10, H / scale + 10, (R, 2))
    return np.stack([rng.integers(0, B, R), x.min(1), y.min(1), x.max(1), y.max(1)], 1).astype(f32)


def test_constant_input():
    rng = np.random.default_rng(1)
    inp = np.full((2, 8, 20, 24), 1.75, f32)
    rois = _rand_rois(rng, 30, 2, 20, 24, 0.25)
    trans = rng.normal(size=(30, 4, 7, 7)).astype(f32)
    out, cnt = psroi_pool(inp, rois, trans, 0, 0.25, 8, 1, 7, 7, 4, 0.3)
    assert (cnt > 0).any() and (cnt == 0).any()
    np.testing.assert_allclose(out[cnt > 0], 1.75, rtol=1e-12)
    assert not out[cnt == 0].any()


def test_no_trans_equals_zero_trans():
    rng = np.random.default_rng(2)
    inp = rng.normal(size=(2, 6, 17, 13)).astype(f32)
    rois = _rand_rois(rng, 12, 2, 17, 13, 0.5)
    a = psroi_pool(inp, rois, None, 1, 0.5, 6, 1, 3, 3, 2, 0.1)
    b = psroi_pool(inp, rois, np.zeros((12, 6, 2, 2), f32), 0, 0.5, 6, 1, 3, 2, 2, 0.1)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_integer_translation_is_a_shift():
    """roi_w = roi_h = 8 px (a power of two): trans * trans_std * roi_w is an exact integer in fp32, so the translated roi pools
    exactly what the untranslated roi moved by that many pixels pools."""
    H, W, P, spp = 24, 28, 4, 2
    inp = _ramp(1, 2, H, W, RAMP_COEF)
    roi = np.array([[0, 6, 9, 13, 16]], f32)                  # round(x2) + 1 - round(x1) = 8
    trans = np.zeros((1, 2, P, P), f32)
    trans[0, 0], trans[0, 1] = 0.5, -1.0                      # x: 0.5 * 0.25 * 8 = 1 px, y: -2 px
    out, cnt = psroi_pool(inp, roi, trans, 0, 1.0, 2, 1, P, P, spp, 0.25)
    ref, rcnt = psroi_pool(inp, roi + np.array([0, 1, -2, 1, -2], f32), None, 1, 1.0, 2, 1, P, P, spp, 0.25)
    np.testing.assert_array_equal(cnt, rcnt)
    np.testing.assert_allclose(out, ref, atol=1e-12)
    unshifted, _ = psroi_pool(inp, roi, None, 1, 1.0, 2, 1, P, P, spp, 0.25)
    np.testing.assert_allclose(out - unshifted, np.array([1.75, -4.5])[None, :, None, None] * np.ones_like(out), atol=1e-9)


def _hat_profile(lo, hi, value):
    """1-D bilinear interpolation of `value` on pixels [lo, hi) and 0 elsewhere, at position t."""
    def f(t):
        xa, xb = math.floor(t), math.ceil(t)
        d = t - xa
        v = lambda i: value if lo <= i < hi else 0.0
        return (1 - d) * v(xa) + d * v(xb)
    return f


def reference_zero_offset_setup():
    inp = np.zeros((2, 16, 64, 64), f32)
    inp[0, :, 16:26, 16:26] = 1.
    inp[1, :, 10:20, 20:30] = 2.
    rois = np.array([[0, 65, 65, 103, 103], [1, 81, 41, 119, 79]], f32)
    return inp, rois


def test_reference_check_pooling_zero_offset():
    """DCNv2/test.py:100-131: each roi's mean by hand.  All 784 samples of a roi are inside the map and the lit block is a product
    of two intervals, so the mean is (mean of the x profile over the 28 sample columns) x (mean of the y profile over the rows)."""
    inp, rois = reference_zero_offset_setup()
    out, cnt = psroi_pool(inp, rois, None, 1, 0.25, 16, 1, 7, 7, 4, 0.0)
    dout, dcnt = psroi_pool(inp, rois, np.zeros((20, 2, 7, 7), f32), 0, 0.25, 16, 1, 7, 7, 4, 0.0)
    np.testing.assert_array_equal(out, dout)
    assert (cnt == 16).all() and (dcnt == 16).all()
    blocks = [((16, 26), (16, 26), 1.0), ((10, 20), (20, 30), 2.0)]      # (rows, cols, value)
    for n, ((r0, r1), (c0, c1), val) in enumerate(blocks):
        _, x1, y1, x2, y2 = rois[n]
        sw, sh = x1 / 4 - 0.5, y1 / 4 - 0.5
        rw, rh = (x2 + 1) / 4 - 0.5 - sw, (y2 + 1) / 4 - 0.5 - sh
        fx, fy = _hat_profile(c0, c1, 1.0), _hat_profile(r0, r1, val)
        mx = np.mean([fx(sw + j * rw / 28) for j in range(28)])
        my = np.mean([fy(sh + j * rh / 28) for j in range(28)])
        assert abs(out[n].mean() - mx * my) < 1e-6, (n, out[n].mean(), mx * my)
    assert out[0].mean() > 0 and out[1].mean() > 0


# ---- the C ABI's host-side checks (no launch: no GPU needed) -------------------------------------------------------------------

def _call(*, ptr=16, B=1, C=4, H=8, W=8, R=1, ct=2, no_trans=0, output_dim=4, gs=1, P=2, part=2, spp=2):
    L = _lib.lib()
    p = ctypes.c_void_p(ptr) if ptr else None
    return L.h3d_dcn_v2_psroi_pooling_forward(p, p, p, p, p, B, C, H, W, R, ct, no_trans, 0.25, output_dim, gs, P, part, spp, 0.1,
                                              None)


def test_c_abi_argument_checks_without_a_gpu():
    L = _lib.lib()
    assert _call(ptr=0) == -5 and b"null pointer" in L.h3d_last_error()
    assert _call(gs=2) == -4 and b"group_size" in L.h3d_last_error()
    assert _call(output_dim=3) == -1 and L.h3d_last_error() == b"input channels and output channels must equal"
    assert _call(ct=6) == -1 and b"num_classes" in L.h3d_last_error()       # 3 classes do not divide 4 channels
    assert _call(ct=3) == -1                                                 # odd trans channels
    assert _call(P=0) == -5
    assert _call(R=0) == 0                                                   # nothing to do: no launch
    m = L.h3d_dcn_pooling_modulated(None, None, None, None, 1, 4, 8, 8, 1, 0.25, 4, 1, 2, 2, 2, 0.1, None)
    assert m == -5
    p = ctypes.c_void_p(16)
    assert L.h3d_dcn_pooling_modulated(p, p, p, p, 1, 4, 8, 8, 1, 0.25, 4, 1, 2, 3, 2, 0.1, None) == -1    # part_size != P
