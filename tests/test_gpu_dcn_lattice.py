"""GPU: the fp32 DCNv2 operator (`dcn_v2.dcn_v2_forward`: csrc/dcn2.hip and the general kernel of csrc/dcn.hip) and `dcn_v2_backward`
(csrc/dcn_bwd.hip, matrix-core and general kernels) on the quarter-pixel lattice of tests/lattice_ref.py (`dcn_grid_case`), bit for bit.

x and grad_y are integers in [-3, 3], w is in {-1, 0, 1}, the offsets lie on k/4 and the masks on k/8: every bilinear weight, its
derivative, every product and every partial sum is a multiple of 1/128 far below 2^24 of them, exact in fp32 in ANY order.  So the forward
and all five gradients -- grad_input under float atomics included -- are compared with torch.equal against the fp64 oracle cast to
float32; tests/test_oracle_dcn_backward.py pins, case by case, that the cast rounds nothing, that at least a quarter of the offsets of
each coordinate are fractional and that every border class (two corners outside the image, a coordinate exactly on the gate at -1 or H
beside a fractional one, beyond the gate) has a sample.  The max-norm rule of tests/test_gpu_dcn_backward.py (4 e32 + 1e-7 max |g64| per
tensor) cannot see an error confined to a tensor's small elements; this comparison has no small elements.

Both arithmetics of the forward are exact here.  `OP_F32_MFMA` runs fmaf chains on the fp32 matrix instruction.  The default splits every
fp32 operand into fp16 terms after scaling the filters and the activations by device-derived scales, and both scales are POWERS OF TWO
(csrc/dcn2.hip: 2^(14 - k) from frexpf of max |w|; csrc/dcn_traits.h dcn_act_exp: 2^e from frexpf of max |x| and max |mask|), so the scaled
lattice is a lattice, every lo term of a split is zero and the fp32 accumulation is exact: equality is asserted there too."""
import pytest
import torch

import lattice_ref as L
from gpu_helpers import DEV
from h3d_amd import dcn_v2

pytestmark = pytest.mark.gpu

GRAD_NAMES = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


def _geo(name):
    k, s, p, d, dg = L.DCN_GRID_CASES[name][6:]
    return (k[0], k[1], s, s, p, p, d, d, dg)


def assert_same(got, ref, what):
    """torch.equal, and on failure how many elements differ, the first one, and whether the differing elements are the small ones."""
    got, ref = got.detach().float().cpu().contiguous(), ref.float().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if torch.equal(got, ref):
        return
    bad = ~(got == ref)
    idx = tuple(bad.nonzero()[0].tolist())
    raise AssertionError("%s: %d of %d elements differ from the exact reference; first at %s: got %r, expected %r; max |difference| %.3g, "
                         "max |ref| %.3g, max |ref| among the differing elements %.3g"
                         % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(ref[idx]), float((got - ref)[bad].abs().max()),
                            float(ref.abs().max()), float(ref[bad].abs().max())))


class _Arith:
    def __init__(self, f32_mfma):
        self.want = f32_mfma

    def __enter__(self):
        self.old = dcn_v2.OP_F32_MFMA
        dcn_v2.OP_F32_MFMA = self.want

    def __exit__(self, *e):
        dcn_v2.OP_F32_MFMA = self.old


# ---- forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("arith", ["f32_mfma", "default"])
@pytest.mark.parametrize("name", sorted(L.DCN_GRID_MFMA))
def test_forward_model_configuration_is_exact(name, arith, channels_last):
    x, w, b, off, m, _ = [t.to(DEV) for t in L.dcn_grid(name)]
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    ref = L.dcn_grid_exact(name)[0]
    with _Arith(arith == "f32_mfma"), torch.no_grad():
        y = dcn_v2.dcn_v2_forward(x, w, b, off, m, *_geo(name))
        again = dcn_v2.dcn_v2_forward(x, w, b, off, m, *_geo(name))
    assert_same(y, ref, "dcn_v2_forward %s %s" % (name, arith))
    assert torch.equal(y, again)


@pytest.mark.parametrize("name", sorted(L.DCN_GRID_GENERAL))
def test_forward_general_kernel_is_exact(name):
    x, w, b, off, m, _ = [t.to(DEV) for t in L.dcn_grid(name)]
    with torch.no_grad():
        y = dcn_v2.dcn_v2_forward(x, w, b, off, m, *_geo(name))
    assert_same(y, L.dcn_grid_exact(name)[0], "dcn_v2_forward (general kernel) " + name)


# ---- backward ------------------------------------------------------------------------------------------------------------------------
def _backward(name, general):
    x, w, b, off, m, gy = [t.to(DEV) for t in L.dcn_grid(name)]
    return dcn_v2._dcn_v2_backward(x, w, b, off, m, gy, *_geo(name), general=general)


@pytest.mark.parametrize("name,general", [(n, g) for n in sorted(L.DCN_GRID_MFMA) for g in (False, True)] + [(n, True) for n in sorted(L.DCN_GRID_GENERAL)])
def test_backward_all_five_gradients_are_exact_and_repeatable(name, general):
    ref = L.dcn_grid_exact(name)[1]
    got = _backward(name, general)
    again = _backward(name, general)
    fails = []
    for nm, g, r, a in zip(GRAD_NAMES, got, ref, again):
        try:
            assert_same(g, r, "%s %s %s" % (name, "general" if general else "matrix-core", nm))
        except AssertionError as e:
            fails.append(str(e))
        if not torch.equal(g, a):
            fails.append("%s %s: two runs differ" % (name, nm))
    assert not fails, "\n".join(fails)


def test_trainable_dcnv2_returns_the_bits_of_the_raw_calls():
    name = "m_2x48to7_13x11"
    seed, B, C, Co, H, W, k, s, p, d, dg = L.DCN_GRID_CASES[name]
    x, w, b, off, m, gy = [t.to(DEV) for t in L.dcn_grid(name)]
    mod = dcn_v2.TrainableDCNv2(C, Co, k, s, p, d, dg).to(DEV)
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(b)
    xg, og, mg = x.clone().requires_grad_(True), off.clone().requires_grad_(True), m.clone().requires_grad_(True)
    y = mod(xg, og, mg)
    y.backward(gy)
    raw = _backward(name, False)
    y_ref, g_ref = L.dcn_grid_exact(name)
    assert_same(y, y_ref, "TrainableDCNv2 forward")
    for nm, g, r, e in zip(GRAD_NAMES, (xg.grad, og.grad, mg.grad, mod.weight.grad, mod.bias.grad), raw, g_ref):
        assert torch.equal(g, r), nm
        assert_same(g, e, "TrainableDCNv2 " + nm)
