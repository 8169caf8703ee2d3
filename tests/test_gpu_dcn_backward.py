"""GPU: `dcn_v2_backward` (csrc/dcn_bwd.hip) against the fp64 oracle (tests/dcn_backward_ref.py: autograd over oracle/dcn.py), general
kernels and matrix-core kernels, the autograd function and the trainable modules.

The rule of every comparison (per case, per gradient tensor): e32 = max |g32 - g64| of the oracle's own float32 autograd run, and
max |g_gpu - g64| <= 4 * e32 + 1e-7 * max |g64|.  The observed ratios are printed (`pytest -s`) and recorded in DESIGN.md."""
import numpy as np
import pytest
import torch

import dcn_backward_ref as R
from gpu_helpers import DEV
from h3d_amd import dcn_v2
from oracle import dcn as odcn

pytestmark = pytest.mark.gpu


def _gpu(case, k, s, p, d, dg, need=(True,) * 5, general=False):
    x, w, b, off, m, go = [t.to(DEV) for t in case]
    return dcn_v2._dcn_v2_backward(x, w, b, off, m, go, k[0], k[1], s, s, p, p, d, d, dg, need=need, general=general)


def _run(name, case, k=(3, 3), s=1, p=1, d=1, dg=1, general=False):
    g64, e32 = R.bounds(*case, k, s, p, d, dg)
    got = _gpu(case, k, s, p, d, dg, general=general)
    return R.check(name, got, g64, e32)


# ---- 4. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(1, 1, 1, 1), (2, 1, 1, 1), (1, 2, 2, 2), (1, 1, 1, 4)])
def test_general_kernels_random_configurations_vs_oracle(cfg):
    s, p, d, dg = cfg
    _run("general %s" % (cfg,), R.make_case(10 + s + 2 * d + dg, 2, 8, 7, 13, 11, (3, 3), s, p, d, dg), (3, 3), s, p, d, dg)


def test_general_kernels_1x1_and_rectangular_kernels_vs_oracle():
    _run("1x1", R.make_case(20, 2, 5, 3, 9, 7, (1, 1), 1, 0, 1, 1), (1, 1), 1, 0, 1, 1)
    _run("3x1 odd", R.make_case(21, 1, 6, 67, 15, 17, (3, 1), 1, 1, 1, 3), (3, 1), 1, 1, 1, 3)


def test_general_kernels_integer_offsets_vs_oracle():
    # fp32 position sums are exact: the floor convention (right-hand derivative, zero on the gate) is compared as it stands
    _run("general int", R.make_case(22, 2, 8, 7, 13, 11, dg=2, fraction=False), dg=2)


@pytest.mark.parametrize("shape", [(1, 512, 256, 16, 16), (2, 128, 128, 64, 64), (1, 64, 64, 128, 128), (2, 48, 7, 13, 11), (1, 64, 200, 9, 9),
                                   (1, 16, 27, 20, 37)])
def test_matrix_core_kernels_model_shapes_vs_oracle(shape):
    B, C, Co, H, W = shape
    _run("mfma %s" % (shape,), R.make_case(30 + C + H, B, C, Co, H, W))


def test_matrix_core_kernels_integer_offsets_vs_oracle():
    _run("mfma int", R.make_case(23, 2, 32, 24, 14, 19, fraction=False))


# ---- 5. matrix-core kernels and general kernels on the same operands --------------------------------------------------------------
def test_matrix_core_and_general_kernels_on_12_random_shapes():
    rs = np.random.RandomState(5)
    for i in range(12):
        C = int(rs.choice([16, 32, 48, 64, 96, 128]))
        Co, H, W, B = int(rs.randint(1, 131)), int(rs.randint(5, 41)), int(rs.randint(5, 41)), int(rs.randint(1, 3))
        case = R.make_case(100 + i, B, C, Co, H, W)
        g64, e32 = R.bounds(*case, (3, 3), 1, 1, 1, 1)
        R.check("shape %d %s mfma" % (i, (B, C, Co, H, W)), _gpu(case, (3, 3), 1, 1, 1, 1), g64, e32)
        R.check("shape %d %s general" % (i, (B, C, Co, H, W)), _gpu(case, (3, 3), 1, 1, 1, 1, general=True), g64, e32)


# ---- 6. input domain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-4, 1.0, 1e4])
def test_input_domain_scaled_x_and_grad_output(scale):
    x, w, b, off, m, go = R.make_case(30 + 64 + 24, 1, 64, 64, 24, 40)
    _run("scale %g" % scale, (x * scale, w, b, off, m, go * scale))


# ---- 7. NULL outputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True])
def test_each_output_alone_equals_the_all_five_result_and_skipped_buffers_are_untouched(general):
    import ctypes
    from h3d_amd import _lib
    B, C, Co, H, W = 2, 32, 24, 14, 19
    case = R.make_case(40, B, C, Co, H, W)
    g64, e32 = R.bounds(*case, (3, 3), 1, 1, 1, 1)
    full = _gpu(case, (3, 3), 1, 1, 1, 1, general=general)
    for i in range(5):
        need = tuple(j == i for j in range(5))
        one = _gpu(case, (3, 3), 1, 1, 1, 1, need=need, general=general)
        assert all((o is None) == (j != i) for j, o in enumerate(one))
        if i == 0:          # grad_input: atomic order -- within the bound
            R.check("alone", (one[0], None, None, None, None), g64, e32)
        else:               # fixed-order sums: bit-identical
            assert torch.equal(one[i], full[i]), R.NAMES[i]
    # sentinel-filled buffers of skipped outputs stay as they are (raw entry point)
    x, w, b, off, m, go = [t.to(DEV).contiguous() for t in case]
    bufs = [torch.full_like(t, 777.0) for t in (x, off, m, w, b)]
    L = _lib.lib()
    geo = (B, C, H, W, Co, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    n = ctypes.c_size_t(0)
    _lib.check(L.h3d_dcn_v2_backward_workspace_bytes(*geo, ctypes.byref(n)), "ws")
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    fn = L.h3d_dcn_v2_backward_general if general else L.h3d_dcn_v2_backward
    for i in range(5):
        outs = [_lib.ptr(bufs[j]) if j == i else None for j in range(5)]
        _lib.check(fn(*[_lib.ptr(t) for t in (x, w, b, off, m, go)], *outs, *geo, _lib.ptr(ws), n.value, _lib.stream_ptr()), "backward")
        torch.cuda.synchronize()
        for j in range(5):
            if j > i:
                assert bool((bufs[j] == 777.0).all()), (i, j)
    # a short workspace is an error, not an overrun
    rc = fn(*[_lib.ptr(t) for t in (x, w, b, off, m, go)], *[_lib.ptr(t) for t in bufs], *geo, _lib.ptr(ws), 64, _lib.stream_ptr())
    assert rc == -5 and b"workspace" in L.h3d_last_error()


# ---- 8. the reference's own gradient test (DCNv2/test.py:69-97), restated ---------------------------------------------------------
def test_reference_check_gradient_dconv_through_the_autograd_function():
    gen = torch.Generator().manual_seed(8)
    N, inC, inH, inW, outC, dg = 2, 2, 4, 4, 2, 1
    x = (torch.rand(N, inC, inH, inW, generator=gen) * 0.01).to(DEV).requires_grad_(True)
    # the reference draws randn * 2; here the same spread with every position kept 0.05 away from an integer (eps = 1e-3 must not straddle a kink)
    off = R.make_offsets(gen, N, dg, (3, 3), inH, inW, int_range=4).to(DEV).requires_grad_(True)
    mask = torch.sigmoid(torch.rand(N, dg * 9, inH, inW, generator=gen)).to(DEV).requires_grad_(True)
    w = torch.randn(outC, inC, 3, 3, generator=gen).to(DEV).requires_grad_(True)
    b = torch.rand(outC, generator=gen).to(DEV).requires_grad_(True)
    # nondet_tol: grad_input is summed by float atomics, so two backward runs may differ in the last bits (|grad_input| < 10 here: an ulp is
    # below 1e-6); the reference's eps / atol / rtol are kept
    assert torch.autograd.gradcheck(dcn_v2.dcn_v2_conv_autograd, (x, off, mask, w, b, 1, 1, 1, dg), eps=1e-3, atol=1e-4, rtol=1e-2,
                                    nondet_tol=1e-5)


# ---- 9. the trainable modules ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(16, 8, 1, 1, 1, 1), (6, 5, 2, 1, 1, 2)])
def test_trainable_dcn_forward_backward_state_dict_and_no_grad(cfg):
    C, Co, s, p, d, dg = cfg
    torch.manual_seed(9)
    ref_mod = dcn_v2.DCN(C, Co, (3, 3), stride=s, padding=p, dilation=d, deformable_groups=dg).to(DEV).eval()
    with torch.no_grad():
        ref_mod.bias.copy_(torch.randn(Co))
        ref_mod.conv_offset_mask.weight.copy_(torch.randn_like(ref_mod.conv_offset_mask.weight) * 0.1)
        ref_mod.conv_offset_mask.bias.copy_(torch.randn_like(ref_mod.conv_offset_mask.bias) * 0.7 + 0.37)
    mod = dcn_v2.TrainableDCN(C, Co, (3, 3), stride=s, padding=p, dilation=d, deformable_groups=dg).to(DEV)
    assert list(mod.state_dict().keys()) == list(ref_mod.state_dict().keys())
    mod.load_state_dict(ref_mod.state_dict())
    x = (torch.rand(2, C, 12, 15) * 2 - 1)
    with torch.no_grad():
        y_ref = ref_mod(x.to(DEV))
        y_ng = mod(x.to(DEV))
    assert y_ng.grad_fn is None and not y_ng.requires_grad
    np.testing.assert_allclose(y_ng.cpu().numpy(), y_ref.cpu().numpy(), rtol=0, atol=3e-4)
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg)
    assert y.grad_fn is not None
    go = torch.rand(y.shape, generator=torch.Generator().manual_seed(1)) * 2 - 1
    (y * go.to(DEV)).sum().backward()
    params = [mod.weight, mod.bias, mod.conv_offset_mask.weight, mod.conv_offset_mask.bias]
    assert all(t.grad is not None for t in params + [xg])

    def oracle(dtype):
        leaves = [t.detach().cpu().to(dtype).requires_grad_(True) for t in [xg] + params]
        out = odcn.dcn_module_forward(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], s, p, d, dg)
        return torch.autograd.grad(out, leaves, go.to(dtype))
    g64, g32 = oracle(torch.float64), oracle(torch.float32)
    fails = []
    for nm, t, r, q in zip(("input", "weight", "bias", "om.weight", "om.bias"), [xg] + params, g64, g32):
        e = float((q.double() - r).abs().max())
        err = float((t.grad.cpu().double() - r).abs().max())
        print("TrainableDCN %s %s: err %.3g e32 %.3g ratio %.3g" % (cfg, nm, err, e, err / e if e else 0))
        if not err <= 4 * e + 1e-7 * float(r.abs().max()):
            fails.append((nm, err, e))
    assert not fails, fails
    # a fine-tuning step changes all four parameters
    before = [t.detach().clone() for t in params]
    torch.optim.SGD(mod.parameters(), lr=0.1).step()
    assert all(not torch.equal(a, t.detach()) for a, t in zip(before, params))
    # the inference classes still refuse
    with pytest.raises(RuntimeError, match="inference-only"):
        ref_mod(x.to(DEV).requires_grad_(True))


def test_trainable_dcnv2_matches_the_autograd_function():
    case = R.make_case(50, 1, 8, 6, 9, 10, dg=2)
    x, w, b, off, m, go = [t.to(DEV) for t in case]
    mod = dcn_v2.TrainableDCNv2(8, 6, (3, 3), 1, 1, 1, 2).to(DEV)
    assert list(mod.state_dict().keys()) == ["weight", "bias"]
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(b)
    xg, og, mg = x.clone().requires_grad_(True), off.clone().requires_grad_(True), m.clone().requires_grad_(True)
    (mod(xg, og, mg) * go).sum().backward()
    g64, e32 = R.bounds(*case, (3, 3), 1, 1, 1, 2)
    R.check("TrainableDCNv2", (xg.grad, og.grad, mg.grad, mod.weight.grad, mod.bias.grad), g64, e32)


# ---- 10. streams ----------------------------------------------------------------------------------------------------------------
def test_backward_on_a_non_default_stream_gives_the_same_result():
    case = R.make_case(60, 2, 32, 24, 14, 19)
    g64, e32 = R.bounds(*case, (3, 3), 1, 1, 1, 1)
    ref = _gpu(case, (3, 3), 1, 1, 1, 1)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = _gpu(case, (3, 3), 1, 1, 1, 1)
    st.synchronize()
    for i in range(1, 5):
        assert torch.equal(got[i], ref[i]), R.NAMES[i]
    R.check("stream", got, g64, e32)
