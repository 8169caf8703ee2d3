"""CPU: the yardstick of the convolution backward (tests/conv_grad_ref.py) checked against itself -- gradcheck, the grid properties that
make the ReLU gate implementation-independent, known answers of the gather-form restatement -- plus the exported symbols and the
argument / limit return codes of include/h3d.h section 2c (every check runs before the first HIP call)."""
import ctypes
import os

import pytest
import torch

import conv_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("geo", [dict(k=3, stride=1, padding=1), dict(k=3, stride=2, padding=1), dict(k=1, stride=1, padding=0),
                                 dict(k=(5, 3), stride=(2, 1), padding=(2, 0)), dict(k=3, stride=1, padding=2, dilation=2)])
@pytest.mark.parametrize("relu", [False, True])
def test_restatement_passes_gradcheck_in_fp64(geo, relu):
    g = torch.Generator().manual_seed(1)
    kh, kw = R._pair(geo["k"])
    st, pd, dl = geo["stride"], geo["padding"], geo.get("dilation", 1)
    Ho, Wo = R.out_size(6, 7, geo["k"], st, pd, dl)
    leaves = [torch.randn(s, generator=g, dtype=torch.float64).requires_grad_(True)
              for s in ((2, 3, 6, 7), (4, 3, kh, kw), (4,), (2, 4, Ho, Wo))]
    assert float(R.pre_act(*leaves, st, pd, dl).detach().abs().min()) > 1e-4      # no pre-activation inside gradcheck's finite-difference step
    assert torch.autograd.gradcheck(lambda x, w, b, r: R.forward(x, w, b, r, st, pd, dl, relu), leaves, eps=1e-6, atol=1e-6)


@pytest.mark.parametrize("name", sorted(n for n, kw in R.CASES.items() if kw.get("relu")))
def test_gridded_cases_have_an_exact_nonzero_pre_activation(name):
    c = R.case(name)
    assert c.pre_bound() < 2 ** 13                              # every partial sum of pre stays below 2^13: exact in fp32 in any order
    p32, p64 = c.pre(torch.float32), c.pre(torch.float64)
    assert torch.equal(p32.double(), p64)                       # fp32 pre equals fp64 pre bit for bit
    assert float(p64.abs().min()) >= 2.0 ** -11
    assert float(p64.abs().max()) < 2 ** 13
    assert float(c.x.abs().max()) <= 2 and float(c.w.abs().max()) <= 1 and float(c.b.abs().max()) < 1
    assert torch.equal(c.x * 16, (c.x * 16).round()) and torch.equal(c.w * 64, (c.w * 64).round())
    assert c.res is None or (torch.equal(c.res * 16, (c.res * 16).round()) and float(c.res.abs().max()) <= 2)
    assert bool(((c.b * 2048).round() == c.b * 2048).all()) and bool(((c.b * 2048).abs() % 2 == 1).all())


@pytest.mark.parametrize("name", R.INT_GY_CASES)
def test_integer_grad_y_cases_are_exact_in_fp32(name):
    """Gridded x, w, b, res and an integer grad_y: float32 autograd gives float64's bits, every gradient lies on its grid, and the sum of
    the absolute values of its terms (the same autograd run on |w|, |x|, |grad_y| with the gate of the real case) stays below 2^24 units,
    so no split or summation order can round."""
    c = R.int_gy_case(name)
    base = R.case(name)
    assert all(torch.equal(a, b) for a, b in ((c.x, base.x), (c.w, base.w), (c.b, base.b))) and (c.res is None or torch.equal(c.res, base.res))
    assert torch.equal(c.gy, c.gy.round()) and float(c.gy.min()) == -8 and float(c.gy.max()) == 8
    g64, g32 = R.grads(c, torch.float64), R.grads(c, torch.float32)
    gate = (c.y(torch.float64) > 0).double() if c.relu else torch.ones_like(c.gy, dtype=torch.float64)
    gg = c.gy.double().abs() * gate
    lin = R.Case(c.x.abs(), c.w.abs(), torch.zeros_like(c.b), None, gg.float(), c.stride, c.padding, c.dilation, False)
    bound = R.grads(lin, torch.float64)
    for nm, a, r, unit, bd in zip(R.NAMES, g32, g64, (64.0, 1.0, 16.0, 1.0), (bound[0], gg, bound[2], bound[3])):
        assert (a is None) == (r is None), nm
        if r is None:
            continue
        assert torch.equal(a.double(), r), nm
        assert torch.equal(r * unit, (r * unit).round()) and float(r.abs().max()) > 0, nm
        assert bool((bd >= r.abs()).all()) and float(bd.max()) * unit < 2.0 ** 24, (nm, float(bd.max()) * unit)
    assert all((a is None and r is None) or torch.equal(a.double(), r) for a, r in zip(R.int_gy_exact(name), g64))


def test_integer_grad_y_case_list():
    assert R.INT_GY_CASES == ("s1_2x9x33_48to80_res_relu", "s1_1x17x40_32to144_res_relu", "s2_7x9_48to80", "s2_8x10_16to32", "k1_448to64",
                              "split_513", "model_64to64", "g_stem7x7", "g_5x3")
    assert all(n in R.CASES for n in R.INT_GY_CASES) and {"g_stem7x7", "g_5x3"} <= set(R.GENERAL_CASES)


def test_random_case_has_a_gate_margin():
    p = R.make_random_case().pre().abs()
    assert float(p.min()) >= 1e-3 * float(p.max()) > 0


def test_split_cases_sit_either_side_of_the_split_length():
    px = {}
    for n in ("split_511", "split_512", "split_513"):
        c = R.case(n)
        px[n] = c.gy.shape[0] * c.gy.shape[2] * c.gy.shape[3]
    assert px["split_512"] == R.SPLIT_PIXELS and px["split_513"] == R.SPLIT_PIXELS + 1 and px["split_511"] == R.SPLIT_PIXELS - 1
    with open(os.path.join(ROOT, "human-3d-reconstruction_amd", "csrc", "conv_bwd.hip")) as f:
        assert "CB_SPLIT_PIXELS = %d" % R.SPLIT_PIXELS in f.read()


def test_case_list_covers_what_it_names():
    from h3d_amd import _lib
    assert len(R.MFMA_CASES) == 60 + 8 + 2 + 3 + 1 and len(R.GENERAL_CASES) == 5
    for n in R.GENERAL_ON_MFMA:
        assert n in R.MFMA_CASES
    for n in R.MFMA_CASES:
        kw = R.CASES[n]
        assert kw["C"] % 16 == 0 and kw["Cout"] % 16 == 0 and max(kw["C"], kw["Cout"]) <= _lib.CONV_BWD_MFMA_CMAX


@pytest.mark.parametrize("name", ["s1_2x9x33_48to80_res_relu", "s2_8x10_16to32", "s2_7x9_48to80", "k1_80to48", "g_stem7x7", "g_3x3_d2", "g_1x1_s2", "g_5x3"])
def test_gather_form_restatement_agrees_with_autograd(name):
    """The definitions of include/h3d.h section 2c, restated with plain loops over the taps, against torch autograd in fp64."""
    c = R.case(name)
    for a, b in zip(R.gather_grads(c), R.grads(c)):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.allclose(a, b, rtol=1e-12, atol=1e-10)


@pytest.mark.parametrize("i", range(5))
def test_known_answers_of_the_restatement(i):
    what, c, ok = R.known_answer_cases()[i]
    gr = R.gather_grads(c)
    assert ok(gr), what
    assert ok([None if t is None else t for t in R.grads(c)]), what


def test_new_symbols_are_exported():
    import h3d_amd
    from h3d_amd import _lib, conv
    assert "conv" in h3d_amd.__all__
    assert callable(conv.conv2d_backward) and callable(conv.conv2d_autograd)
    assert issubclass(conv.TrainableConv2d, torch.nn.Conv2d) and issubclass(conv.TrainableBasicBlock, torch.nn.Module)
    for name in ("h3d_conv2d_backward_workspace_bytes", "h3d_conv2d_backward", "h3d_conv2d_backward_general"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "h3d.h")).read()
    assert "H3D_CONV_BWD_RELU = %d" % _lib.CONV_BWD_RELU in hdr and "#define H3D_ABI_VERSION 4" in hdr
    assert "#define H3D_CONV_BWD_MFMA_CMAX %d" % _lib.CONV_BWD_MFMA_CMAX in hdr
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        conv.conv2d_autograd(torch.zeros(1, 16, 4, 4), torch.zeros(16, 16, 3, 3), None, 1, 1)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        conv.conv2d_backward(torch.zeros(1, 16, 4, 4), torch.zeros(16, 16, 3, 3), None, torch.zeros(1, 16, 4, 4), 1, 1)
    with pytest.raises(ValueError, match="groups"):
        conv.TrainableConv2d(16, 16, 3, groups=2)
    m = conv.TrainableConv2d(16, 32, 3, stride=2, padding=1, bias=False)
    assert sorted(m.state_dict()) == ["weight"] and sorted(conv.TrainableConv2d(16, 32, 1).state_dict()) == ["bias", "weight"]


def test_trainable_basic_block_folds_with_the_engines_folding():
    from h3d_amd import conv
    from h3d_amd.weights import PackedWeights
    sd = R.make_block_state_dict(16, 32, seed=3)
    blk = conv.TrainableBasicBlock(sd, "level2.tree1.", stride=2)
    assert sorted(n for n, _ in blk.named_parameters()) == ["bias1", "bias2", "weight1", "weight2"]
    pw = PackedWeights.from_tensors({k[len("level2.tree1."):]: v for k, v in sd.items()}, "f32", "cpu")
    for i in (1, 2):
        w, b = pw._fold(pw.sd["conv%d.weight" % i], None, "bn%d" % i)
        assert torch.equal(getattr(blk, "weight%d" % i).detach(), w) and torch.equal(getattr(blk, "bias%d" % i).detach(), b)


ERR_SHAPE, ERR_ARG = -1, -5
GEO = dict(B=1, C=16, H=8, W=8, Cout=32, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)


def _call(L, fn="h3d_conv2d_backward", x=0x1000, x_cs=16, w=0x2000, y=0x3000, y_cs=32, gy=0x4000, gy_cs=32, gx=0x5000, gres=0x6000,
          gw=0x7000, gb=0x8000, flags=1, ws=0x100000, ws_bytes=1 << 40, **geo):
    g = dict(GEO, **geo)
    return getattr(L, fn)(x, x_cs, w, y, y_cs, gy, gy_cs, gx, gres, gw, gb, *[g[k] for k in GEO], flags, ws, ws_bytes, None)


def _bytes(L, n, flags=1, **geo):
    g = dict(GEO, **geo)
    return L.h3d_conv2d_backward_workspace_bytes(*[g[k] for k in GEO], flags, ctypes.byref(n) if n is not None else None)


def test_abi_return_codes_without_a_gpu():
    """Only calls that fail an argument check (or ask for nothing): nothing reaches HIP (the pointers are made up)."""
    from h3d_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(7)
    assert _bytes(L, n) == 0 and n.value % 256 == 0
    # the header's formula: N Cout (gg) + taps Cout ceil64(C) (filter image) + S taps Cout C (partials) + Sb Cout, each rounded up to 256 bytes
    r256 = lambda v: (v + 255) // 256 * 256
    assert n.value == r256(64 * 32 * 4) + r256(9 * 32 * 64 * 4) + r256(1 * 9 * 32 * 16 * 4) + r256(1 * 32 * 4)
    with_relu = n.value
    assert _bytes(L, n, flags=0) == 0 and n.value == with_relu - r256(64 * 32 * 4)
    assert _bytes(L, n, B=8, H=128, W=128) == 0 and n.value > with_relu
    assert _bytes(L, n, kh=7, kw=7, ph=3, pw=3, C=3, Cout=16) == 0 and n.value > 0
    assert _bytes(L, None) == ERR_ARG
    assert _bytes(L, n, flags=2) == ERR_ARG and n.value == 0 and b"flags" in L.h3d_last_error()
    for bad in (dict(B=0), dict(C=0), dict(H=-1), dict(W=0), dict(Cout=0), dict(kh=0), dict(sw=0), dict(dh=0), dict(ph=-1),
                dict(kh=11, kw=11, ph=0, pw=0), dict(kh=65, ph=40)):
        assert _bytes(L, n, **bad) == ERR_SHAPE, bad
        for fn in ("h3d_conv2d_backward", "h3d_conv2d_backward_general"):
            assert _call(L, fn, **bad) == ERR_SHAPE, bad
    for fn in ("h3d_conv2d_backward", "h3d_conv2d_backward_general"):
        assert _call(L, fn, x_cs=12) == ERR_SHAPE and b"channel stride" in L.h3d_last_error()
        assert _call(L, fn, x_cs=18) == ERR_SHAPE
        assert _call(L, fn, gy_cs=16) == ERR_SHAPE
        assert _call(L, fn, y_cs=30) == ERR_SHAPE
        assert _call(L, fn, x=0) == ERR_ARG
        assert _call(L, fn, w=0) == ERR_ARG
        assert _call(L, fn, gy=0) == ERR_ARG
        assert _call(L, fn, y=0) == ERR_ARG and b"y" in L.h3d_last_error()
        assert _call(L, fn, flags=4) == ERR_ARG
        for k in ("x", "y", "gy", "gx", "gres"):
            assert _call(L, fn, **{k: 0x1004}) == ERR_ARG and b"aligned" in L.h3d_last_error(), k
        assert _call(L, fn, ws_bytes=1024) == ERR_ARG and b"workspace" in L.h3d_last_error()
        assert _call(L, fn, ws=0) == ERR_ARG and b"workspace" in L.h3d_last_error()
        assert _call(L, fn, ws=0x100010) == ERR_ARG and b"workspace" in L.h3d_last_error()
        # without the ReLU bit y is not read: NULL, any stride
        assert _call(L, fn, flags=0, y=0, y_cs=0, ws=0) == ERR_ARG and b"workspace" in L.h3d_last_error()
        # no output asked for: nothing to do
        assert _call(L, fn, gx=0, gres=0, gw=0, gb=0, ws=0) == 0
