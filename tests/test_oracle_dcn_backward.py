"""CPU (-m "not gpu"): the oracle of dcn_v2_backward (tests/dcn_backward_ref.py: autograd over oracle/dcn.py) pinned by gradcheck and by
hand-derived known answers that do not depend on it; the C ABI declares and binds the new entry points; and the conditions under which
tests/test_gpu_dcn_lattice.py compares the operator and its backward with torch.equal on the quarter-pixel lattice (lattice_ref.dcn_grid_case)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dcn_backward_ref as R
import lattice_ref as LR
from h3d_amd import _lib
from oracle import dcn as odcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gradcheck(seed, B, C, Co, H, W, k, s, p, d, dg):
    x, w, b, off, m, _ = R.make_case(seed, B, C, Co, H, W, k, s, p, d, dg, int_range=2, outside=0.0)
    leaves = [t.double().requires_grad_(True) for t in (x, w, b, off, m)]
    assert torch.autograd.gradcheck(lambda x_, w_, b_, o_, m_: R.forward(x_, w_, b_, o_, m_, k, s, p, d, dg), leaves,
                                    eps=1e-6, atol=1e-6, rtol=1e-5)


def test_oracle_wrapper_gradcheck_dg2():
    _gradcheck(1, 1, 4, 2, 4, 5, (3, 3), 1, 1, 1, 2)


def test_oracle_wrapper_gradcheck_stride2_dilation2():
    _gradcheck(2, 1, 2, 3, 7, 6, (3, 3), 2, 2, 2, 1)


def test_zero_offsets_unit_mask_is_conv2d():
    gen = torch.Generator().manual_seed(3)
    B, C, Co, H, W = 2, 3, 4, 6, 7
    x = torch.rand(B, C, H, W, generator=gen, dtype=torch.float64)
    w = torch.rand(Co, C, 3, 3, generator=gen, dtype=torch.float64) - 0.5
    b = torch.rand(Co, generator=gen, dtype=torch.float64)
    go = torch.rand(B, Co, H, W, generator=gen, dtype=torch.float64) - 0.5
    gi, _, _, gw, gb = R.oracle_grads(x, w, b, torch.zeros(B, 18, H, W), torch.ones(B, 9, H, W), go, (3, 3), 1, 1, 1, 1)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    ri, rw, rb = torch.autograd.grad(F.conv2d(leaves[0], leaves[1], leaves[2], 1, 1), leaves, go)
    for a, r in ((gi, ri), (gw, rw), (gb, rb)):
        assert float((a - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max()))


def test_all_samples_past_the_gate_give_zero_gradients():
    x, w, b, off, m, go = R.make_case(4, 2, 4, 3, 6, 5, dg=2, outside=0.0)
    off = off + 50.0            # every position >= H and >= W
    gi, goff, gm, gw, gb = R.oracle_grads(x, w, b, off, m, go, (3, 3), 1, 1, 1, 2)
    for g in (gi, goff, gm, gw):
        assert float(g.abs().max()) == 0.0
    assert torch.allclose(gb, go.double().sum((0, 2, 3)), rtol=1e-13, atol=0)


def test_integer_offsets_right_hand_derivative_and_zero_on_the_gate():
    k, s, p, d, dg = (3, 3), 1, 1, 1, 1
    B, C, Co, H, W = 1, 2, 3, 5, 5
    x, w, b, off, m, go = R.make_case(5, B, C, Co, H, W, k, s, p, d, dg, int_range=3, outside=0.0, fraction=False)
    x, w, b, off, m, go = [t.double() for t in (x, w, b, off, m, go)]
    goff = R.oracle_grads(x, w, b, off, m, go, k, s, p, d, dg)[1]
    f0 = float((R.forward(x, w, b, off, m, k, s, p, d, dg) * go).sum())
    ys = torch.arange(H).view(H, 1).double() - p
    xs = torch.arange(W).view(1, W).double() - p
    on_gate = torch.zeros_like(off, dtype=torch.bool)
    for t in range(9):
        h_im = ys + (t // 3) + off[0, 2 * t]
        w_im = xs + (t % 3) + off[0, 2 * t + 1]
        g = (h_im == -1) | (w_im == -1)
        on_gate[0, 2 * t] = g
        on_gate[0, 2 * t + 1] = g
    n_gate = int(on_gate.sum())
    assert 0 < n_gate < off.numel()
    step = 1e-6
    flat = off.reshape(-1)
    for j in range(flat.numel()):
        if on_gate.reshape(-1)[j]:
            assert float(goff.reshape(-1)[j]) == 0.0, j           # gated: zero as in the reference
            continue
        o2 = flat.clone()
        o2[j] += step
        fd = (float((R.forward(x, w, b, o2.view_as(off), m, k, s, p, d, dg) * go).sum()) - f0) / step
        assert abs(fd - float(goff.reshape(-1)[j])) <= 1e-4, (j, fd, float(goff.reshape(-1)[j]))


def test_header_declares_and_binding_binds_dcn_v2_backward():
    hdr = open(os.path.join(ROOT, "include", "h3d.h")).read()
    declared = set(re.findall(r"\b(h3d_[a-z0-9_]+)\s*\(", hdr))
    for name in ("h3d_dcn_v2_backward", "h3d_dcn_v2_backward_workspace_bytes"):
        assert name in declared and name in _lib.SIGNATURES, name
    L = _lib.lib()
    import ctypes
    n = ctypes.c_size_t(0)
    assert L.h3d_dcn_v2_backward_workspace_bytes(2, 64, 16, 16, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, ctypes.byref(n)) == 0
    col = 2 * 9 * 64 * 16 * 16 * 4                                  # the [B, 9C, Ho*Wo] buffer the workspace must not hold
    assert 0 < n.value and n.value - 2 * 64 * 16 * 16 * 4 < col     # (beyond the NHWC copy of the input)
    assert L.h3d_dcn_v2_backward_workspace_bytes(2, 64, 16, 16, 64, 3, 3, 1, 1, 1, 1, 1, 1, 3, ctypes.byref(n)) == -1
    assert b"deformable_group" in L.h3d_last_error()
    assert L.h3d_dcn_v2_backward(*([None] * 11), 1, 16, 4, 4, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1, None, 0, None) == -5


# ---- the quarter-pixel lattice cases of tests/test_gpu_dcn_lattice.py ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LR.DCN_GRID_CASES))
def test_grid_cases_are_exact_in_fp32_and_hold_every_border_class(name):
    seed, B, C, Co, H, W, k, s, p, d, dg = LR.DCN_GRID_CASES[name]
    x, w, b, off, m, gy = LR.dcn_grid(name)
    for t, lo, hi in ((x, -3, 3), (gy, -3, 3), (w, -1, 1), (b, -4, 4)):
        assert torch.equal(t, t.round()) and lo <= float(t.min()) and float(t.max()) <= hi
    assert torch.equal(off * 4, (off * 4).round()) and torch.equal(m * 8, (m * 8).round()) and set((m * 8).unique().tolist()) == set(range(9))
    near = off.abs() < H + W                                                 # (the tenth that was pushed past the gate lies beyond)
    assert 0.05 <= float((~near).float().mean()) <= 0.15 and float(off[near].abs().max()) <= 5.75
    fh, fw = LR.dcn_fractional_share(off)
    assert fh >= LR.DCN_MIN_FRACTIONAL and fw >= LR.DCN_MIN_FRACTIONAL, (fh, fw)
    classes = LR.dcn_sample_classes(*LR.dcn_positions(off, H, W, k, s, p, d), H, W)
    assert min(classes.values()) >= 1, classes
    # forward and all five gradients: the float32 oracle gives the float64 oracle's bits, on a grid of 1/128
    y64 = R.forward(*[t.double() for t in (x, w, b, off, m)], k, s, p, d, dg)
    assert torch.equal(R.forward(x, w, b, off, m, k, s, p, d, dg).double(), y64) and torch.equal(y64 * 128, (y64 * 128).round())
    g64 = R.oracle_grads(x, w, b, off, m, gy, k, s, p, d, dg, torch.float64)
    g32 = R.oracle_grads(x, w, b, off, m, gy, k, s, p, d, dg, torch.float32)
    for nm, a, r in zip(R.NAMES, g32, g64):
        assert torch.equal(a.double(), r), nm
        assert torch.equal(r * 128, (r * 128).round()) and float(r.abs().max()) > 0, nm
    y, g = LR.dcn_grid_exact(name)
    assert torch.equal(y.double(), y64) and all(torch.equal(a.double(), r) for a, r in zip(g, g64))
    # partial sums in ANY order stay exact: the sum of the absolute values of a tensor's terms, in units of its grid, is below 2^24.  For
    # the forward, grad_input, grad_mask, grad_weight and grad_bias that sum is the same oracle on |x|, |w|, |grad_y| (a blend of |x| is at
    # least |the blend of x|).  grad_offset (grid 1/32: corner differences times lw / lh on 1/4, times the mask on 1/8) has no such
    # substitute; its own values leave a factor of 64 below 2^24 for partial sums that exceed the final sum.
    ax, aw, ag = x.abs(), w.abs(), gy.abs()
    ya = odcn.dcn_v2_forward_absbound(x, w, off, m, k[0], k[1], s, s, p, p, d, d, dg) + b.abs().double().view(1, -1, 1, 1)
    assert float(ya.max()) * 128 < 2.0 ** 24
    ga = R.oracle_grads(ax, aw, b, off, m, ag, k, s, p, d, dg, torch.float64)
    for i, unit in ((0, 128.0), (2, 16.0), (3, 128.0), (4, 1.0)):            # (grad_mask holds no mask factor: bilinear weights on 1/16)
        assert torch.equal(g64[i] * unit, (g64[i] * unit).round()), R.NAMES[i]
        assert bool((ga[i] >= g64[i].abs()).all()) and float(ga[i].max()) * unit < 2.0 ** 24, (R.NAMES[i], float(ga[i].max()) * unit)
    assert torch.equal(g64[1] * 32, (g64[1] * 32).round()) and float(g64[1].abs().max()) * 32 * 64 < 2.0 ** 24


def test_grid_case_list_is_what_the_gpu_file_runs():
    assert sorted(LR.DCN_GRID_MFMA) == ["m_16to27_20x37", "m_2x48to7_13x11", "m_512to256_16x16", "m_64to64_24x40"]
    for c in LR.DCN_GRID_MFMA.values():
        assert c[6:] == ((3, 3), 1, 1, 1, 1) and c[2] % 16 == 0                  # the matrix-core kernels' configuration
    assert {c[6:] for c in LR.DCN_GRID_GENERAL.values()} == {((3, 3), 2, 1, 1, 1), ((3, 3), 1, 2, 2, 2), ((3, 3), 1, 1, 1, 4), ((1, 1), 1, 0, 1, 1),
                                                             ((3, 1), 1, 1, 1, 3)}
    a, b = LR.dcn_grid_case(*LR.DCN_GRID_CASES["g_s2"]), LR.dcn_grid_case(*LR.DCN_GRID_CASES["g_s2"])
    assert all(torch.equal(s, t) for s, t in zip(a, b))
