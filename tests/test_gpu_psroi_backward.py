"""GPU: deformable PS-ROI pooling backward (csrc/psroi_bwd.hip) against the numpy restatement tests/psroi_grad_ref.py: every gradient
element within the restatement's fp32 error bound (n_terms + c) * 2^-24 * sum |contributions|, grad_trans bit-identical from run to run
and between streams, both grad_input paths, the chunked table, the guards, exact equality on the lattice case, the reference's
check_gradient_dpooling shapes through the autograd function, the modulated backward and the trainable modules."""
import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
from h3d_amd import dcn_v2
import psroi_grad_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, f32))).to(DEV)


def _operator(go, inp, rois, trans, no_trans, scale, P, part, spp, tstd, direct=False, count=None):
    """Forward (for output_count) + backward on the GPU -> (grad_input, grad_trans | None, count) as torch tensors."""
    C = inp.shape[1]
    x, r = _t(inp), _t(rois)
    t = torch.empty(0, device=DEV) if no_trans else _t(trans)
    if count is None:
        _, count = dcn_v2.dcn_v2_psroi_pooling_forward(x, r, t, no_trans, scale, C, 1, P, part, spp, tstd)
    gi, gt = dcn_v2._dcn_v2_psroi_pooling_backward(_t(go), x, r, t, count, no_trans, scale, C, 1, P, part, spp, tstd, direct=direct)
    return gi, (None if no_trans else gt), count


def _check_operator(name, go, inp, rois, trans, no_trans, scale, P, part, spp, tstd, direct=False):
    gi, gt, count = _operator(go, inp, rois, trans, no_trans, scale, P, part, spp, tstd, direct)
    (ri, rt), (bi, bt) = G.bounds(go, inp, rois, trans, count.cpu().numpy(), no_trans, scale, P, part, spp, tstd)
    G.check(name + " grad_input", gi.cpu().numpy(), ri, bi)
    if not no_trans:
        G.check(name + " grad_trans", gt.cpu().numpy(), rt, bt)
    return gi, gt


def _modulated(go, inp, rois, om, scale, P, spp, tstd, direct=False):
    return dcn_v2._dcn_pooling_modulated_backward(_t(go), _t(inp), _t(rois), _t(om), scale, P, inp.shape[1], 1, P, spp, tstd, direct=direct)


def _check_modulated(name, go, inp, rois, om, scale, P, spp, tstd, direct=False):
    gi, gom = _modulated(go, inp, rois, om, scale, P, spp, tstd, direct)
    (ri, rt), (bi, bt) = G.bounds(go, inp, rois, om, None, 0, scale, P, P, spp, tstd, mask=np.asarray(om)[:, 2])
    G.check(name + " grad_input", gi.cpu().numpy(), ri, bi)
    G.check(name + " grad_offset_mask", gom.cpu().numpy(), rt, bt)
    return gi, gom


CASES = []
_g = np.random.default_rng(2025)
for _i in range(12):
    _P = int(_g.choice([1, 3, 7]))
    _ncls = int(_g.choice([1, 2, 4]))
    _C = int(_g.choice([c for c in (1, 3, 16, 64) if c % _ncls == 0]))
    CASES.append(dict(B=int(_g.integers(1, 4)), C=_C, H=int(_g.choice([5, 13, 32])), W=int(_g.choice([5, 13, 32])),
                      R=int(_g.choice([1, 7, 60])), P=_P, part=int(_g.choice([_P, max(1, _P - 2)])), spp=int(_g.choice([1, 2, 4])),
                      scale=float(_g.choice([1.0, 0.25, 0.0625])), tstd=float(_g.choice([0.0, 0.1, 1.0])), ncls=_ncls,
                      no_trans=bool(_i % 5 == 4), seed=_i))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%(B)dC%(C)d_%(H)dx%(W)d_R%(R)d_P%(P)d_part%(part)d_spp%(spp)d_k%(ncls)d" % c)
def test_random_cases_against_bounds(case):
    c = case
    rng = np.random.default_rng(1000 + c["seed"])
    inp = rng.normal(size=(c["B"], c["C"], c["H"], c["W"])).astype(f32)
    rois = G.random_rois(rng, c["R"], c["B"], c["H"], c["W"], c["scale"])
    trans = None if c["no_trans"] else rng.normal(size=(c["R"] + 3, 2 * c["ncls"], c["part"], c["part"])).astype(f32)
    go = rng.normal(size=(c["R"], c["C"], c["P"], c["P"])).astype(f32)
    args = (go, inp, rois, trans, int(c["no_trans"]), c["scale"], c["P"], c["part"], c["spp"], c["tstd"])
    gi, gt = _check_operator("random", *args)
    assert gi.shape == inp.shape
    if c["no_trans"]:
        return
    assert gt.shape == trans.shape and not gt[c["R"]:].any()           # rows of trans beyond the rois: zero
    # grad_trans: no atomics, a fixed order -- the same bits on a second run and on a side stream
    _, gt2, count = _operator(*args)
    assert torch.equal(gt, gt2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _, gt3, _ = _operator(*args, count=count)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(gt, gt3)


def test_both_grad_input_paths_by_construction():
    """Rois of a few pixels at scale 1/16 are combined in LDS; one roi over a whole 64 x 64 map (C 64) is added directly: the path is a
    function of the geometry, which the host evaluates with the kernel's code."""
    rng = np.random.default_rng(21)
    B, C, H, P, spp, scale, tstd = 2, 64, 64, 7, 4, 1 / 16, 0.1
    inp = rng.normal(size=(B, C, H, H)).astype(f32)
    x, y = rng.uniform(0, 900, 6), rng.uniform(0, 900, 6)
    small = np.stack([rng.integers(0, B, 6), x, y, x + rng.uniform(16, 80, 6), y + rng.uniform(16, 80, 6)], 1).astype(f32)
    whole = np.array([[1, 0, 0, 1023, 1023]], f32)
    for name, rois, want in (("small", small, 1), ("whole", whole, 2)):
        R = rois.shape[0]
        trans = (rng.normal(size=(R, 2, P, P)) * 0.5).astype(f32)
        go = rng.normal(size=(R, C, P, P)).astype(f32)
        paths = [dcn_v2.psroi_backward_path(rois[n], trans[n], inp.shape, False, scale, P, P, spp, tstd) for n in range(R)]
        assert paths == [want] * R, (name, paths)
        gi, gt = _check_operator(name, go, inp, rois, trans, 0, scale, P, P, spp, tstd)
        # the other form of the same sum: every contribution its own global atomic; grad_trans does not depend on the path
        assert dcn_v2.psroi_backward_path(rois[0], trans[0], inp.shape, False, scale, P, P, spp, tstd, direct=True) == 2
        gid, gtd = _check_operator(name + " direct", go, inp, rois, trans, 0, scale, P, P, spp, tstd, direct=True)
        assert torch.equal(gt, gtd)


def test_several_channel_groups_per_bin_and_a_chunked_table():
    rng = np.random.default_rng(22)
    # C 64, P 7: 64 * 49 elements per class, channel groups G = 5 -> 13 channels per thread
    inp = rng.normal(size=(2, 64, 13, 13)).astype(f32)
    rois = G.random_rois(rng, 5, 2, 13, 13, 0.25)
    trans = rng.normal(size=(5, 2, 7, 7)).astype(f32)
    go = rng.normal(size=(5, 64, 7, 7)).astype(f32)
    _, gt = _check_operator("C64 P7", go, inp, rois, trans, 0, 0.25, 7, 7, 2, 0.1)
    # (two channel tiles per roi here: the tiling is the geometry's whether or not the LDS tile is used, so grad_trans keeps its bits)
    _, gtd, count = _operator(go, inp, rois, trans, 0, 0.25, 7, 7, 2, 0.1, direct=True)
    _, gtn = dcn_v2._dcn_v2_psroi_pooling_backward(_t(go), _t(inp), _t(rois), _t(trans), count, 0, 0.25, 64, 1, 7, 7, 2, 0.1, need=(False, True))
    assert torch.equal(gt, gtd) and torch.equal(gt, gtn)
    # P 13, spp 4: 169 * 16 = 2704 samples > 2048, the table is walked in chunks of whole sample columns
    inp = rng.normal(size=(1, 4, 32, 32)).astype(f32)
    rois = G.random_rois(rng, 3, 1, 32, 32, 0.25)
    trans = rng.normal(size=(3, 4, 13, 13)).astype(f32)
    go = rng.normal(size=(3, 4, 13, 13)).astype(f32)
    _, gt = _check_operator("P13 spp4", go, inp, rois, trans, 0, 0.25, 13, 13, 4, 0.1)
    om = rng.normal(size=(3, 3, 13, 13)).astype(f32)
    _, gom = _check_modulated("P13 spp4 modulated", go, inp, rois, om, 0.25, 13, 4, 0.1)
    # the channel loop is tiled by the geometry whether or not the LDS tile is used: the same grad_trans bits with every contribution
    # its own atomic, and when grad_input is not asked for
    _, gtd, count = _operator(go, inp, rois, trans, 0, 0.25, 13, 13, 4, 0.1, direct=True)
    assert torch.equal(gt, gtd)
    _, gtn = dcn_v2._dcn_v2_psroi_pooling_backward(_t(go), _t(inp), _t(rois), _t(trans), count, 0, 0.25, 4, 1, 13, 13, 4, 0.1, need=(False, True))
    assert torch.equal(gt, gtn)
    assert torch.equal(gom, _modulated(go, inp, rois, om, 0.25, 13, 4, 0.1, direct=True)[1])
    assert torch.equal(gom, dcn_v2._dcn_pooling_modulated_backward(_t(go), _t(inp), _t(rois), _t(om), 0.25, 13, 4, 1, 13, 4, 0.1,
                                                                   need=(False, True))[1])


def test_edge_rois_and_guards():
    """The forward's edge list plus invalid batch indices and non-finite coordinates, in both modes: far-outside rois give all-zero
    rows, rois with an invalid batch index contribute nothing, rois with non-finite coordinates follow the reference's arithmetic (the
    restatement's), and none of them changes another roi's gradient.  (The geometry of exactly these
    rois is checked on the host first: tests/test_oracle_psroi_backward.py.)"""
    rng = np.random.default_rng(7)
    inp = rng.normal(size=G.EDGE_SHAPE).astype(f32)
    rois = np.concatenate([G.EDGE_ROIS, G.BAD_ROIS])
    R, C = rois.shape[0], inp.shape[1]
    n_edge = G.EDGE_ROIS.shape[0]
    trans = rng.normal(size=(R, 4, 3, 3)).astype(f32)
    go = rng.normal(size=(R, C, 7, 7)).astype(f32)
    gi, _ = _check_operator("edge no_trans", go, inp, rois, None, 1, 0.25, 7, 7, 4, 0.0)
    gi, gt = _check_operator("edge trans", go, inp, rois, trans, 0, 0.25, 7, 3, 4, 0.5)
    # (a roi with infinite coordinates has an infinite width: its own translation gradient is 0 * inf, as in the reference)
    assert torch.isfinite(gi).all() and torch.isfinite(gt[:n_edge]).all()
    assert not gt[3].any() and not gt[4].any()                                              # far outside
    bad_batch = [n_edge + i for i in range(6)]                                              # NaN, -1, B, +-inf, 1e30
    assert not gt[bad_batch].any()
    # without the invalid rois: the same grad_trans rows, bit for bit
    keep = [n for n in range(R) if n not in bad_batch]
    _, gt_keep = _check_operator("edge trans, valid only", go[keep], inp, rois[keep], trans[keep], 0, 0.25, 7, 3, 4, 0.5)
    assert torch.equal(gt[keep].view(torch.int32), gt_keep.view(torch.int32))
    # only invalid rois: nothing at all
    gi0, gt0, _ = _operator(go[bad_batch], inp, rois[bad_batch], trans[bad_batch], 0, 0.25, 7, 3, 4, 0.5)
    assert not gi0.any() and not gt0.any()
    # modulated mode
    om = rng.normal(size=(R, 3, 7, 7)).astype(f32)
    gi, gom = _check_modulated("edge modulated", go, inp, rois, om, 0.25, 7, 4, 0.5)
    assert torch.isfinite(gi).all() and torch.isfinite(gom[:n_edge]).all() and torch.isfinite(gom[:, 2]).all()
    assert not gom[[3, 4] + bad_batch].any()
    _, gom_keep = _check_modulated("edge modulated, valid only", go[keep], inp, rois[keep], om[keep], 0.25, 7, 4, 0.5)
    assert torch.equal(gom[keep].view(torch.int32), gom_keep.view(torch.int32))
    # no rois: zeros, no launch
    gi, gt, _ = _operator(go[:0], inp, rois[:0], trans, 0, 0.25, 7, 3, 4, 0.5)
    assert gi.shape == inp.shape and not gi.any() and gt.shape == trans.shape and not gt.any()
    gi, gom = _modulated(go[:0], inp, rois[:0], om[:0], 0.25, 7, 4, 0.5)
    assert gi.shape == inp.shape and not gi.any() and gom.shape == (0, 3, 7, 7)


def test_lattice_case_is_exact():
    """Every product and every partial sum is exact in fp32 (tests/test_oracle_psroi_backward.py checks the conditions), so the result
    is the float64 restatement's whatever order the atomics arrive in."""
    c = G.lattice_case()
    cfg = (c["scale"], c["P"], c["part"], c["spp"], c["tstd"])
    for direct in (False, True):
        gi, gt, count = _operator(c["grad_out"], c["inp"], c["rois"], c["trans"], 0, *cfg, direct=direct)
        r = G.backward(c["grad_out"], c["inp"], c["rois"], c["trans"], count.cpu().numpy(), 0, *cfg)
        assert torch.equal(gi.cpu().double(), torch.from_numpy(r["g_input"])) and gi.abs().max() > 0
        assert torch.equal(gt.cpu().double(), torch.from_numpy(r["g_trans"])) and gt.abs().max() > 0
        om = np.concatenate([c["trans"][:, :2], np.zeros((c["rois"].shape[0], 1, 2, 2), f32)], 1)       # logit 0: sigmoid 1/2
        gi, gom = _modulated(c["grad_out"], c["inp"], c["rois"], om, c["scale"], c["P"], c["spp"], c["tstd"], direct=direct)
        r = G.backward(c["grad_out"], c["inp"], c["rois"], om, None, 0, *cfg, mask=om[:, 2])
        assert torch.equal(gi.cpu().double(), torch.from_numpy(r["g_input"])) and gi.abs().max() > 0
        assert torch.equal(gom[:, :2].cpu().double(), torch.from_numpy(r["g_trans"][:, :2])) and gom[:, :2].abs().max() > 0


@pytest.mark.parametrize("tstd", [0.0, 0.1])
def test_reference_check_gradient_dpooling_shapes(tstd):
    """DCNv2/test.py:134-166: input [2,3,5,5] * 0.01, 4 rois, offsets [4,2,3,3], scale 1/4, P 3 -- through the autograd function."""
    rng = np.random.default_rng(11)
    inp = (rng.normal(size=(2, 3, 5, 5)) * 0.01).astype(f32)
    N = 4
    x, y = rng.random((N, 1)) * 15, rng.random((N, 1)) * 15
    w, h = rng.random((N, 1)) * 10, rng.random((N, 1)) * 10
    rois = np.concatenate([rng.integers(0, 2, (N, 1)), x, y, x + w, y + h], 1).astype(f32)
    offset = rng.normal(size=(N, 2, 3, 3)).astype(f32)
    go = rng.normal(size=(N, 3, 3, 3)).astype(f32)
    _check_operator("dpooling", go, inp, rois, offset, 0, 0.25, 3, 3, 4, tstd)
    xt, rt, ot = _t(inp).requires_grad_(True), _t(rois).requires_grad_(True), _t(offset).requires_grad_(True)
    out = dcn_v2.dcn_v2_pooling_autograd(xt, rt, ot, 0.25, 3, 3, False, 1, None, 4, tstd)
    ref, cnt = dcn_v2.dcn_v2_psroi_pooling_forward(xt.detach(), rt.detach(), ot.detach(), 0, 0.25, 3, 1, 3, 3, 4, tstd)
    assert torch.equal(out, ref) and out.requires_grad
    out.backward(_t(go))
    (ri, rtr), (bi, bt) = G.bounds(go, inp, rois, offset, cnt.cpu().numpy(), 0, 0.25, 3, 3, 4, tstd)
    G.check("autograd grad_input", xt.grad.cpu().numpy(), ri, bi)
    G.check("autograd grad_offset", ot.grad.cpu().numpy(), rtr, bt)
    assert rt.grad is None                                                       # rois get None
    # needs_input_grad is honoured: an output nobody asks for is not computed
    calls = []
    real = dcn_v2._dcn_v2_psroi_pooling_backward
    try:
        dcn_v2._dcn_v2_psroi_pooling_backward = lambda *a, **k: calls.append(k["need"]) or real(*a, **k)
        for need_x, need_o in ((True, False), (False, True)):
            xt, ot = _t(inp).requires_grad_(need_x), _t(offset).requires_grad_(need_o)
            dcn_v2.dcn_v2_pooling_autograd(xt, _t(rois), ot, 0.25, 3, 3, False, 1, None, 4, tstd).backward(_t(go))
            assert (xt.grad is not None) == need_x and (ot.grad is not None) == need_o
    finally:
        dcn_v2._dcn_v2_psroi_pooling_backward = real
    assert calls == [(True, False), (False, True)]
    gi, gt = real(_t(go), _t(inp), _t(rois), _t(offset), cnt, 0, 0.25, 3, 1, 3, 3, 4, tstd, need=(False, True))
    assert gi is None and torch.equal(gt, ot.grad)
    # the positional twin of the reference's call
    gi, gt = dcn_v2.dcn_v2_psroi_pooling_backward(_t(go), _t(inp), _t(rois), _t(offset), cnt, 0, 0.25, 3, 1, 3, 3, 4, tstd)
    assert torch.equal(gt, ot.grad)
    G.check("function grad_input", gi.cpu().numpy(), ri, bi)
    # it honours the output_count it is given: an element with count <= 0 is skipped
    cnt0 = cnt.clone()
    cnt0[1] = 0
    gi, gt = dcn_v2.dcn_v2_psroi_pooling_backward(_t(go), _t(inp), _t(rois), _t(offset), cnt0, 0, 0.25, 3, 1, 3, 3, 4, tstd)
    (ri, rtr), (bi, bt) = G.bounds(go, inp, rois, offset, cnt0.cpu().numpy(), 0, 0.25, 3, 3, 4, tstd)
    G.check("count 0 grad_input", gi.cpu().numpy(), ri, bi)
    G.check("count 0 grad_trans", gt.cpu().numpy(), rtr, bt)
    assert not gt[1].any()


def test_errors_use_the_forward_texts():
    inp = _t(np.zeros((1, 4, 8, 8)))
    rois = _t([[0, 1, 1, 5, 5]])
    go, cnt = _t(np.zeros((1, 4, 2, 2))), _t(np.ones((1, 4, 2, 2)))
    f = dcn_v2.dcn_v2_psroi_pooling_backward
    with pytest.raises(RuntimeError, match="input channels and output channels must equal"):
        f(go, inp, rois, inp.new(), cnt, 1, 1.0, 3, 1, 2, 2, 2, 0.0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        f(go.cpu(), inp.cpu(), rois.cpu(), inp.new().cpu(), cnt.cpu(), 1, 1.0, 4, 1, 2, 2, 2, 0.0)
    with pytest.raises(RuntimeError, match="expected float32"):
        f(go, inp.double(), rois, inp.new(), cnt, 1, 1.0, 4, 1, 2, 2, 2, 0.0)
    with pytest.raises(RuntimeError, match="group_size"):
        f(go, inp, rois, inp.new(), cnt, 1, 1.0, 4, 2, 2, 2, 2, 0.0)
    with pytest.raises(RuntimeError, match="num_classes"):
        f(go, inp, rois, _t(np.zeros((1, 6, 2, 2))), cnt, 0, 1.0, 4, 1, 2, 2, 2, 0.0)
    with pytest.raises(RuntimeError, match="grad_output"):
        f(go[:, :2], inp, rois, inp.new(), cnt, 1, 1.0, 4, 1, 2, 2, 2, 0.0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        dcn_v2._dcn_pooling_modulated_backward(go, inp, rois, torch.zeros(1, 3, 2, 2), 1.0, 2, 4, 1, 2, 2, 0.0)


def test_modulated_backward_against_restatement():
    """example_mdpooling's geometry (DCNv2/test.py:222-260) shrunk to [2,8,16,16] and 6 rois in a 64-px image, P 3."""
    rng = np.random.default_rng(5)
    inp = rng.normal(size=(2, 8, 16, 16)).astype(f32)
    xy = rng.integers(0, 64, (6, 2))
    wh = rng.integers(0, 16, (6, 2))
    rois = np.concatenate([rng.integers(0, 2, (6, 1)), xy, xy + wh], 1).astype(f32)
    om = rng.normal(size=(6, 3, 3, 3)).astype(f32)
    go = rng.normal(size=(6, 8, 3, 3)).astype(f32)
    gi, gom = _check_modulated("mdpooling", go, inp, rois, om, 0.25, 3, 4, 0.1)
    assert gom[:, 2].abs().max() > 0 and gom[:, :2].abs().max() > 0
    gi2, gom2 = _modulated(go, inp, rois, om, 0.25, 3, 4, 0.1)
    assert torch.equal(gom, gom2)
    gi3, gom3 = dcn_v2._dcn_pooling_modulated_backward(_t(go), _t(inp), _t(rois), _t(om), 0.25, 3, 8, 1, 3, 4, 0.1, need=(False, True))
    assert gi3 is None and torch.equal(gom, gom3)


MODULE_SEED = 4            # the second pass's samples keep >= 1e-3 from every kink (asserted), in float32 and in float64


def _module_setup():
    torch.manual_seed(MODULE_SEED)
    rng = np.random.default_rng(MODULE_SEED)
    P, C, fc = 3, 8, 16
    inp = rng.normal(size=(2, C, 16, 16)).astype(f32)
    rois = G.random_rois(rng, 6, 2, 16, 16, 0.25)
    go = rng.normal(size=(6, C, P, P)).astype(f32)
    kw = dict(spatial_scale=0.25, pooled_size=P, output_dim=C, no_trans=False, sample_per_part=4, trans_std=0.1, deform_fc_dim=fc)
    m = dcn_v2.TrainableDCNPooling(**kw)
    with torch.no_grad():
        m.offset_mask_fc[4].weight.normal_(0, 0.05)
        m.offset_mask_fc[4].bias.normal_(0, 0.5)
    return inp, rois, go, kw, m


def test_trainable_modules():
    inp, rois, go, kw, m = _module_setup()
    sd = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    assert sorted(sd) == sorted("offset_mask_fc.%d.%s" % (i, n) for i in (0, 2, 4) for n in ("weight", "bias"))
    m = m.to(DEV).train()
    ref_module = dcn_v2.DCNPooling(**kw).to(DEV)
    ref_module.load_state_dict(m.state_dict())
    x, r = _t(inp).requires_grad_(True), _t(rois)
    out = m(x, r)
    assert out.requires_grad and torch.equal(out.detach(), ref_module.eval()(x.detach(), r))
    out.backward(_t(go))
    # the module on the CPU in float64 (torch MLP + the restatement), and the same replica in float32 against itself in float64: the
    # yardstick measures the reference alone; summation orders differ, hence the factor 4
    o64, gx64, gp64, kink64 = G.module_replica(sd, inp, rois, go, 0.25, 3, 4, 0.1, torch.float64)
    o32, gx32, gp32, kink32 = G.module_replica(sd, inp, rois, go, 0.25, 3, 4, 0.1, torch.float32)
    assert kink64 >= 1e-3 and kink32 >= 1e-3, (kink64, kink32)
    np.testing.assert_allclose(out.detach().cpu().numpy(), o64.numpy(), atol=1e-5 * max(1.0, np.abs(inp).max()), rtol=0)

    def compare(name, got, g64, g32):
        assert got is not None, name
        e32 = float((g32.double() - g64).abs().max())
        err = float((got.detach().cpu().double() - g64).abs().max())
        print("%s: max |g64| %.3g, fp32 replica error %.3g, kernel error %.3g" % (name, float(g64.abs().max()), e32, err))
        assert float(g64.abs().max()) > 0 and err <= 4 * e32, (name, err, e32)
    compare("input.grad", x.grad, gx64, gx32)
    for name, p in m.named_parameters():
        compare(name, p.grad, gp64[name], gp32[name])
    # TrainableDCNv2Pooling equals the function form
    rng = np.random.default_rng(9)
    offset = rng.normal(size=(6, 2, 3, 3)).astype(f32)
    for no_trans in (False, True):
        mod = dcn_v2.TrainableDCNv2Pooling(0.25, 3, 8, no_trans, sample_per_part=4, trans_std=0.1)
        assert not list(mod.parameters())
        x1, o1 = _t(inp).requires_grad_(True), _t(offset).requires_grad_(True)
        y1 = mod(x1, r, o1)
        x2, o2 = _t(inp).requires_grad_(True), _t(offset).requires_grad_(True)
        y2 = dcn_v2.dcn_v2_pooling_autograd(x2, r, x2.new() if no_trans else o2, 0.25, 3, 8, no_trans, 1, None, 4, 0.1)
        assert torch.equal(y1, y2)
        y1.backward(_t(go))
        y2.backward(_t(go))
        assert (o1.grad is None) == no_trans and (no_trans or torch.equal(o1.grad, o2.grad))
        _, cnt = dcn_v2.dcn_v2_psroi_pooling_forward(x1.detach(), r, o1.detach(), int(no_trans), 0.25, 8, 1, 3, 3, 4, 0.1)
        (ri, _), (bi, _) = G.bounds(go, inp, rois, offset, cnt.cpu().numpy(), int(no_trans), 0.25, 3, 3, 4, 0.1)
        G.check("module grad_input", x1.grad.cpu().numpy(), ri, bi)
        G.check("function grad_input", x2.grad.cpu().numpy(), ri, bi)


def test_inference_classes_still_refuse():
    """After the trainable classes have been imported and used, the inference names behave as before."""
    inp, rois, go, kw, m = _module_setup()
    x, r = _t(inp), _t(rois)
    m.to(DEV)(x.clone().requires_grad_(True), r).sum().backward()
    ref = dcn_v2.DCNPooling(**kw).to(DEV).train()
    y = ref(x, r)
    with pytest.raises(RuntimeError, match="inference-only"):
        y.sum().backward()
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        ref(xg, r)
    with pytest.raises(RuntimeError, match="inference-only"):
        dcn_v2.dcn_v2_pooling(xg, r, x.new(), 0.25, 3, 8, True)
    off = _t(np.zeros((6, 2, 3, 3))).requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        dcn_v2.DCNv2Pooling(0.25, 3, 8, False)(x, r, off)
    assert isinstance(m, dcn_v2.DCNPooling) and isinstance(dcn_v2.TrainableDCNv2Pooling(0.25, 3, 8, True), dcn_v2.DCNv2Pooling)
