"""GPU: `h3d_heads_backward` (csrc/heads_bwd.hip), `heads_autograd` and `TrainableHeads` against the torch restatement of the heads
differentiated by autograd (tests/heads_grad_ref.py).

The rule of every comparison (per case, per gradient tensor; tests/test_gpu_dcn_backward.py's, factor 4): e32 = max |g32 - g64| of the
restatement's own float32 autograd run on the CPU, and max |g_gpu - g64| <= 4 * e32 + 1e-7 * max |g64|.  The generated inputs are
gridded so that the ReLU gate is the same for every correct implementation (heads_grad_ref's docstring).  The observed ratios are
printed (`pytest -s`) and recorded in DESIGN.md section 18."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import heads_grad_ref as R
import losses_ref as LR
from gpu_helpers import DEV
from h3d_amd import _lib, arch, heads, losses, model, smpl, synth, targets
from h3d_amd.detector import Opt

pytestmark = pytest.mark.gpu
SENT = 777.0


def feat_view(y, in_cs=80, coff=8):
    """y [B,64,H,W] cpu -> an NHWC view of 64 channels inside a [B,H,W,in_cs] device buffer whose other channels are NaN."""
    B, _, H, W = y.shape
    coff = min(coff, in_cs - 64)
    buf = torch.full((B, H, W, in_cs), float("nan"), dtype=torch.float32, device=DEV)
    buf[..., coff:coff + 64] = y.permute(0, 2, 3, 1).to(DEV)
    return buf[..., coff:coff + 64]


def gpu_grads(case, want=(True,) * 5, in_cs=80):
    """(grad_feat [B,64,H,W], gw1, gb1, gw2, gb2) of one head through h3d_amd.heads.heads_backward; None where not requested."""
    y, w1, b1, w2, b2, gz = case
    gf, g = heads.heads_backward(feat_view(y, in_cs), [(w1.to(DEV), b1.to(DEV), w2.to(DEV), gz.to(DEV), want[1:])], want_feat=want[0])
    torch.cuda.synchronize()
    return (None if gf is None else gf.permute(0, 3, 1, 2),) + tuple(g[0])


# ---- against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_small_shapes_vs_restatement(name):
    g64, e32 = R.bounds(name)
    R.check(name, gpu_grads(R.case(name)), g64, e32)


@pytest.mark.parametrize("name", sorted(R.MODEL_CASES))
def test_model_shape_128x128_vs_restatement(name):
    g64, e32 = R.bounds(name)
    R.check(name, gpu_grads(R.case(name), in_cs=64), g64, e32)


def test_ungridded_random_case_with_a_gate_margin():
    case = R.make_random_case()
    lo, hi = R.gate_margin(case)
    assert lo >= 1e-3 * hi
    g64, e32 = R.bounds_of(case)
    R.check("random 4x4", gpu_grads(case), g64, e32)


# ---- the raw entry point ---------------------------------------------------------------------------------------------------------------
def raw_call(fv, specs, gfeat_ptr, hc, ws=None):
    """specs: per head dict(w1, b1, w2, C, go=tensor|None, out=(ptr, ptr, ptr, ptr)); everything on the device already."""
    B, H, W = fv.shape[:3]
    arr = (heads.H3dHeadsBwdHead * len(specs))()
    for i, s in enumerate(specs):
        arr[i].w1, arr[i].b1, arr[i].w2, arr[i].C = s["w1"].data_ptr(), s["b1"].data_ptr(), s["w2"].data_ptr(), s["C"]
        arr[i].grad_out = 0 if s["go"] is None else s["go"].data_ptr()
        arr[i].grad_w1, arr[i].grad_b1, arr[i].grad_w2, arr[i].grad_b2 = s["out"]
    if ws is None:
        ws = heads._workspace(fv.device, B, H, W, hc, [s["C"] for s in specs])
    rc = _lib.lib().h3d_heads_backward(fv.data_ptr(), fv.stride(2), B, H, W, hc, len(specs), arr, gfeat_ptr, ws.data_ptr(), ws.numel(),
                                       _lib.stream_ptr())
    _lib.check(rc, "h3d_heads_backward")
    torch.cuda.synchronize()


def two_head_cases():
    a = R.make_case(500, 2, 9, 33, 64, 3)
    c = R.make_case(501, 2, 9, 33, 64, 34)
    return a, (a[0],) + c[1:]


def test_mixed_heads_with_a_skipped_head_between_two_live_ones():
    a, c = two_head_cases()
    fv = feat_view(a[0])
    B, H, W = fv.shape[:3]

    def spec(case, live, off=0):
        y, w1, b1, w2, b2, gz = case
        bufs = [torch.full((t.numel() + 8,), SENT, device=DEV) for t in (w1, b1, w2, b2)]
        return dict(w1=w1.to(DEV), b1=b1.to(DEV), w2=w2.to(DEV), C=w2.shape[0], go=gz.to(DEV) if live else None,
                    out=tuple(b.data_ptr() + 4 * off for b in bufs), bufs=bufs, shapes=[t.shape for t in (w1, b1, w2, b2)])
    skipped = R.make_case(502, 2, 9, 33, 64, 72)
    specs = [spec(a, True), spec((a[0],) + skipped[1:], False), spec(c, True)]
    gf = torch.full((B * H * W * 64 + 8,), SENT, device=DEV)
    raw_call(fv, specs, gf.data_ptr(), 64)
    assert all(bool((b == SENT).all()) for b in specs[1]["bufs"]), "a skipped head's buffers were written"
    assert bool((gf[-8:] == SENT).all())
    got_f = gf[:-8].reshape(B, H, W, 64).permute(0, 3, 1, 2)
    singles = []
    for case, s in ((a, specs[0]), (c, specs[2])):
        g64, e32 = R.bounds_of(case)
        got = [b[:sh.numel()].reshape(sh) for b, sh in zip(s["bufs"], s["shapes"])]
        assert all(bool((b[sh.numel():] == SENT).all()) for b, sh in zip(s["bufs"], s["shapes"]))
        R.check("mixed C=%d" % s["C"], [None] + got, g64, e32)
        one = gpu_grads(case)
        for x, y in zip(got, one[1:]):
            assert torch.equal(x, y)                                 # the same bits as the single-head call
        singles.append((one[0], g64[0], R.grads(*case, dtype=torch.float32)[0]))
    # grad_feat of the two heads: the sum of the single-head runs -- in head order, in fp32: the same bits -- and within the rule
    assert torch.equal(got_f, singles[0][0] + singles[1][0])
    s64 = singles[0][1] + singles[1][1]
    s32 = singles[0][2] + singles[1][2]
    R.check("mixed grad_feat", [got_f], [s64], [float((s32.double() - s64).abs().max())])


def test_every_subset_of_outputs_and_a_second_call_give_the_same_bits():
    case = R.make_case(501, 2, 9, 33, 64, 34)
    full = gpu_grads(case)
    again = gpu_grads(case)
    for nm, x, y in zip(R.NAMES, full, again):
        assert torch.equal(x, y), "run to run: " + nm
    for want in itertools.product((False, True), repeat=5):
        if not any(want):
            continue
        got = gpu_grads(case, want)
        for nm, w, x, y in zip(R.NAMES, want, got, full):
            assert (x is None) == (not w)
            if w:
                assert torch.equal(x, y), (want, nm)


def test_sentinels_behind_every_output_at_misaligned_base_pointers():
    case = R.make_case(503, 1, 17, 40, 256, 3)
    y, w1, b1, w2, b2, gz = case
    full = gpu_grads(case)
    fv = feat_view(y)
    B, H, W = fv.shape[:3]
    PAD = 16
    bufs = [torch.full((t.numel() + 2 * PAD,), SENT, device=DEV) for t in (w1, b1, w2, b2)]
    offs = (1, 3, 5, 7)                                             # floats: 4-byte aligned only
    gf = torch.full((B * H * W * 64 + 2 * PAD,), SENT, device=DEV)
    spec = dict(w1=w1.to(DEV), b1=b1.to(DEV), w2=w2.to(DEV), C=3, go=gz.to(DEV),
                out=tuple(b.data_ptr() + 4 * o for b, o in zip(bufs, offs)))
    raw_call(fv, [spec], gf.data_ptr() + 4 * 4, 256)               # grad_feat: 16-byte aligned (its contract), off the allocation's 256
    for b, o, t, ref in zip(bufs, offs, (w1, b1, w2, b2), full[1:]):
        n = t.numel()
        assert bool((b[:o] == SENT).all()) and bool((b[o + n:] == SENT).all())
        assert torch.equal(b[o:o + n].reshape(ref.shape), ref)
    n = B * H * W * 64
    assert bool((gf[:4] == SENT).all()) and bool((gf[4 + n:] == SENT).all())
    assert torch.equal(gf[4:4 + n].reshape(B, H, W, 64).permute(0, 3, 1, 2), full[0])
    # a short workspace is an error, not an overrun
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        raw_call(fv, [spec], gf.data_ptr() + 16, 256, ws=ws)


def test_non_default_stream():
    case = R.make_case(504, 2, 9, 33, 64, 2)
    full = gpu_grads(case)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        got = gpu_grads(case)
    for x, y in zip(got, full):
        assert torch.equal(x, y)


# ---- autograd function and module --------------------------------------------------------------------------------------------------------
HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}
HC = 64


def draw_head(seed, c, feat64, tries=400):
    """Head parameters (nn.Conv2d's default ranges) whose pre-activations on `feat64` keep min |pre| >= 1e-5 max |pre| (25 times the fp32
    rounding of a 576-term sum relative to the largest): a bounded search on the CPU, so that the gate does not depend on the summation
    order."""
    for s in range(seed, seed + tries):
        g = torch.Generator().manual_seed(s)
        w1 = (torch.rand(HC, 64, 3, 3, generator=g) * 2 - 1) / 24.0
        b1 = (torch.rand(HC, generator=g) * 2 - 1) / 24.0
        p = R.pre_act(feat64, w1.double(), b1.double()).abs()
        if float(p.min()) >= 1e-5 * float(p.max()):
            return w1, b1, (torch.rand(c, HC, 1, 1, generator=g) * 2 - 1) / 8.0, torch.zeros(c)
    raise AssertionError("no head with a gate margin in %d tries" % tries)


@pytest.fixture(scope="module")
def net_x():
    torch.manual_seed(0)
    net = model.dla_net(HEADS, head_conv=HC, dtype="f32")
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True, HC), seed=0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net = net.to(DEV)
    x = torch.from_numpy(synth.synth_images(1, 64, 64)).to(DEV)
    th = heads.TrainableHeads(net)
    feat64 = th.features(x).cpu().double().contiguous()
    for i, (h, c) in enumerate(HEADS.items()):
        w1, b1, w2, b2 = draw_head(1000 * (i + 1), c, feat64)
        if h.startswith("hm"):
            b2 = torch.full((c,), -2.19)
        with torch.no_grad():
            for p, v in zip(th.head_params()[h], (w1, b1, w2, b2)):
                p.copy_(v.to(DEV))
    return net, th, x, feat64


@pytest.fixture(scope="module")
def batch():
    kp = np.zeros((1, 1, 17, 3), np.float32)
    rs = np.random.RandomState(3)
    kp[0, 0, :, 0] = 110 + 85 * rs.rand(17)
    kp[0, 0, :, 1] = 95 + 140 * rs.rand(17)
    kp[0, 0, :, 2] = 2.0
    return targets.multi_pose_targets(np.array([[[103.0, 87.0, 202.0, 242.0]]], np.float32), kp, [1], [[320.0, 240.0]], [640.0],
                                      opt=Opt(output_res=16), device=DEV)


def test_forward_is_bit_equal_to_the_f32_plan_and_follows_the_parameters(net_x):
    net, th, x, _ = net_x
    with torch.no_grad():
        plan_out = {k: v.clone() for k, v in net(x)[0].items()}
        out = th(x)[0]
        assert list(out) == list(HEADS)
        for k in HEADS:
            assert torch.equal(out[k], plan_out[k]), k
        p = th.head_params()["wh"][2]
        old = p.clone()
        p.add_(0.25)
        new = th(x)[0]
        assert not torch.equal(new["wh"], out["wh"]) and torch.equal(new["hps"], out["hps"])
        p.copy_(old)
        assert torch.equal(th(x)[0]["wh"], out["wh"])
    assert [n for n, _ in th.named_parameters()] == [n for n, _ in net.named_parameters() if n.split(".")[0] in HEADS]


def test_end_to_end_parameter_gradients_through_loss_multi_pose(net_x, batch):
    net, th, x, feat64 = net_x
    crit = losses.loss_multi_pose(Opt())
    th.zero_grad()
    out = th(x)[0]
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in out.items()}      # the logits, before the loss rebinds out['hm'] to the sigmoid
    loss, _ = crit([out], batch)
    loss.backward()
    crit([dict(leaf)], batch)[0].backward()
    for h in HEADS:
        w1, b1, w2, b2 = [p.detach().cpu() for p in th.head_params()[h]]
        case = (feat64.float(), w1, b1, w2.reshape(w2.shape[0], -1), b2, leaf[h].grad.cpu())
        lo, hi = R.gate_margin(case)
        assert lo >= 1e-5 * hi
        g64, e32 = R.bounds_of(case)
        got = [p.grad for p in th.head_params()[h]]
        assert all(g is not None for g in got)
        R.check("e2e " + h, [None] + got, g64, e32)
    assert all(p.grad is None for n, p in net.named_parameters() if n.split(".")[0] not in HEADS)


def test_five_sgd_steps_lower_the_loss(net_x, batch):
    net, th, x, feat64 = net_x
    gold = {k: v.cpu() for k, v in batch.items() if torch.is_tensor(v)}
    start = {h: [p.detach().cpu().clone() for p in ps] for h, ps in th.head_params().items()}
    feat32 = feat64.float()

    def cpu_losses(lr):
        ps = {h: [t.clone().requires_grad_(True) for t in v] for h, v in start.items()}
        opt = torch.optim.SGD([t for v in ps.values() for t in v], lr=lr)
        vals = []
        for _ in range(6):
            opt.zero_grad()
            o = {h: R.forward(feat32, v[0], v[1], v[2].reshape(v[2].shape[0], -1), v[3]) for h, v in ps.items()}
            loss = LR.multi_pose(o, gold)[0]
            vals.append(float(loss.detach()))
            loss.backward()
            opt.step()
        return vals
    lr = None
    # chosen on the CPU restatement: the smallest candidate that lowers the loss by >= 10 % in 5 steps (L1 and focal terms on ONE image: the
    # descent is not monotone, and above ~0.5 the heat-map heads diverge)
    for cand in (1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.2, 0.3, 0.4, 0.5, 0.7, 1.0):
        cpu = cpu_losses(cand)
        if np.isfinite(cpu).all() and cpu[5] <= 0.9 * cpu[0]:
            lr = cand
            break
    assert lr is not None, cpu
    crit = losses.loss_multi_pose(Opt())
    opt = torch.optim.SGD(th.parameters(), lr=lr)
    vals = []
    try:
        for _ in range(6):
            opt.zero_grad()
            loss, _ = crit(th(x), batch)
            vals.append(float(loss.detach()))
            loss.backward()
            opt.step()
    finally:
        with torch.no_grad():
            for h, ps in th.head_params().items():
                for p, v in zip(ps, start[h]):
                    p.copy_(v.to(DEV))
    print("SGD lr %g: cpu %s gpu %s" % (lr, cpu, vals))
    assert np.isfinite(vals).all() and vals[5] < vals[0]


def test_pose_and_shape_head_gradients_through_lbs_from_heads():
    g = torch.Generator().manual_seed(9)
    B, H, W = 2, 8, 8
    feat = torch.randn(B, 64, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    params = {}
    for h, c in (("pose", 72), ("shape", 10)):
        params[h] = tuple(t.to(DEV).requires_grad_(True) for t in
                          ((torch.rand(HC, 64, 3, 3, generator=g) * 2 - 1) / 24.0, (torch.rand(HC, generator=g) * 2 - 1) / 24.0,
                           (torch.rand(c, HC, 1, 1, generator=g) * 2 - 1) / 8.0, torch.zeros(c)))
    out = heads.heads_autograd(feat, params)
    small = smpl.SMPLModel.synthetic(seed=0, num_verts=100)
    inds = torch.randint(0, H * W, (B, 4), generator=g).to(DEV)
    verts = smpl.lbs_from_heads(small, out["pose"], out["shape"], inds, 3)
    (verts * torch.randn(verts.shape, generator=g).to(DEV)).sum().backward()
    for h in params:
        for p in params[h]:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, h
