"""GPU: the SMPL keypoint reprojection loss (csrc/smpl_loss.hip) through `smpl_loss.keypoint_loss_forward / _backward`, autograd through
`smpl_loss.smpl_keypoint_loss` on top of `smpl.lbs_from_heads`, and `trainer.HeadsTrainer` with the loss switched on.

The rule of every comparison (tests/smpl_kp_loss_ref.py): max |gpu - f64| <= 4 e32 + 1e-7 max |f64| per tensor, e32 = the float32 restatement's
error on the same inputs; loss scalars pooled over the cases (losses_ref.check_scalars).  Every case passes the L1 sign condition on the
CPU (every masked |pred - hps| of the fp64 restatement >= 1e-3 of the largest; re-drawn by seed otherwise); nothing is excluded from a
comparison.  The observed ratios are printed (`pytest -s`) and the largest recorded in DESIGN.md section 22.

End to end (`test_five_train_steps...`), the fp64 restatement's five-step series of `loss` and `smpl_kp_loss` against the device's, by
the same rule with e32 = the fp32 restatement's deviation from it; both series and the two ratios are printed."""
import copy
import random

import numpy as np
import pytest
import torch

import heads_grad_ref as HR
import losses_ref as LR
import optim_ref
import smpl_grad_ref as G
import smpl_kp_loss_ref as KR
import smpl_ref as R
import targets_ref
import test_gpu_optim as O
from h3d_amd import arch, model, smpl, smpl_loss, synth, train_input, trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, K = 100, 17
SENT = 777.0

_REG, _CASES, _BODY = {}, {}, []


def reg(NV):
    if NV not in _REG:
        _REG[NV] = smpl_loss.KeypointRegressor.synthetic(K, V, NV, seed=0)
    return _REG[NV]


def body():
    if not _BODY:
        _BODY.append(smpl.SMPLModel(**R.jointed_model(V)))
    return _BODY[0]


# name -> (NV, B, max_objs, n): 16 x 16 maps.  n = 35 of 40: 70 person slots = 17 full workgroups of four waves and one with two
SHAPES = {"NV0": (0, 2, 4, 4), "NV1": (1, 2, 4, 4), "NV5": (5, 2, 4, 4), "n35": (5, 2, 40, 35)}


def case(name, **kw):
    key = (name, repr(sorted(kw.items())))
    if key not in _CASES:
        NV, B, M, n = SHAPES[name]
        _CASES[key] = KR.Case(reg(NV), B, M, n, 16, 16, seed=10 * len(name) + NV, **kw)
    return _CASES[key]


def pooled_loss_e32():
    """The largest relative fp32 error of the loss scalar over the four cases (losses_ref.pooled_e32)."""
    r = [case(nm).refs() for nm in SHAPES]
    return LR.pooled_e32([float(r32[0]) for _, r32 in r], [float(r64[0]) for r64, _ in r])


def to_dev(c, mask=None):
    return (c.joints.to(DEV), c.verts.to(DEV) if c.reg.NV else None, c.cam.to(DEV), c.ind.to(DEV), c.hps.to(DEV), (c.mask if mask is None else mask).to(DEV))


def dev_run(c, want=(True, True, True), mask=None, out=None, bwd_out=None):
    """-> (stats [3], kp3d, pred, grad_joints, grad_verts, grad_cam_map) of the raw calls, upstream gradient c.go."""
    stats, kp3d, pred, a = smpl_loss.keypoint_loss_forward(*to_dev(c, mask), c.reg, c.n, out=out)
    go = torch.tensor(c.go, dtype=torch.float32, device=DEV)
    gj, gv, gc = smpl_loss.keypoint_loss_backward(a, stats, kp3d, pred, go, want=want, out=bwd_out)
    torch.cuda.synchronize()
    return stats, kp3d, pred, gj, gv, gc


NAMES = ("loss", "kp3d", "pred", "grad_joints", "grad_verts", "grad_cam_map")


def check_against_refs(name, c, got, e32_loss=None):
    r64, r32 = c.refs()
    ratios = {"loss": LR.check_scalars(name + " loss", [float(got[0][0])], [float(r64[0])], pooled_loss_e32() if e32_loss is None else e32_loss)}
    for nm, g, a, b in zip(NAMES[1:], got[1:], r64[1:], r32[1:]):
        if a is None:
            assert g is None, nm
            continue
        ratios[nm] = LR.check_tensor("%s %s" % (name, nm), g, a, b)
    return ratios


# ---- at the joints / vertices ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_loss_kp3d_pred_and_gradients_by_the_rule(name):
    c = case(name)
    got = dev_run(c)
    assert all(bool(torch.isfinite(t).all()) for t in got if t is not None)
    check_against_refs(name, c, got)
    r64 = c.refs()[0]
    l64 = float(r64[0]) * (float(c.mask[:, :c.n].sum()) + 1e-4)
    assert abs(float(got[0][1]) - l64) <= 1e-5 * l64 and float(got[0][2]) == float(c.mask[:, :c.n].sum())      # stats = {loss, l, num}


def test_nv0_gives_verts_no_gradient_and_equals_zero_vertex_weights():
    c = case("NV0")
    r0 = c.reg
    rz = smpl_loss.KeypointRegressor(r0.joint_w, np.full((K, 2), 7, np.int32), np.zeros((K, 2), np.float32), num_verts=V)
    cz = copy.copy(c)
    cz.reg = rz
    a, b = dev_run(c), dev_run(cz)
    assert a[4] is None and b[4] is not None and float(b[4].abs().max()) == 0.0
    for i in (0, 1, 2, 3, 5):
        assert torch.equal(a[i], b[i]), NAMES[i]
    # autograd: None, not zeros
    j, v, cam = c.joints.to(DEV).requires_grad_(True), c.verts.to(DEV).requires_grad_(True), c.cam.to(DEV).requires_grad_(True)
    loss = smpl_loss.smpl_keypoint_loss(j, v, cam, c.ind.to(DEV), c.hps.to(DEV), c.mask.to(DEV), r0, c.n)
    assert loss.dim() == 0 and torch.equal(loss, a[0][0])
    (loss * c.go).backward()
    assert v.grad is None and torch.equal(j.grad, a[3]) and torch.equal(cam.grad, a[5])
    loss = smpl_loss.smpl_keypoint_loss(j, None, cam, c.ind.to(DEV), c.hps.to(DEV), c.mask.to(DEV), r0)      # verts may be left out, n defaults to P / B
    assert torch.equal(loss, a[0][0])
    # only what is needed is computed
    cam2 = c.cam.to(DEV).requires_grad_(True)
    smpl_loss.smpl_keypoint_loss(j.detach(), None, cam2, c.ind.to(DEV), c.hps.to(DEV), c.mask.to(DEV), r0, c.n).backward()
    assert cam2.grad is not None
    assert smpl_loss.keypoint_loss_backward(*_fwd_parts(c), want=(False, False, True))[:2] == (None, None)


def _fwd_parts(c):
    stats, kp3d, pred, a = smpl_loss.keypoint_loss_forward(*to_dev(c), c.reg, c.n)
    return a, stats, kp3d, pred, torch.tensor(1.0, device=DEV)


def test_shared_vertex_zero_row_and_padding_entry_with_sentinels_on_both_sides():
    c = case("NV5")
    r = c.reg
    _, D = r.dense()
    assert ((D[0] > 0) & (D[1] > 0)).any() and not D[16].any() and not r.joint_w[16].any() and r.vert_w[2, 4] == 0       # what the title says
    P, PAD = c.B * c.n, 9                                         # 9 floats in front: every view starts 4 bytes past a 16-byte boundary
    sizes = {"kp3d": (P, K, 3), "pred": (P, K, 2), "gj": (P, 24, 3), "gv": (P, V, 3), "gc": tuple(c.cam.shape)}
    bufs = {k: torch.full((int(np.prod(s)) + 2 * PAD,), SENT, device=DEV) for k, s in sizes.items()}
    views = {k: bufs[k][PAD:PAD + int(np.prod(s))].view(s) for k, s in sizes.items()}
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views.values())
    got = dev_run(c, out=(views["kp3d"], views["pred"]), bwd_out=(views["gj"], views["gv"], views["gc"]))
    check_against_refs("sentinels", c, got)
    for k, s in sizes.items():
        n = int(np.prod(s))
        assert bool((bufs[k][:PAD] == SENT).all()) and bool((bufs[k][PAD + n:] == SENT).all()), k
    gv = got[4].cpu()
    touched = np.zeros(V, bool)
    touched[r.inv_vertex] = True
    assert float(gv[:, ~touched].abs().max()) == 0.0 and float(gv[..., 2].abs().max()) == 0.0 and float(got[3][..., 2].abs().max()) == 0.0
    assert float(got[1][:, 16].abs().max()) == 0.0                # the all-zero row's keypoint


# kp_bwd_fill_kernel: at most KP_FILL_MAX_BLOCKS = 2048 workgroups of KP_THREADS = 256 threads, each storing four floats per trip of the
# grid-stride loop (both pinned in tests/test_oracle_smpl_backward.py): the loop takes a second trip past 2048 * 256 * 4 floats
FILL_FLOATS_PER_TRIP = 2048 * 256 * 4
BIG_V = 6890


@pytest.mark.parametrize("n", [50, 51])
def test_grad_verts_fill_past_the_grid_cap(n):
    """The real mesh: P = 100 stays below the capped grid's reach (2 068 536 floats of grad_cam_map + grad_verts), P = 102 is past it
    (2 109 876), so the zero fill of grad_verts wraps.  Into sentinel-filled buffers, 16-byte aligned and 4 bytes off."""
    B, NV = 2, 5
    P, floats = B * n, B * 3 * 256 + B * n * BIG_V * 3
    assert (floats > FILL_FLOATS_PER_TRIP) == (n == 51) and floats == {50: 2068536, 51: 2109876}[n]
    assert (P * BIG_V * 3 // 4 > FILL_FLOATS_PER_TRIP // 4) == (n == 51)          # grad_verts' own vector count against the thread count
    if BIG_V not in _REG:
        _REG[BIG_V] = smpl_loss.KeypointRegressor.synthetic(K, BIG_V, NV, seed=0)
    r = _REG[BIG_V]
    key = ("big", n)
    if key not in _CASES:
        _CASES[key] = KR.Case(r, B, n, n, 16, 16, seed=900 + n)
    c = _CASES[key]
    touched = np.zeros(BIG_V, bool)
    touched[r.inv_vertex] = True
    assert 0 < touched.sum() <= K * NV
    sizes = {"gj": (P, 24, 3), "gv": (P, BIG_V, 3), "gc": tuple(c.cam.shape)}
    for pad, misalign in ((4, 0), (5, 4)):                         # floats in front of the view: on a 16-byte boundary, 4 bytes past one
        bufs = {k: torch.full((int(np.prod(s)) + 2 * pad,), SENT, device=DEV) for k, s in sizes.items()}
        views = {k: bufs[k][pad:pad + int(np.prod(s))].view(s) for k, s in sizes.items()}
        assert all(v.data_ptr() % 16 == misalign and v.is_contiguous() for v in views.values())
        got = dev_run(c, bwd_out=(views["gj"], views["gv"], views["gc"]))
        assert got[4].data_ptr() == views["gv"].data_ptr()
        check_against_refs("fill n%d +%dB" % (n, misalign), c, got)
        for k, s in sizes.items():
            size = int(np.prod(s))
            assert bool((bufs[k][:pad] == SENT).all()) and bool((bufs[k][pad + size:] == SENT).all()), (k, misalign)
            assert not bool((views[k] == SENT).any()), (k, misalign)
        gv = got[4]
        assert float(gv[:, torch.from_numpy(~touched).to(DEV)].abs().max()) == 0.0, misalign
        assert float(gv[:, torch.from_numpy(touched).to(DEV)].abs().max()) > 0.0


def test_all_zero_mask_gives_exactly_zero():
    c = case("NV5", mask="none")
    got = dev_run(c)
    assert float(got[0][0]) == 0.0 and float(got[0][1]) == 0.0 and float(got[0][2]) == 0.0
    assert all(float(g.abs().max()) == 0.0 for g in got[3:])
    check_against_refs("zero mask", c, got)


def test_n_below_max_objs_reads_nothing_behind_it():
    NV, B, M, n = 5, 2, 4, 3
    c = KR.Case(reg(NV), B, M, n, 16, 16, seed=77)
    c.ind[:, n:] = 1 << 40                                        # the slots behind n: an index far outside the map, NaN labels
    c.hps[:, n:] = float("nan")
    got = dev_run(c)
    assert all(bool(torch.isfinite(t).all()) for t in got if t is not None)
    check_against_refs("n < max_objs", c, got)


def test_ind_outside_the_map_contributes_nothing():
    c = case("NV5", bad_ind={(0, 1): 256, (1, 2): -1})
    got = dev_run(c)
    check_against_refs("ind outside", c, got)
    for p in (1, 4 + 2):
        assert float(got[2][p].abs().max()) == 0.0 and float(got[3][p].abs().max()) == 0.0 and float(got[4][p].abs().max()) == 0.0
        assert float(got[1][p].abs().max()) > 0.0                 # kp3d does not depend on the camera
    twin = copy.copy(c)                                           # the same two slots on the map and masked out: the same bits
    twin.ind, twin.mask = c.ind.clone(), c.mask.clone()
    twin.ind[0, 1], twin.ind[1, 2] = 3, 5
    twin.mask[0, 1] = 0
    twin.mask[1, 2] = 0
    other = dev_run(twin)
    assert torch.equal(got[0], other[0]) and all(torch.equal(a, b) for a, b in zip(got[3:], other[3:]))


def test_two_calls_a_second_stream_and_the_mask_dtypes_give_the_same_bits():
    c = case("n35")                                               # every slot on a pixel of its own: nothing depends on the order of the atomics
    assert all(len(set(c.ind[b, :c.n].tolist())) == c.n for b in range(c.B))
    first, again = dev_run(c), dev_run(c)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        other = dev_run(c)
    as_float, as_bool = dev_run(c, mask=c.mask.float()), dev_run(c, mask=c.mask.bool())
    for i, nm in enumerate(NAMES):
        for run in (again, other, as_float, as_bool):
            assert torch.equal(first[i], run[i]), nm


def test_refusals_on_the_device_and_cpu_tensors():
    c = case("NV5")
    j, v, cam, ind, hps, mask = to_dev(c)
    f = smpl_loss.smpl_keypoint_loss
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        f(c.joints, v, cam, ind, hps, mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        f(j, v, cam, ind, hps.cpu(), mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        f(j.double(), v, cam, ind, hps, mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        f(j, v, cam.permute(0, 1, 3, 2), ind, hps, mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        f(j, v.transpose(1, 2).contiguous().transpose(1, 2), cam, ind, hps, mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match=r"\[B,3,H,W\]"):
        f(j, v, cam[:, :2].contiguous(), ind, hps, mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match=r"\[P,24,3\]"):
        f(j[:, :23].contiguous(), v, cam, ind, hps, mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match="person slots"):
        f(j, v, cam, ind, hps, mask, c.reg, c.n + 1)
    with pytest.raises(RuntimeError, match="person slots"):
        f(j[:-1].contiguous(), v[:-1].contiguous(), cam, ind, hps, mask, c.reg)
    with pytest.raises(RuntimeError, match="verts must be given"):
        f(j, None, cam, ind, hps, mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match=r"\[P,V,3\]"):
        f(j, v[:, :50].contiguous(), cam, ind, hps, mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match="2K"):
        f(j, v, cam, ind, hps[..., :32].contiguous(), mask, c.reg, c.n)
    with pytest.raises(RuntimeError, match=r"\[B,max_objs\]"):
        f(j, v, cam, ind[:1], hps, mask, c.reg, c.n)


# ---- through lbs_from_heads: the gradients at the pose / shape / cam maps ----------------------------------------------------------------------
class MapsCase:
    """Head maps (pose, shape, cam) on 16 x 16 and label rows whose fp64 restatement passes the sign condition; references once."""

    def __init__(self, NV, B, M, n, seed, share=None, tries=50):
        self.reg, self.B, self.M, self.n = reg(NV), B, M, n
        H = W = 16
        for s in range(seed, seed + tries):
            rs = np.random.RandomState(s)
            f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
            self.pose, self.shape = f(rs.randn(B, 72, H, W) * 0.5), f(rs.randn(B, 10, H, W))
            cam = rs.randn(B, 3, H * W)
            cam[:, 0] = 4.0 + 8.0 * rs.rand(B, H * W)
            self.cam = f(cam.reshape(B, 3, H, W))
            ind = np.stack([rs.permutation(H * W)[:M] for _ in range(B)]).astype(np.int64)
            if share is not None:
                ind[share[0], share[2]] = ind[share[0], share[1]]
            self.ind = torch.from_numpy(ind)
            self.hps = f(rs.randn(B, M, 2 * K) * 3.0)
            pred = KR.maps_loss(self.pose, self.shape, self.cam, self.ind, self.hps, torch.ones(B, M, 2 * K), self.reg, n,
                                G.model_tensors(body().numpy_dict(), torch.float64))[3].reshape(B, n, 2 * K)
            self.hps[:, :n] = (pred + torch.from_numpy(rs.choice([-1.0, 1.0], pred.shape) * rs.uniform(0.25, 4.0, pred.shape))).float()
            mk = rs.rand(B, M, 2 * K) < 0.8
            mk[:, 0] = True
            self.mask = torch.from_numpy(mk.astype(np.uint8))
            self.r64 = self.ref(torch.float64)
            if self.r64[4] >= KR.SIGN_MARGIN:
                self.r32 = self.ref(torch.float32)
                return
        raise AssertionError("no draw with a sign margin in %d tries" % tries)

    def ref(self, dtype):
        return KR.maps_value_and_grads(self.pose, self.shape, self.cam, self.ind, self.hps, self.mask, self.reg, self.n, body().numpy_dict(), dtype)

    def run(self, pose=None, shape=None, cam=None, ind=None):
        pm, sm, cm = [(t if o is None else o).to(DEV).requires_grad_(True) for t, o in ((self.pose, pose), (self.shape, shape), (self.cam, cam))]
        it = (self.ind if ind is None else ind).to(DEV)
        verts, joints = smpl.lbs_from_heads(body(), pm, sm, it, self.n, return_joints=True, exact=True)
        loss = smpl_loss.smpl_keypoint_loss(joints, verts if self.reg.NV else None, cm, it, self.hps.to(DEV), self.mask.to(DEV), self.reg, self.n)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), pm.grad, sm.grad, cm.grad


_MAPS = {}


def maps_case(name):
    if name not in _MAPS:
        NV, B, M, n = SHAPES[name]
        _MAPS[name] = MapsCase(NV, B, M, n, seed=300 + NV + n)
    return _MAPS[name]


MAP_NAMES = ("loss", "grad_pose_map", "grad_shape_map", "grad_cam_map")


def check_maps(name, c, got, refs=None):
    r64, r32 = refs or (c.r64, c.r32)
    ratios = {}
    for nm, g, a, b in zip(MAP_NAMES[1:], got[1:], r64[1:4], r32[1:4]):
        ratios[nm] = LR.check_tensor("%s %s" % (name, nm), g, a, b)
    return ratios


@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_at_the_pose_shape_and_cam_maps_by_the_rule(name):
    c = maps_case(name)
    got = c.run()
    assert all(bool(torch.isfinite(t).all()) for t in got)
    cs = [maps_case(nm) for nm in SHAPES]
    e32 = LR.pooled_e32([float(x.r32[0]) for x in cs], [float(x.r64[0]) for x in cs])
    LR.check_scalars(name + " maps loss", [float(got[0])], [float(c.r64[0])], e32)
    check_maps(name + " maps", c, got)
    # zero off the gathered pixels
    off = torch.ones(c.B, 256, dtype=torch.bool)
    for b in range(c.B):
        off[b, c.ind[b, :c.n]] = False
    for g in got[1:]:
        assert not bool(g.cpu().reshape(c.B, g.shape[1], 256).transpose(1, 2)[off].any())


def test_two_slots_on_one_pixel_add_up():
    NV, B, M, n = SHAPES["NV5"]
    c = MapsCase(NV, B, M, n, seed=500, share=(1, 0, 1))
    pix = int(c.ind[1, 0])
    assert int(c.ind[1, 1]) == pix
    shared = c.run()
    check_maps("shared pixel", c, shared)
    # the two single runs: slot 1 moved to a free pixel that holds a copy of the shared pixel's values -- the same loss, the two
    # contributions on pixels of their own
    free = next(q for q in range(256) if q not in c.ind[1].tolist())
    maps = [t.clone() for t in (c.pose, c.shape, c.cam)]
    for t in maps:
        t.view(B, t.shape[1], 256)[1, :, free] = t.view(B, t.shape[1], 256)[1, :, pix]
    ind = c.ind.clone()
    ind[1, 1] = free
    apart = c.run(*maps, ind=ind)
    assert torch.equal(apart[0], shared[0])
    for nm, s, a, r64, r32 in zip(MAP_NAMES[1:], shared[1:], apart[1:], c.r64[1:4], c.r32[1:4]):
        s, a = s.cpu().double().reshape(B, -1, 256), a.cpu().double().reshape(B, -1, 256)
        want = a.clone()
        want[1, :, pix] = a[1, :, pix] + a[1, :, free]
        want[1, :, free] = 0.0
        e32 = float((r32.double() - r64).abs().max())
        err, limit = float((s - want).abs().max()), KR.FACTOR * e32 + 1e-7 * float(r64.abs().max())
        print("shared pixel against the sum of the two single runs, %s: err %.3g limit %.3g" % (nm, err, limit))
        assert err <= limit, (nm, err, limit)


# ---- the trainer, end to end -------------------------------------------------------------------------------------------------------------------
HEADS9 = dict(O.HEADS, pose=72, shape=10, cam=3)
HC = O.HC
KP_WEIGHT = 0.5
CAM_SCALE = 8.0       # the labelled persons are 24 .. 40 input pixels = 6 .. 10 map pixels tall, the body about 1 unit


def make_net9():
    net = model.dla_net(HEADS9, head_conv=HC, dtype="f32")
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS9, True, HC), seed=0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.to(DEV)


def train_opt9(lr, weight=KP_WEIGHT):
    o = O.train_opt(lr)
    o.smpl_kp_weight = weight
    return o


def new_trainer(lr, start, kp_reg, weight=KP_WEIGHT):
    tr = trainer.HeadsTrainer(train_opt9(lr, weight), make_net9(), smpl_model=body(), kp_regressor=kp_reg)
    if start is not None:
        with torch.no_grad():
            for h, ps in tr.heads.head_params().items():
                for p, v in zip(ps, start[h]):
                    p.copy_(v.to(DEV))
    return tr


@pytest.fixture(scope="module")
def setting9():
    """(batch, start head parameters, regressor, lr, fp64 series, fp32 series): series = [(loss, smpl_kp_loss)] before each of 6 steps."""
    sizes = [(48, 64), (40, 56)]
    rs = np.random.RandomState(13)
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    scenes = [targets_ref.scene(20 + b, 1, M=2, img_w=w, img_h=h, min_size=24.0, max_size=40.0) for b, (h, w) in enumerate(sizes)]
    boxes, kps = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    np.random.seed(17), random.seed(17)
    batch = train_input.multi_pose_train_batch([torch.from_numpy(i).to(DEV) for i in imgs], boxes, kps, [1, 1], O.train_opt(1e-3),
                                               data_rng=np.random.RandomState(123))
    n = batch["ind"].shape[1]
    assert int(batch["hps_mask"].sum()) > 0
    tr = new_trainer(1e-3, None, reg(3))
    feat64 = tr.heads.features(batch["input"]).cpu().double().contiguous()
    start = {}
    for i, (h, c) in enumerate(HEADS9.items()):
        w1, b1, w2, b2 = O.draw_head(1000 * (i + 1), c, feat64)
        if h.startswith("hm"):
            b2 = torch.full((c,), -2.19)
        if h == "cam":
            b2 = torch.tensor([CAM_SCALE, 0.0, 0.0])
        start[h] = [w1, b1, w2, b2]
    gold = {k: v.cpu() for k, v in batch.items() if torch.is_tensor(v)}
    bd = body().numpy_dict()

    def series(lr, dtype, kp_reg, steps=6):
        ps = {h: [t.to(dtype).clone().requires_grad_(True) for t in v] for h, v in start.items()}
        opt = torch.optim.Adam([t for v in ps.values() for t in v], foreach=False, **dict(optim_ref.DEFAULTS, lr=lr))      # optim_ref.torch_adam_run's yardstick
        feat, g, mt = feat64.to(dtype), LR.cast(gold, dtype), G.model_tensors(bd, dtype)
        vals, margin = [], None
        for _ in range(steps):
            opt.zero_grad()
            o = {h: HR.forward(feat, v[0], v[1], v[2].reshape(v[2].shape[0], -1), v[3]) for h, v in ps.items()}
            kp, diff, m, _ = KR.maps_loss(o["pose"], o["shape"], o["cam"], gold["ind"], gold["hps"], gold["hps_mask"], kp_reg, n, mt, dtype)
            if margin is None:
                margin = KR.sign_margin(diff.detach(), m)
            loss = LR.multi_pose(o, g)[0] + KP_WEIGHT * kp
            vals.append((float(loss.detach()), float(kp.detach())))
            loss.backward()
            opt.step()
        return vals, margin

    for seed in range(20):                    # the regressor is re-drawn until the first step's labels pass the sign condition
        kp_reg = smpl_loss.KeypointRegressor.synthetic(K, V, 3, seed=seed)
        if series(1e-4, torch.float64, kp_reg, steps=1)[1] >= KR.SIGN_MARGIN:
            break
    else:
        raise AssertionError("no regressor with a sign margin")
    for lr in O.LRS:                          # the smallest of the list that lowers the restatement's smpl_kp_loss by >= 10 % in 5 steps
        s64, _ = series(lr, torch.float64, kp_reg)
        if np.isfinite(s64).all() and s64[5][1] <= 0.9 * s64[0][1]:
            s32, _ = series(lr, torch.float32, kp_reg)
            return batch, start, kp_reg, lr, s64, s32
    raise AssertionError("no learning rate of %s lowers the restatement's smpl_kp_loss by 10 %%: %s" % (O.LRS, s64))


def head_bits(tr):
    return {h: [p.detach().clone() for p in ps] for h, ps in tr.heads.head_params().items()}


def test_five_train_steps_follow_the_restatement_and_a_resumed_run_has_the_sixth_steps_bits(setting9, tmp_path):
    batch, start, kp_reg, lr, s64, s32 = setting9
    tr = new_trainer(lr, start, kp_reg)
    assert isinstance(tr.loss, smpl_loss.loss_multi_pose_smpl) and len(list(tr.heads.parameters())) == 4 * len(HEADS9) == 36
    vals = []
    for _ in range(5):
        out, loss, stats = tr.train_step(dict(batch))
        vals.append((float(loss.detach()), float(stats["smpl_kp_loss"].detach())))
        assert set(stats) == set(tr.loss_stats) == set(smpl_loss.loss_multi_pose_smpl.KEYS) and set(out) == set(HEADS9)
        assert float(stats["loss"].detach()) == vals[-1][0]
    path = str(tmp_path / "model_last.pth")
    tr.save_model(path, 5)
    print("Adam lr %g, smpl_kp_weight %g" % (lr, KP_WEIGHT))
    for i, nm in enumerate(("loss", "smpl_kp_loss")):
        print("%s: f64 %s\n  f32 %s\n  gpu %s" % (nm, [v[i] for v in s64[:5]], [v[i] for v in s32[:5]], [v[i] for v in vals]))
    assert np.isfinite(vals).all()
    for i, nm in enumerate(("loss", "smpl_kp_loss")):
        LR.check_tensor("five steps " + nm, torch.tensor([v[i] for v in vals], dtype=torch.float64),
                        torch.tensor([v[i] for v in s64[:5]], dtype=torch.float64), torch.tensor([v[i] for v in s32[:5]], dtype=torch.float64))
    assert all(float(tr.optimizer.state[p]["step"]) == 5.0 for p in tr.heads.parameters())
    # the uninterrupted run's sixth step, and a fresh trainer resumed from the checkpoint
    tr.train_step(dict(batch))
    sixth = head_bits(tr)
    other = new_trainer(lr, None, kp_reg)
    assert other.load_model(path, resume=True) == 5
    for g in other.optimizer.param_groups:
        g["lr"] = lr                                              # the uninterrupted run never dropped it
    other.train_step(dict(batch))
    torch.cuda.synchronize()
    for h, ps in head_bits(other).items():
        assert all(torch.equal(a, b) for a, b in zip(ps, sixth[h])), h
    ck = torch.load(path, weights_only=False)
    assert len(ck["optimizer"]["state"]) == 36


def test_one_step_moves_pose_shape_and_cam_and_leaves_the_other_heads_their_own_update(setting9):
    batch, start, kp_reg, lr, _, _ = setting9
    with_kp, without = new_trainer(lr, start, kp_reg), new_trainer(lr, start, kp_reg, weight=0.0)
    assert type(without.loss).__name__ == "loss_multi_pose"
    first = head_bits(with_kp)
    with_kp.train_step(dict(batch))
    without.train_step(dict(batch))
    torch.cuda.synchronize()
    a, b = head_bits(with_kp), head_bits(without)
    for h in HEADS9:
        if h in ("pose", "shape", "cam"):
            assert all(not torch.equal(x, y) for x, y in zip(a[h], first[h])), h         # all four tensors of the head moved
            assert all(torch.equal(x, y) for x, y in zip(b[h], first[h])), h             # ... and only under the new loss
        else:                                                                            # no path from smpl_kp_loss to these heads
            assert all(torch.equal(x, y) for x, y in zip(a[h], b[h])), h
            assert all(not torch.equal(x, y) for x, y in zip(a[h], first[h])), h
