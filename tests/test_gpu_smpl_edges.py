"""GPU: the SMPL kernels (csrc/smpl.hip) on a jointed body, at the tile edges of the person and vertex counts, at the edges of the pose
domain and of the skinning-weight count, and `h3d_smpl_pose_heads` through the raw ABI.

The rule of every comparison with the oracle (tests/smpl_ref.py; per case, per output tensor): e32 = max |f32 restatement - f64| of a plain
float32 run of the same formulas, and max |gpu - f64| <= 4 * e32 + 2^-23 * max |f64|.  Generation 3 (hh + hm + mh of the bf16 split) is
compared with the fp64 emulation of exactly that sum, not with a wider bound.  The observed ratios are printed (`pytest -s`) and recorded
in DESIGN.md section 14."""
import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
import smpl_ref as R
from h3d_amd import _lib, smpl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNELS = ("gen1", "gen3", "gen3x")
SENTINEL = -12345.5

_MODELS, _CASES = {}, {}


def body(V, seed=0, max_nnz=4):
    key = (V, seed, max_nnz)
    if key not in _MODELS:
        _MODELS[key] = smpl.SMPLModel(**R.jointed_model(V, seed, max_nnz))
    return _MODELS[key]


class Case:
    """One (body, persons) pair; its oracle is computed once and shared by the tests of every kernel."""

    def __init__(self, V, P, seed, max_nnz=4):
        self.m = body(V, 0, max_nnz)
        self.betas, self.thetas = R.make_case(P, seed)
        self.bt, self.tt = torch.from_numpy(self.betas).to(DEV), torch.from_numpy(self.thetas).to(DEV)
        self.name = "V%d P%d nnz%d" % (V, P, max_nnz)
        self._ref = {}

    def ref(self, kernel):
        if None not in self._ref:
            self._ref[None] = R.bounds(self.betas, self.thetas, self.m.numpy_dict())
        if kernel == "gen3" and "gen3" not in self._ref:          # the same e32, the target with generation 3's dropped products
            self._ref["gen3"] = (R.lbs(self.betas, self.thetas, self.m.numpy_dict(), np.float64, "gen3"), self._ref[None][1])
        return self._ref["gen3" if kernel == "gen3" else None]

    def check(self, kernel, got):
        target, e32 = self.ref(kernel)
        return R.check("%s %s" % (self.name, kernel), got, target, e32)


def case(V, P, seed, max_nnz=4):
    key = (V, P, seed, max_nnz)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


def pack(m):
    if m._dev is None:
        m._dev = smpl._device_pack(m, torch.device(DEV))
    return m._dev


def raw_pose(m, bt, tt):
    """h3d_smpl_pose alone -> pose_feat [P,207], A [P,24,12], joints [P,24,3]."""
    d, P = pack(m), bt.shape[0]
    pf = torch.full((P, 207), SENTINEL, device=DEV)
    A = torch.full((P, 24, 12), SENTINEL, device=DEV)
    joints = torch.full((P, 24, 3), SENTINEL, device=DEV)
    _lib.check(_lib.lib().h3d_smpl_pose(_lib.ptr(bt), _lib.ptr(tt), _lib.ptr(d["j_template"]), _lib.ptr(d["j_shapedirs"]), _lib.ptr(d["parents"]),
                                        P, _lib.ptr(pf), _lib.ptr(A), _lib.ptr(joints), None, 0, _lib.stream_ptr()), "smpl_pose")
    return pf, A, joints


def raw_verts(m, kernel, bt, pf, A, out):
    """The vertex kernel of `kernel` alone, through the C ABI, into the caller's buffer `out` (>= P*V*3 floats)."""
    d, P, L, st = pack(m), bt.shape[0], _lib.lib(), _lib.stream_ptr()
    assert out.numel() >= P * d["V"] * 3 and out.dtype == torch.float32
    if kernel == "gen1":
        _lib.check(L.h3d_smpl_verts(_lib.ptr(bt), _lib.ptr(pf), _lib.ptr(A), _lib.ptr(d["v_template"]), _lib.ptr(d["shapedirsT"]),
                                    _lib.ptr(d["posedirsT"]), _lib.ptr(d["lbs_idx"]), _lib.ptr(d["lbs_w"]), d["nnz"], P, d["V"], d["Vpad"],
                                    _lib.ptr(out), st), "smpl_verts")
        return
    Ppad = (P + 127) // 128 * 128
    coefK = torch.empty(Ppad, 14, 3, 16, dtype=torch.bfloat16, device=DEV)
    _lib.check(L.h3d_smpl_coef_pack(_lib.ptr(bt), _lib.ptr(pf), P, Ppad, _lib.ptr(coefK), st), "smpl_coef_pack")
    fn = L.h3d_smpl_verts3_exact if kernel == "gen3x" else L.h3d_smpl_verts3
    _lib.check(fn(_lib.ptr(coefK), _lib.ptr(A), _lib.ptr(d["v_template"]), _lib.ptr(d["dirsK3"]), _lib.ptr(d["lbs_idx"]), _lib.ptr(d["lbs_w"]),
                  d["nnz"], P, Ppad, d["V"], d["Vpad"], _lib.ptr(out), st), "smpl_verts3")


def run(c, kernel):
    return smpl.lbs(c.m, c.bt, c.tt, return_joints=True, kernel=kernel)


# ---- 1. the jointed body: all four outputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("V,P", [(333, 40), (6890, 130)])
def test_jointed_body_all_outputs_vs_oracle(V, P, kernel):
    c = case(V, P, 0)
    v, j = run(c, kernel)
    pf, A, j2 = raw_pose(c.m, c.bt, c.tt)
    assert torch.equal(j, j2)
    c.check(kernel, (v, j, pf, A))


# ---- 2. person-count edges ------------------------------------------------------------------------------------------------------------
PERSON_EDGES = [("gen1", P) for P in (1, 2, 63, 64, 65)] + [(k, P) for k in ("gen3", "gen3x") for P in (1, 2, 127, 128, 129, 255, 256, 257)]


@pytest.mark.parametrize("kernel,P", PERSON_EDGES)
def test_person_count_edges(kernel, P):
    c = case(130, P, P)
    v, j = run(c, kernel)
    c.check(kernel, (v, j, None, None))
    # person 0 and person P - 1 run alone through the same kernel instantiation: the same bits.  Generation 1 has two instantiations
    # (8 persons per lane below 64 persons, 32 from there on) and a batch of one always takes the first, so from 64 persons on its
    # same-instantiation twin is the batch rotated by 37 persons (below), which moves every person to another tile and lane slot.
    if kernel != "gen1" or P < 64:
        for i in {0, P - 1}:
            v1, j1 = smpl.lbs(c.m, c.bt[i:i + 1].contiguous(), c.tt[i:i + 1].contiguous(), return_joints=True, kernel=kernel)
            assert torch.equal(v1[0], v[i]) and torch.equal(j1[0], j[i]), (kernel, P, i)
    if P > 1:
        s = 37 % P
        vr, jr = smpl.lbs(c.m, torch.roll(c.bt, s, 0).contiguous(), torch.roll(c.tt, s, 0).contiguous(), return_joints=True, kernel=kernel)
        assert torch.equal(vr, torch.roll(v, s, 0)) and torch.equal(jr, torch.roll(j, s, 0)), (kernel, P)


@pytest.mark.parametrize("P,taken", [(63, "gen1"), (64, "gen3")])
def test_auto_switches_generation_at_64_persons(P, taken):
    c = case(130, P, P)
    va, ja = run(c, "auto")
    vt, jt = run(c, taken)
    assert torch.equal(va, vt) and torch.equal(ja, jt)
    other = run(c, "gen3" if taken == "gen1" else "gen1")[0]
    assert not torch.equal(va, other)                  # (the two generations do differ in their last bits, so the above tells them apart)
    c.check(taken, (va, ja, None, None))


# ---- 3. pose edges in one batch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_pose_edges_in_one_batch(kernel):
    # persons 0..11 are the edges of smpl_ref.special_thetas (rest pose, a zero joint between rotated ones, 1e-7 .. 1e-3, pi, 2 pi, 7 rad
    # about a negative axis, every joint by 3 rad, ...), 12..15 ordinary; every person, the rest pose included, is held to the one rule
    c = case(130, 16, 3)
    th = c.thetas.reshape(16, 24, 3)
    assert not th[0].any() and not th[1, 9].any() and th[1, 6].any() and th[1, 12].any() and (th[2] == np.float32(1e-7)).all()
    assert abs(np.linalg.norm(th[8], axis=1) - 3.0).max() < 1e-6 and th[7, 16, 2] == -7.0
    v, j = run(c, kernel)
    pf, A, _ = raw_pose(c.m, c.bt, c.tt)
    c.check(kernel, (v, j, pf, A))
    assert bool(torch.isfinite(v).all() and torch.isfinite(pf).all() and torch.isfinite(A).all())


# ---- 4. vertex-count edges, and nothing written past the output -------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
def test_vertex_count_edges_and_output_bounds(V, kernel):
    P = 70
    c = case(V, P, 4)
    v, j = run(c, kernel)
    assert v.shape == (P, V, 3)
    c.check(kernel, (v, j, None, None))
    pf, A, _ = raw_pose(c.m, c.bt, c.tt)
    buf = torch.full((P * V * 3 + 64,), SENTINEL, device=DEV)
    raw_verts(c.m, kernel, c.bt, pf, A, buf)
    assert torch.equal(buf[:P * V * 3].view(P, V, 3), v)
    assert bool((buf[P * V * 3:] == SENTINEL).all()), "written past the output tensor"


# ---- 5. skinning-weight counts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("max_nnz", [1, 2, 3])
def test_fewer_than_four_skinning_weights(max_nnz, kernel):
    c = case(130, 70, 5, max_nnz)
    assert pack(c.m)["nnz"] == max_nnz
    v, j = run(c, kernel)
    c.check(kernel, (v, j, None, None))


def test_more_than_four_skinning_weights_take_generation_1_or_raise():
    c = case(130, 70, 5, 6)
    assert pack(c.m)["nnz"] == 6
    v, j = run(c, "gen1")
    c.check("gen1", (v, j, None, None))
    va, ja = run(c, "auto")                              # 70 persons: gen 3 if it could
    assert torch.equal(va, v) and torch.equal(ja, j)
    for k in ("gen3", "gen3x"):
        with pytest.raises(RuntimeError):
            run(c, k)
    B, K, H, W = 2, 8, 4, 6
    pose, shape = torch.zeros(B, 72, H, W, device=DEV), torch.zeros(B, 10, H, W, device=DEV)
    with pytest.raises(RuntimeError):
        smpl.lbs_from_heads(c.m, pose, shape, torch.zeros(B, K, dtype=torch.int64, device=DEV), 4)


# ---- 6. h3d_smpl_pose_heads through the raw ABI ---------------------------------------------------------------------------------------------
def _pose_heads(m, pose, shape, inds, n, with_betas=True):
    d = pack(m)
    B, K = inds.shape
    HW = pose.shape[2] * pose.shape[3]
    P = B * n
    Ppad = (P + 127) // 128 * 128
    pf = torch.full((P, 207), SENTINEL, device=DEV)
    A = torch.full((P, 24, 12), SENTINEL, device=DEV)
    joints = torch.full((P, 24, 3), SENTINEL, device=DEV)
    betas = torch.full((P * 10 + 64,), SENTINEL, device=DEV) if with_betas else None
    coefK = torch.full((Ppad, 14, 3, 16), 1.0, dtype=torch.bfloat16, device=DEV)           # not zeros: the kernel has to write the zero rows
    _lib.check(_lib.lib().h3d_smpl_pose_heads(_lib.ptr(pose), _lib.ptr(shape), _lib.ptr(inds), B, K, n, HW, _lib.ptr(d["j_template"]),
                                              _lib.ptr(d["j_shapedirs"]), _lib.ptr(d["parents"]), _lib.ptr(betas), _lib.ptr(pf), _lib.ptr(A),
                                              _lib.ptr(joints), _lib.ptr(coefK), Ppad, _lib.stream_ptr()), "smpl_pose_heads")
    return {"pf": pf, "A": A, "joints": joints, "betas": betas, "coefK": coefK.view(torch.int16)}


def test_pose_heads_raw_abi_betas_out_index_clamp_and_zero_rows():
    from h3d_amd import synth
    m = body(130)
    B, n, K, H, W = 3, 43, 100, 16, 24                   # n < K, B * n = 129 odd: the last wave holds one person, Ppad = 256
    HW, P = H * W, B * n
    pose = torch.from_numpy(synth.normalish("pose_map", (B, 72, H, W), 0.0, 0.3, 6)).to(DEV)
    shape = torch.from_numpy(synth.normalish("shape_map", (B, 10, H, W), 0.0, 1.0, 6)).to(DEV)
    inds = torch.from_numpy((synth.uniform01("inds", (B, K), 6) * HW).astype(np.int64)).to(DEV)
    inds[0, 0], inds[1, 5], inds[2, n - 1] = -1, HW + 5, HW - 1
    inds[:, n:] = 2 ** 40                                # detections past n are never read
    got = _pose_heads(m, pose, shape, inds, n)
    clamped = inds.clone()
    clamped[0, 0], clamped[1, 5] = 0, HW - 1
    want = _pose_heads(m, pose, shape, clamped, n)
    for k in got:
        assert torch.equal(got[k], want[k]), k           # an index of -1 reads pixel 0, one of HW + 5 reads pixel HW - 1
    sub = clamped[:, :n]
    gather = lambda t: torch.gather(t.view(B, -1, HW), 2, sub[:, None, :].expand(B, t.shape[1], n)).permute(0, 2, 1).reshape(P, -1).contiguous()
    betas, thetas = gather(shape), gather(pose)
    assert torch.equal(got["betas"][:P * 10].view(P, 10), betas)
    assert bool((got["betas"][P * 10:] == SENTINEL).all())
    # the same outputs without betas_out, and the separate launches on the gathered parameters: the same bits
    nob = _pose_heads(m, pose, shape, inds, n, with_betas=False)
    pf, A, joints = raw_pose(m, betas, thetas)
    Ppad = 256
    coefK = torch.full((Ppad, 14, 3, 16), 1.0, dtype=torch.bfloat16, device=DEV)
    _lib.check(_lib.lib().h3d_smpl_coef_pack(_lib.ptr(betas), _lib.ptr(pf), P, Ppad, _lib.ptr(coefK), _lib.stream_ptr()), "smpl_coef_pack")
    for k, t in (("pf", pf), ("A", A), ("joints", joints), ("coefK", coefK.view(torch.int16))):
        assert torch.equal(got[k], t) and torch.equal(nob[k], t), k
    assert not bool((got["coefK"][:P].flatten(1) == 0).all(dim=1).any())          # every person's row carries values,
    assert bool((got["coefK"].view(torch.bfloat16)[P:].float() == 0).all())       # rows P .. Ppad - 1 are zeros,
    assert bool((got["coefK"].view(torch.bfloat16)[:, 13, :, 9:].float() == 0).all())   # and so are the K columns 217 .. 223
    target, e32 = R.bounds(betas.cpu().numpy(), thetas.cpu().numpy(), m.numpy_dict())
    R.check("pose_heads V130 P129", (None, got["joints"], got["pf"], got["A"]), target, e32)


# ---- 7. isolation: one person's non-finite or huge parameters stay with that person ------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_persons_nan_or_huge_parameters_do_not_leak(kernel):
    c = case(130, 130, 7)
    v, j = run(c, kernel)
    others = torch.arange(130, device=DEV) != 77
    for bad in (float("nan"), 1e30):
        bt, tt = c.bt.clone(), c.tt.clone()
        bt[77], tt[77] = bad, bad
        vb, jb = smpl.lbs(c.m, bt, tt, return_joints=True, kernel=kernel)
        assert torch.equal(vb[others], v[others]) and torch.equal(jb[others], j[others]), (kernel, bad)
        assert not bool(torch.isfinite(vb[77]).all())      # (the parameters did arrive)
