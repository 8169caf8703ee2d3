"""GPU: SMPL/LBS kernels against the float64 restatement (oracle/smpl.py): vertex positions
within 1e-4 abs (north_star tolerance).  Parity unpinned by the reference (no SMPL code there)."""
import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
from h3d_amd import smpl, synth
from oracle import smpl as osmpl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    return smpl.SMPLModel.synthetic(seed=0)


@pytest.mark.parametrize("kernel,P", [("gen1", 19), pytest.param("gen2", 19, marks=pytest.mark.extra), pytest.param("gen2", 150, marks=pytest.mark.extra), ("gen1", 70), ("gen3", 19), ("gen3", 150), ("gen3", 300),
                                      ("gen3x", 19), ("gen3x", 300)])
def test_lbs_matches_fp64_oracle(model, kernel, P):
    betas = synth.normalish("betas", (P, 10), 0.0, 1.0, 1)
    thetas = synth.normalish("thetas", (P, 72), 0.0, 0.3, 1)
    thetas[3] = 0.0                                      # rest pose
    thetas[4, :3] = [0.0, 3.0, 0.0]                      # large global rotation
    v, j = smpl.lbs(model, torch.from_numpy(betas).to(DEV), torch.from_numpy(thetas).to(DEV), return_joints=True,
                    kernel=kernel)
    v_ref, j_ref = osmpl.lbs(betas, thetas, model.numpy_dict())
    assert np.abs(v.cpu().numpy() - v_ref).max() < 1e-4
    assert np.abs(j.cpu().numpy() - j_ref).max() < 1e-4


def test_zero_pose_is_shape_blend(model):
    betas = synth.normalish("betas", (3, 10), 0.0, 1.0, 2)
    v = smpl.lbs(model, torch.from_numpy(betas).to(DEV), torch.zeros(3, 72, device=DEV)).cpu().numpy()
    v_s = model.v_template[None] + np.einsum("vck,pk->pvc", model.shapedirs, betas)
    assert np.abs(v - v_s).max() < 2e-6


def test_full_batch_size_properties(model):
    # bench size: 64 images x 100 people; global rotation equivariance as a size-independent check
    P = 6400
    betas = torch.from_numpy(synth.normalish("b", (P, 10), 0, 1, 3)).to(DEV)
    thetas = torch.from_numpy(synth.normalish("t", (P, 72), 0, 0.2, 3)).to(DEV)
    v = smpl.lbs(model, betas, thetas)
    assert v.shape == (P, 6890, 3) and bool(torch.isfinite(v).all())
    v2 = smpl.lbs(model, betas[100:108].contiguous(), thetas[100:108].contiguous())
    # person-tile position invariance (different tile instantiation: same math, fma contraction may differ)
    assert float((v[100:108] - v2).abs().max()) < 1.5e-5   # gen 3 (MFMA, three split products: 2^-16 relative) vs gen 1 (fp32 FMA)
    v3 = smpl.lbs(model, betas[64:192].contiguous(), thetas[64:192].contiguous())
    assert torch.equal(v[64:192], v3)                    # same instantiation, other tile position: bitwise
    v_ref, _ = osmpl.lbs(betas[:2].cpu().numpy(), thetas[:2].cpu().numpy(), model.numpy_dict())
    assert np.abs(v[:2].cpu().numpy() - v_ref).max() < 1e-4


def test_matrix_core_kernel_agrees_with_vector_kernel(model):
    # gen 3 (blend shapes on the bf16 matrix cores: hh + hm + mh of the three-term split, 2^-16 relative per product:
    # 2.2e-6 abs on the displacement in an fp64 emulation) vs gen 2 (fp32 vector FMA)
    P = 640
    betas = torch.from_numpy(synth.normalish("b", (P, 10), 0, 1, 5)).to(DEV)
    thetas = torch.from_numpy(synth.normalish("t", (P, 72), 0, 0.3, 5)).to(DEV)
    v3 = smpl.lbs(model, betas, thetas, kernel="gen3")
    v2 = smpl.lbs(model, betas, thetas, kernel="gen1")          # the fp32 vector kernel (generation 2, the same chain started from the template instead of from zero, is an EXTRA=1 build option)
    assert float((v3 - v2).abs().max()) < 1.5e-5
    # gen 3x (h3d_smpl_verts3_exact: all six products, 2^-24 relative -- ADVICE r2: the variant used to exist only behind a
    # compile-time switch no test built; the f32 parity-mode detectors run it) agrees with the fp32 vector kernel to 2e-6,
    # the bound the tests held before the three products were dropped
    v3x = smpl.lbs(model, betas, thetas, kernel="gen3x")
    assert float((v3x - v2).abs().max()) < 2e-6
    assert float((v3x - v3).abs().max()) > 0.0           # (it is a different kernel instantiation)


@pytest.mark.parametrize("exact", [False, True])
def test_lbs_from_heads_is_bit_identical_to_gathers_plus_lbs(model, exact):
    # the detector's fused tail (h3d_smpl_pose_heads: gathers + pose + coefficient pack in one launch) against the separate
    # launches it replaces, on head maps and indices of the detector's shapes; P = 3 x 50 is not a multiple of 128 (zero rows)
    from h3d_amd.utils import _transpose_and_gather_feat
    B, K, n, H, W = 3, 100, 50, 16, 24
    pose = torch.from_numpy(synth.normalish("pose_map", (B, 72, H, W), 0.0, 0.3, 5)).to(DEV)
    shape = torch.from_numpy(synth.normalish("shape_map", (B, 10, H, W), 0.0, 1.0, 5)).to(DEV)
    inds = torch.from_numpy((synth.uniform01("inds", (B, K), 5) * H * W).astype(np.int64)).to(DEV)
    v1, j1 = smpl.lbs_from_heads(model, pose, shape, inds, n, return_joints=True, exact=exact)
    sub = inds[:, :n].contiguous()
    thetas = _transpose_and_gather_feat(pose, sub).view(B * n, 72)
    betas = _transpose_and_gather_feat(shape, sub).view(B * n, 10)
    v2, j2 = smpl.lbs(model, betas, thetas, return_joints=True, kernel="gen3x" if exact else "gen3")
    assert torch.equal(v1, v2) and torch.equal(j1, j2)
    v_ref, _ = osmpl.lbs(betas[:4].cpu().numpy(), thetas[:4].cpu().numpy(), model.numpy_dict())
    assert np.abs(v1[:4].cpu().numpy() - v_ref).max() < 1e-4
