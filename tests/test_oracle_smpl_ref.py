"""CPU: the yardstick of the SMPL GPU tests (tests/smpl_ref.py) checks out against the oracle, and the model container refuses a
kinematic tree the pose kernel cannot walk."""
import numpy as np
import pytest

import h3d_amd  # noqa: F401
import smpl_ref as R
from h3d_amd import smpl as psmpl
from oracle import smpl as osmpl


@pytest.fixture(scope="module")
def body():
    return R.jointed_model(333, seed=0)


@pytest.fixture(scope="module")
def case(body):
    betas, thetas = R.make_case(40, 0)
    return betas, thetas, R.lbs(betas, thetas, body, np.float64)


def test_float64_restatement_equals_the_oracle_bit_for_bit(body, case):
    betas, thetas, r64 = case
    v, j = osmpl.lbs(betas, thetas, body)
    assert np.array_equal(r64[0], v) and np.array_equal(r64[1], j)
    # pose_feat and A, which the oracle does not return, from its own pieces
    Rm = osmpl.rodrigues(thetas.astype(np.float64).reshape(-1, 24, 3))
    assert np.array_equal(r64[2], (Rm[:, 1:] - np.eye(3)).reshape(-1, 207))
    assert np.array_equal(r64[3].reshape(-1, 24, 3, 4)[:, 0, :, :3], Rm[:, 0])            # the root's rotation is its own
    # A_j maps the rest joint onto the posed joint: A_j . [J_j; 1] = G_j.t
    v_s = body["v_template"].astype(np.float64)[None] + np.einsum("vck,pk->pvc", body["shapedirs"].astype(np.float64), betas.astype(np.float64))
    J = np.einsum("jv,pvc->pjc", body["J_regressor"].astype(np.float64), v_s)
    A = r64[3].reshape(-1, 24, 3, 4)
    np.testing.assert_allclose(np.einsum("pjab,pjb->pja", A[..., :3], J) + A[..., 3], j, atol=1e-14)


def test_float32_restatement_is_float32_throughout_and_within_1e_6(body, case):
    betas, thetas, r64 = case
    r32 = R.lbs(betas, thetas, body, np.float32)
    for nm, a, r in zip(R.NAMES, r32, r64):
        assert a.dtype == np.float32
        err = np.abs(a.astype(np.float64) - r).max()
        print("e32 %s %.3g (max |f64| %.3g)" % (nm, err, np.abs(r).max()))
        assert 0 < err < 1e-6, (nm, err)


def test_gen3_emulation_drops_less_than_the_kernel_states(body, case):
    betas, thetas, r64 = case
    em = R.lbs(betas, thetas, body, np.float64, emulate="gen3")
    d = np.abs(em[0] - r64[0]).max()
    print("gen3 emulation vs float64: %.3g" % d)
    assert 0 < d < 2.2e-6                    # the figure csrc/smpl.hip states for the three dropped products
    for a, r in zip(em[1:], r64[1:]):        # joints, pose features and transforms never pass through the matrix cores
        assert np.array_equal(a, r)


def test_bf16_split_is_round_to_nearest_even_like_the_device_pack():
    import torch
    x = np.concatenate([np.random.RandomState(0).randn(4096).astype(np.float32) * 0.03,
                        np.array([0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39, 65280.0], np.float32)])   # ties both ways
    h, m = R.split_hm(x)
    t = torch.from_numpy(x)
    th = t.to(torch.bfloat16).float()
    tm = (t - th).to(torch.bfloat16).float()
    assert np.array_equal(h, th.double().numpy()) and np.array_equal(m, tm.double().numpy())


@pytest.mark.parametrize("V", [333, 6890])
def test_jointed_model_has_a_skeleton_and_every_weight_count(V):
    m = R.jointed_model(V, seed=0)
    again = R.jointed_model(V, seed=0)
    assert all(np.array_equal(m[k], again[k]) for k in m)                      # a pure function of its arguments
    J = m["J_regressor"].astype(np.float64) @ m["v_template"].astype(np.float64)
    bone = np.linalg.norm(J[1:] - J[R.PARENTS[1:]], axis=1)
    print("V %d: bones %.3f .. %.3f, extent %.3f" % (V, bone.min(), bone.max(), np.abs(m["v_template"]).max()))
    assert bone.min() >= 0.05
    assert 0.5 < np.abs(m["v_template"]).max() < 2.0
    cnt = (m["weights"] != 0).sum(1)
    assert set(np.unique(cnt)) == {1, 2, 3, 4}
    np.testing.assert_allclose(m["weights"].sum(1), 1.0, atol=1e-6)
    np.testing.assert_allclose(m["J_regressor"].sum(1), 1.0, atol=1e-6)
    assert ((m["J_regressor"] != 0).sum(1) == 12).all()
    psmpl.SMPLModel(**m)                                                       # and the container takes it


def test_jointed_model_weight_count_limits():
    for mx in (1, 2, 3, 6):
        cnt = (R.jointed_model(130, seed=mx, max_nnz=mx)["weights"] != 0).sum(1)
        assert cnt.max() == mx and cnt.min() == 1


def test_model_refuses_parents_that_are_not_parents_first():
    m = R.jointed_model(64, seed=0)
    ok = psmpl.SMPLModel(**m)
    assert np.array_equal(ok.parents, psmpl.PARENTS)
    for bad in ([0] + list(psmpl.PARENTS[1:]),                                  # root with a parent
                [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 23],    # joint 23 its own parent
                [-1, 2, 0] + list(psmpl.PARENTS[3:]),                         # child before its parent
                [-1, -1] + list(psmpl.PARENTS[2:]),                           # a second root
                list(psmpl.PARENTS[:23])):                                    # 23 joints
        with pytest.raises(ValueError):
            psmpl.SMPLModel(**dict(m, parents=np.array(bad, np.int32)))
