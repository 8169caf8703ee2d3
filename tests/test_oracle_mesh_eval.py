"""CPU: the host mirror mesh_eval.evaluate_numpy of include/h3d.h section 8b against its plain-loop restatement (tests/mesh_eval_ref.py, bit
for bit) and against the textbook closed form through LAPACK (mesh_eval_cases.closed_form, on the error values), and the argument checks of
the two entry points, which run before any HIP call.

The bound on |mirror - closed form| / extent is 64 x the worst measured per family over 140 seeds x n in {3, 4, 14, 24, 65, 6890}
(DESIGN.md section 27 holds the table; the factor covers another LAPACK build).  A family whose measured worst is below one rounding of
the scale, 2^-53, is held to 64 x 2^-53: a smaller figure cannot be told from 0.  Every bound is far below 1e-12, beyond which the
Jacobi loop would not be converging."""
import ctypes

import numpy as np
import pytest

import mesh_eval_cases as cases
import mesh_eval_ref as ref
from h3d_amd import _lib, mesh_eval as ME

NS = (3, 4, 14, 24, 65, 6890)
SEEDS = 12
MEASURED_WORST = {"general": 4.99e-16, "reflected": 1.95e-15, "coplanar_source": 4.09e-16, "coplanar_target": 8.34e-16,
                  "collinear_source": 2.22e-16, "equal_source": 2.74e-16, "equal_target": 0.0}
ROTATION_BOUND = 64 * 2.0 ** -53          # |det R - 1| and max |R^T R - I|: three unit vectors and at most 15 plane rotations, a few roundings each


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_the_mirror_equals_the_loop_restatement_bit_for_bit():
    checked = 0
    for n, with_root, root in ((1, False, (0, 0)), (3, True, (1, 2)), (24, True, (2, 2)), (65, False, (0, 0)), (257, True, (0, 1)), (600, False, (0, 0))):
        c = cases.device_case(n, 9, 40 + n, with_root, root)
        err, count, tr = ME.evaluate_numpy(c["pred"], c["gt"], c["pred_idx"], c["gt_idx"], c["weight"], c["pred_root"], c["gt_root"], root)
        for k, (a, b) in enumerate(zip(c["pred_idx"], c["gt_idx"])):
            if not (0 <= a < len(c["pred"]) and 0 <= b < len(c["gt"])):
                assert count[k] == 0 and not err[k].any() and not tr[k].any()
                continue
            rp, rg = (c["pred_root"][a], c["gt_root"][b]) if with_root else (None, None)
            plain, aligned, cnt, transform = ref.pair_errors(c["pred"][a], c["gt"][b], c["weight"][b], rp, rg, root)
            assert cnt == count[k] and np.array_equal(bits([plain, aligned]), bits(err[k])), (n, k)
            assert np.array_equal(bits(transform), bits(tr[k])), (n, k)
            checked += 1
        assert (count == 0).any() and (count == 1).any() and count.max() > 1 or n == 1
    assert checked >= 30
    # without weights, and the degenerate families (rank 2, 1 and 0) through both
    for family in cases.FAMILIES:
        x, y = cases.family_pair(family, 24, 3)
        err, count, tr = ME.evaluate_numpy(x[None], y[None], [0], [0])
        plain, aligned, cnt, transform = ref.pair_errors(x, y)
        assert cnt == 24 and np.array_equal(bits([plain, aligned]), bits(err[0])) and np.array_equal(bits(transform), bits(tr[0])), family


def test_one_mesh_of_6890_points_equals_the_loop_restatement():
    x, y = cases.family_pair("general", 6890, 1)
    err, count, tr = ME.evaluate_numpy(x[None], y[None], [0], [0])
    plain, aligned, cnt, transform = ref.pair_errors(x, y)
    assert cnt == 6890 and np.array_equal(bits([plain, aligned]), bits(err[0])) and np.array_equal(bits(transform), bits(tr[0]))


def test_metric_means_mirror_equals_the_loop_restatement():
    rs = np.random.RandomState(5)
    for P in (0, 1, 64, 65, 1000):
        err, count = rs.uniform(0, 0.2, (P, 2)), rs.randint(0, 3, P).astype(np.int32)
        means, pairs = ME.metric_means_numpy(err, count)
        want, want_pairs = ref.metric_means(err.tolist(), count.tolist())
        assert pairs == want_pairs == int((count > 0).sum()) and np.array_equal(bits(means), bits(want)), P
    means, pairs = ME.metric_means_numpy(rs.uniform(0, 1, (7, 2)), np.zeros(7, np.int32))
    assert pairs == 0 and not means.any()


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_the_mirror_against_the_lapack_closed_form(family):
    bound = 64 * max(MEASURED_WORST[family], 2.0 ** -53)
    assert bound < 1e-12
    worst = worst_rot = 0.0
    for n in NS:
        xs, ys = zip(*[cases.family_pair(family, n, s) for s in range(SEEDS)])
        err, count, tr, sweeps = ME.evaluate_numpy(np.stack(xs), np.stack(ys), np.arange(SEEDS), np.arange(SEEDS), return_sweeps=True)
        assert np.isfinite(err).all() and np.isfinite(tr).all() and (count == n).all()
        assert sweeps.max() < _lib.MESH_EVAL_MAX_SWEEPS, "the Jacobi loop ran into its cap"
        for k in range(SEEDS):
            value = cases.closed_form(xs[k], ys[k])[0]
            worst = max(worst, abs(err[k, 1] - value) / cases.extent(family, ys[k]))
            R = tr[k, 1:10].reshape(3, 3)
            worst_rot = max(worst_rot, abs(np.linalg.det(R) - 1.0), np.abs(R.T @ R - np.eye(3)).max())
    print("%s: worst |mirror - closed form| / extent %.3g (bound %.3g), rotation defect %.3g" % (family, worst, bound, worst_rot))
    assert worst <= bound and worst_rot <= ROTATION_BOUND


def test_a_line_in_general_position_is_held_to_the_optimality_of_its_residual():
    # collinear only to float32 rounding: R about the line is ill-determined for any SVD (mesh_eval_cases.family_pair), so the transform is
    # judged by what it minimises -- the residual sum of squares, in long double, is not above LAPACK's by more than 1e-13 of it
    L = np.longdouble
    for n in (3, 24, 6890):
        for seed in range(6):
            x, y = cases.family_pair("near_collinear_source", n, seed)
            _, _, tr = ME.evaluate_numpy(x[None], y[None], [0], [0])
            _, s, R, t = cases.closed_form(x, y)

            def ssq(s_, R_, t_):
                q = L(s_) * (x.astype(L) @ np.asarray(R_, L).T) + np.asarray(t_, L) - y.astype(L)
                return float((q * q).sum())
            mine, lapack = ssq(tr[0, 0], tr[0, 1:10].reshape(3, 3), tr[0, 10:]), ssq(s, R, t)
            assert np.isfinite(tr).all() and mine <= lapack * (1 + 1e-13), (n, seed, mine, lapack)
            Rm = tr[0, 1:10].reshape(3, 3)
            assert abs(np.linalg.det(Rm) - 1.0) <= ROTATION_BOUND and np.abs(Rm.T @ Rm - np.eye(3)).max() <= ROTATION_BOUND


@pytest.mark.parametrize("n", [3, 14, 65, 6890])
def test_known_answer_on_a_lattice(n):
    for seed in range(5):
        x, y, R0, t0 = cases.lattice_case(n, seed)
        err, count, tr = ME.evaluate_numpy(x[None], y[None], [0], [0])
        ext = cases.extent("general", y)
        print("lattice n = %d seed %d: aligned %.3g of extent %.3g, s - 0.5 = %.3g" % (n, seed, err[0, 1], ext, tr[0, 0] - 0.5))
        assert err[0, 1] <= 1e-13 * ext and abs(tr[0, 0] - 0.5) <= 1e-13
        assert np.abs(tr[0, 1:10].reshape(3, 3) - R0).max() <= 1e-13 and np.abs(tr[0, 10:] - t0).max() <= 1e-13
        # the plain error by hand: the mean of |x - (0.5 R0 x + t0)|, every difference exact in float64, summed in the stated order
        d = x.astype(np.float64) - y.astype(np.float64)
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        want = ref.block_sum(n, [True] * n, lambda i: float(dist[i])) / float(n)
        assert err[0, 0] == want and abs(want - float(np.mean(dist))) <= 1e-14 * want


def test_roots_weights_and_invalid_pairs():
    x, y, _, _ = cases.lattice_case(24, 1)
    pred, gt = np.stack([x, x + 0.5]), np.stack([y, y])
    w = np.ones((2, 24), np.uint8)
    w[1, 5:] = 0
    err, count, tr = ME.evaluate_numpy(pred, gt, [0, 1, 1, -1, 0, 2], [0, 0, 1, 0, 2, 0], w, pred, gt, (1, 2))
    assert count.tolist() == [24, 24, 5, 0, 0, 0] and not err[3:].any() and not tr[3:].any()
    # a shift of the prediction moves its root along: the rooted plain error does not see it
    assert err[0, 0] > 0 and err[1, 0] == err[0, 0] and abs(err[1, 1]) <= 1e-13
    same = ME.evaluate_numpy(pred, gt, [0], [0], w, pred, gt, (2, 2))[0]
    assert same[0, 0] != err[0, 0]                                     # another root, another plain error
    one = ME.evaluate_numpy(pred, gt, [0], [0], np.eye(24, dtype=np.uint8)[:2])
    assert one[1].tolist() == [1] and one[0][0, 1] == 0.0 and one[2][0, 0] == 1.0 and np.array_equal(one[2][0, 1:10], np.eye(3).ravel())


def test_argument_checks_return_before_any_hip_call():
    L = _lib.lib()
    f32, i32, f64 = (ctypes.c_float * 9)(), (ctypes.c_int32 * 1)(), (ctypes.c_double * 13)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    ok = [p(f32), 1, p(f32), 1, 3, p(i32), p(i32), 1, None, None, None, 0, 0, 0, p(f64), p(i32), None, None]

    def call(**change):
        names = ["pred", "Np", "gt", "Ng", "n", "pred_idx", "gt_idx", "P", "weight", "pred_root", "gt_root", "nr", "root_a", "root_b", "err",
                 "count", "transform", "stream"]
        args = list(ok)
        for k, v in change.items():
            args[names.index(k)] = v
        return L.h3d_pointset_errors(*args)
    for change, text in ((dict(n=0), b"n = 0"), (dict(n=-3), b"n = -3"), (dict(P=-1), b"P = -1"), (dict(pred=None), b"null"),
                         (dict(gt=None), b"null"), (dict(pred_idx=None), b"null"), (dict(gt_idx=None), b"null"), (dict(err=None), b"null"),
                         (dict(count=None), b"null"), (dict(pred_root=p(f32)), b"root"), (dict(pred_root=p(f32), gt_root=p(f32), nr=3, root_a=3), b"roots"),
                         (dict(pred_root=p(f32), gt_root=p(f32), nr=0), b"roots"), (dict(err=ctypes.c_void_p(ctypes.addressof(f64) + 4)), b"misaligned")):
        assert call(**change) == -5 and text in L.h3d_last_error(), change
    assert call(P=0, pred_idx=None, err=None) == 0                        # nothing to do: nothing is launched
    assert L.h3d_metric_means(p(f64), p(i32), -1, p(f64), p(i32), None) == -5 and b"P = -1" in L.h3d_last_error()
    assert L.h3d_metric_means(None, p(i32), 1, p(f64), p(i32), None) == -5 and b"null" in L.h3d_last_error()
    assert L.h3d_metric_means(p(f64), p(i32), 1, None, p(i32), None) == -5
    assert L.h3d_metric_means(p(f64), p(i32), 1, p(f64), None, None) == -5


def test_ground_truth_3d_container_and_the_summary():
    joints, verts = np.zeros((3, 2, 24, 3), np.float32), np.arange(3 * 2 * 5 * 3, dtype=np.float32).reshape(3, 2, 5, 3)
    g = ME.GroundTruth3D(joints, verts, [[1, 0], [1, 1], [0, 0]], np.ones((3, 2, 24)))
    sel = g.select([2, 0])
    assert (sel.N, sel.G) == (2, 2) and sel.valid.tolist() == [[0, 0], [1, 0]] and np.array_equal(sel.verts.numpy(), verts[[2, 0]])
    flat = g.flat("cpu")
    assert tuple(flat["verts"].shape) == (6, 5, 3) and tuple(flat["joint_weight"].shape) == (6, 24) and g.to("cpu")["valid"].dtype.is_floating_point is False
    with pytest.raises(ValueError):
        ME.GroundTruth3D(joints, verts[:2], [[1, 0], [1, 1], [0, 0]])
    r = ME.MeshEvalResult((np.array([0.0501, 0.0312]), 7, None, None), None)
    lines = r.summarize()
    assert len(lines) == 4 and "50.10 mm" in lines[0] and "31.20 mm" in lines[1] and "n/a" in lines[2] and r.n_pairs == 7
