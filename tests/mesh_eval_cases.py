"""The point-set cases tests/test_oracle_mesh_eval.py and tests/test_gpu_mesh_eval.py share, and the LAPACK closed form the mirror is held to."""
import numpy as np

FAMILIES = ("general", "reflected", "coplanar_source", "coplanar_target", "collinear_source", "equal_source", "equal_target")


def rotation(rs):
    """A random rotation (float64) by QR, determinant +1."""
    q, r = np.linalg.qr(rs.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def family_pair(family, n, seed):
    """-> (source [n,3], target [n,3]) float32.  Coordinates of order 1, offsets of order 1: a body in metres near the origin."""
    rs = np.random.RandomState(1000 * (FAMILIES + ("near_collinear_source",)).index(family) + seed)
    x = rs.standard_normal((n, 3)) * 0.3 + rs.uniform(-0.5, 0.5, 3)
    R0, s0, t0 = rotation(rs), rs.uniform(0.6, 1.6), rs.uniform(-0.5, 0.5, 3)
    noise = rs.standard_normal((n, 3)) * 0.02
    if family == "coplanar_source":
        x[:, 2] = 0.25                                     # exactly coplanar on odd seeds; rotated (coplanar to fp32 rounding) on even ones
        if seed % 2 == 0:
            x = x @ rotation(rs).T
    if family in ("collinear_source", "near_collinear_source"):
        # exactly collinear: a dyadic base point plus multiples of 1/64 of a direction of multiples of 1/4, all exact in float32.  (A line
        # in general position is collinear only to float32 rounding: M then has two singular values 1e-11 of the first, R about the line
        # is determined to 1e-4 only, by any SVD, and the error VALUE moves by 1e-14 of the extent with the rounding of M -- such sets
        # are held to the optimality of the residual instead, near_collinear_source.)
        alpha = rs.randint(-64, 65, n) / 64.0
        alpha[:2] = (-1.0, 1.0)
        d = rs.randint(-4, 5, 3) / 4.0
        d[seed % 3] = 1.0
        if family == "near_collinear_source":
            d = rotation(rs)[0]
        x = np.array([0.25, -0.5, 0.125]) + alpha[:, None] * d
    if family == "equal_source":
        x = np.broadcast_to(rs.uniform(-0.5, 0.5, 3), (n, 3))
    y = s0 * x @ R0.T + t0 + noise
    if family == "reflected":
        y = x * np.array([-1.0, 1.0, 1.0]) + noise
    if family == "coplanar_target":
        y[:, 1] = -0.375
        if seed % 2 == 0:
            y = y @ rotation(rs).T
    if family == "equal_target":
        y = np.broadcast_to(rs.uniform(-0.5, 0.5, 3) + 0.75, (n, 3))
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


def closed_form(x, y):
    """The textbook similarity Procrustes through LAPACK on the float32 points widened to float64: R = U diag(1, 1, det(U V^T)) V^T,
    s = trace(diag(1, 1, d) S) / var, t = mu_y - s R mu_x -> (mean |s R x + t - y|, s, R, t).  var == 0: R = I, s = 1."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx, my = x.mean(0), y.mean(0)
    xc, yc = x - mx, y - my
    var = (xc * xc).sum()
    if var == 0.0:
        R, s = np.eye(3), 1.0
    else:
        U, S, Vt = np.linalg.svd(yc.T @ xc)
        d = 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0
        R = U @ np.diag([1.0, 1.0, d]) @ Vt
        s = (S[0] + S[1] + d * S[2]) / var
    t = my - s * R @ mx
    return float(np.linalg.norm(s * x @ R.T + t - y, axis=1).mean()), s, R, t


def extent(family, y):
    """What an error of the aligned distance is measured against: the extent of the centred target, max |y - mu_y|.  A target whose points
    are all equal has none (the centred points are rounding noise of the mean); its error is measured against |y|, the size of the numbers
    s R x + t - y is computed from."""
    y = np.asarray(y, np.float64)
    if family == "equal_target":
        return float(np.linalg.norm(y, axis=1).max())
    return float(np.linalg.norm(y - y.mean(0), axis=1).max())


def lattice_case(n, seed):
    """The known answer: source coordinates multiples of 1/64 in [-1,1], target = 0.5 R0 x + t0 with R0 a signed permutation of
    determinant +1 and t0 dyadic -- exact in float32, so the true aligned error is 0 and the plain error can be computed by hand
    -> (x, y, R0, t0)."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-64, 65, (n, 3)) / 64.0
    x[:min(n, 3)] = np.eye(3)[:min(n, 3)]                   # (three points off one line, whatever the draw)
    perms = [((0, 1, 2), (1, 1, 1)), ((1, 2, 0), (1, -1, -1)), ((2, 0, 1), (-1, 1, -1)), ((1, 0, 2), (1, 1, -1)), ((0, 2, 1), (-1, 1, 1))]
    perm, sign = perms[seed % len(perms)]
    R0 = np.zeros((3, 3))
    for r in range(3):
        R0[r, perm[r]] = sign[r]
    assert round(np.linalg.det(R0)) == 1
    t0 = np.array([0.25, -1.5, 0.625])
    y = 0.5 * x @ R0.T + t0
    xf, yf = x.astype(np.float32), y.astype(np.float32)
    assert np.array_equal(xf.astype(np.float64), x) and np.array_equal(yf.astype(np.float64), y)
    return xf, yf, R0, t0


def device_case(n, P, seed, with_root, root):
    """A case of the bit-equality test: Np = 4 predictions and Ng = 5 ground truths of n points; P pairs with repeats in pred_idx, -1 on
    both sides, an out-of-range index on both sides; weight with an all-zero row (ground truth 3) and a one-valid-point row (4)
    -> dict of numpy arrays (root sources of nr = 3 points when with_root)."""
    rs = np.random.RandomState(seed)
    Np, Ng = 4, 5
    pred = (rs.standard_normal((Np, n, 3)) * 0.3 + rs.uniform(-0.5, 0.5, (Np, 1, 3))).astype(np.float32)
    gt = (rs.standard_normal((Ng, n, 3)) * 0.3 + rs.uniform(-0.5, 0.5, (Ng, 1, 3))).astype(np.float32)
    R0 = rotation(rs)
    gt[1] = (1.3 * pred[1].astype(np.float64) @ R0.T + 0.2 + rs.standard_normal((n, 3)) * 0.01).astype(np.float32)   # one close pair
    weight = (rs.uniform(size=(Ng, n)) < 0.8).astype(np.uint8)
    weight[:2] = 1
    weight[3] = 0
    weight[4] = 0
    weight[4, n // 2] = 1
    pred_idx = rs.randint(0, Np, P).astype(np.int32)
    gt_idx = rs.randint(0, Ng, P).astype(np.int32)
    fixed = [(1, 1), (1, 3), (2, 4), (-1, 0), (Np, 1), (0, -1), (1, Ng), (1, 0), (1, 2)]
    if P == 1:                                              # one pair cannot be all of them: the seed picks which
        fixed = [fixed[seed % 5]]
    for k, (a, b) in enumerate(fixed[:P]):
        pred_idx[k], gt_idx[k] = a, b
    out = dict(pred=pred, gt=gt, pred_idx=pred_idx, gt_idx=gt_idx, weight=weight, pred_root=None, gt_root=None, root=root)
    if with_root:
        out["pred_root"] = (rs.standard_normal((Np, 3, 3)) * 0.2).astype(np.float32)
        out["gt_root"] = (rs.standard_normal((Ng, 3, 3)) * 0.2).astype(np.float32)
    return out
