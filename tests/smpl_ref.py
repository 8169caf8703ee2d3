"""TEST INFRASTRUCTURE ONLY -- the yardstick of the SMPL comparisons: a plain restatement of oracle/smpl.py with a `dtype` argument (float64
for the value, float32 for the error a correct fp32 implementation of the same formulas makes), an fp64 emulation of what the
generation-3 kernel is meant to compute (hh + hm + mh of the three-term bf16 split), a jointed test body, and the rule of the comparison.
Shared by tests/test_oracle_smpl_ref.py and tests/test_gpu_smpl_edges.py; no GPU needed."""
import numpy as np

from oracle import smpl as osmpl

PARENTS = osmpl.PARENTS
NAMES = ("verts", "joints", "pose_feat", "A")
NJ, NB, NPF = 24, 10, 207


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def rodrigues(theta, dtype):
    """oracle.smpl.rodrigues with every intermediate in `dtype` (smplx convention: angle = ||theta + 1e-8||)."""
    dt = np.dtype(dtype).type
    theta = np.asarray(theta, dtype)
    if dt is np.float64:
        angle = np.linalg.norm(theta + 1e-8, axis=-1, keepdims=True)          # the oracle's own expression: bit-identical
    else:
        e = theta + dt(1e-8)
        angle = np.sqrt(e[..., 0:1] * e[..., 0:1] + e[..., 1:2] * e[..., 1:2] + e[..., 2:3] * e[..., 2:3])
    d = theta / angle
    s = np.sin(angle)[..., None]
    c = np.cos(angle)[..., None]
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    zero = np.zeros_like(x)
    K = np.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(theta.shape[:-1] + (3, 3))
    R = np.eye(3, dtype=dtype) + s * K + (dt(1) - c) * (K @ K)
    assert R.dtype == np.dtype(dtype)
    return R


def _rne_bf16(x):
    """float32 -> the nearest bf16 value (ties to even), returned as float32: the rounding of smpl._dirs_k3 and of split3."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split_hm(x):
    """The first two terms (h, m) of the three-term bf16 split of the float32 value of x, as float64."""
    x = np.asarray(x, np.float32)
    h = _rne_bf16(x)
    m = _rne_bf16(x - h)                     # x - h is exact in float32
    return h.astype(np.float64), m.astype(np.float64)


def _blend(D, coef, dtype, emulate):
    """sum_k D[v,c,k] * coef[p,k] -> [P,V,3].  float64: the oracle's einsum (bit-identical to it).  float32: a plain chain, one k after the
    other over float32 arrays, so that its error is that of 217 sequential roundings and not of numpy's blocked summation.
    emulate="gen3": float64 with every product d*c replaced by dh*ch + dh*cm + dm*ch."""
    if emulate == "gen3":
        dh, dm = split_hm(D)
        ch, cm = split_hm(coef)
        return (np.einsum("vck,pk->pvc", dh, ch) + np.einsum("vck,pk->pvc", dh, cm)) + np.einsum("vck,pk->pvc", dm, ch)
    assert emulate is None, emulate
    if np.dtype(dtype) == np.float64:
        return np.einsum("vck,pk->pvc", D, coef)
    acc = np.zeros((coef.shape[0],) + D.shape[:2], dtype)
    for k in range(D.shape[2]):
        acc += D[None, :, :, k] * coef[:, None, None, k]
    return acc


def lbs(betas, thetas, model, dtype=np.float64, emulate=None):
    """oracle.smpl.lbs restated: -> verts [P,V,3], joints [P,24,3], pose_feat [P,207], A [P,24,12] (rows [R | t] of the 3x4 skinning
    transforms, the layout of h3d_smpl_pose), all in `dtype`.  In float64 verts and joints equal oracle.smpl.lbs bit for bit."""
    dt = np.dtype(dtype)
    assert emulate is None or dt == np.float64
    v_t, S, Pd, Jreg, W = [np.asarray(model[k], dt) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")]
    parents = np.asarray(model["parents"])
    betas = np.asarray(betas, dt)
    thetas = np.asarray(thetas, dt).reshape(-1, NJ, 3)
    P = betas.shape[0]
    v_s = v_t[None] + _blend(S, betas, dt, emulate)
    # the joints come from the exact shape blend in every mode: the kernels never form them from the matrix-core product
    J = np.einsum("jv,pvc->pjc", Jreg, v_s if emulate is None else v_t[None] + _blend(S, betas, dt, None))
    R = rodrigues(thetas, dt)
    pf = (R[:, 1:] - np.eye(3, dtype=dt)).reshape(P, NPF)
    v_p = v_s + _blend(Pd, pf, dt, emulate)
    G = np.zeros((P, NJ, 4, 4), dt)
    for j in range(NJ):
        T = np.zeros((P, 4, 4), dt)
        T[:, :3, :3] = R[:, j]
        T[:, 3, 3] = 1
        if parents[j] < 0:
            T[:, :3, 3] = J[:, j]
            G[:, j] = T
        else:
            T[:, :3, 3] = J[:, j] - J[:, parents[j]]
            G[:, j] = G[:, parents[j]] @ T
    joints = G[:, :, :3, 3].copy()
    A = G.copy()
    A[:, :, :3, 3] -= np.einsum("pjab,pjb->pja", G[:, :, :3, :3], J)
    Tv = np.einsum("vj,pjab->pvab", W, A)
    vh = np.concatenate([v_p, np.ones((P, v_p.shape[1], 1), dt)], -1)
    verts = np.einsum("pvab,pvb->pva", Tv, vh)[..., :3]
    out = verts, joints, pf, np.ascontiguousarray(A[:, :, :3, :]).reshape(P, NJ, 12)
    assert all(o.dtype == dt for o in out)
    return out


# ---- the test body -----------------------------------------------------------------------------------------------------------------
_DOWN, _UP = (1, 2, 4, 5, 7, 8, 10, 11), (3, 6, 9, 12, 15)


def jointed_model(V, seed=0, max_nnz=4):
    """A body with a skeleton, as the numpy dict of SMPLModel.numpy_dict(); a pure function of its arguments.
    Limbs of length 0.1 .. 0.3 on the 24-joint tree (legs down, spine up, arms sideways: extent about 1 m), every vertex within 0.08 of
    a joint, each regressor row over the 12 vertices nearest to its joint, skinning weights on the vertex's nearest joints with a
    per-vertex count drawn from 1 .. max_nnz (so exact zeros are present, and max_nnz > 4 gives a model for the dense skinning loop)."""
    rs = np.random.RandomState(seed)
    Jpos = np.zeros((NJ, 3))
    for j in range(1, NJ):
        side = -1.0 if j % 2 else 1.0
        base = np.array([0.0, -1.0, 0.0]) if j in _DOWN else np.array([0.0, 1.0, 0.0]) if j in _UP else np.array([side, 0.0, 0.0])
        if j in (1, 2):
            base = np.array([side, -0.5, 0.0])
        d = base + rs.uniform(-0.3, 0.3, 3)
        Jpos[j] = Jpos[PARENTS[j]] + d / np.linalg.norm(d) * rs.uniform(0.1, 0.3)
    own = rs.permutation(NJ)[np.arange(V) % NJ]                    # every joint owns V/24 vertices (round robin)
    off = rs.uniform(-1.0, 1.0, (V, 3))
    off *= (0.08 * rs.uniform(0.0, 1.0, (V, 1)) ** (1.0 / 3.0)) / np.maximum(np.linalg.norm(off, axis=1, keepdims=True), 1e-12)
    vt = Jpos[own] + off
    dist = np.linalg.norm(vt[:, None] - Jpos[None], axis=-1)      # [V,24]
    near = np.argsort(dist, axis=1, kind="stable")
    count = rs.randint(1, max_nnz + 1, V)
    count[:max_nnz] = np.arange(1, max_nnz + 1)[:V]                # every count is present whatever the draw
    W = np.zeros((V, NJ))
    for v in range(V):
        W[v, near[v, :count[v]]] = rs.uniform(0.1, 1.0, count[v])
    W /= W.sum(1, keepdims=True)
    Jr = np.zeros((NJ, V))
    n = min(12, V)
    for j in range(NJ):
        Jr[j, np.argsort(dist[:, j], kind="stable")[:n]] = rs.uniform(0.1, 1.0, n)
    Jr /= Jr.sum(1, keepdims=True)
    return {"v_template": vt.astype(np.float32), "shapedirs": rs.uniform(-0.03, 0.03, (V, 3, NB)).astype(np.float32),
            "posedirs": rs.uniform(-0.01, 0.01, (V, 3, NPF)).astype(np.float32), "J_regressor": Jr.astype(np.float32),
            "weights": W.astype(np.float32), "parents": PARENTS.copy()}


def special_thetas(P, seed, scale=0.5):
    """[P,72] float32: N(0, scale) poses; the first 12 persons (as many as fit) are the pose edges: rest pose, one zero joint between
    rotated neighbours, all components 1e-7 / 1e-5 / 1e-3 (1 - cos cancels), one joint at (0, pi, 0), at (2 pi, 0, 0) and at 7 rad about
    a negative axis (argument reduction), every joint by 3 rad, random poses of scale 3 rad, 1e-6 and 1e-4."""
    rs = np.random.RandomState(seed)
    th = (rs.randn(P, NJ, 3) * scale).astype(np.float32)
    big = (rs.randn(NJ, 3) * 3.0).astype(np.float32)
    ax = rs.randn(NJ, 3)
    ax = 3.0 * ax / np.linalg.norm(ax, axis=1, keepdims=True)
    one = np.zeros((3, NJ, 3), np.float32)
    one[0, 6] = [0.0, np.pi, 0.0]
    one[1, 1] = [2 * np.pi, 0.0, 0.0]
    one[2, 16] = [0.0, 0.0, -7.0]
    edges = [np.zeros((NJ, 3)), None, np.full((NJ, 3), 1e-7), np.full((NJ, 3), 1e-5), np.full((NJ, 3), 1e-3), one[0], one[1], one[2], ax, big,
             np.full((NJ, 3), 1e-6), np.full((NJ, 3), 1e-4)]
    for i, e in enumerate(edges[:P]):
        if e is None:
            th[i, 9] = 0.0                   # spine3 at rest between a rotated spine2 and rotated neck / collars
        else:
            th[i] = e
    return th.reshape(P, 72)


def make_case(P, seed):
    """betas [P,10] ~ N(0,1) and the thetas of special_thetas (float32)."""
    return np.random.RandomState(1000 + seed).randn(P, NB).astype(np.float32), special_thetas(P, seed)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def bounds(betas, thetas, model, emulate=None):
    """(target, e32): target = the four float64 tensors a kernel is compared with (emulate="gen3": what generation 3 is meant to compute);
    e32[i] = max |float32 restatement - float64 restatement| over the whole tensor i, the error of the same formulas in plain float32."""
    r64 = lbs(betas, thetas, model, np.float64)
    r32 = lbs(betas, thetas, model, np.float32)
    e32 = [float(np.abs(a.astype(np.float64) - r).max()) for a, r in zip(r32, r64)]
    return (lbs(betas, thetas, model, np.float64, emulate) if emulate else r64), e32


def check(name, got, target, e32, factor=4.0):
    """The rule, per output tensor (a None in `got` is skipped): max |gpu - f64| <= factor * e32 + 2^-23 * max |f64| -- `factor` times the
    error of a plain float32 run plus one rounding of the output at the body's extent.  Returns the observed ratios err / e32."""
    ratios, fails = {}, []
    for nm, g, r, e in zip(NAMES, got, target, e32):
        if g is None:
            continue
        g = np.asarray(g.detach().cpu().numpy() if hasattr(g, "detach") else g, np.float64).reshape(r.shape)
        err = float(np.abs(g - r).max())
        limit = factor * e + 2.0 ** -23 * float(np.abs(r).max())
        ratios[nm] = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s: err %.3g e32 %.3g ratio %.3g limit %.3g max|f64| %.3g" % (name, nm, err, e, ratios[nm], limit, float(np.abs(r).max())))
        if not err <= limit:
            fails.append((nm, err, limit))
    assert not fails, (name, fails)
    return ratios
