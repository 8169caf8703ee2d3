"""The rasteriser's definition (include/h3d.h section 4d) twice, in numpy, and the cases its tests share.

    render(...)            the fp32 mirror: brute force, every face over its clipped bounding box; integer edge functions in int64, every float
                           step one float32 operation in the header's order, the key minimum with numpy.  The kernels must equal it bit for bit.
    render(..., fp64=True) the same snapping and the same integer coverage; the depth in float64.  Also returns the two nearest depths per
                           pixel, so that a test can tell a real difference from a near tie.
    shade(...)             the shading, float32 in the header's order, or float64.
    render(..., debug=True) adds `counts`: how many faces cover each pixel with no depth test and no culling (watertightness).
"""
import numpy as np

F32 = np.float32
NEGATE_Z, CULL_BACK = 1, 2
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = 2 ** 19


def _bias(dx, dy):
    """0 for a top edge (dy == 0, dx > 0) or a left edge (dy < 0): a pixel centre on it is inside; 1 otherwise."""
    return 0 if (dy < 0 or (dy == 0 and dx > 0)) else 1


def project(v, s, tx, ty, cx, cy, up, dzp, flags):
    """v [V,3] float32 and float32 scalars -> xi, yi (int64), d (float32), ok (bool): the header's PROJECTION, one float32 op per step."""
    with np.errstate(all="ignore"):
        upf = F32(up)
        xs = upf * ((s * v[:, 0] + tx) + F32(cx))
        ys = upf * ((s * v[:, 1] + ty) + F32(cy))
        fx, fy = np.rint(F32(16) * xs), np.rint(F32(16) * ys)
        d = (-v[:, 2] if flags & NEGATE_Z else v[:, 2]) + dzp
        assert xs.dtype == F32 and fx.dtype == F32 and d.dtype == F32
        ok = (np.abs(fx) <= F32(GUARD)) & (np.abs(fy) <= F32(GUARD)) & (np.abs(d) < F32(np.inf))
    xi = np.where(ok, fx, 0).astype(np.int64)
    yi = np.where(ok, fy, 0).astype(np.int64)
    return xi, yi, d, ok


def render(verts, faces, cam_map, ind, n, up=1, valid=None, dz=None, flags=0, fp64=False, debug=False):
    """verts [P,V,3] f32, faces [F,3], cam_map [B,3,H,W] f32, ind [B,M] -> dict(face_id i32 [B,Hr,Wr], depth, keys u64 (fp32 only);
    fp64: depth and second = the two nearest depths; debug: counts)."""
    verts = np.ascontiguousarray(verts, F32).reshape(-1, verts.shape[-2], 3)
    cam_map = np.ascontiguousarray(cam_map, F32)
    faces = np.asarray(faces).astype(np.int64)
    B, _, H, W = cam_map.shape
    P, V, _ = verts.shape
    F = faces.shape[0]
    assert P == B * n and n * F < 2 ** 31
    Hr, Wr = up * H, up * W
    keys = np.full((B, Hr, Wr), NO_KEY, np.uint64)
    best = np.full((B, Hr, Wr), np.inf)
    second = np.full((B, Hr, Wr), np.inf)
    fid64 = np.full((B, Hr, Wr), -1, np.int32)
    counts = np.zeros((B, Hr, Wr), np.int32)
    negz = bool(flags & NEGATE_Z)
    for p in range(P):
        b, m = divmod(p, n)
        at = int(ind[b, m])
        if at < 0 or at >= H * W or (valid is not None and not valid.reshape(-1)[p]):
            continue
        s, tx, ty = (cam_map[b, c].reshape(-1)[at] for c in range(3))
        if not (s > 0 and s < np.inf):
            continue
        dzp = F32(0) if dz is None else F32(np.asarray(dz).reshape(-1)[p])
        xi, yi, d, ok = project(verts[p], s, tx, ty, at % W, at // W, up, dzp, flags)
        for f in range(F):
            i0, i1, i2 = (int(i) for i in faces[f])
            if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= V or not (ok[i0] and ok[i1] and ok[i2]):
                continue
            x0, y0, x1, y1, x2, y2 = (int(t) for t in (xi[i0], yi[i0], xi[i1], yi[i1], xi[i2], yi[i2]))
            o = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            if o == 0:
                continue
            culled = bool(flags & CULL_BACK) and ((o > 0) != negz)
            if o < 0:
                x1, y1, x2, y2, i1, i2, o = x2, y2, x1, y1, i2, i1, -o
            bx0, bx1 = max(0, -(-min(x0, x1, x2) // 16)), min(Wr - 1, max(x0, x1, x2) // 16)
            by0, by1 = max(0, -(-min(y0, y1, y2) // 16)), min(Hr - 1, max(y0, y1, y2) // 16)
            if bx0 > bx1 or by0 > by1:
                continue
            px = 16 * np.arange(bx0, bx1 + 1, dtype=np.int64)[None, :]
            py = 16 * np.arange(by0, by1 + 1, dtype=np.int64)[:, None]
            w0 = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1)
            w1 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2)
            w2 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
            assert (w0 + w1 + w2 == o).all()
            inside = (w0 >= _bias(x2 - x1, y2 - y1)) & (w1 >= _bias(x0 - x2, y0 - y2)) & (w2 >= _bias(x1 - x0, y1 - y0))
            sl = (b, slice(by0, by1 + 1), slice(bx0, bx1 + 1))
            counts[sl] += inside
            if culled or not inside.any():
                continue
            fid = m * F + f
            if fp64:
                d0, d1, d2 = float(d[i0]), float(d[i1]), float(d[i2])
                with np.errstate(all="ignore"):
                    dep = d0 + (w1 * (d1 - d0) + w2 * (d2 - d0)) / float(o)
                take = inside & ~np.isnan(dep)
                cb, cs, cf = best[sl], second[sl], fid64[sl]
                new = take & (dep < cb)              # faces come in ascending id: an equal depth keeps the smaller id
                second[sl] = np.where(new, cb, np.where(take, np.minimum(cs, dep), cs))
                best[sl] = np.where(new, dep, cb)
                fid64[sl] = np.where(new, fid, cf)
            else:
                with np.errstate(all="ignore"):
                    e1, e2 = d[i1] - d[i0], d[i2] - d[i0]
                    dep = d[i0] + (w1.astype(F32) * e1 + w2.astype(F32) * e2) / F32(o)
                assert dep.dtype == F32 and e1.dtype == F32
                take = inside & ~np.isnan(dep)
                u = dep.view(np.uint32)
                hi = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
                key = (hi << np.uint64(32)) | np.uint64(fid)
                keys[sl] = np.where(take, np.minimum(keys[sl], key), keys[sl])
    out = {"counts": counts} if debug else {}
    if fp64:
        out.update(face_id=fid64, depth=best, second=second)
        return out
    bg = keys == NO_KEY
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    dep = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7FFFFFFF), ~hi).astype(np.uint32).view(F32)
    out.update(face_id=np.where(bg, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32),
               depth=np.where(bg, F32(np.inf), dep).astype(F32), keys=keys)
    return out


def _rgb_of(packed):
    return np.array([(packed >> 16) & 255, (packed >> 8) & 255, packed & 255], np.uint8)


def shade(face_id, verts, faces, n, image=None, colour=None, alpha=0.7, ambient=0.3, background=0, default_colour=0xE6B48C, fp64=False):
    """face_id [B,Hr,Wr] (-1 = background) -> rgb [B,Hr,Wr,3] uint8: the header's SHADING in float32 (one op per step) or in float64."""
    T = np.float64 if fp64 else F32
    verts = np.ascontiguousarray(verts, F32).reshape(-1, verts.shape[-2], 3)
    faces = np.asarray(faces).astype(np.int64)
    B, Hr, Wr = face_id.shape
    V, F = verts.shape[1], faces.shape[0]
    img = np.broadcast_to(_rgb_of(background), (B, Hr, Wr, 3)) if image is None else np.asarray(image)
    out = np.array(img, np.uint8)
    m, f = np.divmod(face_id.astype(np.int64), F)
    fg = (face_id >= 0) & (m < n)
    tri = faces[np.where(fg, f, 0)]
    fg &= (tri >= 0).all(-1) & (tri < V).all(-1)
    bb, yy, xx = np.nonzero(fg)
    if len(bb) == 0:
        return out
    p = bb * n + m[bb, yy, xx]
    tri = tri[bb, yy, xx]
    v0, v1, v2 = (verts[p, tri[:, k]].astype(T) for k in range(3))
    alpha, ambient = T(F32(alpha)), T(F32(ambient))
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        inten = np.where(ln == 0, T(0), ambient + (T(1) - ambient) * (np.abs(nz) / ln))
        col = (np.broadcast_to(_rgb_of(default_colour), (len(p), 3)) if colour is None else np.asarray(colour).reshape(-1, 3)[p]).astype(T)
        val = np.rint(alpha * (inten[:, None] * col) + (T(1) - alpha) * img[bb, yy, xx].astype(T))
        assert val.dtype == T and inten.dtype == T
        sat = np.where(val >= 255, 255, np.where(val >= 0, val, 0))
    out[bb, yy, xx] = sat.astype(np.uint8)
    return out


# ---- bodies and cases ----------------------------------------------------------------------------------------------------------------
def rotation(rs):
    """A seeded random rotation matrix (float64)."""
    q = rs.randn(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def camera(B, H, W, n, seed, s_range=(4.0, 10.0), max_objs=None, centre=None):
    """A seeded `cam` map [B,3,H,W] (noise everywhere, so that a read at the wrong pixel shows) and ind [B,max_objs] whose first n slots per
    image are distinct pixels of the inner part of the map; (s, tx, ty) there: s in s_range, t in [-0.5, 0.5]."""
    rs = np.random.RandomState(seed)
    M = max_objs or n + 1
    cam = rs.randn(B, 3, H, W).astype(F32)
    ind = np.full((B, M), -1, np.int64)
    for b in range(B):
        ys, xs = np.meshgrid(np.arange(H // 4, H - H // 4), np.arange(W // 4, W - W // 4), indexing="ij")
        pick = rs.permutation(ys.size)[:M]
        ind[b] = ys.reshape(-1)[pick] * W + xs.reshape(-1)[pick] if centre is None else centre
        for mm in range(M):
            cam[b, :, ind[b, mm] // W, ind[b, mm] % W] = (rs.uniform(*s_range), rs.uniform(-0.5, 0.5), rs.uniform(-0.5, 0.5))
    return cam, ind


def capsule_case(seed, n=3, up=1, rings=5, segments=8, B=2, H=16, W=16, flags=0, with_dz=True, s_range=(4.0, 10.0)):
    """B x n randomly turned capsules (h3d_amd.render.capsule_mesh) at random centres: a dict of render()'s arguments."""
    from h3d_amd import render as hrender
    rs = np.random.RandomState(1000 + seed)
    v, faces = hrender.capsule_mesh(rings, segments)
    verts = np.stack([(v.astype(np.float64) @ rotation(rs).T) for _ in range(B * n)]).astype(F32)
    cam, ind = camera(B, H, W, n, seed, s_range)
    dz = rs.uniform(2.0, 6.0, B * n).astype(F32) if with_dz else None
    return dict(verts=verts, faces=faces, cam_map=cam, ind=ind, n=n, up=up, valid=None, dz=dz, flags=flags)


def square_case(shift=(0, 0), up=1, H=16, W=16):
    """Two triangles on the square (2,2) .. (6,6) of map pixels, s = 1, t = 0, centre pixel 0, moved by `shift` lattice steps of 1/16 pixel
    (exact in float32): slot 0 of image 0; image 1 is empty (ind = -1)."""
    dx, dy = shift[0] / 16.0, shift[1] / 16.0
    verts = np.zeros((2, 4, 3), F32)
    verts[0] = [[2 + dx, 2 + dy, 0], [6 + dx, 2 + dy, 0], [6 + dx, 6 + dy, 0], [2 + dx, 6 + dy, 0]]
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    cam = np.zeros((2, 3, H, W), F32)
    cam[:, 0] = 1.0
    ind = np.array([[0], [-1]], np.int64)
    return dict(verts=verts, faces=faces, cam_map=cam, ind=ind, n=1, up=up, valid=None, dz=None, flags=0)


def triangle_case(up=1):
    """One triangle whose vertices project exactly on the pixel centres (3,2), (9,4), (5,11) of the map (s = 2 about centre pixel (1,1))."""
    H = W = 16
    pts = np.array([[3, 2], [9, 4], [5, 11]], np.float64)
    verts = np.zeros((2, 3, 3), F32)
    verts[0, :, :2] = (pts - 1.0) / 2.0
    verts[0, :, 2] = [0.5, -0.25, 1.0]
    cam = np.zeros((2, 3, H, W), F32)
    cam[:, 0] = 2.0
    ind = np.array([[W + 1], [-1]], np.int64)
    return dict(verts=verts, faces=np.array([[0, 1, 2]], np.int32), cam_map=cam, ind=ind, n=1, up=up, valid=None, dz=None, flags=0)


def render_case(case, **kw):
    args = dict(case, **kw)
    return render(args.pop("verts"), args.pop("faces"), args.pop("cam_map"), args.pop("ind"), args.pop("n"), **args)
