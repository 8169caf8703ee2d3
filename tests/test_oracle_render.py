"""CPU (-m "not gpu"): the rasteriser's definition (include/h3d.h section 4d) checked on its own -- known answers that need no mirror, the
watertightness of the coverage rule, the fp32 mirror against the fp64 version (tests/render_ref.py) -- and the host logic of
h3d_amd/render.py and of the three entry points (every check of theirs runs before the first HIP call, so without a GPU)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
from h3d_amd import _lib, detector, render, smpl

import render_ref as RR


# ---- 1. known answers ----------------------------------------------------------------------------------------------------------------
def _square_pixels(shift):
    """Pixel centres i with 2 + shift/16 <= i < 6 + shift/16, from integers alone (top and left borders in, bottom and right out)."""
    return [i for i in range(16) if 32 + shift <= 16 * i < 96 + shift]


@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1)])
def test_square_of_two_triangles_covers_each_of_its_pixels_once(shift):
    r = RR.render_case(RR.square_case(shift), debug=True)
    want = np.zeros((16, 16), np.int32)
    xs, ys = _square_pixels(shift[0]), _square_pixels(shift[1])
    want[np.ix_(ys, xs)] = 1
    assert len(xs) == 4 and len(ys) == 4 and (xs == [2, 3, 4, 5]) == (shift[0] <= 0)
    assert np.array_equal(r["counts"][0], want) and not r["counts"][1].any()
    assert np.array_equal(r["face_id"][0] >= 0, want == 1) and (r["face_id"][1] == -1).all()
    assert (r["depth"][0][want == 1] == 0).all() and np.isposinf(r["depth"][0][want == 0]).all()
    # the diagonal (2,2) .. (6,6) is the LEFT edge of face 0 (the upper right triangle) and neither top nor left for face 1: face 0 takes it
    # (with the same shift in x and y the diagonal still runs through pixel centres)
    if shift[0] == shift[1]:
        assert [int(r["face_id"][0, y, x]) for y, x in zip(ys, xs)] == [0, 0, 0, 0]
        assert all(r["face_id"][0, y, x] == (0 if x >= y else 1) for y in ys for x in xs)
    assert set(r["face_id"][0][want == 1].tolist()) == {0, 1}


@pytest.mark.parametrize("up,covered", [(1, 24), (2, 98)])
def test_triangle_with_vertices_on_pixel_centres(up, covered):
    # Pick's theorem on the lattice of pixel centres.  up = 1: area 25, 4 boundary points -> 24 interior; the only boundary points are the
    # vertices and (6,3) on v0 -> v1, none on a top or left edge alone -> 24 pixels.  up = 2: area 100, 8 boundary points -> 97 interior, and
    # the left edge v2 -> v0 holds one point between its ends -> 98.
    r = RR.render_case(RR.triangle_case(up), debug=True)
    c = r["counts"][0]
    assert int(c.sum()) == covered and c.max() == 1
    for x, y in ((3, 2), (9, 4), (5, 11)):          # every vertex lies on an edge that is neither top nor left
        assert c[up * y, up * x] == 0
    assert c[up * 3, up * 6] == 0                   # on v0 -> v1, whose inside is below it but which is not horizontal: out
    assert c[up * 3 + 1, up * 6] == 1
    if up == 2:
        assert c[13, 8] == 1                        # the midpoint of the left edge (10,22) -> (6,4)
    # depth is the barycentric combination: at an interior pixel within float32 rounding of the plane through the vertices
    d = r["depth"][0]
    A = np.array([[3, 2, 1], [9, 4, 1], [5, 11, 1]], np.float64)
    plane = np.linalg.solve(A, np.array([0.5, -0.25, 1.0]))
    ys, xs = np.nonzero(c)
    assert np.abs(d[ys, xs] - (plane[0] * xs / up + plane[1] * ys / up + plane[2])).max() < 1e-6


def _edges(faces):
    e = {}
    for a, b, c in faces.tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            e[(u, v)] = e.get((u, v), 0) + 1
    return e


@pytest.mark.parametrize("rings,segments", [(2, 3), (5, 8), (6, 7), (82, 84)])
def test_capsule_mesh_is_a_closed_outward_oriented_sphere(rings, segments):
    v, f = render.capsule_mesh(rings, segments)
    V, F = rings * segments + 2, 2 * rings * segments
    assert v.shape == (V, 3) and v.dtype == np.float32 and f.shape == (F, 3) and f.dtype == np.int32
    assert f.min() == 0 and f.max() == V - 1 and len(np.unique(f)) == V
    e = _edges(f)
    assert all(n == 1 for n in e.values()) and all((b, a) in e for a, b in e)       # every edge in two faces, once in each direction
    assert V - len(e) // 2 + F == 2
    tri = v.astype(np.float64)[f]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("fc,fc->f", nrm, tri.mean(1)) > 0).all()                      # convex about the origin: outward = away from it
    assert np.linalg.norm(nrm, axis=1).min() > 0
    if (rings, segments) == (82, 84):
        assert (V, F) == (smpl.NUM_VERTS, 13776)


# ---- 2. / 3. the mirror on closed bodies ---------------------------------------------------------------------------------------------
# (seed, n, up, rings, segments, flags): seeds chosen so that in every case the fp32 mirror and the fp64 version pick the same face on all
# but at most 1 % of the covered pixels (asserted below)
CAPSULES = [(0, 1, 1, 5, 8, 0), (1, 3, 1, 4, 6, 0), (2, 3, 2, 5, 8, 0), (3, 1, 4, 3, 5, 0), (4, 3, 4, 6, 7, RR.NEGATE_Z), (5, 3, 2, 5, 8, RR.CULL_BACK)]
_cache = {}


def _capsule(i):
    if i not in _cache:
        seed, n, up, rings, segments, flags = CAPSULES[i]
        case = RR.capsule_case(seed, n=n, up=up, rings=rings, segments=segments, flags=flags, with_dz=i != 3)      # (one case without dz)
        _cache[i] = (case, RR.render_case(case, debug=True), RR.render_case(case, fp64=True, debug=True))
    return _cache[i]


@pytest.mark.parametrize("i", range(len(CAPSULES)))
def test_closed_convex_bodies_cover_every_pixel_twice_or_not_at_all(i):
    case, r32, _ = _capsule(i)
    c = r32["counts"]
    # one convex body alone: 0 or 2 (front and back); several: every count even
    assert (c % 2 == 0).all() and c.max() >= 2
    for p in range(2 * case["n"]):
        valid = np.zeros(2 * case["n"], np.uint8)
        valid[p] = 1
        one = RR.render_case(case, valid=valid, debug=True)["counts"]
        assert set(np.unique(one).tolist()) == {0, 2}
    assert (r32["face_id"] >= 0).sum() >= 10


def _face_dmax(case):
    """[B, n F]: the largest |d| over the three vertices of every (slot, face)."""
    B, n, F = case["cam_map"].shape[0], case["n"], case["faces"].shape[0]
    H, W = case["cam_map"].shape[2:]
    out = np.zeros((B, n * F), np.float32)
    for p in range(B * n):
        b, m = divmod(p, n)
        at = int(case["ind"][b, m])
        s, tx, ty = case["cam_map"][b, :, at // W, at % W]
        dzp = np.float32(0) if case["dz"] is None else case["dz"][p]
        d = RR.project(case["verts"][p], s, tx, ty, at % W, at // W, case["up"], dzp, case["flags"])[2]
        out[b, m * F:(m + 1) * F] = np.abs(d)[case["faces"]].max(1)
    return out


@pytest.mark.parametrize("i", range(len(CAPSULES)))
def test_fp32_mirror_against_the_fp64_version(i):
    case, r32, r64 = _capsule(i)
    assert np.array_equal(r32["counts"], r64["counts"])
    cov = r32["face_id"] >= 0
    assert np.array_equal(cov, r64["face_id"] >= 0) and np.array_equal(cov, np.isfinite(r32["depth"]))
    same = cov & (r32["face_id"] == r64["face_id"])
    # depth: within 4 ulp of the largest |d| of the face
    dmax = np.take_along_axis(_face_dmax(case), np.where(cov, r32["face_id"], 0).reshape(2, -1), 1).reshape(cov.shape)
    err = np.abs(r32["depth"][same].astype(np.float64) - r64["depth"][same]) / np.spacing(dmax[same]).astype(np.float64)
    print("case %d: covered %d, depth error max %.2f ulp, face_id differs on %d" % (i, cov.sum(), err.max(), (cov & ~same).sum()))
    assert err.max() <= 4
    # face_id: equal wherever the two nearest fp64 depths differ by more than 1e-5 relative; the near ties are at most 1 % of a case
    # (a pixel only one face covers has no second depth: second = inf)
    with np.errstate(invalid="ignore"):
        scale = np.where(np.isfinite(r64["second"]), np.maximum(np.abs(r64["depth"]), np.abs(r64["second"])), np.abs(r64["depth"]))
        clear = cov & ((r64["second"] - r64["depth"]) > 1e-5 * scale)
    assert np.array_equal(r32["face_id"][clear], r64["face_id"][clear])
    assert (cov & ~clear).sum() <= 0.01 * cov.sum()
    # rgb: each version shades its own winners
    rs = np.random.RandomState(i)
    image = rs.randint(0, 256, cov.shape + (3,)).astype(np.uint8)
    colour = rs.randint(0, 256, (2 * case["n"], 3)).astype(np.uint8)
    for kw in (dict(image=image, colour=colour, alpha=0.7, ambient=0.3), dict(image=None, colour=None, alpha=1.0, ambient=0.0, background=0x102030)):
        a = RR.shade(r32["face_id"], case["verts"], case["faces"], case["n"], **kw)
        b = RR.shade(r64["face_id"], case["verts"], case["faces"], case["n"], fp64=True, **kw)
        assert np.abs(a.astype(np.int32) - b.astype(np.int32)).max() <= 1
        assert np.array_equal(a[~cov], (image if kw["image"] is not None else np.broadcast_to([0x10, 0x20, 0x30], a.shape))[~cov])
        assert (a[cov] != b[cov]).mean() < 0.05


def test_mirror_flags_and_skips_follow_the_header():
    case = RR.capsule_case(7, n=2, up=2)
    base = RR.render_case(case)
    # NEGATE_Z is the mesh with Z negated; culling a closed outward body changes nothing; an inside-out body shows its far side
    flipped = dict(case, verts=case["verts"] * np.array([1, 1, -1], np.float32))
    neg = RR.render_case(flipped, flags=RR.NEGATE_Z)
    assert np.array_equal(neg["keys"], base["keys"])
    cull = RR.render_case(case, flags=RR.CULL_BACK)
    assert np.array_equal(cull["keys"], base["keys"])
    inside_out = dict(case, faces=case["faces"][:, ::-1].copy())
    far = RR.render_case(inside_out, flags=RR.CULL_BACK)
    cov = base["face_id"] >= 0
    assert np.array_equal(far["face_id"] >= 0, cov) and (far["depth"][cov] >= base["depth"][cov]).all()
    assert (far["depth"][cov] > base["depth"][cov]).mean() > 0.9 and not (far["face_id"][cov] == base["face_id"][cov]).any()
    # the skipped slots write nothing
    n = case["n"]
    for kind in ("ind", "valid", "s0", "sneg", "snan"):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
        at = int(case["ind"][0, 1])
        if kind == "ind":
            c["ind"][0, 1] = 16 * 16
        elif kind == "valid":
            c["valid"] = np.array([1, 0] + [1] * n, np.uint8)
        else:
            c["cam_map"][0, 0, at // 16, at % 16] = {"s0": 0.0, "sneg": -1.0, "snan": np.nan}[kind]
        twin = RR.render_case(case, valid=np.array([1, 0] + [1] * n, np.uint8))
        got = RR.render_case(c)
        assert np.array_equal(got["keys"], twin["keys"]), kind
        assert not np.array_equal(got["keys"][0], base["keys"][0]) and np.array_equal(got["keys"][1], base["keys"][1])


# ---- 4. host logic ---------------------------------------------------------------------------------------------------------------------
FAKE = 0x10000
OK, SHAPE, UNSUPPORTED, ARG = 0, -1, -4, -5


def _rasterize_rc(**over):
    a = dict(verts=FAKE, faces=FAKE, cam=FAKE, ind=FAKE, valid=None, dz=None, B=2, max_objs=4, n=3, V=100, F=196, H=16, W=16, up=2, flags=0,
             face_id=FAKE, depth=FAKE, ws=FAKE, ws_bytes=2 * 32 * 32 * 8)
    a.update(over)
    return _lib.lib().h3d_render_rasterize(a["verts"], a["faces"], a["cam"], a["ind"], a["valid"], a["dz"], a["B"], a["max_objs"], a["n"], a["V"],
                                           a["F"], a["H"], a["W"], a["up"], a["flags"], a["face_id"], a["depth"], a["ws"], a["ws_bytes"], None)


def _shade_rc(**over):
    a = dict(keys=FAKE, verts=FAKE, faces=FAKE, colour=None, image=None, B=2, n=3, V=100, F=196, Hr=32, Wr=32, alpha=0.7, ambient=0.3,
             default_colour=0xFFFFFF, background=0, rgb=FAKE)
    a.update(over)
    return _lib.lib().h3d_render_shade(a["keys"], a["verts"], a["faces"], a["colour"], a["image"], a["B"], a["n"], a["V"], a["F"], a["Hr"], a["Wr"],
                                       a["alpha"], a["ambient"], a["default_colour"], a["background"], a["rgb"], None)


def test_header_exports_and_ctypes_mirror():
    L = _lib.lib()
    for name in ("h3d_render_workspace_bytes", "h3d_render_rasterize", "h3d_render_shade"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "h3d.h")).read()
    for name, value in (("NEGATE_Z", 1), ("CULL_BACK", 2), ("MAX_V", _lib.RENDER_MAX_V), ("MAX_SIDE", 16384)):
        assert "#define H3D_RENDER_%s %d\n" % (name, value) in hdr and getattr(_lib, "RENDER_" + name) == value
    assert render.MAX_V == _lib.RENDER_MAX_V >= smpl.NUM_VERTS and (render.NEGATE_Z, render.CULL_BACK) == (1, 2)
    assert L.h3d_abi_version() == _lib.ABI_VERSION == 4          # additive: three new entry points, nothing existing changed
    # the largest multiple of 64 whose staging fits the 160 KiB of LDS beside the 6 KiB queue and 256 B of static LDS
    assert 12 * _lib.RENDER_MAX_V + 6144 + 256 <= 160 * 1024 < 12 * (_lib.RENDER_MAX_V + 64) + 6144 + 256


def test_workspace_bytes_and_its_return_codes():
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.h3d_render_workspace_bytes(2, 64, 48, ctypes.byref(n)) == OK and n.value == 2 * 64 * 48 * 8
    assert L.h3d_render_workspace_bytes(1, 3, 5, ctypes.byref(n)) == OK and n.value == 256
    assert L.h3d_render_workspace_bytes(1, 4, 4, None) == ARG and b"null pointer" in L.h3d_last_error()
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 16385, 4), (1, 4, 16385), (9, 16384, 16384)):
        assert L.h3d_render_workspace_bytes(*bad, ctypes.byref(n)) == SHAPE, bad


def test_rasterize_return_codes_without_a_gpu():
    L = _lib.lib()
    for kw in ({"verts": None}, {"faces": None}, {"cam": None}, {"ind": None}, {"face_id": None}, {"depth": None}):
        assert _rasterize_rc(**kw) == ARG and b"null pointer" in L.h3d_last_error(), kw
    for kw in ({"ws": None}, {"ws_bytes": 2 * 32 * 32 * 8 - 1}, {"ws": FAKE + 4}):
        assert _rasterize_rc(**kw) == ARG and b"workspace" in L.h3d_last_error(), kw
    assert _rasterize_rc(flags=4) == ARG and b"flags" in L.h3d_last_error()
    for kw in ({"B": 0}, {"max_objs": 0}, {"n": 0}, {"V": 0}, {"F": -1}, {"H": 0}, {"W": 0}, {"n": 5}, {"up": 0}, {"up": -2}, {"up": 1025},
               {"H": 16385, "up": 1}):
        assert _rasterize_rc(**kw) == SHAPE, kw
    assert _rasterize_rc(V=_lib.RENDER_MAX_V + 1) == UNSUPPORTED and b"LDS" in L.h3d_last_error()
    assert _rasterize_rc(n=4, F=2 ** 29) == UNSUPPORTED and b"2^31" in L.h3d_last_error()
    assert _rasterize_rc(n=3, max_objs=4, F=(2 ** 31) // 3 + 1) == UNSUPPORTED
    with pytest.raises(RuntimeError, match="unsupported error"):
        _lib.check(_rasterize_rc(V=20000), "h3d_render_rasterize")


def test_shade_return_codes_without_a_gpu():
    L = _lib.lib()
    for kw in ({"keys": None}, {"verts": None}, {"faces": None}, {"rgb": None}):
        assert _shade_rc(**kw) == ARG and b"null pointer" in L.h3d_last_error(), kw
    assert _shade_rc(keys=FAKE + 4) == ARG and b"aligned" in L.h3d_last_error()
    for kw in ({"alpha": 1.5}, {"alpha": -0.1}, {"alpha": float("nan")}, {"ambient": 2.0}, {"ambient": float("nan")}):
        assert _shade_rc(**kw) == ARG and b"[0, 1]" in L.h3d_last_error(), kw
    for kw in ({"B": 0}, {"Hr": 0}, {"Wr": 16385}, {"n": 0}, {"V": 0}, {"F": 0}):
        assert _shade_rc(**kw) == SHAPE, kw
    assert _shade_rc(n=4, F=2 ** 29) == UNSUPPORTED


def test_opt_smpl_cam_adds_the_cam_head_and_nothing_else_changes():
    base = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}
    assert detector.Opt().heads == base and detector.Opt(smpl_cam=True).heads == base          # smpl_cam alone: no SMPL stage, no head
    assert detector.Opt(smpl=True).heads == dict(base, pose=72, shape=10)
    assert detector.Opt(smpl=True, smpl_cam=True).heads == dict(base, pose=72, shape=10, cam=3)
    assert list(detector.Opt(smpl=True, smpl_cam=True).heads)[-1] == "cam" and detector.Opt().smpl_cam is False
    assert "cam" not in detector.Opt(task="ctdet", smpl=True, smpl_cam=True).heads


def test_smpl_model_carries_optional_faces(tmp_path):
    m = smpl.SMPLModel.synthetic(seed=0, num_verts=42)
    assert m.faces is None and "faces" not in m.numpy_dict() and len(m.numpy_dict()) == 6
    _, f = render.capsule_mesh(5, 8)
    d = m.numpy_dict()
    mf = smpl.SMPLModel(d["v_template"], d["shapedirs"], d["posedirs"], d["J_regressor"], d["weights"], d["parents"], faces=f.astype(np.int64))
    assert mf.faces.dtype == np.int32 and np.array_equal(mf.faces, f) and np.array_equal(mf.numpy_dict()["faces"], f)
    for bad in (f + 1, f[:, :2], f.astype(np.float32), -f):
        with pytest.raises(ValueError, match="faces"):
            smpl.SMPLModel(d["v_template"], d["shapedirs"], d["posedirs"], d["J_regressor"], d["weights"], faces=bad)
    for key in (None, "faces", "f"):
        path = str(tmp_path / ("m_%s.npz" % key))
        np.savez(path, **dict(d, **({key: f} if key else {})))
        back = smpl.SMPLModel.from_npz(path)
        assert (back.faces is None) if key is None else np.array_equal(back.faces, f)
        assert np.array_equal(back.v_template, m.v_template)


def test_renderer_refusals():
    v, f = render.capsule_mesh(5, 8)
    verts = torch.from_numpy(np.stack([v, v]))
    cam, ind = (torch.from_numpy(t) for t in RR.camera(2, 16, 16, 1, 0))
    r = render.MeshRenderer(f, up=2)
    assert r.F == 80 and r.faces.dtype == np.int32
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        r(verts, cam, ind, 1)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        render.rasterize(verts, torch.from_numpy(f), cam, ind, 1)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        render.shade(torch.zeros(2, 32, 32, dtype=torch.int64), verts, torch.from_numpy(f))
    # a bad face index: at construction (negative, beyond any supported V) and at the call (beyond this body's V)
    for bad in (-f - 1, f + render.MAX_V, f.astype(np.float32), f[:, :2]):
        with pytest.raises(ValueError, match="faces|face indices"):
            render.MeshRenderer(bad)
    with pytest.raises(RuntimeError, match="index vertex 41, verts hold 30"):
        r(verts[:, :30].contiguous(), cam, ind, 1)
    # V beyond the limit
    wide = torch.zeros(2, render.MAX_V + 1, 3)
    with pytest.raises(RuntimeError, match="at most %d in LDS" % render.MAX_V):
        r(wide, cam, ind, 1)
    with pytest.raises(RuntimeError, match="at most %d in LDS" % render.MAX_V):
        render.rasterize(wide, torch.from_numpy(f), cam, ind, 1)
    # n F too large
    n = 2 ** 15
    many = torch.zeros(n, 3, 3)
    big = render.MeshRenderer(np.zeros((2 ** 16, 3), np.int32), up=1)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        big(many, cam[:1], torch.zeros(1, n, dtype=torch.int64), n)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        render.rasterize(many, torch.zeros(2 ** 16, 3, dtype=torch.int32), cam[:1], torch.zeros(1, n, dtype=torch.int64), n)
    # shapes that do not fit together
    with pytest.raises(RuntimeError, match="person slots"):
        render.rasterize(verts, torch.from_numpy(f), cam, ind, 2)
    with pytest.raises(RuntimeError, match="int32"):
        render.rasterize(verts, torch.from_numpy(f).long(), cam, ind, 1)
    with pytest.raises(RuntimeError, match="up = 0"):
        render.rasterize(verts, torch.from_numpy(f), cam, ind, 1, up=0)
    for kw in ({"up": 0}, {"alpha": 1.5}, {"ambient": -1.0}, {"focal": 0.0}, {"colours": np.zeros((3, 4), np.uint8)}):
        with pytest.raises(ValueError):
            render.MeshRenderer(f, **kw)
    assert math.isclose(render.MeshRenderer(f, alpha=0.25).alpha, 0.25)
