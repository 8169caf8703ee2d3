"""GPU: csrc/render.hip against the fp32 mirror of tests/render_ref.py.  The rule of every comparison: face_id, depth, the keys and rgb
are BIT-EQUAL to the mirror; nothing is excluded.  Everything fits a 16 x 16 map (targets of at most 64 x 64 pixels)."""
import ctypes

import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
from h3d_amd import _lib, arch, detector, render, smpl, synth

import render_ref as RR
import smpl_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHADE = dict(alpha=0.7, ambient=0.3)


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(DEV)


def _image(case, seed=0):
    B, _, H, W = case["cam_map"].shape
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 256, (B, case["up"] * H, case["up"] * W, 3)).astype(np.uint8),
            rs.randint(0, 256, (B * case["n"], 3)).astype(np.uint8))


def gpu_render(case, shade=True):
    """The case through render.rasterize (+ render.shade over a seeded image with seeded colours) -> numpy dict."""
    verts, faces = _dev(case["verts"]), _dev(case["faces"], np.int32)
    fid, dep, keys = render.rasterize(verts, faces, _dev(case["cam_map"]), _dev(case["ind"]), case["n"], case["up"], valid=_dev(case["valid"]),
                                      dz=_dev(case["dz"]), flags=case["flags"])
    out = {"face_id": fid.cpu().numpy(), "depth": dep.cpu().numpy(), "keys": keys.cpu().numpy().view(np.uint64)}
    if shade:
        image, colour = _image(case)
        out["rgb"] = render.shade(keys, verts, faces, image=_dev(image), colour=_dev(colour), **SHADE).cpu().numpy()
    return out


def mirror(case, shade=True):
    out = RR.render_case(case)
    if shade:
        image, colour = _image(case)
        out["rgb"] = RR.shade(out["face_id"], case["verts"], case["faces"], case["n"], image=image, colour=colour, **SHADE)
    return out


def same_bits(a, b, what=""):
    for k in b:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].dtype, b[k].dtype)
        x, y = (t.view(np.uint32) if t.dtype == np.float32 else t for t in (a[k], b[k]))
        assert np.array_equal(x, y), (what, k, int((x != y).sum()))


def check(case, what="", min_covered=1):
    got, want = gpu_render(case), mirror(case)
    same_bits(got, want, what)
    assert (want["face_id"] >= 0).sum() >= min_covered, what
    assert np.isposinf(got["depth"][got["face_id"] < 0]).all()
    return got


# ---- bodies ----------------------------------------------------------------------------------------------------------------------------
def body_verts(P, seed=0, V=100):
    model = smpl_ref.jointed_model(V, seed)
    betas, thetas = smpl_ref.make_case(P, seed)
    return smpl_ref.lbs(betas, thetas, model, dtype=np.float32)[0], model["v_template"]


def neighbour_faces(template, F, seed):
    """F seeded triangles over nearest neighbours of the template: small faces."""
    rs = np.random.RandomState(seed)
    near = np.argsort(np.linalg.norm(template[:, None] - template[None], axis=-1), axis=1)[:, 1:5]
    a = rs.randint(0, len(template), F)
    pick = np.stack([rs.permutation(4)[:2] for _ in range(F)])
    return np.stack([a, near[a, pick[:, 0]], near[a, pick[:, 1]]], 1).astype(np.int32)


def body_case(F, up, seed=0, n=3, s_range=(4.0, 7.0)):
    """B = 2 images of n posed 100-vertex bodies on neighbouring centres (they overlap), each with its own depth offset."""
    verts, template = body_verts(2 * n, seed)
    cam, ind = RR.camera(2, 16, 16, n, seed, s_range)
    rs = np.random.RandomState(seed)
    for b in range(2):
        for m in range(n):
            cx, cy = 7 + (m + b) % 2, 7 + m // 2
            cam[b, :, cy, cx] = cam[b, :, ind[b, m] // 16, ind[b, m] % 16]
            ind[b, m] = cy * 16 + cx
    return dict(verts=verts, faces=neighbour_faces(template, F, seed), cam_map=cam, ind=ind, n=n, up=up, valid=None,
                dz=rs.uniform(-0.3, 0.3, 2 * n).astype(np.float32), flags=0)


# ---- 1. the small-face path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,up", [(1500, 1), (1500, 2), (1500, 4), (3 * 1024 + 77, 2), (37, 4)])
def test_small_faces_of_overlapping_posed_bodies(F, up):
    case = body_case(F, up, seed=F % 7)
    got = check(case, min_covered=30)
    people = np.unique(got["face_id"][got["face_id"] >= 0] // F)
    assert len(people) >= (2 if F > 1000 else 1)                            # the slots overlap, none hides all the others


# ---- 2. the wave path and the queue ----------------------------------------------------------------------------------------------------
def one_slot_case(verts0, verts1, faces, up=4, s=1.0, flags=0, dz=None):
    """B = 2, n = 1: mesh verts0 in image 0, verts1 in image 1, in map pixels about the map's corner pixel (s = 1, t = 0)."""
    cam = np.random.RandomState(5).randn(2, 3, 16, 16).astype(np.float32)
    cam[:, :, 0, 0] = (s, 0.0, 0.0)
    return dict(verts=np.stack([verts0, verts1]).astype(np.float32), faces=np.asarray(faces, np.int32), cam_map=cam,
                ind=np.zeros((2, 2), np.int64), n=1, up=up, valid=None, dz=dz, flags=flags)


def test_a_triangle_over_the_whole_target_and_far_outside_it():
    # 64 x 64 pixels, all of them inside; the vertices up to 5000 map pixels = 320 000 lattice steps out: the edge functions need 64 bits
    big = [[-5000.0, -3000.0, 1.0], [6000.0, -2500.0, -2.0], [100.0, 7000.0, 3.0]]
    part = [[-40.0, 5.0, 0.0], [11.3, -900.0, 1.0], [9.7, 300.0, 5.0]]                  # image 1: a sliver through the target
    got = check(one_slot_case(big, part, [[0, 1, 2]]))
    assert (got["face_id"][0] == 0).all() and 0 < (got["face_id"][1] == 0).sum() < 64 * 64


def _large_faces(count, seed):
    """`count` seeded triangles of 2 to 5 map pixels extent (8 .. 20 target pixels at up = 4: every one beyond the lane cut-off of 16 pixels)."""
    rs = np.random.RandomState(seed)
    c = rs.uniform(1.0, 15.0, (count, 1, 2))
    tri = c + rs.uniform(-2.5, 2.5, (count, 3, 2))
    tri[:, 0] = c[:, 0] + [-1.5, -1.5]
    tri[:, 1] = c[:, 0] + [1.5, -1.0]
    tri[:, 2] = c[:, 0] + [0.0, 1.5] + rs.uniform(-0.5, 0.5, (count, 2))
    z = rs.uniform(-1.0, 1.0, (count, 3, 1))
    return np.concatenate([tri, z], -1).reshape(-1, 3), np.arange(3 * count).reshape(-1, 3)


def test_more_large_faces_than_the_queue_holds():
    # 1700 > 1536 queue entries: the queue is drained and refilled (after the first round of 1024 faces), nothing is dropped
    v0, f = _large_faces(1700, 1)
    v1, _ = _large_faces(1700, 2)
    got = check(one_slot_case(v0, v1, f))
    assert len(np.unique(got["face_id"])) > 300


def test_large_and_small_faces_mixed_in_one_slot():
    verts, template = body_verts(2, seed=3)
    faces = np.concatenate([neighbour_faces(template, 900, 3), np.random.RandomState(3).randint(0, 100, (300, 3)).astype(np.int32)])
    faces = faces[np.random.RandomState(4).permutation(len(faces))]
    cam = np.random.RandomState(6).randn(2, 3, 16, 16).astype(np.float32)
    cam[:, :, 8, 8] = (6.0, 0.25, -0.5)
    case = dict(verts=verts, faces=faces, cam_map=cam, ind=np.full((2, 1), 8 * 16 + 8, np.int64), n=1, up=4, valid=None, dz=None, flags=0)
    check(case, min_covered=500)


# ---- 3. the fill rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1)])
def test_fill_rule_squares(shift):
    got = check(RR.square_case(shift), min_covered=16)
    assert (got["face_id"] >= 0).sum() == 16


@pytest.mark.parametrize("up,covered", [(1, 24), (2, 98), (4, 396)])
def test_fill_rule_triangle_on_pixel_centres(up, covered):
    # Pick's theorem (tests/test_oracle_render.py); up = 4: area 400, 16 boundary points -> 393 interior, plus the 3 points inside the left edge
    got = check(RR.triangle_case(up))
    assert (got["face_id"] >= 0).sum() == covered


# ---- 4. the depth test -----------------------------------------------------------------------------------------------------------------
def test_intersecting_and_coincident_triangles():
    # image 0: two triangles that cross, the visible one changes along a line; image 1: the same triangle twice (under two vertex sets) at
    # equal depth: the smaller id wins everywhere
    a = [[1.0, 1.0, -1.0], [14.0, 2.0, 1.0], [6.0, 14.0, 0.0], [2.0, 12.0, 1.0], [13.0, 13.0, -1.0], [8.0, 1.5, 0.2]]
    b = [[1.0, 1.0, 0.5], [14.0, 2.0, 0.7], [6.0, 14.0, -0.2], [1.0, 1.0, 0.5], [14.0, 2.0, 0.7], [6.0, 14.0, -0.2]]
    got = check(one_slot_case(a, b, [[3, 4, 5], [0, 1, 2]]), min_covered=100)
    ids0 = got["face_id"][0]
    assert (ids0 == 0).sum() > 100 and (ids0 == 1).sum() > 100
    ids1 = got["face_id"][1]
    assert set(np.unique(ids1).tolist()) == {-1, 0}


def test_negate_z_cull_back_and_reversed_faces():
    case = RR.capsule_case(11, n=2, up=4, rings=6, segments=9)
    base = check(case, min_covered=200)
    flipped = dict(case, verts=case["verts"] * np.array([1, 1, -1], np.float32), flags=RR.NEGATE_Z)
    same_bits(check(flipped), base, "negate_z")
    same_bits(check(dict(case, flags=RR.CULL_BACK)), base, "cull_back")
    far = check(dict(case, faces=case["faces"][:, ::-1].copy(), flags=RR.CULL_BACK))
    cov = base["face_id"] >= 0
    assert np.array_equal(far["face_id"] >= 0, cov) and (far["depth"][cov] >= base["depth"][cov]).all()
    assert not (far["face_id"][cov] == base["face_id"][cov]).any()
    # culling under NEGATE_Z follows the viewer: the mirrored body is inside out, its reversed faces are outward again and the same ones
    # are seen (the depth is anchored at another vertex of the reversed face: equal up to rounding, not in bits)
    both = check(dict(flipped, faces=case["faces"][:, ::-1].copy(), flags=RR.NEGATE_Z | RR.CULL_BACK))
    assert np.array_equal(both["face_id"], base["face_id"]) and np.abs(both["depth"][cov] - base["depth"][cov]).max() < 1e-5


# ---- 5. the skips ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ind_high", "ind_negative", "valid", "s_zero", "s_negative", "s_nan", "s_inf"])
def test_a_skipped_slot_equals_the_case_without_it(kind):
    case = body_case(600, 2, seed=2)
    n = case["n"]
    twin = dict(case, n=n - 1, verts=case["verts"].reshape(2, n, -1, 3)[:, :n - 1].reshape(-1, 100, 3), dz=case["dz"].reshape(2, n)[:, :n - 1].copy())
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    at = int(c["ind"][0, n - 1])
    valid = np.ones((2, n), np.uint8)
    if kind == "valid":
        valid[0, n - 1] = 0
        c["ind"][1, n - 1] = -7                       # (image 1 loses its last slot another way)
    else:
        valid[1, n - 1] = 0
        if kind.startswith("ind"):
            c["ind"][0, n - 1] = 16 * 16 if kind == "ind_high" else -1
        else:
            c["cam_map"][0, 0, at // 16, at % 16] = {"s_zero": 0.0, "s_negative": -3.0, "s_nan": np.nan, "s_inf": np.inf}[kind]
            # (another slot of image 0 may sit on the same pixel only if the centres coincide: body_case keeps them apart)
    c["valid"] = valid
    got, want = gpu_render(c, shade=False), gpu_render(twin, shade=False)
    same_bits(got, want, kind)
    same_bits(got, mirror(c, shade=False), kind)
    assert not np.array_equal(got["face_id"], gpu_render(case, shade=False)["face_id"])


def _with_extra_faces(extra_verts, extra_faces):
    """A body (B = 2, n = 1) and the same with vertices and faces appended in image 0 and 1 alike: -> (twin, case)."""
    verts, template = body_verts(2, seed=5)
    faces = neighbour_faces(template, 300, 5)
    cam = np.random.RandomState(7).randn(2, 3, 16, 16).astype(np.float32)
    cam[:, :, 8, 7] = (5.0, 0.0, 0.5)
    twin = dict(verts=verts, faces=faces, cam_map=cam, ind=np.full((2, 1), 8 * 16 + 7, np.int64), n=1, up=2, valid=None, dz=None, flags=0)
    ev = np.broadcast_to(np.asarray(extra_verts, np.float32), (2,) + np.shape(extra_verts))
    case = dict(twin, verts=np.concatenate([verts, ev], 1), faces=np.concatenate([faces, np.asarray(extra_faces, np.int32)]))
    return twin, case


@pytest.mark.parametrize("kind", ["nan", "inf", "guard_band", "huge", "index", "degenerate"])
def test_a_skipped_face_equals_the_case_without_it(kind):
    if kind == "index":
        # through render.rasterize, which hands the device tensor to the entry point unchecked
        twin, case = _with_extra_faces(np.zeros((0, 3)), [[0, 1, 100], [-1, 2, 3], [4, 2 ** 31 - 1, 5], [6, 7, -2 ** 31]])
    elif kind == "degenerate":
        twin, case = _with_extra_faces([[0.5, 0.5, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, -1.0]], [[3, 3, 9], [100, 101, 102], [100, 100, 100], [7, 100, 7]])
    else:
        bad = {"nan": [np.nan, 0.0, 0.0], "inf": [0.0, 0.0, np.inf], "guard_band": [0.0, 2.0 ** 19 / 160 + 1.0, -5.0], "huge": [1e30, -1e30, 0.0]}[kind]
        twin, case = _with_extra_faces([bad], [[100, 1, 2], [3, 100, 4], [5, 6, 100]])
    got = gpu_render(case)
    same_bits(got, gpu_render(twin), kind)
    same_bits(got, mirror(case), kind)
    assert (got["face_id"] >= 0).sum() > 50
    if kind == "guard_band":
        # one lattice step inside the band the vertex is used: 16 * 2 * (5 y + 8.5) = 2^19 exactly
        twin, case = _with_extra_faces([[0.0, (2.0 ** 19 / 32 - 8.5) / 5, -5.0]], [[100, 1, 2], [3, 100, 4], [5, 6, 100]])
        inside = check(case)
        assert not np.array_equal(inside["face_id"], got["face_id"])


def test_a_slot_of_image_1_over_image_0s_people_leaves_image_0_alone():
    case = body_case(600, 2, seed=4)
    alone = dict(case, valid=np.array([[1, 1, 1], [0, 0, 0]], np.uint8))
    got, want = check(case), check(alone)
    for k in ("face_id", "depth", "rgb"):
        assert np.array_equal(got[k][0], want[k][0])
    assert (want["face_id"][1] == -1).all() and (got["face_id"][1] >= 0).any()
    assert int(case["ind"][1, 0]) == int(case["ind"][0, 1])                  # image 1's first body stands on the centre of one of image 0's


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------------------
def _raw(case, arena, offs, stream=None, colour=None, image=None):
    """Both entry points through the raw ABI with the outputs at given byte offsets of `arena`."""
    L = _lib.lib()
    B, _, H, W = case["cam_map"].shape
    n, up = case["n"], case["up"]
    V, F = case["verts"].shape[-2], case["faces"].shape[0]
    ins = [_dev(case["verts"]), _dev(case["faces"], np.int32), _dev(case["cam_map"]), _dev(case["ind"]), _dev(case["valid"]), _dev(case["dz"])]
    base = arena.data_ptr()
    st = _lib.stream_ptr() if stream is None else ctypes.c_void_p(stream.cuda_stream)
    _lib.check(L.h3d_render_rasterize(*[_lib.ptr(t) for t in ins], B, case["ind"].shape[1], n, V, F, H, W, up, case["flags"], base + offs["face_id"],
                                      base + offs["depth"], base + offs["ws"], offs["ws_bytes"], st), "h3d_render_rasterize")
    _lib.check(L.h3d_render_shade(base + offs["ws"], _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(colour), _lib.ptr(image), B, n, V, F, up * H, up * W,
                                  SHADE["alpha"], SHADE["ambient"], render.DEFAULT_COLOUR, 0, base + offs["rgb"], st), "h3d_render_shade")
    return ins


def test_sentinels_misaligned_outputs_garbage_and_streams():
    case = body_case(600, 2, seed=6)
    want = mirror(case)
    B, Hr, Wr = want["face_id"].shape
    npix = B * Hr * Wr
    ws_bytes = ctypes.c_size_t(0)
    _lib.check(_lib.lib().h3d_render_workspace_bytes(B, Hr, Wr, ctypes.byref(ws_bytes)), "workspace_bytes")
    assert ws_bytes.value == (npix * 8 + 255) // 256 * 256
    # every output 4 bytes past a 16-byte boundary (the workspace 8: it holds 64-bit keys), 256 guard bytes between them
    offs, at = {}, 256
    for name, size, shift in (("face_id", 4 * npix, 4), ("depth", 4 * npix, 4), ("rgb", 3 * npix, 4), ("ws", ws_bytes.value, 8)):
        offs[name] = at + shift
        at = (at + shift + size + 256 + 15) // 16 * 16
    offs["ws_bytes"] = ws_bytes.value
    image, colour = _image(case)
    d_image, d_colour = _dev(image), _dev(colour)
    used = np.zeros(at, bool)
    for name, size in (("face_id", 4 * npix), ("depth", 4 * npix), ("rgb", 3 * npix), ("ws", npix * 8)):
        used[offs[name]:offs[name] + size] = True

    def run(stream=None, fill=0xA5):
        arena = torch.full((at,), fill, dtype=torch.uint8, device=DEV)           # garbage in every output: each byte is rewritten
        assert (arena.data_ptr() + offs["face_id"]) % 16 == 4 and (arena.data_ptr() + offs["ws"]) % 16 == 8
        if stream is None:
            keep = _raw(case, arena, offs, colour=d_colour, image=d_image)
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                keep = _raw(case, arena, offs, stream, colour=d_colour, image=d_image)
            torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        del keep
        host = arena.cpu().numpy()
        assert (host[~used] == fill).all()                                    # the sentinels around every output and the workspace
        return {"face_id": host[offs["face_id"]:][:4 * npix].view(np.int32).reshape(B, Hr, Wr),
                "depth": host[offs["depth"]:][:4 * npix].view(np.float32).reshape(B, Hr, Wr),
                "keys": host[offs["ws"]:][:8 * npix].view(np.uint64).reshape(B, Hr, Wr),
                "rgb": host[offs["rgb"]:][:3 * npix].reshape(B, Hr, Wr, 3)}

    first = run()
    same_bits(first, want, "first")
    same_bits(run(fill=0x00), want, "second call, other garbage")
    same_bits(run(torch.cuda.Stream()), want, "second stream")


def test_shade_twice_on_one_key_buffer_leaves_the_keys():
    case = RR.capsule_case(13, n=3, up=4)
    verts, faces = _dev(case["verts"]), _dev(case["faces"], np.int32)
    fid, dep, keys = render.rasterize(verts, faces, _dev(case["cam_map"]), _dev(case["ind"]), case["n"], case["up"], dz=_dev(case["dz"]))
    before = keys.clone()
    want = RR.render_case(case)
    image, colour = _image(case, 1)
    a = render.shade(keys, verts, faces, image=_dev(image), colour=_dev(colour), alpha=0.5, ambient=0.2)
    b = render.shade(keys, verts, faces, image=None, colour=None, alpha=1.0, ambient=0.0, background=(16, 32, 48), default_colour=0x80FF40)
    assert torch.equal(keys, before) and np.array_equal(keys.cpu().numpy().view(np.uint64), want["keys"])
    assert np.array_equal(a.cpu().numpy(), RR.shade(want["face_id"], case["verts"], case["faces"], 3, image=image, colour=colour, alpha=0.5, ambient=0.2))
    assert np.array_equal(b.cpu().numpy(), RR.shade(want["face_id"], case["verts"], case["faces"], 3, alpha=1.0, ambient=0.0, background=0x102030,
                                                     default_colour=0x80FF40))
    assert not torch.equal(a, b)
    # a key buffer of another mesh cannot make the kernel read out of bounds: ids beyond n F and faces beyond V shade as background
    small = render.shade(keys, verts[:2 * 3, :20].contiguous(), faces[:50].contiguous(), background=0x010203)
    ids = want["face_id"]
    ok = (ids >= 0) & (ids // 50 < 3) & (case["faces"][np.where(ids >= 0, ids % 50, 0)].max(-1) < 20)
    assert np.array_equal(small.cpu().numpy()[~ok], np.broadcast_to(np.array([1, 2, 3], np.uint8), small.shape)[~ok])


# ---- 7. through the detector -------------------------------------------------------------------------------------------------------------
def test_render_detections_equals_the_mirror_on_the_detectors_outputs():
    opt = detector.Opt(input_h=64, input_w=64, smpl=True, smpl_cam=True, smpl_people=3, dtype="f32", K=10)
    sd = synth.synth_state_dict(arch.state_dict_shapes(opt.heads, True), seed=0)
    sd["cam.2.bias"] = np.asarray(sd["cam.2.bias"]).copy()
    sd["cam.2.bias"][0] = 5.0                                   # s = the first channel: positive at every pixel
    v, f = render.capsule_mesh(7, 14)                           # 100 vertices: the capsule's faces on a synthetic 100-vertex body
    d = smpl_ref.jointed_model(100, 1)
    body = smpl.SMPLModel(d["v_template"], d["shapedirs"], d["posedirs"], d["J_regressor"], d["weights"], d["parents"], faces=f)
    det = detector.MultiPoseDetector(opt, {k: torch.from_numpy(np.asarray(t)) for k, t in sd.items()}, smpl_model=body, device=DEV)
    x = torch.from_numpy(synth.synth_images(2, 64, 64)).to(DEV)
    res = det.run(x)
    assert tuple(res["verts"].shape) == (2, 3, 100, 3) and tuple(res["heads"]["cam"].shape) == (2, 3, 16, 16)
    scores = res["dets"][:, :3, 4]
    thresh = float(scores.flatten().sort().values[2])           # half of the six slots are above it
    frames = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (2, 64, 64, 3)).astype(np.uint8)).to(DEV)
    r = render.MeshRenderer(body.faces, up=4)
    out = render.render_detections(r, res, frames, vis_thresh=thresh)
    cam = res["heads"]["cam"].cpu().numpy()
    ind = res["inds"].cpu().numpy()
    valid = (scores > thresh).cpu().numpy().astype(np.uint8)
    s = np.stack([cam[b, 0].reshape(-1)[ind[b, :3]] for b in range(2)])
    assert 0 < valid.sum() < 6 and (s > 0).all()
    dz = np.float32(64.0) / s                                   # focal = the target's width
    verts = res["verts"].cpu().numpy()
    want = RR.render(verts, f, cam, ind, 3, up=4, valid=valid, dz=dz)
    want["rgb"] = RR.shade(want["face_id"], verts, f, 3, image=frames.cpu().numpy(), colour=np.tile(render.PALETTE[:3], (2, 1)), alpha=r.alpha,
                           ambient=r.ambient)
    got = {k: out[k].cpu().numpy() for k in ("face_id", "depth", "rgb")}
    same_bits(got, {k: want[k] for k in got}, "detector")
    assert (got["face_id"] >= 0).any()
    person = out["person"].cpu().numpy()
    assert np.array_equal(person, np.where(got["face_id"] >= 0, got["face_id"] // r.F, -1))
    assert set(np.unique(person).tolist()) <= {-1} | {m for b in range(2) for m in range(3) if valid[b, m]}
    # without the cam head the hook says what is missing
    with pytest.raises(KeyError, match="smpl_cam"):
        render.render_detections(r, dict(res, heads={k: t for k, t in res["heads"].items() if k != "cam"}))


# ---- 8. the refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    case = RR.capsule_case(0, n=1, up=1)
    verts, faces, cam, ind = _dev(case["verts"]), _dev(case["faces"], np.int32), _dev(case["cam_map"]), _dev(case["ind"])
    with pytest.raises(RuntimeError, match="argument error.*flags"):
        render.rasterize(verts, faces, cam, ind, 1, flags=4)
    with pytest.raises(RuntimeError, match="at most %d in LDS" % render.MAX_V):
        render.rasterize(torch.zeros(2, render.MAX_V + 1, 3, device=DEV), faces, cam, ind, 1)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        render.rasterize(torch.zeros(2 ** 15, 3, 3, device=DEV), torch.zeros(2 ** 16, 3, dtype=torch.int32, device=DEV), cam[:1],
                         torch.zeros(1, 2 ** 15, dtype=torch.int64, device=DEV), 2 ** 15)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        render.rasterize(verts.double(), faces, cam, ind, 1)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        render.rasterize(verts.cpu(), faces, cam, ind, 1)
    fid, dep, keys = render.rasterize(verts, faces, cam, ind, 1)
    with pytest.raises(ValueError, match="alpha"):
        render.shade(keys, verts, faces, alpha=1.5)
    with pytest.raises(RuntimeError, match="image"):
        render.shade(keys, verts, faces, image=torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="int64"):
        render.shade(keys.int(), verts, faces)
    # the largest supported V runs (the whole 160 KiB of LDS): a single triangle over three of its vertices
    V = render.MAX_V
    big = torch.zeros(2, V, 3, device=DEV)
    big[:, V - 2] = torch.tensor([8.0, 0.0, 0.0])
    big[:, V - 1] = torch.tensor([0.0, 8.0, 1.0])
    tri = torch.tensor([[0, V - 2, V - 1]], dtype=torch.int32, device=DEV)
    case = dict(verts=big.cpu().numpy(), faces=tri.cpu().numpy(), cam_map=case["cam_map"], ind=case["ind"], n=1, up=1, valid=None, dz=None, flags=0)
    check(case, min_covered=1)
