"""Rendering the SMPL meshes into the image: a z-buffered visibility-buffer rasteriser under the weak-perspective camera the `cam` head
is trained for (csrc/render.hip, include/h3d.h section 4d).  There is no rendering code in the reference, so the
definition is the project's own; tests/render_ref.py restates it in numpy and the kernels are bit-equal to that.

    rasterize(verts, faces, cam_map, ind, n, up, valid, dz, flags) -> (face_id, depth, keys)     one memset + two launches
    shade(keys, verts, faces, image, colour, alpha, ambient, background) -> rgb                    one launch on an existing key buffer
    MeshRenderer(faces, up, focal, alpha, ambient, colours)          callable: face_id, depth, person and the shaded overlay
    render_detections(renderer, res, images_uint8, vis_thresh)       the same from MultiPoseDetector.run's result (Opt(smpl_cam=True))
    capsule_mesh(rings, segments, radius, half_height)               a closed test body; (82, 84) has SMPL's vertex and face counts

A vertex (X, Y, Z) of person slot p = b n + m lands at up * (s (X, Y) + (tx, ty) + (cx, cy)) with (s, tx, ty) = cam_map[b, :, ind[b,m]]
and (cx, cy) the integer map pixel of ind: exactly where smpl_loss's `pred` puts a regressed keypoint, scaled to the target.  Nothing is
synchronised with the host."""
import numpy as np
import torch

from . import _lib

NEGATE_Z, CULL_BACK = _lib.RENDER_NEGATE_Z, _lib.RENDER_CULL_BACK
MAX_V, MAX_SIDE = _lib.RENDER_MAX_V, _lib.RENDER_MAX_SIDE
DEFAULT_COLOUR = 0xE6B48C           # 0xRRGGBB
# per person slot of an image, cycled
PALETTE = np.array([[230, 180, 140], [120, 170, 230], [150, 220, 130], [235, 130, 130], [200, 150, 230], [240, 210, 110], [120, 215, 210],
                    [190, 190, 190]], np.uint8)


def capsule_mesh(rings, segments, radius=0.15, half_height=0.3):
    """A capsule about the y axis: a pole, `rings` rings of `segments` vertices (the upper half on the sphere about (0, +half_height, 0),
    the lower half on the one about (0, -half_height, 0)), a pole -> (verts [V,3] float32, faces [F,3] int32) with V = rings segments + 2
    and F = 2 rings segments: a closed genus-0 surface, every face counter-clockwise seen from outside (right-handed frame)."""
    if rings < 2 or segments < 3:
        raise ValueError("capsule_mesh: rings >= 2 and segments >= 3, got %d, %d" % (rings, segments))
    theta = (np.arange(rings) + 1.0) * np.pi / (rings + 1.0)
    phi = np.arange(segments) * 2.0 * np.pi / segments
    upper = np.arange(rings) < (rings + 1) // 2
    y = radius * np.cos(theta) + np.where(upper, half_height, -half_height)
    rad = radius * np.sin(theta)
    ring = np.stack([rad[:, None] * np.cos(phi)[None], np.broadcast_to(y[:, None], (rings, segments)), rad[:, None] * np.sin(phi)[None]], -1)
    verts = np.concatenate([[[0.0, half_height + radius, 0.0]], ring.reshape(-1, 3), [[0.0, -half_height - radius, 0.0]]]).astype(np.float32)
    j = np.arange(segments)
    jn = (j + 1) % segments
    faces = [np.stack([np.zeros(segments, np.int64), 1 + jn, 1 + j], -1)]
    for k in range(rings - 1):
        a, b = 1 + k * segments, 1 + (k + 1) * segments
        faces.append(np.stack([a + j, a + jn, b + j], -1))
        faces.append(np.stack([a + jn, b + jn, b + j], -1))
    last, pole = 1 + (rings - 1) * segments, rings * segments + 1
    faces.append(np.stack([last + j, last + jn, np.full(segments, pole)], -1))
    return verts, np.concatenate(faces).astype(np.int32)


def _f32(t, name, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError("%s: %s must be a contiguous float32 tensor" % (what, name))
    return t


def _mesh_operands(what, verts, faces, B, n):
    """verts [P,V,3] or [B,n,V,3], faces [F,3] int32 -> (verts [P,V,3], n, V, F), checked against the kernels' limits."""
    if verts.dim() == 4:
        if n is not None and verts.shape[1] != n:
            raise RuntimeError("%s: verts %s hold %d slots per image, n = %d" % (what, tuple(verts.shape), verts.shape[1], n))
        n = verts.shape[1]
        verts = verts.reshape(-1, verts.shape[2], 3) if verts.shape[3] == 3 else verts
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise RuntimeError("%s: verts must be [P,V,3] or [B,n,V,3], got %s" % (what, tuple(verts.shape)))
    if n is None:
        n = verts.shape[0] // B if B else 0
    if n < 1 or verts.shape[0] != B * n:
        raise RuntimeError("%s: verts hold %d person slots, B * n = %d * %d expected" % (what, verts.shape[0], B, n))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.dtype != torch.int32 or not faces.is_contiguous():
        raise RuntimeError("%s: faces must be a contiguous int32 tensor [F,3], got %s %s" % (what, faces.dtype, tuple(faces.shape)))
    V, F = verts.shape[1], faces.shape[0]
    if V < 1:
        raise RuntimeError("%s: verts hold no vertices" % what)
    if V > MAX_V:
        raise RuntimeError("%s: V = %d vertices, the raster kernel stages at most %d in LDS" % (what, V, MAX_V))
    if n * F >= 2 ** 31:
        raise RuntimeError("%s: n F = %d * %d face ids, they must stay below 2^31" % (what, n, F))
    return verts, n, V, F


def rasterize(verts, faces, cam_map, ind, n=None, up=1, valid=None, dz=None, flags=0):
    """verts [P,V,3] or [B,n,V,3] f32, faces [F,3] i32, cam_map [B,3,H,W] f32, ind [B,max_objs] (the first n slots of every image are
    used), valid [P] or [B,n] (bool / uint8; None = all), dz [P] or [B,n] f32 (None = 0), flags NEGATE_Z | CULL_BACK ->
    face_id [B,up H,up W] i32 (m F + f, -1 = background), depth f32 (+inf = background), keys i64 (the visibility buffer, for `shade`)."""
    what = "rasterize"
    if cam_map.dim() != 4 or cam_map.shape[1] != 3:
        raise RuntimeError("%s: cam_map must be [B,3,H,W], got %s" % (what, tuple(cam_map.shape)))
    B, H, W = cam_map.shape[0], cam_map.shape[2], cam_map.shape[3]
    if ind.dim() != 2 or ind.shape[0] != B:
        raise RuntimeError("%s: ind must be [B,max_objs], got %s" % (what, tuple(ind.shape)))
    verts, n, V, F = _mesh_operands(what, verts, faces, B, n)
    M = ind.shape[1]
    if n > M:
        raise RuntimeError("%s: n = %d person slots per image, ind holds %d" % (what, n, M))
    up = int(up)
    if up < 1 or up * H > MAX_SIDE or up * W > MAX_SIDE:
        raise RuntimeError("%s: up = %d on a %d x %d map, the target is at most %d a side" % (what, up, H, W, MAX_SIDE))
    _lib.require_cuda(verts, faces, cam_map, ind, valid, dz)
    dev = cam_map.device
    _f32(verts, "verts", what)
    _f32(cam_map, "cam_map", what)
    ind = ind.detach().to(device=dev, dtype=torch.int64).contiguous()
    if valid is not None:
        valid = valid.detach().reshape(-1)
        valid = (valid.contiguous().view(torch.uint8) if valid.dtype == torch.bool else valid.to(torch.uint8)).to(dev).contiguous()
        if valid.numel() != B * n:
            raise RuntimeError("%s: valid holds %d entries, B * n = %d expected" % (what, valid.numel(), B * n))
    if dz is not None:
        dz = dz.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        if dz.numel() != B * n:
            raise RuntimeError("%s: dz holds %d entries, B * n = %d expected" % (what, dz.numel(), B * n))
    if verts.device != dev or faces.device != dev:
        raise RuntimeError("%s: verts, faces and cam_map must be on one device" % what)
    Hr, Wr = up * H, up * W
    face_id = torch.empty(B, Hr, Wr, dtype=torch.int32, device=dev)
    depth = torch.empty(B, Hr, Wr, dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.h3d_render_workspace_bytes, B, Hr, Wr, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.h3d_render_rasterize(_lib.ptr(verts.detach()), _lib.ptr(faces), _lib.ptr(cam_map.detach()), _lib.ptr(ind), _lib.ptr(valid),
                                          _lib.ptr(dz), B, M, n, V, F, H, W, up, int(flags), _lib.ptr(face_id), _lib.ptr(depth), _lib.ptr(ws),
                                          ws.numel(), _lib.stream_ptr()), "h3d_render_rasterize")
    keys = ws[:B * Hr * Wr * 8].view(torch.int64).view(B, Hr, Wr)
    return face_id, depth, keys


def _packed(colour, name):
    """(r, g, b) or 0xRRGGBB -> 0xRRGGBB."""
    if isinstance(colour, (tuple, list, np.ndarray)):
        r, g, b = (int(c) for c in colour)
        if not all(0 <= c <= 255 for c in (r, g, b)):
            raise ValueError("%s: components must lie in 0 .. 255, got %s" % (name, (r, g, b)))
        return r << 16 | g << 8 | b
    colour = int(colour)
    if not 0 <= colour <= 0xFFFFFF:
        raise ValueError("%s: 0xRRGGBB expected, got %#x" % (name, colour))
    return colour


def shade(keys, verts, faces, image=None, colour=None, alpha=0.7, ambient=0.3, background=0, default_colour=DEFAULT_COLOUR):
    """keys [B,Hr,Wr] i64 (rasterize's), the verts / faces they were rasterised from, image [B,Hr,Wr,3] u8 (None = the colour
    `background`), colour [P,3] or [B,n,3] u8 (None = default_colour) -> rgb [B,Hr,Wr,3] u8: headlight Lambert shading of every pixel's
    winning face, blended over the image with weight alpha.  The keys are only read."""
    what = "shade"
    if keys.dim() != 3 or keys.dtype != torch.int64 or not keys.is_contiguous():
        raise RuntimeError("%s: keys must be a contiguous int64 tensor [B,Hr,Wr], got %s %s" % (what, keys.dtype, tuple(keys.shape)))
    B, Hr, Wr = keys.shape
    verts, n, V, F = _mesh_operands(what, verts, faces, B, None)
    if not (0.0 <= alpha <= 1.0 and 0.0 <= ambient <= 1.0):
        raise ValueError("%s: alpha = %r and ambient = %r must lie in [0, 1]" % (what, alpha, ambient))
    background, default_colour = _packed(background, "background"), _packed(default_colour, "default_colour")
    _lib.require_cuda(keys, verts, faces, image, colour)
    dev = keys.device
    _f32(verts, "verts", what)
    for name, t, shape in (("image", image, (B, Hr, Wr, 3)), ("colour", colour, None)):
        if t is None:
            continue
        if t.dtype != torch.uint8 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape) or t.device != dev:
            raise RuntimeError("%s: %s must be a contiguous uint8 tensor%s on the keys' device, got %s %s"
                               % (what, name, " %s" % (shape,) if shape else "", t.dtype, tuple(t.shape)))
    if colour is not None and (colour.numel() != B * n * 3 or colour.shape[-1] != 3):
        raise RuntimeError("%s: colour must be [P,3] = [%d,3], got %s" % (what, B * n, tuple(colour.shape)))
    if verts.device != dev or faces.device != dev:
        raise RuntimeError("%s: keys, verts and faces must be on one device" % what)
    rgb = torch.empty(B, Hr, Wr, 3, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().h3d_render_shade(_lib.ptr(keys), _lib.ptr(verts.detach()), _lib.ptr(faces), _lib.ptr(colour), _lib.ptr(image), B, n, V, F,
                                               Hr, Wr, float(alpha), float(ambient), default_colour, background, _lib.ptr(rgb), _lib.stream_ptr()),
                   "h3d_render_shade")
    return rgb


class MeshRenderer:
    """faces [F,3] (integers, host or device: checked here, the device copy is kept), up = target pixels per map pixel (4 = the network's
    input resolution), focal (None = the target's width), alpha / ambient of `shade`, colours [k,3] u8 cycled over the person slots of an
    image (None = PALETTE).
    __call__(verts, cam_map, ind, n, image, valid) -> dict(face_id, depth, person = face_id // F with -1 for background, rgb).
    Depth between people: dz[p] = focal / s[p], the pinhole distance at which a body shows at scale s, so that a larger person is in
    front.  It is one small torch expression on the device (a gather of cam_map's first channel at ind and a division), not part of the
    kernels: slots the kernel skips (ind outside the map, s <= 0) may hold anything there."""

    def __init__(self, faces, up=4, focal=None, alpha=0.7, ambient=0.3, colours=None, flags=0):
        f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
        if f.dtype.kind not in "iu" or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError("MeshRenderer: faces must be integers [F,3], got %s %s" % (f.dtype, f.shape))
        if int(f.min()) < 0 or int(f.max()) >= MAX_V:
            raise ValueError("MeshRenderer: face indices must lie in [0, V) with V <= %d, got %d .. %d" % (MAX_V, f.min(), f.max()))
        if int(up) < 1:
            raise ValueError("MeshRenderer: up = %r" % (up,))
        if not (0.0 <= alpha <= 1.0 and 0.0 <= ambient <= 1.0):
            raise ValueError("MeshRenderer: alpha = %r and ambient = %r must lie in [0, 1]" % (alpha, ambient))
        if focal is not None and not (np.isfinite(focal) and focal > 0):
            raise ValueError("MeshRenderer: focal = %r" % (focal,))
        pal = PALETTE if colours is None else np.asarray(colours)
        if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
            raise ValueError("MeshRenderer: colours must be uint8 [k,3], got %s %s" % (pal.dtype, pal.shape))
        self.faces = np.ascontiguousarray(f, np.int32)
        self.F, self.max_index = self.faces.shape[0], int(f.max())
        self.up, self.focal, self.alpha, self.ambient, self.flags, self.palette = int(up), focal, float(alpha), float(ambient), int(flags), pal
        self._dev = {}

    def _on(self, dev, B, n):
        d = self._dev.get(dev)
        if d is None:
            d = self._dev[dev] = {"faces": torch.from_numpy(self.faces).to(dev)}
        if (B, n) not in d:
            d[(B, n)] = torch.from_numpy(np.ascontiguousarray(np.tile(self.palette[np.arange(n) % len(self.palette)], (B, 1)))).to(dev)
        return d["faces"], d[(B, n)]

    def __call__(self, verts, cam_map, ind, n=None, image=None, valid=None):
        what = "MeshRenderer"
        V = verts.shape[-2] if verts.dim() >= 3 else 0
        if self.max_index >= V:
            raise RuntimeError("%s: the faces index vertex %d, verts hold %d" % (what, self.max_index, V))
        if V > MAX_V:
            raise RuntimeError("%s: V = %d vertices, the raster kernel stages at most %d in LDS" % (what, V, MAX_V))
        if n is None:
            n = verts.shape[1] if verts.dim() == 4 else verts.shape[0] // max(cam_map.shape[0], 1)
        if n * self.F >= 2 ** 31:
            raise RuntimeError("%s: n F = %d * %d face ids, they must stay below 2^31" % (what, n, self.F))
        _lib.require_cuda(verts, cam_map, ind, image, valid)
        dev = cam_map.device
        B, HW = cam_map.shape[0], cam_map.shape[2] * cam_map.shape[3]
        faces, colour = self._on(dev, B, n)
        focal = float(self.focal if self.focal is not None else self.up * cam_map.shape[3])
        at = ind.detach().to(device=dev, dtype=torch.int64)[:, :n].clamp(0, HW - 1)
        s = cam_map.detach()[:, 0].reshape(B, HW).gather(1, at)
        dz = torch.full_like(s, focal) / s             # (a division of two tensors: `focal / s` would be s.reciprocal() * focal)
        face_id, depth, keys = rasterize(verts, faces, cam_map, ind, n, self.up, valid=valid, dz=dz, flags=self.flags)
        rgb = shade(keys, verts, faces, image=image, colour=colour, alpha=self.alpha, ambient=self.ambient)
        person = torch.div(face_id, self.F, rounding_mode="floor")
        return {"face_id": face_id, "depth": depth, "person": person, "rgb": rgb}


def render_detections(renderer, res, images_uint8=None, vis_thresh=0.3):
    """MultiPoseDetector.run's result of a detector built with Opt(smpl=True, smpl_cam=True) -> the renderer's dict: res['verts'] placed by
    res['heads']['cam'] at res['inds'], the slots with a detection score res['dets'][..., 4] above vis_thresh.  images_uint8
    [B, up H, up W, 3] (up = 4: the network's input frames) or None."""
    for k in ("verts", "inds", "dets", "heads"):
        if k not in res:
            raise KeyError("render_detections: the result has no %r (run a detector built with Opt(smpl=True, smpl_cam=True))" % k)
    if "cam" not in res["heads"]:
        raise KeyError("render_detections: the detector has no `cam` head (Opt(smpl_cam=True))")
    verts = res["verts"]
    n = verts.shape[1]
    cam = res["heads"]["cam"]
    if cam.dtype != torch.float32 or not cam.is_contiguous():
        cam = cam.float().contiguous()
    valid = res["dets"][:, :n, 4] > vis_thresh
    return renderer(verts.contiguous(), cam, res["inds"], n, image=images_uint8, valid=valid)
