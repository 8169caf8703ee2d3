"""GPU: h3d_amd.targets (csrc/targets.hip) against the reference's own output (tests/golden/targets_ref.npz) and, for the cases
generated here, the restatement of tests/targets_ref.py (pinned to that file by tests/test_oracle_targets.py).

Rules.  Integer and mask outputs, gt_count and which map pixels are non-zero: exact.  Float rows and gt_det: within 2^-16 (2 ulp of
float32 at magnitude 128: each box edge carries one float32 rounding of a float64 sum whose last bit may differ, and w and ct combine two
edges).  Maps: |delta| <= 2^-24 (one float32 ulp below 1: two float64 exp implementations of at most 1 ulp each) at every pixel, and at
most 1 pixel in 10^4 of a tensor may differ at all.  hm is exactly 1.0 at every live centre.  The observed counts are printed
(`pytest -s`) and recorded in DESIGN.md section 17.

A radius larger than the map is not reachable through the ABI: r3 of gaussian_radius (utils/image.py:112-116) tends to 0.6 h w / (h + w),
which for a box clipped to the map stays below 0.6 of the map's shorter side.  Its reachable form is a WINDOW 2r + 1 larger than the map
in one axis: an elongated box on an elongated ctdet map (8 x 256: 9 rows on 8; 32 x 1024: cut at both opposite borders at once; both
asserted on the scenes).  The
clipping of a splat at each border and in each corner, r = 0 and windows taller than a render workgroup's rows are covered by the
multi_pose scenes and asserted on them."""
import os

import numpy as np
import pytest
import torch

import losses_ref as LR
import targets_ref as R
from conftest import GOLDEN
from gpu_helpers import DEV
from h3d_amd import losses, targets
from h3d_amd.detector import Opt

pytestmark = pytest.mark.gpu
ROW_TOL, MAP_TOL = 2.0 ** -16, 2.0 ** -24
INT_KEYS = ("ind", "reg_mask", "hps_mask", "hp_ind", "hp_mask", "cat_spec_mask", "gt_count")
MAP_KEYS = ("hm", "hm_hp")
IMG_W, IMG_H = 640, 480


def _golden():
    z = np.load(os.path.join(GOLDEN, "targets_ref.npz"))
    cases = {}
    for key in z.files:
        name, kind, field = key.split(".")
        cases.setdefault(name, {"in": {}, "out": {}})[kind][field] = z[key]
    return cases


CASES = _golden()
POSE_NAMES = sorted(n for n in CASES if n.startswith("mp_"))
CTDET_NAMES = sorted(n for n in CASES if n.startswith("ct_"))


def compare(name, got, ref, centres=True):
    """got: {key: device tensor}; ref: {key: array} with a leading batch axis or without.  -> differing map pixels."""
    differing = 0
    for key, r in ref.items():
        if key not in got:
            continue
        g = got[key].cpu().numpy()
        r = np.asarray(r).reshape(g.shape)
        assert g.dtype == r.dtype, (name, key, g.dtype, r.dtype)
        if key in INT_KEYS:
            assert np.array_equal(g, r), (name, key, np.flatnonzero(g.reshape(-1) != r.reshape(-1))[:8])
        elif key in MAP_KEYS:
            assert np.array_equal(g != 0, r != 0), (name, key, "non-zero pattern", int(((g != 0) != (r != 0)).sum()))
            d = np.abs(g.astype(np.float64) - r)
            nd = int((d != 0).sum())
            print("%s %s: %d of %d pixels differ, max |delta| %.3g" % (name, key, nd, g.size, d.max() if d.size else 0.0))
            assert d.size == 0 or d.max() <= MAP_TOL, (name, key, float(d.max()))
            assert nd * 10 ** 4 <= g.size, (name, key, nd, g.size)
            differing += nd
        else:
            err = float(np.abs(g.astype(np.float64) - r).max()) if g.size else 0.0
            assert err <= ROW_TOL, (name, key, err)
    if centres and "hm" in got and "ind" in ref and "hm_hp" in ref:
        hm = got["hm"].cpu().numpy()
        hm = hm.reshape(hm.shape[0], -1)
        ind, cnt = np.asarray(ref["ind"]).reshape(hm.shape[0], -1), np.asarray(ref["gt_count"]).reshape(-1)
        live = np.asarray(ref["wh"]).reshape(hm.shape[0], -1, 2).all(axis=2)
        for b in range(hm.shape[0]):
            if (np.asarray(ref["hm"]).reshape(hm.shape)[b] == R.HM_ROT).all():
                continue                                         # a rotated image: hm is the constant
            assert (hm[b, ind[b][live[b]]] == 1.0).all() and live[b].sum() == cnt[b], (name, b)
    return differing


def dev(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)


def identity_trans(B, res_w, res_h, img_w=IMG_W, img_h=IMG_H, rot=None):
    c = np.tile(np.array([img_w / 2, img_h / 2], np.float32), (B, 1))
    s = np.full(B, float(max(img_w, img_h)))
    return targets.target_transforms(c, s, rot, res_w, res_h).numpy()


def pose_raw(boxes, kps, num, trans, res, rot_flag=None, flipped=None, width=None, max_objs=32, out=None, want=targets.POSE_OUTPUTS):
    pairs = dev(np.array(R.FLIP_IDX), torch.int32) if flipped is not None else None
    return targets.multi_pose_targets_raw(dev(boxes, torch.float32), dev(kps, torch.float32), dev(num, torch.int32), dev(trans, torch.float64),
                                          dev(rot_flag, torch.int32), dev(flipped, torch.int32), dev(width, torch.int32), pairs, res, res, max_objs,
                                          want=want, out=out)


def pose_ref(boxes, kps, num, trans, res, rot_flag=None, flipped=None, width=None, max_objs=32):
    return R.multi_pose_batch(boxes, kps, num, trans, rot_flag, flipped, width, out_h=res, out_w=res, max_objs=max_objs)


def edge_scene(res, seed=0):
    """One image whose boxes, given in OUTPUT pixels and mapped back through the crop, sit in the four corners and on the four borders, one of
    a single pixel (r = 0), one over the whole map, some random ones; keypoints on and around each box, also outside the map."""
    rs = np.random.RandomState(seed)
    a, m = 0.45 * res, res - 1.0
    out_boxes = [(-2, -2, a, a), (m - a, -3, m + 4, a), (-1, m - a, a, m + 2), (m - a, m - a, m + 3, m + 3),          # corners
                 (0.3 * res, -2, 0.3 * res + a, 0.5 * a), (0.3 * res, m - 0.5 * a, 0.3 * res + a, m + 2),              # top, bottom
                 (-3, 0.3 * res, 0.5 * a, 0.3 * res + a), (m - 0.5 * a, 0.3 * res, m + 2, 0.3 * res + a),              # left, right
                 (0.5 * res, 0.5 * res, 0.5 * res + 0.6, 0.5 * res + 0.7), (-5, -5, res + 5, res + 5)]                 # r = 0, the whole map
    for _ in range(4):
        x, y = rs.uniform(0, 0.7 * res, 2)
        out_boxes.append((x, y, x + rs.uniform(1, 0.5 * res), y + rs.uniform(1, 0.5 * res)))
    k = IMG_W / res                                              # c = image centre, s = 640: out = (src - centre) res / 640 + res / 2
    n = len(out_boxes)
    boxes, kps = np.zeros((n, 4), np.float32), np.zeros((n, 17, 3), np.float32)
    for i, (x0, y0, x1, y1) in enumerate(out_boxes):
        sx0, sy0, sx1, sy1 = x0 * k, (y0 - res / 2) * k + IMG_H / 2, x1 * k, (y1 - res / 2) * k + IMG_H / 2
        boxes[i] = sx0, sy0, sx1 - sx0, sy1 - sy0
        kps[i, :, 0] = rs.uniform(sx0 - 0.2 * (sx1 - sx0), sx1 + 0.2 * (sx1 - sx0), 17)
        kps[i, :, 1] = rs.uniform(sy0 - 0.2 * (sy1 - sy0), sy1 + 0.2 * (sy1 - sy0), 17)
        kps[i, :, 2] = rs.randint(0, 3, 17)
        for j, (ox, oy) in enumerate(((x0, y0), (x1, y0), (x0, y1), (x1, y1))):          # joints 0..3: the box's corners, pulled into the map
            kps[i, j] = (min(max(ox, 0), m) + 0.4) * k, (min(max(oy, 0), m) + 0.4 - res / 2) * k + IMG_H / 2, 2
    return boxes, kps


# ---- 1-3: the reference's own output, end to end through the public functions --------------------------------------------------------
@pytest.mark.parametrize("name", POSE_NAMES)
def test_multi_pose_targets_against_the_reference(name):
    i, o = CASES[name]["in"], CASES[name]["out"]
    res = int(i["res"])
    got = targets.multi_pose_targets(i["boxes"][None], i["keypoints"][None], [int(i["num"])], i["c"][None], [float(i["s"])], rot=[float(i["rot"])],
                                     flipped=[int(i["flipped"])], width=[int(i["width"])], opt=Opt(output_res=res, max_objs=32), device=DEV)
    assert set(got) == {"hm", "reg_mask", "ind", "wh", "hps", "hps_mask", "reg", "hm_hp", "hp_offset", "hp_ind", "hp_mask", "meta"}
    flat = dict(got, gt_det=got["meta"]["gt_det"], gt_count=got["meta"]["gt_count"])
    del flat["meta"]
    compare(name, flat, o)
    assert int(flat["gt_count"][0]) == int(o["gt_count"]) and (int(i["num"]) <= 32 or name == "mp_res33_clamp")
    if name == "mp_empty":
        assert all(not bool(t.any()) for t in flat.values())
    if name == "mp_res33_clamp":
        assert int(i["num"]) == 40 and i["boxes"].shape[0] == 40
    # the keys follow the options
    few = targets.multi_pose_targets(i["boxes"][None], i["keypoints"][None], [int(i["num"])], i["c"][None], [float(i["s"])],
                                     opt=Opt(output_res=res, reg_offset=False, hm_hp=False, reg_hp_offset=False), device=DEV)
    assert set(few) == {"hm", "reg_mask", "ind", "wh", "hps", "hps_mask", "meta"}


@pytest.mark.parametrize("cat_spec_wh", [False, True])
@pytest.mark.parametrize("name", CTDET_NAMES)
def test_ctdet_targets_against_the_reference(name, cat_spec_wh):
    i, o = CASES[name]["in"], CASES[name]["out"]
    opt = Opt(task="ctdet", num_classes=int(i["classes"]), cat_spec_wh=cat_spec_wh, max_objs=32)
    opt.output_h, opt.output_w = int(i["out_h"]), int(i["out_w"])
    s = i["s"][None] if i["s"].ndim else [float(i["s"])]
    got = targets.ctdet_targets(i["boxes"][None], i["cls"][None], [int(i["num"])], i["c"][None], s, flipped=[int(i["flipped"])],
                                width=[int(i["width"])], opt=opt, device=DEV)
    keys = {"hm", "reg_mask", "ind", "reg", "meta"} | ({"cat_spec_wh", "cat_spec_mask"} if cat_spec_wh else {"wh"})
    assert set(got) == keys
    flat = dict(got, gt_det=got["meta"]["gt_det"], gt_count=got["meta"]["gt_count"])
    del flat["meta"]
    compare(name, flat, o, centres=False)
    hm = flat["hm"].cpu().numpy()[0]
    slots = np.flatnonzero(o["reg_mask"])                         # live slots; their class from the reference's cat_spec_mask
    assert len(slots) == int(o["gt_count"]) > 0
    assert (hm.reshape(hm.shape[0], -1)[o["cat_spec_mask"][slots].argmax(axis=1) // 2, o["ind"][slots]] == 1.0).all()
    if int(i["classes"]) == 80:                                  # two objects of one class, and classes with none
        assert i["cls"][0] == i["cls"][1] and not hm[[c for c in range(80) if c not in set(i["cls"].tolist())]].any()


# ---- 4: a batch equals its images alone --------------------------------------------------------------------------------------------
def test_a_batch_of_three_equals_its_images_alone():
    res, M = 20, 9
    counts = [0, 3, 9]
    boxes, kps = np.zeros((3, M, 4), np.float32), np.zeros((3, M, 17, 3), np.float32)
    for b, n in enumerate(counts):
        boxes[b], kps[b] = R.scene(40 + b, n, M=M, quarter=False)
    rot, flipped, width = np.array([0.0, 23.0, 0.0]), np.array([0, 0, 1]), np.array([IMG_W] * 3)
    trans = identity_trans(3, res, res, rot=rot)
    got = pose_raw(boxes, kps, counts, trans, res, rot != 0, flipped, width)
    compare("batch3", got, pose_ref(boxes, kps, counts, trans, res, rot != 0, flipped, width))
    assert got["gt_count"].tolist()[0] == 0
    for b in range(3):
        alone = pose_raw(boxes[b:b + 1], kps[b:b + 1], counts[b:b + 1], trans[b:b + 1], res, (rot != 0)[b:b + 1], flipped[b:b + 1], width[b:b + 1])
        for key, t in alone.items():
            assert torch.equal(t[0], got[key][b]), (b, key)


# ---- 5: map sizes, borders, corners, r = 0 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [8, 20, 33, 128])
def test_map_sizes_with_splats_clipped_at_every_border_and_corner(res):
    boxes, kps = edge_scene(res, seed=res)
    n = len(boxes)
    trans = identity_trans(1, res, res)
    ref = pose_ref(boxes[None], kps[None], [n], trans, res)
    # the scene does what its name says: windows cut at each border and in each corner, a radius of 0, and (at 128) windows taller than the
    # 8 rows of a render workgroup
    live = ref["wh"][0].any(axis=1)
    r = np.repeat(R.gaussian_radius(ref["wh"][0][:, 1], ref["wh"][0][:, 0])[0], 17)[ref["hp_mask"][0] > 0]          # keypoint splats: the object's radius
    x, y = ref["hp_ind"][0][ref["hp_mask"][0] > 0] % res, ref["hp_ind"][0][ref["hp_mask"][0] > 0] // res
    lo_x, hi_x, lo_y, hi_y = x - r < 0, x + r > res - 1, y - r < 0, y + r > res - 1
    assert (lo_x & lo_y).any() and (hi_x & lo_y).any() and (lo_x & hi_y).any() and (hi_x & hi_y).any()
    assert (lo_x & ~lo_y & ~hi_y).any() and (hi_x & ~lo_y & ~hi_y).any() and (lo_y & ~lo_x & ~hi_x).any() and (hi_y & ~lo_x & ~hi_x).any()
    assert (r == 0).any() and (res < 128 or (2 * r + 1).max() > 16)
    assert ref["hp_mask"].sum() > 0 and (ref["hp_mask"][0].reshape(-1, 17).sum(axis=1)[:n][live[:n]] < (kps[:, :, 2] > 0).sum(axis=1)[live[:n]]).any()   # keypoints outside
    got = pose_raw(boxes[None], kps[None], [n], trans, res)
    compare("edges res %d" % res, got, ref)


def test_ctdet_map_of_12_by_20_and_80_classes():
    H, W, C, n = 12, 20, 80, 14
    boxes, _ = edge_scene(20, seed=5)
    boxes = boxes[:n]
    cls = np.random.RandomState(3).randint(0, C, n).astype(np.int32)
    cls[1], cls[5] = cls[0], -1                                   # two objects of one class; a class index outside the map: skipped
    c, s = np.array([[IMG_W / 2, IMG_H / 2]], np.float32), np.array([[640.0, 384.0]], np.float32)
    trans = targets.target_transforms(c, s, None, W, H).numpy()
    ref = R.ctdet_batch(boxes[None], cls[None], [n], trans, out_h=H, out_w=W, num_classes=C, max_objs=16)
    got = targets.ctdet_targets_raw(dev(boxes[None], torch.float32), dev(cls[None], torch.int32), dev([n], torch.int32), dev(trans, torch.float64),
                                    None, None, H, W, C, 16)
    compare("ctdet 12x20", got, ref, centres=False)
    assert 0 < int(ref["gt_count"][0]) < n and not ref["hm"][0][[k for k in range(C) if k not in set(cls.tolist())]].any()


@pytest.mark.parametrize("H,W", [(8, 256), (256, 8), (32, 1024), (1024, 32)])
def test_ctdet_window_larger_than_the_map(H, W):
    """A box over a whole elongated map.  8 x 256: h = 7, w = 255, r = 4, a 9-row window on 8 rows (rows -1..7 around the centre row 3:
    cut at the top, flush with the bottom).  32 x 1024: r = 17 around row 15, rows -2..32, cut at the top and the bottom at once.  The
    transposed maps do the same to the columns, on rows narrower than one render workgroup's span."""
    short = min(H, W)
    c, s = np.array([[W / 2, H / 2]], np.float32), np.array([[float(W), float(H)]], np.float32)      # the crop is the identity
    boxes = np.array([[[-3.0, -3.0, W + 6.0, H + 6.0], [0.3 * W, 0.3 * H, 0.31 * W, 0.32 * H], [0.6 * W, 0.1 * H, 0.3 * W, 0.85 * H]]], np.float32)
    cls = np.array([[1, 1, 0]], np.int32)
    trans = targets.target_transforms(c, s, None, W, H).numpy()
    ref = R.ctdet_batch(boxes, cls, [3], trans, out_h=H, out_w=W, num_classes=2, max_objs=4)
    r = int(R.gaussian_radius(ref["wh"][0][:1, 1], ref["wh"][0][:1, 0])[0][0])
    assert int(ref["gt_count"][0]) == 3 and 2 * r + 1 > short and r == (4 if short == 8 else 17), r
    y0, x0 = divmod(int(ref["ind"][0, 0]), W)
    centre = y0 if H < W else x0
    assert centre - r < 0 and centre + r >= short - 1 and (short == 8 or centre + r > short - 1)
    got = targets.ctdet_targets_raw(dev(boxes, torch.float32), dev(cls, torch.int32), dev([3], torch.int32), dev(trans, torch.float64),
                                    None, None, H, W, 2, 4)
    compare("ctdet %dx%d" % (H, W), got, ref, centres=False)
    assert int((ref["hm"][0, 1] > 0).all(axis=0 if H < W else 1).sum()) >= 2 * r + 1          # whole columns (rows) of the map are covered


# ---- 6: overlapping splats: the maximum, whatever the order -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5])
def test_overlapping_splats_take_the_maximum_and_ignore_the_object_order(n):
    res = 33
    base, kp = R.scene(77, 1, quarter=False, min_size=200.0, max_size=260.0)
    boxes, kps = np.repeat(base, n, axis=0), np.repeat(kp, n, axis=0)
    boxes[:, 0] += 37.0 * np.arange(n)                            # shifted copies: their splats overlap on hm and on every joint's map
    kps[:, :, 0] += 37.0 * np.arange(n)[:, None]
    kps[:, :, 2] = 2
    trans = identity_trans(1, res, res)
    ref = pose_ref(boxes[None], kps[None], [n], trans, res)
    got = pose_raw(boxes[None], kps[None], [n], trans, res)
    compare("overlap %d" % n, got, ref)
    assert float(got["hm"].max()) == 1.0 and int((got["hm"] == 1.0).sum()) == n and float(got["hm_hp"].max()) == 1.0
    assert int(((ref["hm"] > 0) & (ref["hm"] < 1)).sum()) > 0
    perm = np.random.RandomState(n).permutation(n)
    again = pose_raw(boxes[perm][None], kps[perm][None], [n], trans, res)
    assert torch.equal(again["hm"], got["hm"]) and torch.equal(again["hm_hp"], got["hm_hp"])
    assert torch.equal(again["ind"][0, :n], got["ind"][0, perm.tolist()])


# ---- 7: no keypoints, keypoints outside, a box clipped to zero width ---------------------------------------------------------------------
@pytest.mark.parametrize("rot", [0.0, 17.0])
def test_person_without_keypoints_points_outside_and_a_box_clipped_away(rot):
    res = 20
    boxes, kps = R.scene(91, 4, quarter=False)
    kps[1, :, 2] = 0                                              # all v = 0
    boxes[2] = (-300.0, 100.0, 120.0, 90.0)                       # left of the image: both x edges clip to 0
    kps[2, :, 0] -= 2000.0                                        # its keypoints far outside
    kps[3, :8, 0] += 5000.0
    trans = identity_trans(1, res, res, rot=np.array([rot]))
    flag = np.array([rot != 0])
    ref = pose_ref(boxes[None], kps[None], [4], trans, res, flag)
    got = pose_raw(boxes[None], kps[None], [4], trans, res, flag)
    compare("gates rot %g" % rot, got, ref)
    assert int(ref["gt_count"][0]) == (4 if rot else 3)           # the clipped box is live only under rot
    assert ref["wh"][0, 2, 0] == 0 and (ref["reg_mask"][0, :4].tolist() == ([0, 0, 0, 0] if rot else [1, 0, 0, 1]))
    if rot:
        assert bool((got["hm"] == np.float32(0.9999)).all()) and not bool(got["hps_mask"].any()) and bool(got["hp_mask"].any())


# ---- 9: NULL outputs, sentinels behind every output, misaligned bases -------------------------------------------------------------------
def guarded(shape, dtype):
    """A contiguous tensor at 4 mod 16 (int64: 8 mod 16, the least torch can view) with sentinels in front and 64 behind."""
    n = int(np.prod(shape))
    lead = 4 if dtype == torch.uint8 else 1
    buf = torch.full((lead + n + 64,), 77, dtype=dtype, device=DEV)
    view = buf[lead:lead + n].view(shape)
    assert view.data_ptr() % 16 == (8 if dtype == torch.int64 else 4)
    return buf, view, lead


@pytest.mark.parametrize("res", [20, 33])
def test_null_outputs_sentinels_and_misaligned_bases(res):
    boxes, kps = edge_scene(res, seed=3)
    n = len(boxes)
    trans = identity_trans(2, res, res)
    args = (np.stack([boxes, boxes[::-1]]), np.stack([kps, kps[::-1]]), [n, 5], trans, res)
    plain = pose_raw(*args, max_objs=16)
    bufs = {k: guarded(shape, dt) for k, (shape, dt) in targets.pose_output_specs(2, 16, 17, res, res).items()}
    got = pose_raw(*args, max_objs=16, out={k: v[1] for k, v in bufs.items()})
    for k, (buf, view, lead) in bufs.items():
        assert torch.equal(view, plain[k]), k
        assert bool((buf[:lead] == 77).all()) and bool((buf[lead + view.numel():] == 77).all()), k
    # a call that wants two outputs writes those two
    for k, (buf, view, lead) in bufs.items():
        buf.fill_(77)
    some = pose_raw(*args, max_objs=16, out={k: bufs[k][1] for k in ("hm_hp", "wh")})
    assert set(some) == {"hm_hp", "wh"}
    for k, (buf, view, lead) in bufs.items():
        if k in some:
            assert torch.equal(view, plain[k]), k
            assert bool((buf[:lead] == 77).all()) and bool((buf[lead + view.numel():] == 77).all()), k
        else:
            assert bool((buf == 77).all()), k
    rows = pose_raw(*args, max_objs=16, want=("ind", "gt_count"))          # no map: no workspace, no render launch
    assert torch.equal(rows["ind"], plain["ind"]) and torch.equal(rows["gt_count"], plain["gt_count"])


# ---- 10: reproducible, and on a side stream -------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_a_side_stream_works():
    res = 33
    boxes, kps = R.scene(55, 12, quarter=False)
    trans = identity_trans(1, res, res)
    a = pose_raw(boxes[None], kps[None], [12], trans, res)
    b = pose_raw(boxes[None], kps[None], [12], trans, res)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = pose_raw(boxes[None], kps[None], [12], trans, res)
    side.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    compare("stream", c, pose_ref(boxes[None], kps[None], [12], trans, res))


# ---- 11: the dict feeds loss_multi_pose ------------------------------------------------------------------------------------------------------
def test_targets_feed_loss_multi_pose_like_the_reference_batch():
    i, o = CASES["mp_plain"]["in"], CASES["mp_plain"]["out"]
    res = int(i["res"])
    batch = targets.multi_pose_targets(i["boxes"][None], i["keypoints"][None], [int(i["num"])], i["c"][None], [float(i["s"])],
                                       opt=Opt(output_res=res), device=DEV)
    gold = {k: torch.from_numpy(o[k][None]) for k in ("hm", "hm_hp", "hps", "hps_mask", "ind", "wh", "reg", "reg_mask", "hp_offset", "hp_mask", "hp_ind")}
    heads = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}
    v64, v32, got = [], [], []
    for seed in range(200, 208):
        g = torch.Generator().manual_seed(seed)
        output = {k: torch.randn(1, c, res, res, generator=g) * (2.0 if k.startswith("hm") else 4.0) - (2.0 if k.startswith("hm") else 0.0)
                  for k, c in heads.items()}
        v64.append(LR.multi_pose(LR.cast(output, torch.float64), LR.cast(gold, torch.float64))[0])
        v32.append(LR.multi_pose(output, LR.cast(gold, torch.float32))[0])
        loss, stats = losses.loss_multi_pose(Opt())([{k: v.to(DEV) for k, v in output.items()}], batch)
        got.append(loss.cpu())
        assert set(stats) == set(losses.loss_multi_pose.KEYS)
    LR.check_scalars("loss_multi_pose on device targets", got, v64, LR.pooled_e32(v32, v64))
