"""GPU: h3d_train_input (csrc/augment.hip) through h3d_amd.train_input against the numpy restatement of the reference's training input
(tests/train_input_ref.py, mean_mode "f64": the exact grey mean the device's fp64 sum gives).  Every comparison is torch.equal: the warp
is integer arithmetic, the colour steps are single IEEE operations, the grey sum is exact below 2^18 pixels."""
import itertools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import targets_ref
import train_input_ref as R
import h3d_amd  # noqa: F401
from h3d_amd import preprocess as pre
from h3d_amd import targets, train_input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(37, 91), (48, 64), (33, 250)]                    # (h, w)


def frames(seed, sizes=SIZES):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]


def colour_params(seed, B, p):
    rs = np.random.RandomState(seed)
    orders = list(itertools.permutations(range(3)))
    p["order"] = np.array([orders[(b + seed) % 6] for b in range(B)], np.int32)
    p["alpha"] = 1.0 + rs.uniform(-0.4, 0.4, (B, 3))
    p["light"] = np.dot(rs.normal(scale=0.1, size=(B, 3)) * train_input.EIG_VAL, train_input.EIG_VEC.T.astype(np.float64))
    return p


def three_params(seed=3):
    """Image 0: s at 0.6 x the long side around a centre near the right edge, so that the crop leaves the frame (border 0), unrotated;
    image 1: mirrored, +17 degrees, s at 1.3 x; image 2: -31 degrees."""
    p = {"c": np.array([[80.0, 30.0], [64 - 21.0 - 1, 20.0], [120.5, 17.25]], np.float32), "s": np.array([0.6 * 91, 1.3 * 64, 0.9 * 250]),
         "rot": np.array([0.0, 17.0, -31.0]), "flipped": np.array([False, True, False])}
    return colour_params(seed, 3, p)


def padded(img, dev=DEV, pad=16):
    """The frame as a view into rows of (w + pad) pixels: row_bytes = 3 (w + pad)."""
    h, w, _ = img.shape
    wide = torch.full((h, w + pad, 3), 255, dtype=torch.uint8, device=dev)
    wide[:, :w] = torch.from_numpy(img).to(dev)
    return wide[:, :w]


def on_device(imgs):
    return [padded(img) if k == 1 else torch.from_numpy(img).to(DEV) for k, img in enumerate(imgs)]


@pytest.fixture(scope="module")
def three():
    imgs, p = frames(1), three_params()
    want, means = R.train_batch(imgs, p, 64, 64)
    return imgs, p, want, means


def test_three_sizes_rotations_mirror_and_border(three):
    imgs, p, want, means = three
    dev_imgs = on_device(imgs)
    assert dev_imgs[1].stride(0) == 3 * (64 + 16)
    got, gs_mean = train_input.train_input(dev_imgs, p, 64, return_gs_mean=True)
    assert got.shape == (3, 3, 64, 64) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(gs_mean.cpu(), torch.from_numpy(means))                                       # the float32 mean, bit for bit
    # the crop of image 0 leaves the frame: its right-hand columns are warped border (0 in front of the colour steps)
    plain = train_input.train_input(dev_imgs, p, 64, color_aug=False).cpu().numpy()
    border = ((0 - R.MEAN) / R.STD).reshape(3)
    assert all((plain[0, c, :, -4:] == border[c]).all() for c in range(3)) and not (plain[0, 0, 32, :32] == border[0]).all()


@pytest.mark.parametrize("res_h,res_w", [(33, 33), (48, 80), (72, 72)])
def test_odd_wide_and_two_workgroup_inputs(res_h, res_w):
    """33 x 33: scalar stores, a pixel count that fills no whole workgroup and no whole vector; 48 x 80: ctdet's input_h != input_w;
    72 x 72 = 5184 pixels: six partial sums, two workgroups of the colour launch, the second one partly idle."""
    imgs, p = frames(res_h), three_params(res_w)
    want, means = R.train_batch(imgs, p, res_w, res_h)
    got, gs_mean = train_input.train_input(on_device(imgs), p, (res_h, res_w), train_input.CTDET_MEAN, train_input.CTDET_STD, return_gs_mean=True)
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and torch.equal(gs_mean.cpu(), torch.from_numpy(means))


def test_all_six_orders_of_the_colour_operations():
    img = frames(7, [(40, 56)])[0]
    orders = list(itertools.permutations(range(3)))
    p = colour_params(0, 6, {"c": np.tile(np.array([[27.0, 19.0]], np.float32), (6, 1)), "s": np.full(6, 50.0), "rot": np.full(6, 5.0),
                             "flipped": np.zeros(6, bool)})
    p["order"] = np.array(orders, np.int32)
    p["alpha"][:] = p["alpha"][0]                           # the same three factors in six orders
    want, _ = R.train_batch([img] * 6, p, 40, 40)
    got = train_input.train_input(torch.from_numpy(np.stack([img] * 6)).to(DEV), p, 40).cpu()
    assert torch.equal(got, torch.from_numpy(want))
    assert len({got[k].numpy().tobytes() for k in range(6)}) == 6                 # and the order matters


def test_no_color_aug_and_the_val_crop(three):
    imgs, p, _, _ = three
    want, _ = R.train_batch(imgs, p, 64, 64, color=False)
    got = train_input.train_input(on_device(imgs), p, 64, color_aug=False)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    # rot = 0, no mirror, c = centre, s = the long side: the val branch, which pre_process computes
    same = torch.from_numpy(np.stack(frames(9, [(37, 91)] * 2))).to(DEV)
    val, c, s = pre.pre_process(same, input_res=64)
    again = train_input.train_input(same, {"c": c, "s": s}, 64, color_aug=False)
    assert torch.equal(again, val)


def test_two_runs_are_identical_and_an_unaligned_output_takes_the_scalar_stores(three):
    imgs, p, want, _ = three
    dev_imgs = on_device(imgs)
    a = train_input.train_input(dev_imgs, p, 64)
    b = train_input.train_input(dev_imgs, p, 64)
    assert torch.equal(a, b)
    flat = torch.zeros(3 * 3 * 64 * 64 + 2, dtype=torch.float32, device=DEV)
    out = flat[1:-1].view(3, 3, 64, 64)                     # 4 bytes past a 16-byte boundary
    assert out.data_ptr() % 16 == 4
    assert train_input.train_input(dev_imgs, p, 64, out=out) is out
    assert torch.equal(out, a) and float(flat[0]) == 0.0 and float(flat[-1]) == 0.0


def test_list_and_tensor_forms_agree():
    imgs = frames(11, [(48, 64)] * 3)
    p = three_params(5)
    p["c"] = np.array([[30.0, 20.0], [64 - 21.0 - 1, 20.0], [40.5, 17.25]], np.float32)
    as_list = train_input.train_input([torch.from_numpy(i).to(DEV) for i in imgs], p, 33)
    as_tensor = train_input.train_input(torch.from_numpy(np.stack(imgs)).to(DEV), p, 33)
    assert torch.equal(as_list, as_tensor)
    want, _ = R.train_batch(imgs, p, 33, 33)
    assert torch.equal(as_tensor.cpu(), torch.from_numpy(want))


def test_multi_pose_train_batch_returns_the_whole_item():
    import random
    sizes = [(48, 64), (40, 56)]
    imgs = frames(13, sizes)
    scenes = [targets_ref.scene(20 + b, 3, M=4, img_w=w, img_h=h, min_size=6.0, max_size=30.0) for b, (h, w) in enumerate(sizes)]
    boxes, kps = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    opt = NS(input_res=64, output_res=16, not_rand_crop=False, aug_rot=1.0, rotate=30.0, flip=0.5, no_color_aug=False)
    np.random.seed(17), random.seed(17)
    item = train_input.multi_pose_train_batch([torch.from_numpy(i).to(DEV) for i in imgs], boxes, kps, [3, 3], opt, data_rng=np.random.RandomState(123))
    np.random.seed(17), random.seed(17)
    p = train_input.draw_params(sizes, opt, "multi_pose", data_rng=np.random.RandomState(123))
    assert p["rot"].any()
    want, _ = R.train_batch(imgs, p, 64, 64)
    assert torch.equal(item["input"].cpu(), torch.from_numpy(want))
    labels = targets.multi_pose_targets(boxes, kps, [3, 3], p["c"], p["s"], rot=p["rot"], flipped=p["flipped"], width=[w for _, w in sizes], opt=opt,
                                        device=DEV)
    assert set(item) == set(labels) | {"input"}
    for k, v in labels.items():
        if k == "meta":
            assert all(torch.equal(item["meta"][m].cpu(), v[m].cpu()) for m in v)
        else:
            assert torch.equal(item[k], v), k
    # the same parameters handed in: nothing is drawn
    state = np.random.get_state()[1].copy()
    again = train_input.multi_pose_train_batch([torch.from_numpy(i).to(DEV) for i in imgs], boxes, kps, [3, 3], opt, params=p)
    assert torch.equal(again["input"], item["input"]) and np.array_equal(np.random.get_state()[1], state)


def test_ctdet_train_batch_returns_the_whole_item():
    import random
    sizes = [(48, 64), (48, 64)]
    imgs = np.stack(frames(15, sizes))
    boxes = np.array([[[10, 8, 20, 16], [30, 20, 18, 22]]] * 2, np.float32)
    cls = np.array([[0, 2], [1, 1]], np.int32)
    opt = NS(input_h=48, input_w=80, output_h=12, output_w=20, num_classes=3, max_objs=8, flip=0.5)
    np.random.seed(19), random.seed(19)
    item = train_input.ctdet_train_batch(torch.from_numpy(imgs).to(DEV), boxes, cls, [2, 2], opt, data_rng=np.random.RandomState(123))
    np.random.seed(19), random.seed(19)
    p = train_input.draw_params(sizes, opt, "ctdet", data_rng=np.random.RandomState(123))
    assert not p["rot"].any()
    want, _ = R.train_batch(list(imgs), p, 80, 48)
    assert tuple(item["input"].shape) == (2, 3, 48, 80) and torch.equal(item["input"].cpu(), torch.from_numpy(want))
    labels = targets.ctdet_targets(boxes, cls, [2, 2], p["c"], p["s"], flipped=p["flipped"], width=[64, 64], opt=opt, device=DEV)
    assert all(torch.equal(item[k], labels[k]) for k in ("hm", "wh", "reg", "ind", "reg_mask"))


def test_cpu_tensors_raise():
    p = {"c": np.array([[4, 4]], np.float32), "s": np.array([8.0])}
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        train_input.train_input(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), p, 8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        train_input.train_input(torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV), p, 8, color_aug=False,
                                out=torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        train_input.train_input(torch.zeros(1, 8, 8, 3, device=DEV), p, 8)              # not uint8
