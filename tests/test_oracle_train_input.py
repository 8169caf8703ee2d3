"""CPU: the restatement of tests/train_input_ref.py and the draws of h3d_amd.train_input.draw_params against the reference's own
training-input code (tests/golden/train_input_ref.npz, written by tools/gen_train_input_golden.py), the distance between the reference's
float32 grey mean and the exact one the device computes, the ABI of include/h3d.h section 3b and its argument checks through calls that
return before any launch."""
import ctypes
import os
import random
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import train_input_ref as R
from h3d_amd import _lib, train_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_ARG = -1, -5
OPT_KEYS = ("not_rand_crop", "shift", "scale", "aug_rot", "rotate", "flip", "no_color_aug")


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "train_input_ref.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split(".")
        cases.setdefault(name, {})[field] = z[key]
    return cases


def drawn(case):
    """draw_params under the case's seeds, as tools/gen_train_input_golden.py seeds the reference."""
    opt = NS(**{k: case["opt_" + k].item() for k in OPT_KEYS})
    seed = int(case["seed"])
    np.random.seed(seed)
    random.seed(seed)
    return train_input.draw_params([case["img"].shape[:2]], opt, str(case["task"]), data_rng=np.random.RandomState(123)), opt


def mirror(case, mean_mode):
    p, opt = drawn(case)
    in_h, in_w = (int(v) for v in case["input"])
    inp, gs_mean = R.train_batch([case["img"]], p, in_w, in_h, color=not opt.no_color_aug, mean_mode=mean_mode)
    return inp[0], gs_mean


def test_golden_holds_the_cases_the_issue_names(golden):
    assert {"mp_rand_crop", "mp_not_rand_crop", "mp_rot", "mp_flip", "mp_no_color_aug", "ct_40x56"} <= set(golden)
    assert float(golden["mp_rot"]["rot"]) != 0 and bool(golden["mp_flip"]["flipped"]) and bool(golden["mp_no_color_aug"]["opt_no_color_aug"])
    assert bool(golden["mp_not_rand_crop"]["opt_not_rand_crop"]) and golden["ct_40x56"]["inp"].shape == (3, 40, 56)
    for case in golden.values():
        assert case["img"].shape[0] <= 48 and case["img"].shape[1] <= 64 and max(case["inp"].shape[1:]) <= 64


def test_draw_params_reproduces_the_reference_draws(golden):
    for name, case in golden.items():
        p, _ = drawn(case)
        assert p["c"].dtype == np.float32 and np.array_equal(p["c"][0], case["c"]), (name, p["c"], case["c"])
        assert p["s"].dtype == np.float64 and p["s"][0] == float(case["s"]), (name, p["s"], case["s"])
        assert p["rot"][0] == float(case["rot"]) and bool(p["flipped"][0]) == bool(case["flipped"]), name
        assert sorted(p["order"][0]) == [0, 1, 2] and np.all(np.abs(p["alpha"] - 1) <= 0.4)


def test_draws_of_a_batch_follow_one_another(golden):
    """Image b of a batch gets the draws the reference's b-th item gets from the same three streams."""
    opt = NS(not_rand_crop=False, aug_rot=1.0, rotate=30.0, flip=0.5, no_color_aug=False)
    sizes = [(48, 64), (37, 91), (33, 250)]
    np.random.seed(5), random.seed(5)
    batch = train_input.draw_params(sizes, opt, "multi_pose", data_rng=np.random.RandomState(123))
    np.random.seed(5), random.seed(5)
    rng = np.random.RandomState(123)
    for b, size in enumerate(sizes):
        one = train_input.draw_params([size], opt, "multi_pose", data_rng=rng)
        for k, v in one.items():
            assert np.array_equal(v[0], batch[k][b]), (b, k)
    assert batch["s"].shape == (3,) and batch["light"].dtype == np.float64
    keep = train_input.draw_params([(48, 64)], NS(keep_res=True, pad=31, flip=0.0, no_color_aug=True), "ctdet")
    assert keep["s"].shape == (1, 2) and abs(keep["s"][0, 0] / keep["s"][0, 1] - 1.5) < 1e-12           # (64 | 31) + 1 = 96, (48 | 31) + 1 = 64


def test_mirror_equals_the_reference_bit_for_bit(golden):
    for name, case in golden.items():
        inp, _ = mirror(case, "numpy")
        assert inp.dtype == np.float32 and inp.shape == case["inp"].shape, name
        assert np.array_equal(inp.view(np.uint32), case["inp"].view(np.uint32)), (name, int((inp != case["inp"]).sum()))


def test_exact_grey_mean_stays_within_the_derived_distance_of_the_float32_one(golden):
    """The device's grey mean is the correctly rounded one, the reference's is numpy's float32 pairwise mean.  Only contrast_ reads it:
    x = x + float32(gs_mean * (1 - alpha)) with |1 - alpha| <= 0.4, so the two image values differ by at most 0.4 * |difference of the two
    means| in front of that float32 add, whose rounding can turn it into one more ulp of the image value (taken at the largest image value of
    the case); the standardisation divides both by std.  Bound: (0.4 * |mean difference| + one float32 rounding of x) / min(std).
    (The rounding is counted where it happens, in front of the division by std >= 0.274: counted as one ulp of the OUTPUT instead, the bound
    would be 2.06e-07 for mp_rand_crop, whose inputs differ by 2.38e-07 = (one ulp of x = 5.96e-08) / 0.274 rounded to the output's grid.)
    Measured over the golden cases: the means differ by at most 5.96e-08 (one ulp), the inputs by at most 2.38e-07."""
    worst = 0.0
    for name, case in golden.items():
        if bool(case["opt_no_color_aug"]):
            continue
        a, ma = mirror(case, "numpy")
        b, mb = mirror(case, "f64")
        dmean = abs(float(ma[0]) - float(mb[0]))
        x_max = np.float32(np.abs(a.astype(np.float64).transpose(1, 2, 0) * R.STD + R.MEAN).max())       # the largest image value in front of the standardisation
        bound = (0.4 * dmean + float(np.spacing(x_max))) / float(R.STD.min())
        diff = float(np.abs(a.astype(np.float64) - b).max())
        print("%s: gs_mean %.9g (numpy) %.9g (f64), |difference| %.3g, inputs differ by at most %.3g, bound %.3g" % (name, ma[0], mb[0], dmean, diff, bound))
        assert diff <= bound, (name, diff, bound)
        worst = max(worst, diff)
    print("largest difference between the two mean modes: %.3g" % worst)


def test_f64_sum_of_grey_values_is_exact_in_any_order():
    """What lets the device tests ask for bit equality: every grey value is a multiple of 2^-35 below 2, so a float64 sum of up to 2^18
    of them is exact whatever the order."""
    rs = np.random.RandomState(0)
    img = (rs.randint(0, 256, (64, 64, 3)).astype(np.float32) / np.float32(255.))
    gs = R.grayscale(img).astype(np.float64).reshape(-1)
    assert np.all(gs * 2.0 ** 35 == np.round(gs * 2.0 ** 35)) and gs.max() < 2
    want = sum(int(v * 2 ** 35) for v in gs)
    for order in (np.arange(gs.size), rs.permutation(gs.size), np.argsort(gs)):
        acc = 0.0
        for v in gs[order]:
            acc += v
        assert int(acc * 2 ** 35) == want and acc * 2.0 ** 35 == want


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def _c_layout(body):
    """name -> (offset, bytes) of a C struct body of fixed-width scalars and arrays, natural alignment; and the struct's size."""
    sizes = {"double": 8, "int64_t": 8, "int32_t": 4, "float": 4}
    at, out, align = 0, {}, 1
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for name in names.split(","):
            m = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", name)
            sz = sizes[ctype]
            at = (at + sz - 1) // sz * sz
            out[m.group(1)] = (at, sz * int(m.group(2) or 1))
            at += out[m.group(1)][1]
            align = max(align, sz)
    return out, (at + align - 1) // align * align


def test_abi_is_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "h3d.h")).read()
    L = _lib.lib()
    for name in ("h3d_train_input", "h3d_train_input_workspace_bytes"):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M) and hasattr(L, name) and name in _lib.SIGNATURES
    body = re.search(r"struct h3d_train_image \{(.*?)\n\};", hdr, flags=re.S).group(1)
    fields, size = _c_layout(body)
    assert size == ctypes.sizeof(_lib.H3dTrainImage) == 136 == train_input._DESC.itemsize
    assert [n for n, _ in _lib.H3dTrainImage._fields_] == list(fields)
    for name, (at, nbytes) in fields.items():
        f = getattr(_lib.H3dTrainImage, name)
        assert (f.offset, f.size) == (at, nbytes) and train_input._DESC.fields[name][1] == at, name
    for name in ("BRIGHTNESS", "CONTRAST", "SATURATION", "INPUT_NO_COLOR_AUG"):
        assert int(re.search(r"#define H3D_TRAIN_%s (\d+)" % name, hdr).group(1)) == getattr(_lib, "TRAIN_" + name)
    src = open(os.path.join(ROOT, "human-3d-reconstruction_amd", "csrc", "Makefile")).read()
    assert " augment.o" in src and re.search(r"^augment\.o:.*\n\t.*-ffp-contract=off", src, flags=re.M)


def _desc(n=1, **kw):
    d = np.zeros(n, train_input._DESC)
    d["h"], d["w"], d["row_bytes"] = 8, 8, 24
    d["order"] = [0, 1, 2]
    for k, v in kw.items():
        d[k] = v
    return d


def _call(L, d, **kw):
    a = dict(images=64, images_bytes=1 << 20, desc=d.ctypes.data, desc_dev=64, B=len(d), mean=64, std=64, res_h=8, res_w=8, options=0, ws=256,
             ws_bytes=1 << 20, out=64, gs=0)
    a.update(kw)
    return L.h3d_train_input(a["images"], a["images_bytes"], a["desc"], a["desc_dev"], a["B"], a["mean"], a["std"], a["res_h"], a["res_w"],
                             a["options"], a["ws"], a["ws_bytes"], a["out"], a["gs"], None)


def test_abi_return_codes_for_bad_arguments():
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    size = L.h3d_train_input_workspace_bytes
    assert size(64, 512, 512, 0, ctypes.byref(n)) == 0 and n.value == 64 * 512 * 512 * 4 + 64 * 256 * 8
    assert size(2, 33, 33, 0, ctypes.byref(n)) == 0 and n.value == (2 * 1092 * 4 + 255) // 256 * 256 + 256      # 1089 pixels: 1092 with the vector padding, 2 slots
    assert size(2, 33, 33, _lib.TRAIN_INPUT_NO_COLOR_AUG, ctypes.byref(n)) == 0 and n.value == 0
    assert size(2, 33, 33, 0, None) == ERR_ARG and size(2, 33, 33, 2, ctypes.byref(n)) == ERR_ARG
    assert size(0, 33, 33, 0, ctypes.byref(n)) == ERR_SHAPE and size(2, 0, 33, 0, ctypes.byref(n)) == ERR_SHAPE
    assert size(2, 33, 32768, 0, ctypes.byref(n)) == ERR_SHAPE
    good = _desc()
    for name in ("images", "desc", "desc_dev", "mean", "std", "out"):
        assert _call(L, good, **{name: 0}) == ERR_ARG and b"null pointer" in L.h3d_last_error(), name
    for name, value in (("desc_dev", 68), ("mean", 66), ("std", 65), ("out", 66), ("gs", 66)):
        assert _call(L, good, **{name: value}) == ERR_ARG and b"misaligned" in L.h3d_last_error(), name
    assert _call(L, good, B=0) == ERR_SHAPE and _call(L, good, B=-1) == ERR_SHAPE and _call(L, good, B=32768) == ERR_SHAPE
    assert _call(L, good, res_h=0) == ERR_SHAPE and _call(L, good, res_w=32768) == ERR_SHAPE and _call(L, good, res_w=-3) == ERR_SHAPE
    assert _call(L, good, options=2) == ERR_ARG
    for field, value in (("h", 0), ("w", -1), ("h", 32768), ("w", 32768), ("row_bytes", 23)):
        assert _call(L, _desc(**{field: value})) == ERR_SHAPE, (field, value)
    assert _call(L, _desc(2, h=[8, 0])) == ERR_SHAPE and b"image 1" in L.h3d_last_error()              # every descriptor is read
    assert _call(L, good, images_bytes=8 * 24 - 1) == ERR_SHAPE and b"leaves the source buffer" in L.h3d_last_error()
    assert _call(L, _desc(offset=1), images_bytes=8 * 24) == ERR_SHAPE and _call(L, _desc(offset=-1)) == ERR_SHAPE
    assert _call(L, _desc(flipped=2)) == ERR_ARG
    for order in ([0, 0, 1], [0, 1, 3], [-1, 1, 2], [2, 2, 2]):
        assert _call(L, _desc(order=order)) == ERR_ARG and b"permutation" in L.h3d_last_error(), order
    assert _call(L, good, ws=0) == ERR_ARG and b"workspace" in L.h3d_last_error()
    assert _call(L, good, ws_bytes=8 * 8 * 4 + 7) == ERR_ARG and b"workspace" in L.h3d_last_error()
    assert _call(L, good, ws=264) == ERR_ARG and b"workspace" in L.h3d_last_error()


def test_cpu_tensors_and_bad_images_raise():
    import torch
    p = {"c": np.array([[4, 4]], np.float32), "s": np.array([8.0])}
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        train_input.train_input(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), p, 8, color_aug=False)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        train_input.train_input([torch.zeros(8, 8, 3, dtype=torch.uint8)], p, 8, color_aug=False)
    with pytest.raises(ValueError):
        train_input.draw_params([(8, 8)], NS(), "exdet")
