"""CPU: pin the restatement of the PS-ROI pooling backward (tests/psroi_grad_ref.py) without trusting it -- its forward half against
the existing yardstick tests/psroi_ref.py, its gradients against central differences and the adjoint identity, the lattice conditions
the GPU test's exact comparison rests on -- and the host side of the feature: header, binding and exports, the C ABI's argument checks,
and the shared sample geometry (csrc/psroi_geom.h) run by a stand-alone host program under AddressSanitizer / UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import psroi_grad_ref as G
from psroi_ref import psroi_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FD_STEP = 1e-6


def _case(seed, B=2, C=4, H=9, W=11, R=5, P=3, spp=2, ncls=2, scale=0.25):
    rng = np.random.default_rng(seed)
    inp = rng.normal(size=(B, C, H, W)).astype(f32)
    rois = G.random_rois(rng, R, B, H, W, scale)
    trans = rng.normal(size=(R, 2 * ncls, P, P)).astype(f32)
    go = rng.normal(size=(R, C, P, P)).astype(f32)
    mask = rng.normal(size=(R, P, P)).astype(f32)
    return inp, rois, trans, go, mask


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_float32_forward_equals_the_existing_restatement(seed):
    inp, rois, trans, _, mask = _case(seed, C=8, H=13, W=10, R=7, P=7, spp=4)
    for args, kw in (((inp, rois, trans, 0, 0.25, 7, 7, 4, 0.3), {}), ((inp, rois, None, 1, 0.25, 7, 7, 4, 0.3), {}),
                     ((inp, rois, trans[:, :2], 0, 0.25, 7, 7, 4, 0.3), {"mask": rng_mask(seed)})):
        out, cnt = G.forward(*args, **kw)
        ref, rcnt = psroi_pool(args[0], args[1], args[2], args[3], args[4], 8, 1, *args[5:], **kw)
        np.testing.assert_array_equal(cnt, rcnt)
        np.testing.assert_array_equal(out, ref)
    # part_size != pooled_size
    ref, rcnt = psroi_pool(inp, rois, trans[:, :, :5, :5], 0, 0.25, 8, 1, 7, 5, 4, 0.3)
    out5, cnt5 = G.forward(inp, rois, trans[:, :, :5, :5], 0, 0.25, 7, 5, 4, 0.3)
    np.testing.assert_array_equal(out5, ref)
    np.testing.assert_array_equal(cnt5, rcnt)


def rng_mask(seed):
    return np.random.default_rng(100 + seed).normal(size=(7, 7, 7)).astype(f32)


def _fd(fn, x):
    g = np.zeros_like(x)
    for i in np.ndindex(x.shape):
        a, b = x.copy(), x.copy()
        a[i] += FD_STEP
        b[i] -= FD_STEP
        g[i] = (fn(a) - fn(b)) / (2 * FD_STEP)
    return g


# seeds whose samples keep >= 1e-3 from every kink (asserted below): the gradient is then the derivative of ONE smooth piece across the
# whole finite-difference stencil
@pytest.mark.parametrize("seed", [3, 5])
def test_float64_trans_gradient_against_central_differences(seed):
    inp, rois, trans, go, _ = _case(seed)
    cfg = (0.25, 3, 3, 2, 0.1)
    _, cnt, kink = G.forward(inp, rois, trans, 0, *cfg, geometry=np.float64, want_kink=True)
    assert kink >= 1e-3, kink
    r = G.backward(go, inp, rois, trans, cnt, 0, *cfg, geometry=np.float64)
    loss = lambda t: float((go.astype(np.float64) * G.forward(inp, rois, t, 0, *cfg, geometry=np.float64)[0]).sum())
    fd = _fd(loss, trans.astype(np.float64))
    # the loss is linear in one translation inside a piece, so the difference quotient carries rounding only: two float64 evaluations
    # of ~50 operations each on sum |grad_out| * pooled(|input|)
    a = float((np.abs(go) * G.forward(np.abs(inp), rois, trans, 0, *cfg, geometry=np.float64)[0]).sum())
    tol = 100 * 2.0 ** -53 * a / (2 * FD_STEP)
    err = np.abs(fd - r["g_trans"]).max()
    print("seed %d: kink %.3g, max |g| %.3g, FD error %.3g, tolerance %.3g" % (seed, kink, np.abs(fd).max(), err, tol))
    assert np.abs(fd).max() > 0.1 and err <= tol, (err, tol)


@pytest.mark.parametrize("seed", [3, 5])
def test_float64_modulated_gradients_against_central_differences(seed):
    inp, rois, trans, go, mask = _case(seed, ncls=1)
    om = np.concatenate([trans, mask[:, None]], 1).astype(np.float64)
    cfg = (0.25, 3, 3, 2, 0.1)
    _, _, kink = G.forward(inp, rois, om, 0, *cfg, mask=om[:, 2], geometry=np.float64, want_kink=True)
    assert kink >= 1e-3, kink
    r = G.backward(go, inp, rois, om, None, 0, *cfg, mask=om[:, 2], geometry=np.float64)
    loss = lambda t: float((go.astype(np.float64) * G.forward(inp, rois, t, 0, *cfg, mask=t[:, 2], geometry=np.float64)[0]).sum())
    fd = _fd(loss, om)
    a = float((np.abs(go) * G.forward(np.abs(inp), rois, om, 0, *cfg, mask=om[:, 2], geometry=np.float64)[0]).sum())
    # rounding as above; the sigmoid adds a truncation term h^2 / 6 * |L'''|, |sigmoid'''| <= 1/8
    tol = 100 * 2.0 ** -53 * a / (2 * FD_STEP) + FD_STEP ** 2 / 48 * a
    err = np.abs(fd - r["g_trans"]).max()
    print("seed %d: kink %.3g, max |g offsets| %.3g, max |g mask| %.3g, FD error %.3g, tolerance %.3g"
          % (seed, kink, np.abs(fd[:, :2]).max(), np.abs(fd[:, 2]).max(), err, tol))
    assert np.abs(fd[:, 2]).max() > 0.01 and err <= tol, (err, tol)


@pytest.mark.parametrize("mode", ["operator", "no_trans", "modulated"])
def test_grad_input_is_the_adjoint_of_the_forward(mode):
    """The op is linear in the input: <grad_input, d> = <grad_out, forward(d)> for any d."""
    inp, rois, trans, go, mask = _case(7, C=4, H=9, W=11, R=6, P=3, spp=2, ncls=1 if mode == "modulated" else 2)
    d = np.random.default_rng(8).normal(size=inp.shape).astype(f32)
    cfg = (0.25, 3, 3, 2, 0.1)
    for geometry in (np.float32, np.float64):
        if mode == "modulated":
            om = np.concatenate([trans, mask[:, None]], 1)
            r = G.backward(go, inp, rois, om, None, 0, *cfg, mask=om[:, 2], geometry=geometry)
            fwd = G.forward(d, rois, om, 0, *cfg, mask=om[:, 2], geometry=geometry)[0]
        else:
            nt = int(mode == "no_trans")
            cnt = G.forward(inp, rois, trans, nt, *cfg, geometry=geometry)[1]
            r = G.backward(go, inp, rois, trans, cnt, nt, *cfg, geometry=geometry)
            fwd = G.forward(d, rois, trans, nt, *cfg, geometry=geometry)[0]
        lhs, rhs = float((r["g_input"] * d).sum()), float((go.astype(np.float64) * fwd).sum())
        scale = float((np.abs(r["g_input"]) * np.abs(d)).sum())
        assert abs(lhs) > 0.1 and abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


def test_lattice_case_is_exact_in_float32():
    """On the lattice case every gradient times 16 (modulated mode, sigmoid 1/2: times 64) is an integer below 2^24, so every partial sum
    of every fp32 summation order is exact and the GPU test may ask for equality -- under atomics too."""
    c = G.lattice_case()
    cfg = (c["scale"], c["P"], c["part"], c["spp"], c["tstd"])
    _, cnt = G.forward(c["inp"], c["rois"], c["trans"], 0, *cfg)
    r = G.backward(c["grad_out"], c["inp"], c["rois"], c["trans"], cnt, 0, *cfg)
    assert set(np.unique(cnt)) <= {0.0, 1.0, 2.0, 3.0, 4.0} and cnt.max() == 4 and (cnt == 0).any()
    for name, unit in (("g_input", 16), ("g_trans", 16)):
        v = r[name] * unit
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() > 0, name
        # the absolute sums bound every partial sum
        assert (r["a_" + name[2:]] * unit).max() < 2 ** 24, name
    om = np.concatenate([c["trans"][:, :2], np.zeros((c["rois"].shape[0], 1, 2, 2), f32)], 1)
    r = G.backward(c["grad_out"], c["inp"], c["rois"], om, None, 0, *cfg, mask=om[:, 2])
    for v, a in ((r["g_input"] * 64, r["a_input"] * 64), (r["g_trans"][:, :2] * 64, r["a_trans"][:, :2] * 64)):
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() > 0 and a.max() < 2 ** 24


def test_bounds_hold_for_a_float32_evaluation_of_the_restatement():
    """The bound is for any fp32 evaluation: the restatement's own float32 mode (numpy's summation order) must meet it."""
    inp, rois, trans, go, mask = _case(11, C=8, H=13, W=10, R=7, P=3, spp=4)
    cfg = (0.25, 3, 3, 4, 0.5)
    _, cnt = G.forward(inp, rois, trans, 0, *cfg)
    (gi, gt), (bi, bt) = G.bounds(go, inp, rois, trans, cnt, 0, *cfg)
    r32 = G.backward(go, inp, rois, trans, cnt, 0, *cfg, acc=np.float32)
    G.check("grad_input", r32["g_input"], gi, bi)
    G.check("grad_trans", r32["g_trans"], gt, bt)
    om = np.concatenate([trans[:, :2], mask[:, None]], 1)
    (gi, gt), (bi, bt) = G.bounds(go, inp, rois, om, None, 0, *cfg, mask=om[:, 2])
    r32 = G.backward(go, inp, rois, om, None, 0, *cfg, mask=om[:, 2], acc=np.float32)
    G.check("modulated grad_input", r32["g_input"], gi, bi)
    G.check("modulated grad_offset_mask", r32["g_trans"], gt, bt)


# ---- header, binding, exports, argument checks (no launch: no GPU needed) ----------------------------------------------------------

NEW = ("h3d_dcn_v2_psroi_pooling_backward", "h3d_dcn_pooling_modulated_backward", "h3d_psroi_backward_path")


def test_header_binding_and_library_declare_the_new_entry_points():
    from h3d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "h3d.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert re.search(r"#define H3D_ABI_VERSION 4\b", hdr) and _lib.ABI_VERSION == 4 and L.h3d_abi_version() == 4
    from h3d_amd import dcn_v2
    for name in ("dcn_v2_psroi_pooling_backward", "dcn_v2_pooling_autograd", "TrainableDCNv2Pooling", "TrainableDCNPooling"):
        assert hasattr(dcn_v2, name), name
    assert sorted(dcn_v2.TrainableDCNPooling(0.25, 3, 4, False, deform_fc_dim=8).state_dict()) == \
        sorted(dcn_v2.DCNPooling(0.25, 3, 4, False, deform_fc_dim=8).state_dict())


def test_c_abi_argument_checks_without_a_gpu():
    from h3d_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)

    def call(*, ptr=p, R=1, rows=1, ct=2, no_trans=0, output_dim=4, gs=1, P=2, part=2, spp=2):
        return L.h3d_dcn_v2_psroi_pooling_backward(ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1, 4, 8, 8, R, rows, ct, no_trans, 0.25, output_dim, gs,
                                                   P, part, spp, 0.1, 0, None)
    assert call(ptr=None) == -5 and b"null pointer" in L.h3d_last_error()
    assert call(gs=2) == -4 and b"group_size" in L.h3d_last_error()
    assert call(output_dim=3) == -1 and L.h3d_last_error() == b"input channels and output channels must equal"
    assert call(ct=6) == -1 and b"num_classes" in L.h3d_last_error()
    assert call(ct=3) == -1
    assert call(P=0) == -5
    assert call(P=46) == -4 and b"pooled_size 46 > 45" in L.h3d_last_error()
    assert call(spp=5000) == -4
    assert call(R=3, rows=2) == -1 and b"rows" in L.h3d_last_error()
    m = lambda ptr, part: L.h3d_dcn_pooling_modulated_backward(ptr, ptr, ptr, ptr, ptr, ptr, 1, 4, 8, 8, 1, 0.25, 4, 1, 2, part, 2, 0.1, 0, None)
    assert m(None, 2) == -5
    assert m(p, 3) == -1 and b"part_size" in L.h3d_last_error()


def test_backward_path_is_a_function_of_the_geometry():
    """A roi of a few pixels is combined in LDS; one covering a 64 x 64 map is added directly; an invalid or far one adds nothing."""
    from h3d_amd import dcn_v2
    shape = (2, 64, 64, 64)
    small, whole = [0, 100, 120, 180, 190], [1, 0, 0, 1023, 1023]
    assert dcn_v2.psroi_backward_path(small, None, shape, True, 1 / 16, 7, 7, 4, 0.1) == 1
    assert dcn_v2.psroi_backward_path(whole, None, shape, True, 1 / 16, 7, 7, 4, 0.1) == 2
    assert dcn_v2.psroi_backward_path(small, None, shape, True, 1 / 16, 7, 7, 4, 0.1, direct=True) == 2
    assert dcn_v2.psroi_backward_path([2, 100, 120, 180, 190], None, shape, True, 1 / 16, 7, 7, 4, 0.1) == 0
    assert dcn_v2.psroi_backward_path([np.nan, 100, 120, 180, 190], None, shape, True, 1 / 16, 7, 7, 4, 0.1) == 0
    assert dcn_v2.psroi_backward_path([0, 5000, 5000, 6000, 6000], None, shape, True, 1 / 16, 7, 7, 4, 0.1) == 0
    # a translation moves the samples: the same roi pushed out of the map by its offsets
    far = np.full((2, 7, 7), 1000.0, f32)
    assert dcn_v2.psroi_backward_path(small, far, shape, False, 1 / 16, 7, 7, 4, 0.1) == 0
    assert dcn_v2.psroi_backward_path(small, np.zeros((2, 7, 7), f32), shape, False, 1 / 16, 7, 7, 4, 0.1) == 1


# ---- the shared geometry header on the host, under sanitizers -----------------------------------------------------------------------

def _host_compiler():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")):
        if c and os.path.exists(c):
            return c
    return None


def _build_host_program(tmp_path):
    """The program, built with -fsanitize=address,undefined where that links (nothing is preloaded: the program has its own main)."""
    cc = _host_compiler()
    assert cc, "no host C++ compiler"
    src = os.path.join(ROOT, "tests", "psroi_geom_host.cpp")
    inc = os.path.join(ROOT, "human-3d-reconstruction_amd", "csrc")
    exe = str(tmp_path / "psroi_geom_host")
    base = [cc, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I", inc, src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:
        subprocess.run(base, check=True, capture_output=True, text=True)
    print("host program: %s, sanitizers %s" % (cc, "on" if sanitized else "OFF (the sanitizer link failed: %s)" % r.stderr[-300:]))
    return exe


@pytest.mark.parametrize("no_trans", [1, 0])
def test_geometry_header_on_the_host_keeps_every_corner_inside_its_plane(tmp_path, no_trans):
    B, C, H, W = G.EDGE_SHAPE
    scale, P, part, spp, tstd, ncls = 0.25, 7, (7 if no_trans else 3), 4, (0.0 if no_trans else 0.5), (1 if no_trans else 2)
    rois = np.concatenate([G.EDGE_ROIS, G.BAD_ROIS])
    R = rois.shape[0]
    trans = np.random.default_rng(7).normal(size=(R, 2 * ncls, part, part)).astype(f32)
    if not no_trans:
        trans[5, 0, 1, 2], trans[6, 1, 0, 0], trans[7, 2, 2, 2], trans[7, 3, 1, 1] = np.nan, np.inf, -np.inf, 1e30
    case = tmp_path / "case.txt"
    with open(case, "w") as f:
        f.write("%d %d %d %r %d %d %d %r %d %d %d\n" % (B, H, W, scale, P, part, spp, tstd, no_trans, ncls, R))
        for row in rois:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
        if not no_trans:
            f.write(" ".join(repr(float(v)) for v in trans.ravel()) + "\n")
    exe = _build_host_program(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got, key = {}, None
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "roi":
            key = (int(t[1]), int(t[3]))
            got[key] = None if t[-1] == "invalid" else []
        else:
            got[key].append([int(v) for v in t])
    assert len(got) == R * ncls
    # the restatement's float32 geometry, sample by sample
    want = {(n, k): s for n, k, _, _, _, _, s in G._classes(np.zeros(G.EDGE_SHAPE, f32), rois, trans, no_trans, scale, P, part, spp, tstd,
                                                              None, f32)}
    flagged = 0
    for key, rows in got.items():
        if rows is None:
            assert key not in want, key          # invalid batch index: nothing is formed
            continue
        valid, xa, ya, xb, yb, dx, dy, _ = want[key]
        a = np.array(rows, np.int64).reshape(P, P, spp, spp, 8)
        flags, off = a[..., 4], a[..., 5]
        np.testing.assert_array_equal(flags & 1, valid.astype(np.int64))
        v = valid
        np.testing.assert_array_equal(off[v], (ya * W + xa)[v])
        np.testing.assert_array_equal(a[..., 6][v], dx.astype(f32).view(np.uint32)[v])
        np.testing.assert_array_equal(a[..., 7][v], dy.astype(f32).view(np.uint32)[v])
        np.testing.assert_array_equal(((flags >> 1) & 1)[v], (xb > xa)[v])
        np.testing.assert_array_equal(((flags >> 2) & 1)[v], (yb > ya)[v])
        assert (flags[~v] == 0).all()
        # every flagged offset and the far corners its flags admit lie inside [0, H * W)
        far = off + ((flags >> 1) & 1) + ((flags >> 2) & 1) * W
        assert (off[v] >= 0).all() and (far[v] < H * W).all()
        assert ((off % W + ((flags >> 1) & 1))[v] < W).all()
        flagged += int(v.sum())
    assert flagged > 1000
