"""CPU: the yardstick of the max-pool / up-sample + add backward (tests/pool_up_ref.py) checked against itself -- the numpy restatement
of the header's formulas against torch autograd, the tie rule, the exactness condition of every lattice case -- plus the exported symbols
and the argument return codes of include/h3d.h section 2d (every check runs before the first HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pool_up_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape,ties", [((1, 4, 2, 2), True), ((2, 20, 5, 7), True), ((1, 64, 8, 6), True), ((2, 8, 7, 9), False),
                                        ((1, 4, 3, 5), True), ((1, 4, 2, 3), True)])
def test_pool_restatement_is_torchs_rule_in_both_precisions(shape, ties):
    x, gy = R.pool_case(shape, 3, ties)
    y_np, gx_np = R.pool_numpy(x.numpy(), gy.numpy())
    for dt in (torch.float64, torch.float32):
        y, gx = R.pool_yardstick(x, gy, dt)
        assert torch.equal(y.float(), torch.from_numpy(y_np)) and torch.equal(gx.float(), torch.from_numpy(gx_np))
    H, W = shape[2:]
    if H % 2:
        assert not gx_np[:, :, H - 1].any()
    if W % 2:
        assert not gx_np[:, :, :, W - 1].any()
    if ties and H >= 2 and W >= 2:
        win = np.stack([x.numpy()[:, :, j // 2:H // 2 * 2:2, j % 2:W // 2 * 2:2] for j in range(4)], -1)
        # four draws from four values: the maximum is unique with probability 36 / 64, so 44 % of the windows tie
        assert win[..., 0].size < 100 or ((win == win.max(-1, keepdims=True)).sum(-1) > 1).mean() > 0.35
        assert (np.count_nonzero(np.stack([gx_np[:, :, j // 2:H // 2 * 2:2, j % 2:W // 2 * 2:2] for j in range(4)], -1), -1) == 1).all()


def test_pool_tie_goes_to_the_first_maximum():
    x = torch.tensor([[2.0, 2.0], [2.0, 2.0]]).view(1, 1, 2, 2).repeat(1, 4, 1, 1)
    x[0, 1, 0, 0] = 1.0                 # -> (0,1)
    x[0, 2, 0, :] = 1.0                 # -> (1,0)
    x[0, 3] = torch.tensor([[0.0, 1.0], [1.0, 2.0]])      # -> (1,1)
    _, gx = R.pool_numpy(x.numpy(), np.full((1, 4, 1, 1), 5.0, np.float32))
    assert [int(np.flatnonzero(gx[0, c].reshape(-1))[0]) for c in range(4)] == [0, 1, 2, 3]
    assert torch.equal(R.pool_yardstick(x, torch.full((1, 4, 1, 1), 5.0), torch.float32)[1], torch.from_numpy(gx))


@pytest.mark.parametrize("name", sorted(R.UP_CASES))
def test_up_restatement_agrees_with_autograd(name):
    c = R.up_case(name)
    _, gx, gw, gs = c.run(torch.float64)
    gx_np, gw_np = R.up_numpy(c.x, c.w, c.gy, c.f)
    assert np.allclose(gx.numpy(), gx_np, rtol=1e-12, atol=1e-12) and np.allclose(gw.numpy(), gw_np, rtol=1e-12, atol=1e-12)
    assert torch.equal(gs, c.gy)                        # the skip's gradient is grad_y itself
    assert float(gx.abs().max()) > 0 and float(gw.abs().max()) > 0


@pytest.mark.parametrize("name", R.LATTICE_CASES)
def test_lattice_cases_are_exact_in_fp32(name):
    """Bilinear weights (dyadic, unit 1 / 2f a side) and integers in [-8, 8]: the float32 yardstick gives float64's bits, every output
    lies on its grid, and the sum of the absolute values of its terms stays below 2^24 units, so no summation order can round."""
    c = R.up_case(name, True)
    unit = float((2 * c.f) ** 2)
    assert torch.equal(c.w * unit, (c.w * unit).round()) and float(c.w.max()) <= 1 and float(c.w.min()) > 0
    for t in (c.x, c.skip, c.gy):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 8
    r64, r32 = c.run(torch.float64), c.run(torch.float32)
    sums = R.lattice_abs_sums(c)
    for nm, a, r, u in zip(R.NAMES[:3], r32, r64, (unit, unit, 1.0)):
        assert torch.equal(a.double(), r), nm
        assert torch.equal(r * u, (r * u).round()), nm
        assert sums[nm] < 2.0 ** 24 and sums[nm] >= float(r.abs().max()) * u, (nm, sums[nm])
    gx_np, gw_np = R.up_numpy(c.x, c.w, c.gy, c.f)
    assert np.array_equal(gx_np, r64[1].numpy()) and np.array_equal(gw_np, r64[2].numpy())


def test_case_list_sits_either_side_of_the_kernels_tile():
    src = open(os.path.join(ROOT, "human-3d-reconstruction_amd", "csrc", "pool_up_bwd.hip")).read()
    for f, t in R.TILE.items():
        assert "struct UpBwd<%d> { static constexpr int TH = %d, TW = %d," % (f, t, t) in src
        hs = {R.UP_CASES[n][2] for n in R.UP_CASES if n.startswith("f%d_tile" % f)}
        ws = {R.UP_CASES[n][3] for n in R.UP_CASES if n.startswith("f%d_tile" % f)}
        assert hs == {t - 1, t, t + 1} and ws == {max(t - 1, 1), t, t + 1}
    assert len(R.UP_CASES) == 23 and len(R.LATTICE_CASES) == 20


def test_new_symbols_are_exported():
    import h3d_amd
    from h3d_amd import _lib, pool_up, train_model, trainer
    assert "pool_up" in h3d_amd.__all__ and "train_model" in h3d_amd.__all__
    for name in ("h3d_maxpool2_backward", "h3d_upsample_backward_workspace_bytes", "h3d_upsample_backward"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "h3d.h")).read()
    assert "#define H3D_ABI_VERSION 4" in hdr and "h3d_upsample_backward(" in hdr and "h3d_maxpool2_backward(" in hdr
    for fn, args in ((pool_up.max_pool2_autograd, (torch.zeros(1, 4, 4, 4),)),
                     (pool_up.max_pool2_backward, (torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 2, 2))),
                     (pool_up.up_add_autograd, (torch.zeros(1, 4, 2, 2), torch.zeros(4, 1, 4, 4), torch.zeros(1, 4, 4, 4), 2)),
                     (pool_up.upsample_backward, (torch.zeros(1, 4, 2, 2), torch.zeros(4, 1, 4, 4), torch.zeros(1, 4, 4, 4), 2))):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(*args)
    w = R.fill_up_weights(4, 2).float()
    assert torch.equal(pool_up.pack_up_weight(w), w.reshape(4, 16).t())
    assert issubclass(trainer.NetworkTrainer, trainer.HeadsTrainer) and trainer.HeadsTrainer.MODULE.__name__ == "TrainableHeads"
    assert issubclass(train_model.TrainableDLASeg, torch.nn.Module)


HEADS = {"hm": 1, "wh": 2, "hps": 34}


def _net(use_dcn=True, hc=64):
    from h3d_amd import arch, model, synth
    net = model.dla_net(HEADS, head_conv=hc, not_use_dcn=not use_dcn, dtype="f32")
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, use_dcn, hc), seed=0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net


@pytest.mark.parametrize("use_dcn", [True, False])
def test_trainable_dla_seg_parameters_and_export_on_the_cpu(use_dcn):
    """Construction, the parameter list and the export need no GPU: the folded tensors are weights.PackedWeights._fold's, the export of
    an untrained object has the reference's keys and reproduces every tensor up to the rounding of W' / scale, the re-fold is the inverse."""
    from h3d_amd import arch, train_model
    from h3d_amd.weights import PackedWeights
    net = _net(use_dcn)
    t = train_model.TrainableDLASeg(net)
    sd = net.state_dict()
    n_bn = sum(k.endswith(".running_mean") for k in sd) - 2                 # level3 / level4 `project`: computed, never used
    n_plain = sum(".conv_offset_mask." in k or ".up_" in k for k in sd)
    params = dict(t.named_parameters())
    assert len(params) == 2 * n_bn + n_plain + 4 * len(HEADS)
    assert all(p is q for p, q in zip(t.head_params()["hm"], [net.state_dict(keep_vars=True)["hm." + k] for k in ("0.weight", "0.bias", "2.weight", "2.bias")]))
    pw = PackedWeights.from_tensors({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}, "f32", "cpu")
    w, b = pw._fold(pw.sd["base.level2.tree1.conv1.weight"], None, "base.level2.tree1.bn1")
    assert torch.equal(t._p("base.level2.tree1.conv1.weight").detach(), w) and torch.equal(t._p("base.level2.tree1.conv1.bias").detach(), b)
    w, b = pw._fold(pw.sd["ida_up.proj_1.conv.weight"], pw.sd["ida_up.proj_1.conv.bias"], "ida_up.proj_1.actf.0")
    assert torch.equal(t._p("ida_up.proj_1.conv.weight").detach(), w) and torch.equal(t._p("ida_up.proj_1.conv.bias").detach(), b)
    ex = t.export_state_dict()
    assert list(ex) == list(sd) and set(ex) == set(arch.state_dict_shapes(HEADS, use_dcn, 64))
    for k, v in sd.items():
        if v.dtype == torch.float32:
            assert torch.allclose(ex[k], v, rtol=1e-6, atol=1e-6 * float(v.abs().max()) + 1e-7), k
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")) or (k.endswith(".weight") and v.dim() == 1) or \
                ".project." in k and k.startswith(("base.level3.project", "base.level4.project")) or k.endswith(".conv.bias"):
            assert torch.equal(ex[k], v), k
    full = t.state_dict()
    assert set(full) - set(ex) == {train_model.FOLDED_PREFIX + n.replace("__", ".") for n in t.folded}
    # train: move every parameter, export into a fresh model, wrap it again -> the same folded tensors up to rounding; with the full
    # state_dict the very bits
    with torch.no_grad():
        for p in t.parameters():
            p.mul_(1.25).add_(0.01)
    moved = {n: p.detach().clone() for n, p in t.folded.items()}
    other = train_model.TrainableDLASeg(_net(use_dcn))
    other.load_state_dict(t.export_state_dict())
    for n, p in other.folded.items():
        assert torch.allclose(p.detach(), moved[n], rtol=1e-5, atol=1e-6 * float(moved[n].abs().max())), n
    other.load_state_dict(t.state_dict())
    assert all(torch.equal(p.detach(), moved[n]) for n, p in other.folded.items())
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(other.head_params()["hps"], t.head_params()["hps"]))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        t(torch.zeros(1, 3, 64, 64))


def test_stale_folded_entries_never_win_over_the_reference_keys():
    """checkpoint.load_model fills every key a checkpoint lacks from the object's own state_dict: a reference-only checkpoint then arrives
    with the OBJECT's folded tensors beside its own reference keys.  However close the two are, the re-fold of the reference keys is taken."""
    from h3d_amd import train_model
    src = train_model.TrainableDLASeg(_net())
    with torch.no_grad():
        for p in src.folded.values():
            p.mul_(1.0 + 2e-6)                        # within any tolerance a closeness test would use
    ref_only = src.export_state_dict()
    dst = train_model.TrainableDLASeg(_net())
    own = dst.state_dict()
    mixed = dict(ref_only, **{k: v for k, v in own.items() if k.startswith(train_model.FOLDED_PREFIX)})
    dst.load_state_dict(mixed)
    want = dst._fold_all(ref_only)
    changed = 0
    for key, t in want.items():
        assert torch.equal(dst._p(key).detach(), t), key
        changed += int(not torch.equal(t, own[train_model.FOLDED_PREFIX + key]))
    assert changed > len(want) // 2                   # the stale entries did differ


@pytest.mark.parametrize("use_dcn,B", [(True, 1), (True, 2), (False, 1), (False, 2)])
def test_no_parameter_of_the_network_yardstick_has_a_zero_gradient(use_dcn, B):
    """The CPU half of tests/test_gpu_train_model.py: under the fixed linear functional every parameter tensor of TrainableDLASeg has a
    non-zero float64 gradient (no tensor passes the GPU comparison vacuously), and the float32 run is close to it."""
    import network_grad_ref as N
    o64, g64, o32, g32 = N.functional_runs(use_dcn, B)
    assert len(g64) == len(g32) > 100
    for k, g in g64.items():
        assert N.l2(g) > 0, k
        assert N.l2(g32[k].double() - g) <= 1e-3 * N.l2(g), k


def test_a_zero_folded_scale_is_refused():
    from h3d_amd import train_model
    net = _net()
    with torch.no_grad():
        net.base.level2.tree1.bn1.weight[3] = 0.0
    with pytest.raises(ValueError, match="scale"):
        train_model.TrainableDLASeg(net)
    with pytest.raises(ValueError, match="f32"):
        from h3d_amd import model
        train_model.TrainableDLASeg(model.dla_net(HEADS, head_conv=64, dtype="bf16"))


ERR_SHAPE, ERR_ARG = -1, -5


def _pool(L, x=0x1000, x_cs=8, gy=0x2000, gy_cs=8, gx=0x3000, gx_cs=8, B=1, C=8, H=4, W=4):
    return L.h3d_maxpool2_backward(x, x_cs, gy, gy_cs, gx, gx_cs, B, C, H, W, None)


def _up(L, x=0x1000, x_cs=8, w=0x2000, gy=0x3000, gy_cs=8, gx=0x4000, gx_cs=8, gw=0x5000, B=1, C=8, H=4, W=4, f=2, ws=0x100000, ws_bytes=1 << 40):
    return L.h3d_upsample_backward(x, x_cs, w, gy, gy_cs, gx, gx_cs, gw, B, C, H, W, f, ws, ws_bytes, None)


def test_abi_return_codes_without_a_gpu():
    """Only calls that fail an argument check (or ask for nothing): nothing reaches HIP (the pointers are made up)."""
    from h3d_amd import _lib
    L = _lib.lib()
    for bad in (dict(B=0), dict(C=0), dict(H=-1), dict(W=0), dict(C=6), dict(x_cs=4), dict(x_cs=10), dict(gy_cs=6), dict(gx_cs=7)):
        assert _pool(L, **bad) == ERR_SHAPE, bad
        assert _up(L, **bad) == ERR_SHAPE, bad
    assert _pool(L, x_cs=10) == ERR_SHAPE and b"channel stride" in L.h3d_last_error()
    for bad in (dict(x=0), dict(gy=0), dict(x=0x1004), dict(gy=0x2008), dict(gx=0x3004)):
        assert _pool(L, **bad) == ERR_ARG, bad
    assert _pool(L, gx=0) == 0                                    # no output asked for: nothing to do
    assert _pool(L, gx=0, gy=0, H=1) == 0                         # no output pixel: grad_y is not read
    for f in (0, 1, 3, 16):
        assert _up(L, f=f) == ERR_SHAPE, f
    for bad in (dict(x=0), dict(w=0), dict(gy=0), dict(x=0x1004), dict(w=0x2004), dict(gy=0x3008), dict(gx=0x4004), dict(gw=0x5002)):
        assert _up(L, **bad) == ERR_ARG, bad
    for bad in (dict(ws=0), dict(ws=0x100010), dict(ws_bytes=16)):
        assert _up(L, **bad) == ERR_ARG and b"workspace" in L.h3d_last_error(), bad
    assert _up(L, gx=0, gw=0, ws=0) == 0
    n = ctypes.c_size_t(7)
    r256 = lambda v: (v + 255) // 256 * 256
    assert L.h3d_upsample_backward_workspace_bytes(1, 8, 4, 4, 2, ctypes.byref(n)) == 0 and n.value == r256(1 * 16 * 8 * 4)
    # B = 8, 64 x 64 at f = 2: S = 8 * 64 tiles -> G = 8 chains of 64
    assert L.h3d_upsample_backward_workspace_bytes(8, 64, 64, 64, 2, ctypes.byref(n)) == 0 and n.value == r256(512 * 16 * 64 * 4) + r256(8 * 16 * 64 * 4)
    # S = 65 -> G = 2 chains, 33 rows: one zeroed slot
    assert L.h3d_upsample_backward_workspace_bytes(65, 4, 2, 2, 8, ctypes.byref(n)) == 0 and n.value == r256(66 * 256 * 4 * 4) + r256(2 * 256 * 4 * 4)
    assert L.h3d_upsample_backward_workspace_bytes(1, 8, 4, 4, 3, ctypes.byref(n)) == ERR_SHAPE and n.value == 0
    assert L.h3d_upsample_backward_workspace_bytes(1, 8, 4, 4, 2, None) == ERR_ARG
