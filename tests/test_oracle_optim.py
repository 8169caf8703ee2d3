"""CPU: the definition of the Adam step (tests/optim_ref.py, the numpy mirror of csrc/optim.hip), the host side of h3d_adam_step, the
optimiser class and the checkpoint round trip.

Why the yardstick is float64 Adam and not torch's float32 bits: the mirror -- every line one IEEE binary32 operation -- is not bit-equal
to torch.optim.Adam(foreach=False) on float32 CPU tensors: for 4097 elements about half of the state words differ (parameters by at
most 2 ulp), as torch's vectorised CPU kernels contract some of the products.  Those bits belong to one CPU kernel build.
The rule is the project's own (DESIGN.md sections 13, 18, 21): per case and per kind (param, exp_avg, exp_avg_sq, pooled over the case's
tensors) max |x - x64| <= 4 e32 + 1e-7 max |x64|, x64 = torch.optim.Adam on float64, e32 = the error of torch's float32 CPU Adam on the
same inputs.  Cases pool >= ~1000 elements so that e32 is not 0 by accident."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as R
from h3d_amd import _lib, checkpoint, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _lib.H3dAdamTensor


# ---- the mirror -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.RULE_CASES))
def test_mirror_against_float64_adam_over_12_steps(name):
    c = R.RULE_CASES[name]
    params, grads = R.make_case(**c["case"])
    assert sum(p.size for p in params) >= 1000 and len(grads) == 12
    ref = R.run_mirror(params, grads, c.get("groups"), **c["hyper"])
    R.rule_check(name, (ref.p, ref.m, ref.v), params, grads, c.get("groups"), **c["hyper"])


def test_mirror_first_step_moves_by_lr_against_the_sign_of_the_gradient():
    rs = np.random.RandomState(0)
    p0 = rs.uniform(-1, 1, 257).astype(np.float32)
    g = (10.0 ** rs.uniform(-3, 1, 257) * rs.choice([-1.0, 1.0], 257)).astype(np.float32)
    lr, eps = 1e-3, 1e-8
    ref = R.run_mirror([p0], [[g]], lr=lr, eps=eps)
    # step 1: m / bc1 = g, sqrt(v / bc2) = |g|: p1 = p0 - lr g / (|g| + eps); the eps term is eps / |g| <= 1e-5 relative, the rest is
    # fp32 rounding of p (|p| <= 1: 6e-8) and of the quotient (a few 1e-7 relative of lr)
    want = p0.astype(np.float64) - lr * np.sign(g)
    tol = lr * (eps / np.abs(g).astype(np.float64)) + 1e-6 * lr + 1.2e-7
    assert (np.abs(ref.p[0] - want) <= tol).all()


def test_mirror_zero_gradient_leaves_the_parameter_unchanged():
    p0 = np.random.RandomState(1).uniform(-1, 1, 100).astype(np.float32)
    ref = R.run_mirror([p0], [[np.zeros(100, np.float32)]] * 3, lr=0.1)
    assert np.array_equal(ref.p[0], p0) and not ref.m[0].any() and not ref.v[0].any() and ref.t == [3]


# ---- the entry point --------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_declared():
    L = _lib.lib()
    assert hasattr(L, "h3d_adam_step") and "h3d_adam_step" in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "h3d.h")).read()
    assert re.search(r"^int h3d_adam_step\(const h3d_adam_tensor \*tensors[^)]*, int n_tensors, void \*stream\);", hdr, flags=re.M)
    assert "#define H3D_ADAM_CAPACITY %d\n" % _lib.ADAM_CAPACITY in hdr and "#define H3D_ADAM_CHUNK %d\n" % _lib.ADAM_CHUNK in hdr
    assert "#define H3D_ABI_VERSION 4 " in hdr
    # the descriptor: four pointers, int64 n, seven floats, padded to 8: the block of CAPACITY of them + the prefix table stays under 4 KB
    assert ctypes.sizeof(T) == 72 and T.n.offset == 32 and T.one_minus_b1.offset == 40 and T.weight_decay.offset == 64
    assert _lib.ADAM_CAPACITY * 72 + 4 * (_lib.ADAM_CAPACITY + 2) <= 4096


def good(n=4, base=0x1000):
    d = T()
    d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.n = base, base + 0x100, base + 0x200, base + 0x300, n
    d.one_minus_b1, d.b2, d.one_minus_b2, d.bc2_sqrt, d.eps, d.neg_step_size, d.weight_decay = 0.1, 0.999, 0.001, 0.03, 1e-8, -1e-3, 0.0
    return d


BAD = [
    ("null pointer", -5, dict(param=0)), ("null pointer", -5, dict(grad=0)), ("null pointer", -5, dict(exp_avg=0)),
    ("null pointer", -5, dict(exp_avg_sq=0)), ("n = -1", -1, dict(n=-1)),
    ("misaligned", -5, dict(param=0x1002)), ("misaligned", -5, dict(grad=0x1101)), ("misaligned", -5, dict(exp_avg=0x1203)),
    ("misaligned", -5, dict(exp_avg_sq=0x1302)),
    ("non-finite", -5, dict(one_minus_b1=float("nan"))), ("non-finite", -5, dict(b2=float("inf"))), ("non-finite", -5, dict(one_minus_b2=float("nan"))),
    ("non-finite", -5, dict(bc2_sqrt=float("inf"))), ("non-finite", -5, dict(eps=float("nan"))), ("non-finite", -5, dict(neg_step_size=float("-inf"))),
    ("non-finite", -5, dict(weight_decay=float("nan"))),
    ("out of range", -5, dict(b2=1.0)), ("out of range", -5, dict(b2=-0.5)), ("out of range", -5, dict(eps=-1e-8)),
    ("out of range", -5, dict(bc2_sqrt=0.0)), ("out of range", -5, dict(bc2_sqrt=-1.0)),
]


@pytest.mark.parametrize("msg,code,change", BAD, ids=["%s %s" % (m, "/".join(c)) for m, _, c in BAD])
def test_every_argument_check_returns_its_code_without_a_gpu(msg, code, change):
    L = _lib.lib()
    arr = (T * 2)(good(), good())              # the bad tensor is the second: every tensor is checked before anything is launched
    for k, v in change.items():
        setattr(arr[1], k, v)
    assert L.h3d_adam_step(arr, 2, None) == code
    err = L.h3d_last_error().decode()
    assert msg in err and "tensor 1" in err, err


def test_list_level_checks_and_the_calls_that_launch_nothing():
    L = _lib.lib()
    assert L.h3d_adam_step(None, -1, None) == -1 and "n_tensors" in L.h3d_last_error().decode()
    assert L.h3d_adam_step(None, 1, None) == -5 and "null tensor list" in L.h3d_last_error().decode()
    assert L.h3d_adam_step(None, 0, None) == 0
    empty = good(n=0)
    empty.param = empty.grad = empty.exp_avg = empty.exp_avg_sq = 0
    assert L.h3d_adam_step((T * 2)(empty, good(n=0)), 2, None) == 0
    with pytest.raises(RuntimeError, match="argument error"):
        _lib.check(L.h3d_adam_step((T * 1)(), 1, None), "h3d_adam_step")             # all-zero scalars: bc2_sqrt <= 0


def test_host_scalars_are_the_single_tensor_path_ones():
    got = optim.scalars(1.25e-4, 0.9, 0.999, 1e-8, 0.0, 3)
    assert got == (1 - 0.9, 0.999, 1 - 0.999, (1 - 0.999 ** 3) ** 0.5, 1e-8, -(1.25e-4 / (1 - 0.9 ** 3)), 0.0)
    d = T()
    d.one_minus_b1, d.bc2_sqrt = got[0], got[3]
    assert d.one_minus_b1 == float(np.float32(got[0])) and d.bc2_sqrt == float(np.float32(got[3]))      # rounded to float once, to nearest
    assert [float(x) for x in R.scalars(1.25e-4, (0.9, 0.999), 1e-8, 0.0, 3)] == [float(np.float32(x)) for x in got]


# ---- the optimiser class ----------------------------------------------------------------------------------------------------------------
def small_model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.ReLU(), torch.nn.Linear(7, 3))


def stepped_torch_adam(model, steps=3, **kw):
    opt = torch.optim.Adam(model.parameters(), **kw)
    g = torch.Generator().manual_seed(1)
    for _ in range(steps):
        opt.zero_grad()
        model(torch.randn(4, 5, generator=g)).square().sum().backward()
        opt.step()
    return opt


def assert_same_state(a, b):
    assert a["param_groups"] == b["param_groups"] and a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for n in a["state"][k]:
            x, y = a["state"][k][n], b["state"][k][n]
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), (k, n)


def test_constructor_defaults_and_state_layout_are_torch_adams():
    model = small_model()
    ours, theirs = optim.Adam(model.parameters()), torch.optim.Adam(model.parameters())
    assert isinstance(ours, torch.optim.Optimizer)
    for k in ("lr", "betas", "eps", "weight_decay"):
        assert ours.defaults[k] == theirs.defaults[k], k
    assert set(ours.param_groups[0]) <= set(theirs.param_groups[0]) and ours.state_dict()["state"] == {}


def test_state_dict_loads_into_torch_adam_and_back_with_equal_tensors():
    model = small_model()
    src = stepped_torch_adam(model, lr=1.25e-4, weight_decay=0.01)
    ours = optim.Adam(model.parameters())
    ours.load_state_dict(src.state_dict())
    assert_same_state(ours.state_dict(), src.state_dict())
    assert ours.param_groups[0]["lr"] == 1.25e-4 and ours.param_groups[0]["weight_decay"] == 0.01
    for p in model.parameters():
        st = ours.state[p]
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 3.0
    back = torch.optim.Adam(small_model(1).parameters())
    back.load_state_dict(ours.state_dict())
    assert_same_state(back.state_dict(), src.state_dict())
    # ... and torch goes on from it
    model2 = small_model(1)
    back2 = torch.optim.Adam(model2.parameters())
    back2.load_state_dict(ours.state_dict())
    model2(torch.ones(1, 5)).sum().backward()
    back2.step()
    assert float(back2.state[next(model2.parameters())]["step"]) == 4.0


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(foreach=True),
                                dict(fused=True), dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)),
                                dict(weight_decay=-1.0)], ids=lambda kw: next(iter(kw)))
def test_constructor_refuses_what_is_not_implemented(kw):
    with pytest.raises(ValueError):
        optim.Adam(small_model().parameters(), **kw)


def test_step_refusals():
    def with_grad(p):
        p = torch.nn.Parameter(p)
        p.grad = torch.ones_like(p)
        return p
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        optim.Adam([with_grad(torch.zeros(3))]).step()
    with pytest.raises(TypeError, match="float32"):
        optim.Adam([with_grad(torch.zeros(3, dtype=torch.float64))]).step()
    with pytest.raises(TypeError, match="float32"):
        optim.Adam([with_grad(torch.zeros(3, dtype=torch.bfloat16))]).step()
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.zeros(4, 3).to_sparse()
    with pytest.raises(TypeError, match="sparse"):
        optim.Adam([p]).step()
    q = torch.nn.Parameter(torch.zeros(4, 6)[:, ::2])
    q.grad = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="contiguous"):
        optim.Adam([q]).step()
    # a refused option that arrives through a loaded state is refused at the step
    model = small_model()
    src = stepped_torch_adam(model, amsgrad=True)
    ours = optim.Adam(model.parameters())
    ours.load_state_dict(src.state_dict())
    with pytest.raises(ValueError, match="amsgrad"):
        ours.step()
    # no gradient anywhere: nothing to do, nothing launched, the closure's value is returned
    assert optim.Adam(small_model().parameters()).step(lambda: 5.0) == 5.0


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_old_call_forms_are_unchanged(tmp_path, capsys):
    model = small_model()
    path = str(tmp_path / "m.pth")
    assert checkpoint.save_model(path, 3, model) is None
    assert set(torch.load(path, weights_only=False)) == {"epoch", "state_dict"}
    fresh = small_model(1)
    assert checkpoint.load_model(fresh, path) is fresh
    assert capsys.readouterr().out == "loaded {}, epoch 3\n".format(path)
    for a, b in zip(fresh.state_dict().values(), model.state_dict().values()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("epoch,factor", [(1, 1.0), (2, 0.1), (5, 0.1 * 0.1)])
def test_checkpoint_round_trip_resumes_the_optimiser_with_the_schedules_rate(tmp_path, capsys, epoch, factor):
    model = small_model()
    src = stepped_torch_adam(model, lr=1.25e-4)
    saver = optim.Adam(model.parameters(), lr=1.25e-4)
    saver.load_state_dict(src.state_dict())
    path = str(tmp_path / "m.pth")
    checkpoint.save_model(path, epoch, model, saver)
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer"} and ck["epoch"] == epoch
    fresh = small_model(1)
    opt = optim.Adam(fresh.parameters(), lr=1.25e-4)
    capsys.readouterr()
    m, o, start = checkpoint.load_model(fresh, path, opt, True, 1.25e-4, [2, 4])
    lr = 1.25e-4
    for s in (2, 4):
        if epoch >= s:
            lr *= 0.1
    assert m is fresh and o is opt and start == epoch
    assert [g["lr"] for g in opt.param_groups] == [lr] and abs(lr - 1.25e-4 * factor) <= 1e-18
    assert capsys.readouterr().out == "loaded {}, epoch {}\nResumed optimizer with start lr {}\n".format(path, epoch, lr)
    want = src.state_dict()
    want["param_groups"][0]["lr"] = lr
    assert_same_state(opt.state_dict(), want)
    for a, b in zip(fresh.state_dict().values(), model.state_dict().values()):
        assert torch.equal(a, b)
    # without resume the optimiser is left alone; the three values still come back
    opt2 = optim.Adam(fresh.parameters(), lr=1.25e-4)
    assert checkpoint.load_model(fresh, path, opt2) == (fresh, opt2, 0) and opt2.state_dict()["state"] == {}
    # the torch optimiser resumes from the same file
    opt3 = torch.optim.Adam(fresh.parameters(), lr=1.25e-4)
    assert checkpoint.load_model(fresh, path, opt3, True, 1.25e-4, [2, 4])[2] == epoch
    assert_same_state(opt3.state_dict(), want)


def test_checkpoint_without_optimiser_state_says_so(tmp_path, capsys):
    model = small_model()
    path = str(tmp_path / "m.pth")
    checkpoint.save_model(path, 7, model)
    opt = optim.Adam(model.parameters())
    capsys.readouterr()
    assert checkpoint.load_model(model, path, opt, True, 1e-3, [2, 4]) == (model, opt, 0)
    assert capsys.readouterr().out == "loaded {}, epoch 7\nNo optimizer parameters in checkpoint.\n".format(path)
    assert opt.param_groups[0]["lr"] == 1e-3
