"""GPU: `h3d_adam_step` (csrc/optim.hip), `optim.Adam`, `trainer.HeadsTrainer` and the optimiser half of `checkpoint`.

The device must have the BITS of the numpy mirror (tests/optim_ref.py: every line one IEEE binary32 operation in the kernel's order) on
param, exp_avg and exp_avg_sq after each of 5 steps -- whichever access path an element takes (16-byte body, 4-byte head / tail, 4-byte
only for bases that disagree inside 16 bytes).  Only the case whose exp_avg_sq is subnormal is held to the fp64 rule of
test_oracle_optim.py instead (and reports whether it was bit-equal all the same).

End to end (`test_five_train_steps...`): the device loss series against the CPU restatement (heads_grad_ref + losses_ref +
torch.optim.Adam on float32) is held to what tests/test_gpu_heads_backward.py's SGD test holds its series to -- finite, and the loss
after five steps below the first -- and both series are printed.  Adam moves every parameter by about lr per step whatever its
gradient's size, so a gradient element near zero whose sign differs between two correct fp32 implementations sends them apart by
2 lr: no bound tighter than that could be derived for the losses themselves."""
import random
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import heads_grad_ref as HR
import losses_ref as LR
import optim_ref as R
import targets_ref
from gpu_helpers import DEV
from h3d_amd import _lib, arch, model, optim, synth, train_input, trainer

pytestmark = pytest.mark.gpu
CH, CAP = _lib.ADAM_CHUNK, _lib.ADAM_CAPACITY
SENT = 777.0
STEPS = 5


def dev_param(a):
    return torch.nn.Parameter(torch.from_numpy(np.asarray(a, np.float32)).to(DEV))


def same(t, a, nan_ok=False):
    """Device tensor against a mirror array: torch.equal; with nan_ok NaNs must sit at the same places (their payload is not compared)
    and everything else, infinities included, must be equal."""
    t, a = t.detach().cpu().reshape(-1), torch.from_numpy(np.asarray(a)).reshape(-1)
    if not nan_ok:
        return torch.equal(t, a)
    nt, na = torch.isnan(t), torch.isnan(a)
    return torch.equal(nt, na) and torch.equal(torch.where(nt, torch.zeros_like(t), t), torch.where(na, torch.zeros_like(a), a))


def drive(params, grads_per_step, groups=None, place=dev_param, nan_ok=False, opt=None, ps=None, ref=None, **hyper):
    """`grads_per_step` through optim.Adam on the device and through the mirror, compared after every step.  -> (opt, ps, ref)."""
    if ps is None:
        ps = [place(a) for a in params]
    if opt is None:
        spec = ps if groups is None else [dict({k: v for k, v in g.items() if k != "params"}, params=[ps[i] for i in g["params"]]) for g in groups]
        opt = optim.Adam(spec, **hyper)
    if ref is None:
        ref = R.MirrorAdam(params, groups, **hyper)
    for s, grads in enumerate(grads_per_step):
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(np.asarray(g, np.float32)).to(DEV)
        opt.step()
        ref.step(grads)
        torch.cuda.synchronize()
        for i, p in enumerate(ps):
            assert same(p, ref.p[i], nan_ok), ("param", s, i)
            if ref.t[i]:
                st = opt.state[p]
                assert same(st["exp_avg"], ref.m[i], nan_ok), ("exp_avg", s, i)
                assert same(st["exp_avg_sq"], ref.v[i], nan_ok), ("exp_avg_sq", s, i)
                assert float(st["step"]) == ref.t[i] and st["step"].device.type == "cpu"
            else:
                assert p not in opt.state or len(opt.state[p]) == 0
    return opt, ps, ref


# ---- sizes and access paths --------------------------------------------------------------------------------------------------------------
def test_sizes_around_the_chunk():
    params, grads = R.make_case(21, [1, 2, 3, 5, CH - 1, CH, CH + 1, 4 * CH + 3], steps=STEPS)
    drive(params, grads, lr=1.25e-4)


def test_parameter_that_starts_one_element_into_its_storage():
    sizes = [1, 6, CH + 2]
    params, grads = R.make_case(22, sizes, steps=STEPS)

    stores = []

    def place(a):
        store = torch.full((a.size + 1,), SENT, device=DEV)
        store[1:] = torch.from_numpy(a).to(DEV)
        stores.append(store)
        p = torch.nn.Parameter(store[1:])
        assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        return p
    drive(params, grads, place=place, lr=1e-3)
    assert all(float(st[0]) == SENT for st in stores)               # the element in front of the view


def raw_case(n, offs, steps=2, hyper=(1e-3, 0.9, 0.999, 1e-8, 0.01), seed=0, PAD=8):
    """One tensor through the raw entry point: its four buffers sit `offs` floats behind a 16-byte boundary inside sentinel-filled
    allocations.  Bits against the mirror and sentinels on both sides of all four after every step."""
    params, grads = R.make_case(seed + n, [n], steps=steps)
    bufs = [torch.full((n + 2 * PAD + 4,), SENT, device=DEV) for _ in range(4)]
    views = [b[PAD + o:PAD + o + n] for b, o in zip(bufs, offs)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    p, g, m, v = views
    p.copy_(torch.from_numpy(params[0]))
    m.zero_(), v.zero_()
    ref = R.MirrorAdam(params, lr=hyper[0], betas=hyper[1:3], eps=hyper[3], weight_decay=hyper[4])
    for s in range(steps):
        g.copy_(torch.from_numpy(grads[s][0]))
        d = (_lib.H3dAdamTensor * 1)()
        optim.fill(d[0], p, g, m, v, optim.scalars(*hyper, step=s + 1))
        optim.launch(d)
        ref.step(grads[s])
        torch.cuda.synchronize()
        assert same(p, ref.p[0]) and same(m, ref.m[0]) and same(v, ref.v[0]) and same(g, grads[s][0]), (n, offs, s)
        for b, o in zip(bufs, offs):
            assert bool((b[:PAD + o] == SENT).all()) and bool((b[PAD + o + n:] == SENT).all()), (n, offs, s)


SIZES = (1, 2, 3, 4, 5, 7, CH - 1, CH, CH + 1, CH + 6, 4 * CH + 3)


@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 1, 2, 3), (1, 0, 0, 0), (0, 0, 0, 2), (4, 0, 8, 12)],
                         ids=lambda o: "p%d g%d m%d v%d" % o)
def test_aligned_shared_and_mixed_offsets_with_sentinels_behind_all_four_buffers(offs):
    for n in SIZES:
        raw_case(n, offs)


def test_more_tensors_than_one_launch_holds():
    sizes = [1 + i % 5 for i in range(CAP + 1)]
    params, grads = R.make_case(23, sizes, steps=STEPS)
    drive(params, grads, lr=1e-3)
    # ... and two full blocks and a rest, with empty tensors in between that take no slot
    sizes = [(1 + i % 5) if i % 7 else 0 for i in range(2 * CAP + 20)]
    params, grads = R.make_case(24, sizes, steps=2)
    drive(params, grads, lr=1e-3)


def test_empty_parameter():
    params, grads = R.make_case(25, [0, 5, 0], steps=STEPS)
    opt, ps, _ = drive(params, grads, lr=1e-3)
    assert float(opt.state[ps[0]]["step"]) == STEPS and opt.state[ps[0]]["exp_avg"].numel() == 0
    drive(*R.make_case(26, [0], steps=2), lr=1e-3)                  # nothing but an empty tensor: nothing is launched


def test_parameter_without_a_gradient_on_steps_2_and_3_keeps_its_state_and_its_own_count():
    params, grads = R.make_case(27, [33, CH + 1, 5], steps=STEPS, none_at={(1, 1), (2, 1)})
    ps = [dev_param(a) for a in params]
    opt = optim.Adam(ps, lr=1e-3)
    ref = R.MirrorAdam(params, lr=1e-3)
    drive(params, grads[:1], opt=opt, ps=ps, ref=ref)
    held = [t.clone() for t in (ps[1].detach(), opt.state[ps[1]]["exp_avg"], opt.state[ps[1]]["exp_avg_sq"])]
    drive(params, grads[1:3], opt=opt, ps=ps, ref=ref)
    assert all(torch.equal(a, b) for a, b in zip(held, (ps[1].detach(), opt.state[ps[1]]["exp_avg"], opt.state[ps[1]]["exp_avg_sq"])))
    drive(params, grads[3:], opt=opt, ps=ps, ref=ref)
    assert [float(opt.state[p]["step"]) for p in ps] == [5.0, 3.0, 5.0] and ref.t == [5, 3, 5]


def test_two_parameter_groups_with_their_own_hyperparameters():
    groups = [dict(params=[0, 2], lr=1.25e-4), dict(params=[1], lr=1e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)]
    params, grads = R.make_case(28, [CH + 3, 2 * CH + 1, 7], steps=STEPS)
    drive(params, grads, groups=groups)


def test_gradients_from_1e_minus_6_to_1e3():
    params, grads = R.make_case(29, [3 * CH + 1], steps=STEPS, lo=-6.0, hi=3.0)
    drive(params, grads, lr=1e-3, weight_decay=1e-2)


def test_nan_and_inf_gradient_elements_propagate_as_in_the_mirror_and_reach_no_neighbour():
    n = CH + 9
    params, grads = R.make_case(30, [n], steps=STEPS)
    clean = [[g[0].copy()] for g in grads]
    bad = {0: np.nan, 3: np.inf, 4: -np.inf, 5: np.nan, CH - 1: np.inf, CH: np.nan, n - 1: -np.inf}      # body, both sides of a vector and a chunk edge, tail
    for k, x in bad.items():
        grads[1][0][k] = x
    opt, ps, ref = drive(params, grads, nan_ok=True, lr=1e-3)
    assert np.isnan(ref.p[0][list(bad)]).all()
    # every other element has the bits of the run without them
    _, qs, _ = drive(params, clean, lr=1e-3)
    keep = torch.ones(n, dtype=torch.bool)
    keep[list(bad)] = False
    for a, b in ((ps[0], qs[0]),):
        assert torch.equal(a.detach().cpu()[keep], b.detach().cpu()[keep]) and bool(torch.isfinite(a.detach().cpu()[keep]).all())


def test_subnormal_second_moment_by_the_fp64_rule():
    rs = np.random.RandomState(11)
    n = 1500
    params = [rs.uniform(-1, 1, n).astype(np.float32)]
    grads = [[(10.0 ** rs.uniform(-19.5, -18.5, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)] for _ in range(STEPS)]
    ps = [dev_param(params[0])]
    opt = optim.Adam(ps, lr=1.25e-4)
    ref = R.run_mirror(params, grads, lr=1.25e-4)
    for g in grads:
        ps[0].grad = torch.from_numpy(g[0]).to(DEV)
        opt.step()
    st = opt.state[ps[0]]
    got = [[t.detach().cpu().numpy()] for t in (ps[0], st["exp_avg"], st["exp_avg_sq"])]
    assert 0 < got[2][0].max() < 1.1754944e-38, "exp_avg_sq is meant to be subnormal"
    print("subnormal case bit-equal to the mirror:", [bool(np.array_equal(a[0], b[0])) for a, b in zip(got, (ref.p, ref.m, ref.v))])
    R.rule_check("subnormal v", got, params, grads, lr=1.25e-4)


# ---- streams, repeatability, interchange with torch.optim.Adam -----------------------------------------------------------------------------
def final_bits(params, grads, **hyper):
    ps = [dev_param(a) for a in params]
    opt = optim.Adam(ps, **hyper)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g).to(DEV)
        opt.step()
    torch.cuda.synchronize()
    return [t.detach().clone() for p in ps for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]


def test_second_stream_and_a_second_optimiser_give_the_same_bits():
    params, grads = R.make_case(31, [5, 2 * CH + 3], steps=3)
    first = final_bits(params, grads, lr=1e-3)
    again = final_bits(params, grads, lr=1e-3)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        other = final_bits(params, grads, lr=1e-3)
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_load_state_dict_from_torch_adam_continues_with_the_mirrors_bits():
    params, grads = R.make_case(32, [7, CH + 5], steps=2 + STEPS)
    hyper = dict(lr=1e-3, betas=(0.85, 0.995), eps=1e-7, weight_decay=0.02)
    ts = [dev_param(a) for a in params]
    topt = torch.optim.Adam(ts, **hyper)
    for gs in grads[:2]:
        for p, g in zip(ts, gs):
            p.grad = torch.from_numpy(g).to(DEV)
        topt.step()
    ps = [dev_param(p.detach().cpu().numpy()) for p in ts]
    opt = optim.Adam(ps)                                            # the hyper-parameters arrive with the state
    opt.load_state_dict(topt.state_dict())
    ref = R.MirrorAdam([p.detach().cpu().numpy() for p in ts], **hyper)
    ref.m = [topt.state[p]["exp_avg"].cpu().numpy().copy() for p in ts]
    ref.v = [topt.state[p]["exp_avg_sq"].cpu().numpy().copy() for p in ts]
    ref.t = [2, 2]
    drive(None, grads[2:], opt=opt, ps=ps, ref=ref)
    assert [float(opt.state[p]["step"]) for p in ps] == [7.0, 7.0]
    # ... and back: torch goes on from this optimiser's state
    back = torch.optim.Adam([dev_param(p.detach().cpu().numpy()) for p in ps])
    back.load_state_dict(opt.state_dict())
    assert back.param_groups[0]["betas"] == (0.85, 0.995) and float(next(iter(back.state.values()))["step"]) == 7.0


def test_non_contiguous_gradient_is_copied_and_refusals_on_the_device():
    a = np.random.RandomState(33).uniform(-1, 1, (6, 5)).astype(np.float32)
    g = np.random.RandomState(34).uniform(-1, 1, (5, 6)).astype(np.float32)
    p = dev_param(a)
    p.grad = torch.from_numpy(g).to(DEV).t()
    assert not p.grad.is_contiguous()
    opt = optim.Adam([p], lr=1e-3)
    opt.step()
    ref = R.run_mirror([a], [[g.T.copy()]], lr=1e-3)
    torch.cuda.synchronize()
    assert same(p, ref.p[0]) and same(opt.state[p]["exp_avg"], ref.m[0])
    q = torch.nn.Parameter(torch.zeros(4, 6, device=DEV)[:, ::2])
    q.grad = torch.zeros(4, 3, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        optim.Adam([q]).step()
    h = torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))
    h.grad = torch.zeros_like(h)
    with pytest.raises(TypeError, match="float32"):
        optim.Adam([h]).step()


# ---- the trainer, end to end ---------------------------------------------------------------------------------------------------------------
HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}
HC = 64
LRS = (1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1)


def draw_head(seed, c, feat64, tries=400):
    """test_gpu_heads_backward.py's: head parameters in nn.Conv2d's default ranges whose pre-activations on `feat64` keep
    min |pre| >= 1e-5 max |pre|, searched on the CPU."""
    for s in range(seed, seed + tries):
        g = torch.Generator().manual_seed(s)
        w1 = (torch.rand(HC, 64, 3, 3, generator=g) * 2 - 1) / 24.0
        b1 = (torch.rand(HC, generator=g) * 2 - 1) / 24.0
        p = HR.pre_act(feat64, w1.double(), b1.double()).abs()
        if float(p.min()) >= 1e-5 * float(p.max()):
            return w1, b1, (torch.rand(c, HC, 1, 1, generator=g) * 2 - 1) / 8.0, torch.zeros(c)
    raise AssertionError("no head with a gate margin in %d tries" % tries)


def make_net():
    net = model.dla_net(HEADS, head_conv=HC, dtype="f32")
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True, HC), seed=0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.to(DEV)


def train_opt(lr):
    return NS(task="multi_pose", lr=lr, lr_step=[2, 4], num_iters=-1, input_res=64, output_res=16, not_rand_crop=False, aug_rot=0.0, rotate=0.0,
              flip=0.5, no_color_aug=False)


@pytest.fixture(scope="module")
def setting():
    """(batch, start head parameters on the CPU, feat32 on the CPU, the chosen lr, the restatement's 7 losses)."""
    sizes = [(48, 64), (40, 56)]
    rs = np.random.RandomState(13)
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    scenes = [targets_ref.scene(20 + b, 1, M=2, img_w=w, img_h=h, min_size=24.0, max_size=40.0) for b, (h, w) in enumerate(sizes)]
    boxes, kps = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    np.random.seed(17), random.seed(17)
    batch = train_input.multi_pose_train_batch([torch.from_numpy(i).to(DEV) for i in imgs], boxes, kps, [1, 1], train_opt(1e-3),
                                               data_rng=np.random.RandomState(123))
    # the regression losses scatter their gradients with float atomic adds: up to two adds into a zeroed cell commute, so with no cell
    # hit three times every gradient -- and with it the resumed run of the test below -- is bit-identical from run to run
    for ind, mask in (("ind", "reg_mask"), ("hp_ind", "hp_mask")):
        for b in range(len(sizes)):
            live = batch[ind][b][batch[mask][b] > 0]
            assert live.numel() > 0 and int(torch.bincount(live).max()) <= 2, (ind, b)
    tr = trainer.HeadsTrainer(train_opt(1e-3), make_net())
    feat64 = tr.heads.features(batch["input"]).cpu().double().contiguous()
    start = {}
    for i, (h, c) in enumerate(HEADS.items()):
        w1, b1, w2, b2 = draw_head(1000 * (i + 1), c, feat64)
        if h.startswith("hm"):
            b2 = torch.full((c,), -2.19)
        start[h] = [w1, b1, w2, b2]
    gold = {k: v.cpu() for k, v in batch.items() if torch.is_tensor(v)}
    feat32 = feat64.float()

    def cpu_losses(lr, steps=7):
        ps = {h: [t.clone().requires_grad_(True) for t in v] for h, v in start.items()}
        opt = torch.optim.Adam([t for v in ps.values() for t in v], lr=lr)
        vals = []
        for _ in range(steps):
            opt.zero_grad()
            o = {h: HR.forward(feat32, v[0], v[1], v[2].reshape(v[2].shape[0], -1), v[3]) for h, v in ps.items()}
            loss = LR.multi_pose(o, gold)[0]
            vals.append(float(loss.detach()))
            loss.backward()
            opt.step()
        return vals
    for lr in LRS:          # the smallest of the list that lowers the restatement's loss by >= 10 % in 5 steps
        cpu = cpu_losses(lr)
        if np.isfinite(cpu).all() and cpu[5] <= 0.9 * cpu[0]:
            return batch, start, lr, cpu
    raise AssertionError("no learning rate of %s lowers the restatement's loss by 10 %%: %s" % (LRS, cpu))


def fresh_trainer(lr, start):
    tr = trainer.HeadsTrainer(train_opt(lr), make_net())
    with torch.no_grad():
        for h, ps in tr.heads.head_params().items():
            for p, v in zip(ps, start[h]):
                p.copy_(v.to(DEV))
    return tr


def head_bits(tr):
    return [p.detach().clone() for ps in tr.heads.head_params().values() for p in ps]


def test_five_train_steps_lower_the_loss_as_the_restatement_does_and_a_resumed_run_has_the_sixth_steps_bits(setting, tmp_path):
    batch, start, lr, cpu = setting
    tr = fresh_trainer(lr, start)
    assert isinstance(tr.optimizer, optim.Adam) and len(list(tr.heads.parameters())) == 4 * len(HEADS)
    vals = []
    for _ in range(5):
        out, loss, stats = tr.train_step(dict(batch))
        vals.append(float(loss.detach()))
        assert set(stats) == set(tr.loss_stats) and set(out) == set(HEADS)
    path = str(tmp_path / "model_last.pth")
    tr.save_model(path, 5)
    with torch.no_grad():
        vals.append(float(tr.model_with_loss(dict(batch))[1]))
    print("Adam lr %g: cpu %s gpu %s" % (lr, cpu[:6], vals))
    assert np.isfinite(vals).all() and vals[5] < vals[0]
    assert all(float(tr.optimizer.state[p]["step"]) == 5.0 for p in tr.heads.parameters())
    # the uninterrupted run's sixth step
    tr.train_step(dict(batch))
    sixth = head_bits(tr)
    # a fresh trainer (other head parameters, no optimiser state) resumed from the checkpoint
    other = trainer.HeadsTrainer(train_opt(lr), make_net())
    assert other.load_model(path, resume=True) == 5
    assert other.optimizer.param_groups[0]["lr"] == lr * 0.1 * 0.1                     # lr_step [2, 4], epoch 5
    for g in other.optimizer.param_groups:
        g["lr"] = lr                                                                    # the uninterrupted run never dropped it
    other.train_step(dict(batch))
    torch.cuda.synchronize()
    for a, b in zip(head_bits(other), sixth):
        assert torch.equal(a, b)
    assert all(float(other.optimizer.state[p]["step"]) == 6.0 for p in other.heads.parameters())
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer"} and len(ck["optimizer"]["state"]) == 4 * len(HEADS)


def test_run_epoch_end_epoch_and_val(setting):
    batch, start, lr, _ = setting
    tr = fresh_trainer(lr, start)
    before = head_bits(tr)
    ret, results = tr.run_epoch("val", 0, [dict(batch)])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, head_bits(tr))) and len(tr.optimizer.state) == 0 and results == {}
    assert set(ret) == set(tr.loss_stats) | {"time"}
    first = ret["loss"]
    tr.opt.num_iters = 2
    ret, _ = tr.run_epoch("train", 1, [dict(batch)] * 3)                               # num_iters cuts the loader short
    assert all(float(tr.optimizer.state[p]["step"]) == 2.0 for p in tr.heads.parameters())
    # the running average, weighted by batch size, of the losses BEFORE each step: the first is the val loss
    again = fresh_trainer(lr, start)
    l0 = float(again.train_step(dict(batch))[1].detach())
    l1 = float(again.train_step(dict(batch))[1].detach())
    assert l0 == first and ret["loss"] == (l0 * 2 + l1 * 2) / 4 and ret["time"] >= 0
    assert tr.end_epoch(1) is None and tr.optimizer.param_groups[0]["lr"] == lr
    assert tr.end_epoch(2) == lr * 0.1 ** 1 and tr.optimizer.param_groups[0]["lr"] == lr * 0.1 ** 1
    assert tr.end_epoch(4) == lr * 0.1 ** 2 and tr.optimizer.param_groups[0]["lr"] == lr * 0.1 ** 2
    with pytest.raises(ValueError, match="task"):
        trainer.HeadsTrainer(NS(task="exdet", lr=lr), make_net())
