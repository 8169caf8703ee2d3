"""The numpy mirror of csrc/optim.hip's Adam step (include/h3d.h section 7): float32 arrays, every line ONE IEEE binary32 operation in
the kernel's order; the scalars formed in Python doubles and rounded to float32 once.  numpy's float32 sqrt and divide are correctly
rounded and keep denormals, as the kernel's are.

    ref = MirrorAdam([p0, p1, ...], groups=[dict(params=[0, 1], lr=..., betas=..., eps=..., weight_decay=...), ...])
    ref.step([g0, None, ...])       # None = no gradient this step: the tensor's state and its own step count stay

and the yardstick of the fp64 rule (test_oracle_optim.py's docstring): torch.optim.Adam on float64 and on float32 CPU tensors."""
import math

import numpy as np
import torch

F = np.float32
DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)


def scalars(lr, betas, eps, weight_decay, t):
    b1, b2 = betas
    bc1 = 1 - b1 ** t
    bc2s = math.sqrt(1 - b2 ** t)
    step_size = lr / bc1
    return F(1 - b1), F(b2), F(1 - b2), F(bc2s), F(eps), F(-step_size), F(weight_decay)


def step_arrays(p, g, m, v, sc):
    """In place on float32 arrays p, m, v."""
    omb1, b2, omb2, bc2s, eps, nss, wd = sc
    with np.errstate(all="ignore"):
        if wd != 0:
            g = g + wd * p
        m += omb1 * (g - m)
        v *= b2
        v += (omb2 * g) * g
        den = np.sqrt(v) / bc2s + eps
        p += nss * (m / den)


class MirrorAdam:
    def __init__(self, params, groups=None, **hyper):
        self.p = [np.array(x, dtype=F).copy() for x in params]
        self.m = [np.zeros_like(x) for x in self.p]
        self.v = [np.zeros_like(x) for x in self.p]
        self.t = [0] * len(self.p)
        if groups is None:
            groups = [dict(params=list(range(len(self.p))), **hyper)]
        self.groups = [dict(DEFAULTS, **g) for g in groups]

    def step(self, grads):
        for grp in self.groups:
            for i in grp["params"]:
                if grads[i] is None:
                    continue
                self.t[i] += 1
                sc = scalars(grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"], self.t[i])
                step_arrays(self.p[i], np.asarray(grads[i], dtype=F), self.m[i], self.v[i], sc)


def torch_adam_run(params, grads_per_step, dtype, groups=None, **hyper):
    """torch.optim.Adam(foreach=False) on CPU tensors of `dtype` -> (p, exp_avg, exp_avg_sq) lists after the last step (float64 numpy)."""
    ps = [torch.tensor(np.asarray(x, dtype=np.float64), dtype=dtype, requires_grad=True) for x in params]
    if groups is None:
        spec = [dict(params=ps)]
        kw = dict(DEFAULTS, **hyper)
    else:
        spec = [dict({k: v for k, v in g.items() if k != "params"}, params=[ps[i] for i in g["params"]]) for g in groups]
        kw = dict(DEFAULTS)
    opt = torch.optim.Adam(spec, foreach=False, **kw)
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.tensor(np.asarray(g, dtype=np.float64), dtype=dtype)
        opt.step()
    z = [np.zeros(p.shape) for p in ps]
    get = lambda k: [opt.state[p][k].double().numpy() if p in opt.state and k in opt.state[p] else z[i] for i, p in enumerate(ps)]  # noqa: E731
    return [p.detach().double().numpy() for p in ps], get("exp_avg"), get("exp_avg_sq")


KINDS = ("param", "exp_avg", "exp_avg_sq")


def rule_check(name, got, params, grads_per_step, groups=None, report=None, **hyper):
    """The fp64 rule, per kind pooled over the case's tensors: max |x - x64| <= 4 e32 + 1e-7 max |x64|, e32 = the error of torch's own
    float32 CPU Adam on the same inputs.  got = (p list, m list, v list) of arrays.  -> {kind: err / e32}."""
    r64 = torch_adam_run(params, grads_per_step, torch.float64, groups, **hyper)
    r32 = torch_adam_run(params, grads_per_step, torch.float32, groups, **hyper)
    ratios = {}
    for kind, g, a64, a32 in zip(KINDS, got, r64, r32):
        cat = lambda xs: np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in xs])  # noqa: E731
        x, x64, x32 = cat(g), cat(a64), cat(a32)
        err, e32, top = float(np.abs(x - x64).max()), float(np.abs(x32 - x64).max()), float(np.abs(x64).max())
        ratios[kind] = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s: err %.3g e32 %.3g ratio %.3g (max |x64| %.3g)" % (name, kind, err, e32, ratios[kind], top))
        if report is not None:
            report[(name, kind)] = ratios[kind]
        assert err <= 4 * e32 + 1e-7 * top, (name, kind, err, e32, top)
    return ratios


# ---- the cases of the fp64 rule: >= ~1000 pooled elements each, 12 steps, gradient magnitudes 1e-3 .. 10 -------------------------------
def make_case(seed, sizes, steps=12, lo=-3.0, hi=1.0, none_at=()):
    """params ~ U(-1, 1); gradient magnitudes 10^U(lo, hi) with random signs, drawn anew per step.  none_at: {(step, tensor)} without a
    gradient."""
    rs = np.random.RandomState(seed)
    params = [rs.uniform(-1, 1, n).astype(F) for n in sizes]
    grads = []
    for s in range(steps):
        grads.append([None if (s, i) in none_at else (10.0 ** rs.uniform(lo, hi, n) * rs.choice([-1.0, 1.0], n)).astype(F)
                      for i, n in enumerate(sizes)])
    return params, grads


RULE_CASES = {
    "plain 4097": dict(case=dict(seed=1, sizes=[4097]), hyper=dict(lr=1.25e-4)),
    "heads-like mix": dict(case=dict(seed=2, sizes=[1, 2304, 64, 128, 2]), hyper=dict(lr=1.25e-4)),
    "weight decay": dict(case=dict(seed=3, sizes=[1500, 3]), hyper=dict(lr=1e-3, weight_decay=0.01)),
    "skipped steps": dict(case=dict(seed=4, sizes=[1200, 1100], none_at={(1, 1), (2, 1), (7, 0)}), hyper=dict(lr=1.25e-4)),
    "two groups": dict(case=dict(seed=5, sizes=[1300, 1400]), hyper={},
                       groups=[dict(params=[0], lr=1.25e-4), dict(params=[1], lr=1e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)]),
}


def run_mirror(params, grads_per_step, groups=None, **hyper):
    ref = MirrorAdam(params, groups, **hyper)
    for grads in grads_per_step:
        ref.step(grads)
    return ref
