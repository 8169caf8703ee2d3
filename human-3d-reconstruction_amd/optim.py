"""The optimiser of the reference trainer, `torch.optim.Adam(model.parameters(), opt.lr)` (trains/trainer.py:166), on the device in
one launch per step (csrc/optim.hip, include/h3d.h section 7).

`Adam` keeps torch.optim.Adam's constructor defaults and its state layout -- state[p] = {'step': CPU float tensor, 'exp_avg',
'exp_avg_sq'}, created on a parameter's first gradient -- so state_dict() / load_state_dict() / param_groups / zero_grad() are torch's
own and a checkpoint written by either optimiser loads into the other.  What the kernel does not implement is refused, never computed
some other way."""
import math

import torch

from . import _lib
from ._lib import H3dAdamTensor

_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "foreach", "fused")


def scalars(lr, beta1, beta2, eps, weight_decay, step):
    """(one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, neg_step_size, weight_decay) of a tensor at its `step`-th step (>= 1): formed in
    Python doubles as torch.optim.Adam's single-tensor path forms them, each rounded to float once by the descriptor."""
    bc1 = 1 - beta1 ** step
    bc2_sqrt = math.sqrt(1 - beta2 ** step)
    step_size = lr / bc1
    return (1 - beta1, beta2, 1 - beta2, bc2_sqrt, eps, -step_size, weight_decay)


def fill(desc, param, grad, exp_avg, exp_avg_sq, values):
    """One h3d_adam_tensor from four device tensors of the same number of elements and scalars(...)."""
    desc.param, desc.grad, desc.exp_avg, desc.exp_avg_sq = param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()
    desc.n = param.numel()
    (desc.one_minus_b1, desc.b2, desc.one_minus_b2, desc.bc2_sqrt, desc.eps, desc.neg_step_size, desc.weight_decay) = values


def launch(descs, n=None):
    """h3d_adam_step over a ctypes array of H3dAdamTensor on torch's current stream."""
    n = len(descs) if n is None else n
    if n == 0:
        return
    _lib.check(_lib.lib().h3d_adam_step(descs, n, _lib.stream_ptr()), "h3d_adam_step")


def _check_tensor(t, what):
    if t.is_sparse or t.layout != torch.strided:
        raise TypeError("Adam: sparse %s are not supported" % what)
    if t.dtype != torch.float32:
        raise TypeError("Adam: %s must be float32, got %s" % (what, t.dtype))


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None):
        given = dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable, foreach=foreach, fused=fused)
        for k in _REFUSED:
            if given[k]:
                raise ValueError("Adam: %s is not implemented" % k)
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("Adam: lr and betas must be Python floats")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        # the keys of torch.optim.Adam's groups, so that a state_dict of this class is one of that class
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group in self.param_groups:
            for k in _REFUSED:
                if group.get(k):
                    raise ValueError("Adam: %s is not implemented (set by a loaded state or a param group)" % k)
            if group.get("decoupled_weight_decay"):
                raise ValueError("Adam: decoupled_weight_decay (AdamW) is not implemented")
            beta1, beta2 = group["betas"]
            lr = group["lr"]
            if isinstance(lr, torch.Tensor):
                raise ValueError("Adam: lr must be a Python float")
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad
                _check_tensor(p, "parameters")
                _check_tensor(grad, "gradients")
                if not p.is_contiguous():
                    raise ValueError("Adam: parameters must be contiguous")
                _lib.require_cuda(p, grad)
                if not grad.is_contiguous():
                    grad = grad.contiguous()
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                for t in (m, v):
                    _check_tensor(t, "optimiser states")
                    if not t.is_contiguous() or t.numel() != p.numel():
                        raise ValueError("Adam: an optimiser state must be contiguous and of its parameter's size")
                    _lib.require_cuda(t)
                if not torch.is_tensor(state["step"]):
                    state["step"] = torch.tensor(float(state["step"]), dtype=torch.float32)
                work.append((p, grad, m, v, state, (float(lr), beta1, beta2, group["eps"], group["weight_decay"])))
        # nothing is advanced before every tensor has passed its checks
        descs = (H3dAdamTensor * max(len(work), 1))()
        formed = {}                                  # (hyper-parameters, step) -> scalars: the tensors of a group mostly share them
        if work:
            torch._foreach_add_([w[4]["step"] for w in work], 1)     # one dispatch for all step counts (CPU scalars), as torch advances them
        for d, (p, grad, m, v, state, hyper) in zip(descs, work):
            key = hyper + (state["step"].item(),)
            if key not in formed:
                formed[key] = scalars(*key)
            fill(d, p, grad, m, v, formed[key])
        launch(descs, len(work))
        return loss
