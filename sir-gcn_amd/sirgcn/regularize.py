"""Native L1 / L2 parameter penalty on MI355X: drop-in for the ``regularizer(model, args)`` of the
reference's training loops (``benchmark-datasets/zinc/train.py:49-52`` and its six siblings),

    (args.l1 * sum_p sum|p| + args.l2 * sum_p sum p^2) * int(model.training)    over model.parameters()

    loss = loss_fn(preds, targets) + sirgcn.regularizer(model, args)

``param_norms(params) -> (l1, l2)`` computes the two sums over the whole list with one multi-tensor kernel
(``sir_param_norms_fwd``: one launch per ``sir_param_norms_max_tensors()`` tensors plus a one-block combine) and
their gradients with another (``sir_param_norms_bwd``: no combine), instead of about ten tiny launches per
parameter tensor.  Deterministic, no atomics, no host synchronisation, graph-capturable.  The gradients are
returned through autograd in the ordinary way (hooks, ``torch.autograd.grad``, DDP buckets and a ``GradScaler``
see them), bit for bit what autograd gives through the torch composition.

The native route is taken when every tensor is CUDA, fp32 and contiguous on one device (a view at a 4-byte
aligned offset counts); anything else — CPU, another dtype, a non-contiguous tensor, mixed devices — takes the
torch composition for the whole call.  ``param_norms.last_route`` says which one ran ("native" / "torch").
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native


def chunk_count(numels, chunk):
    """Chunks of a list: every tensor is cut into ``chunk``-element pieces counted from its own start."""
    return sum((n + chunk - 1) // chunk for n in numels)


def slot_layout(numels, needs):
    """Offsets (in floats) of the gradient slots inside one flat fp32 buffer, every slot at a multiple of 4
    floats (16 bytes); None for a tensor without a slot.  Returns (offsets, total floats)."""
    offs, total = [], 0
    for n, need in zip(numels, needs):
        if not need:
            offs.append(None)
            continue
        offs.append(total)
        total += (n + 3) // 4 * 4
    return offs, total


class _Plan:
    """The host arrays of one parameter list: device addresses and element counts as ctypes arrays (what
    ``sir_param_norms_fwd`` / ``_bwd`` read), the chunk count and the workspace size."""
    __slots__ = ("T", "numels", "params_arr", "numel_arr", "n_chunks", "work_floats", "layouts")

    def __init__(self, key):
        self.T = len(key)
        self.numels = [n for _, n in key]
        self.params_arr = (ctypes.c_void_p * max(self.T, 1))(*[ptr for ptr, _ in key])
        self.numel_arr = (ctypes.c_int64 * max(self.T, 1))(*self.numels)
        self.n_chunks = chunk_count(self.numels, _native.param_norms_chunk())
        self.work_floats = _native.param_norms_work_floats(self.n_chunks)
        self.layouts = {}

    def layout(self, needs):
        got = self.layouts.get(needs)
        if got is None:
            got = self.layouts[needs] = slot_layout(self.numels, needs)
        return got


_PLANS = {}
_PLANS_MAX = 16


def _plan(params):
    """The cached plan of this list: the key is the tuple of (data_ptr, numel), so a step does not rebuild
    the arrays and a parameter that moved (a new ``data_ptr``) gets new ones."""
    key = tuple((p.data_ptr(), p.numel()) for p in params)
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) >= _PLANS_MAX:
            _PLANS.pop(next(iter(_PLANS)))
        plan = _PLANS[key] = _Plan(key)
    return plan


class ParamNormsFunction(torch.autograd.Function):
    """(l1, l2) = (sum |p|, sum p^2) over the list (``sir_param_norms_fwd``); backward: one flat buffer of
    16-byte aligned slots filled by ``sir_param_norms_bwd``, returned as views shaped like their parameters."""

    @staticmethod
    def forward(ctx, plan, *params):
        dev = params[0].device
        out2 = torch.empty((2,), device=dev, dtype=torch.float32)
        work = torch.empty((plan.work_floats,), device=dev, dtype=torch.float32)
        _native.param_norms_fwd(plan.params_arr, plan.numel_arr, plan.T, work, out2)
        ctx.plan = plan
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*params)
        return out2.unbind(0)

    @staticmethod
    @once_differentiable
    def backward(ctx, g1, g2):
        plan, params = ctx.plan, ctx.saved_tensors
        needs = tuple(ctx.needs_input_grad[1:])
        if (g1 is None and g2 is None) or not any(needs):
            return (None,) * (1 + plan.T)
        dev = params[0].device
        offs, total = plan.layout(needs)
        buf = torch.empty((total,), device=dev, dtype=torch.float32)
        base = buf.data_ptr()
        grads_arr = (ctypes.c_void_p * plan.T)(*[None if o is None else base + 4 * o for o in offs])
        g1 = None if g1 is None else g1.to(device=dev, dtype=torch.float32)
        g2 = None if g2 is None else g2.to(device=dev, dtype=torch.float32)
        _native.param_norms_bwd(plan.params_arr, plan.numel_arr, grads_arr, plan.T, g1, g2, dev)
        return (None,) + tuple(None if o is None else buf[o:o + n].view(p.shape)
                               for o, n, p in zip(offs, plan.numels, params))


def _composed(params):
    """The same two sums from torch ops: per-tensor sums, stacked and summed (on the first tensor's device)."""
    dev = params[0].device
    l1 = torch.stack([p.abs().sum().to(dev) for p in params]).sum()
    l2 = torch.stack([p.pow(2).sum().to(dev) for p in params]).sum()
    return l1, l2


def _native_ok(params):
    dev = params[0].device
    if dev.type != "cuda":
        return False
    for p in params:
        if p.device != dev or p.dtype is not torch.float32 or not p.is_contiguous():
            return False
    return True


def param_norms(params):
    """``(l1, l2) = (sum_p sum |p|, sum_p sum p^2)`` over an iterable of tensors: two 0-dim tensors,
    differentiable once.  Duplicates are taken as given (``model.parameters()`` already deduplicates); a frozen
    parameter counts in the sums and gets no gradient.  An empty list gives zeros."""
    params = tuple(params)
    if not params:
        param_norms.last_route = "native"
        return torch.zeros(()), torch.zeros(())
    if not _native_ok(params):
        param_norms.last_route = "torch"
        return _composed(params)
    param_norms.last_route = "native"
    plan = _plan(params)
    if plan.n_chunks == 0:                     # no element anywhere: the kernels would be no-ops
        z = torch.zeros((2,), device=params[0].device, dtype=torch.float32)
        return z[0], z[1]
    return ParamNormsFunction.apply(plan, *params)


param_norms.last_route = None


def regularizer(model, args):
    """The reference's ``regularizer(model, args)``: ``(args.l1 * l1 + args.l2 * l2) * int(model.training)``
    over ``model.parameters()``.  The scalar arithmetic is torch's, and the multiply by ``int(model.training)``
    is kept: a NaN parameter gives NaN in eval mode too, as in the reference."""
    l1, l2 = param_norms(model.parameters())
    return (args.l1 * l1 + args.l2 * l2) * int(model.training)
