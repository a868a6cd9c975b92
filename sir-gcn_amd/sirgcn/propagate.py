"""Native Correct & Smooth on MI355X: drop-ins for ``label_spreading`` and the correct / smooth steps of
``run()`` in the reference's ``ogbn-arxiv/correct_and_smooth.py`` (lines 41-58 and 80, 86-96) — the
post-processing behind its best ogbn-arxiv number.

    smoothed = sirgcn.correct_and_smooth(graph, predictions, labels, train_idx)       # run()'s smoothed_y
    y = sirgcn.label_spreading(graph, y0, nprop=10, alpha=0.8, post_step=sirgcn.Clamp(0, 1))

One propagation step — ``update_all(copy_u, sum | mean)`` between the two norm multiplies, the mix with
``y0`` and the post step — is one native launch (``sir_label_prop_step``) over the destination CSR the
graph's plan already holds: a per-row gather-sum in edge order, no atomics, no ``[V, C]`` temporary, no
host synchronisation once the plan is built, so a whole C&S run captures into a HIP graph.  A row of at
most ``DEFAULT_CHUNK`` in-edges is the reference's CPU result bit for bit; longer rows are summed per
chunk and combined in chunk order (deterministic, tolerance-level).  The symmetric norm is the in-degree
normaliser on both sides, as the reference takes it (``in_degrees()`` for the source factor too).  No
autograd (the reference never differentiates through it).  CUDA fp32 runs the kernel; any other CUDA
dtype runs a torch composition with the same semantics.  No CPU fallback.
"""
import torch

from . import _native
from .graph import get_plan
from .readout import _rows


class Clamp:
    """Post step ``lambda x: x.clamp(lo, hi)``, fused into the step kernel (a NaN stays NaN)."""

    def __init__(self, lo, hi):
        self.lo, self.hi = float(lo), float(hi)

    def __call__(self, x):
        return x.clamp(self.lo, self.hi)


class FixRows:
    """Post step ``x[idx] = y[idx]`` (the reference's ``partial(fix_input, y=y, mask=idx)``), fused into the
    step kernel: the rows of ``idx`` (an index tensor or a boolean mask) are never gathered.  The ``[V]``
    uint8 flag is built once per device."""

    def __init__(self, y, idx):
        self.y, self.idx = y, idx
        self._flag = None

    def flag(self, V, device):
        if self._flag is None or self._flag.device != device or self._flag.numel() != V:
            idx = torch.as_tensor(self.idx).to(device)
            if idx.dtype is torch.bool:
                if idx.numel() != V:
                    raise ValueError(f"sirgcn.FixRows: a mask of {idx.numel()} rows, the input has {V}")
                f = idx.reshape(V).to(torch.uint8)
            else:       # index_fill_ takes its scalar as a kernel argument: nothing is copied from the host
                f = torch.zeros(V, dtype=torch.uint8, device=device).index_fill_(0, idx.reshape(-1).long(), 1)
            self._flag = f
        return self._flag

    def __call__(self, x):
        idx = torch.as_tensor(self.idx).to(x.device)
        x[idx] = self.y.to(x.dtype)[idx]
        return x


def _check(graph, y, what):
    V = int(graph.num_nodes())
    if y.dim() != 2 or y.shape[0] != V:
        raise ValueError(f"sirgcn.{what}: input of shape {tuple(y.shape)}, the graph needs [{V}, C]")
    if not y.is_cuda:
        raise RuntimeError(f"sirgcn.{what} needs a ROCm GPU tensor (no CPU fallback)")
    return V


def _spread_native(plan, y0, nprop, alpha, use_sym, post_step):
    csr = plan.dst
    V, F = y0.shape
    dev = y0.device
    Y0 = _rows(y0, F)
    agg = "sym" if use_sym else "mean"
    norm = plan.norms("sym")[0] if use_sym else None          # the in-degree normaliser on both sides
    beta = 1.0 - alpha                                        # in double; rounded to fp32 at the call
    post, lo, hi, fixed, Yfix = _native.LP_POST_NONE, 0.0, 0.0, None, None
    if isinstance(post_step, Clamp):
        post, lo, hi = _native.LP_POST_CLAMP, post_step.lo, post_step.hi
    elif isinstance(post_step, FixRows):
        if post_step.y.shape != y0.shape:
            raise ValueError(f"sirgcn.FixRows: y of shape {tuple(post_step.y.shape)}, the input is {tuple(y0.shape)}")
        post, fixed = _native.LP_POST_FIX, post_step.flag(V, dev)
        Yfix = _rows(post_step.y.to(dev, torch.float32), F)
    partial = torch.empty((csr.n_slots * F,), device=dev, dtype=torch.float32) if csr.n_splits else None
    bufs = (torch.empty((V, F), device=dev, dtype=torch.float32), torch.empty((V, F), device=dev, dtype=torch.float32))
    cur = Y0
    for i in range(nprop):
        out = bufs[i % 2]
        _native.label_prop_step(csr, cur, Y0, norm, agg, alpha, beta, out, post, lo, hi, fixed, Yfix, partial)
        if post == _native.LP_POST_NONE and post_step is not None:
            out = _rows(post_step(out), F)
        cur = out
    return cur


def _spread_composed(plan, y0, nprop, alpha, use_sym, post_step):
    """The same steps from torch ops (CUDA dtypes the kernel does not take): ``index_add_`` over the plan's
    CSR order, the norm rounded to the input's dtype."""
    csr = plan.dst
    V, F = y0.shape
    dev = y0.device
    src = csr.col.long()
    deg = plan.in_deg.to(dev)
    dst = torch.repeat_interleave(torch.arange(V, device=dev), deg, output_size=src.numel())
    degf = deg.clamp(min=1).to(y0.dtype)[:, None]
    norm = plan.norms("sym")[0].to(y0.dtype)[:, None] if use_sym else None    # the CPU's pow(deg, -0.5) bits
    y = y0
    for _ in range(nprop):
        m = y * norm if use_sym else y
        s = torch.zeros_like(y0).index_add_(0, dst, m[src])
        p = s * norm if use_sym else s / degf
        y = alpha * p + (1 - alpha) * y0
        if post_step is not None:
            y = post_step(y)
    return y


def label_spreading(graph, y0, nprop=10, alpha=0.1, use_sym=True, post_step=None):
    """``label_spreading`` of ``correct_and_smooth.py:41-58`` with its signature and defaults.  ``graph`` is
    anything :func:`sirgcn.get_plan` takes; ``post_step`` is ``None``, :class:`Clamp`, :class:`FixRows`
    (both run inside the step kernel) or any callable ``y -> y`` (run after each step, so the reference's
    own ``partial(fix_input, ...)`` and ``lambda x: x.clamp(0, 1)`` work unchanged).  ``y0`` is never
    written; ``nprop=0`` returns it."""
    _check(graph, y0, "label_spreading")
    if post_step is not None and not callable(post_step):
        raise TypeError("sirgcn.label_spreading: post_step must be None, Clamp, FixRows or a callable")
    if nprop <= 0 or y0.shape[1] == 0:
        return y0
    with torch.no_grad():
        plan = get_plan(graph, y0.device)
        spread = _spread_native if y0.dtype is torch.float32 else _spread_composed
        return spread(plan, y0, int(nprop), float(alpha), bool(use_sym), post_step)


def correct_and_smooth(graph, predictions, labels, train_idx, alpha_c=0.8, nprop_c=10, alpha_s=0.8, nprop_s=10,
                       use_sym=True, num_classes=None):
    """The correct and smooth steps of ``run()`` (``correct_and_smooth.py:80, 86-96``); returns its
    ``smoothed_y``.  ``predictions`` [V, C] (probabilities; not modified), ``labels`` [V] or [V, 1] integer
    classes, ``train_idx`` an index tensor.  ``num_classes`` defaults to ``predictions.shape[1]`` (the
    reference's ``torch.unique(labels)`` would be a host synchronisation)."""
    V = _check(graph, predictions, "correct_and_smooth")
    C = int(predictions.shape[1] if num_classes is None else num_classes)
    if C != predictions.shape[1]:
        raise ValueError(f"sirgcn.correct_and_smooth: {C} classes, predictions have {predictions.shape[1]} columns")
    dev = predictions.device
    labels = torch.as_tensor(labels)
    if labels.numel() != V:
        raise ValueError(f"sirgcn.correct_and_smooth: {labels.numel()} labels, the graph has {V} nodes")
    with torch.no_grad():
        train_idx = torch.as_tensor(train_idx).to(dev)
        lab = labels.to(dev).reshape(V)[train_idx].to(torch.int64)
        onehot = torch.zeros((lab.numel(), C), device=dev, dtype=predictions.dtype).scatter_(1, lab[:, None], 1.0)
        y = predictions.clone()
        # correct: spread the training residual, the training rows held at their residual
        dy = torch.zeros((V, C), device=dev, dtype=predictions.dtype)
        dy[train_idx] = onehot - y[train_idx]
        smoothed_dy = label_spreading(graph, dy, nprop=nprop_c, alpha=alpha_c, use_sym=use_sym,
                                      post_step=FixRows(dy, train_idx))
        y = y + alpha_c * smoothed_dy
        # smooth: spread the corrected predictions, the training rows set to their labels
        y[train_idx] = onehot
        return label_spreading(graph, y, nprop=nprop_s, alpha=alpha_s, use_sym=use_sym, post_step=Clamp(0, 1))
