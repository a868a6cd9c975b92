"""Native norms on MI355X: GraphNorm, and BatchNorm1d / LayerNorm over node features.

``GraphBatchNorm`` / ``GraphLayerNorm`` / ``GetNorm`` are drop-ins for ``models/norm.py:53-60,68-82``:
torch's own constructors and ``state_dict`` keys, ``forward(graphs, feats)`` or ``forward(feats)``, and
``forward_act(graphs, feats, activation, resid)`` = ``activation(norm(feats)) + resid`` in one pass per
direction (``sir_batch_norm_*`` / ``sir_layer_norm_*``), which ``SIRStack`` picks up.  ``forward_act(...,
dropout=(seed, p))`` puts the layer's ``nn.Dropout`` between the activation and the residual add in the same
pass (``sir_*_norm_act_drop_*``): a hashed mask that is never stored, recomputed by the backward.

Fused GraphNorm on MI355X — drop-in for the reference ``models/norm.py:7-29`` ``GraphNorm``.

Same constructor ``GraphNorm(normalized_shape, eps=1e-05, bias=True, mean_scale=True)``, same
parameters (``weight``, ``bias`` (or the int 0), ``mean_scale`` (or the int 1)) and
``forward(graphs, feats)`` over a batched graph (``graphs.batch_num_nodes()``; a DGLGraph or
``sirgcn.graph.batch([...])``).  Per graph: mean / variance of the mean_scale-shifted values,
exactly as the reference (the variance is taken of ``feats - mean * mean_scale``).  One native
kernel per direction (``sir_graph_norm_fwd`` / ``sir_graph_norm_bwd``) replaces the reference's
~8 torch kernels (scatter_add x2, repeat_interleave x2, elementwise).
"""
import torch
from torch import nn

from . import _native
from .graph import node_offsets


class GraphNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, weight, bias, mean_scale, off, eps):
        if X.device.type != "cuda":
            raise RuntimeError("sirgcn.GraphNorm needs a ROCm GPU tensor (no CPU fallback)")
        X = X.contiguous().float()
        B = off.numel() - 1
        F = X.shape[1]
        Y = torch.empty_like(X)
        mean = torch.empty((B, F), device=X.device, dtype=torch.float32)
        std = torch.empty_like(mean)
        w = weight.contiguous().float()
        b = bias.contiguous().float() if bias is not None else None
        ms = mean_scale.contiguous().float() if mean_scale is not None else None
        _native.graph_norm_fwd(off, X, w, b, ms, eps, Y, mean, std)
        ctx.save_for_backward(X, w, ms if ms is not None else w, mean, std, off)
        ctx.has_b, ctx.has_ms = bias is not None, mean_scale is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, w, ms, mean, std, off = ctx.saved_tensors
        ms = ms if ctx.has_ms else None
        dY = dY.contiguous().float()
        dX = torch.empty_like(X)
        # the per-graph partials of dw, db (and dms) as slabs of one [n, B, F] buffer, reduced over
        # the graphs by ONE launch (molecule batches are launch-bound: three column sums were six)
        parts = torch.empty((3 if ms is not None else 2,) + tuple(mean.shape), device=X.device, dtype=torch.float32)
        _native.graph_norm_bwd(off, X, dY, w, ms, mean, std, dX, parts[0], parts[2] if ms is not None else None,
                               parts[1])
        sums = parts.sum(1)
        dw = sums[0]
        db = sums[1] if ctx.has_b else None
        dms = sums[2] if ms is not None else None
        return dX, dw, db, dms, None, None


class GraphNormActFunction(torch.autograd.Function):
    """act(GraphNorm(X)) + R in one kernel per direction (``sir_graph_norm_act_fwd`` / ``_bwd``):
    the stack loop's ``norm -> activation -> + resid`` (ogbn-arxiv/model.py:65-73,
    ogbg-molhiv/model.py:76-84; R = None: zinc/model.py:54-55).  The same ops as the three torch
    calls, so the same bits; R's gradient is the incoming gradient itself.  ``drop`` = (seed, p) or None:
    the layer dropout between the activation and the add (``sir_graph_norm_act_drop_*``), its seed an int or
    a one-element int64 device tensor, kept on ``ctx`` so that the backward recomputes the same bits."""

    @staticmethod
    def forward(ctx, X, weight, bias, mean_scale, off, eps, act, slope, R, drop=None):
        X = X.contiguous().float()
        B = off.numel() - 1
        F = X.shape[1]
        Y = torch.empty_like(X)
        mean = torch.empty((B, F), device=X.device, dtype=torch.float32)
        std = torch.empty_like(mean)
        w = weight.contiguous().float()
        b = bias.contiguous().float() if bias is not None else None
        ms = mean_scale.contiguous().float() if mean_scale is not None else None
        Rc = R.contiguous() if R is not None else None
        _native.graph_norm_act_fwd(off, X, w, b, ms, eps, act, slope, Rc, Y, mean, std, drop)
        ctx.save_for_backward(X, w, b if b is not None else w, ms if ms is not None else w, mean, std, off)
        ctx.has_b, ctx.has_ms, ctx.has_r = bias is not None, mean_scale is not None, R is not None
        ctx.act, ctx.slope, ctx.drop = act, slope, drop
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, w, b, ms, mean, std, off = ctx.saved_tensors
        b = b if ctx.has_b else None
        ms = ms if ctx.has_ms else None
        dY = dY.contiguous().float()
        dX = torch.empty_like(X)
        parts = torch.empty((3 if ms is not None else 2,) + tuple(mean.shape), device=X.device, dtype=torch.float32)
        _native.graph_norm_act_bwd(off, X, dY, w, b, ms, mean, std, ctx.act, ctx.slope, dX, parts[0],
                                   parts[2] if ms is not None else None, parts[1], ctx.drop)
        sums = parts.sum(1)
        return (dX, sums[0], sums[1] if ctx.has_b else None, sums[2] if ms is not None else None, None, None, None,
                None, dY if ctx.has_r else None, None)


def _act_code(m):
    """(code, slope) of an activation module the fused kernel applies, else None."""
    if isinstance(m, nn.ReLU):
        return _native.ACT_RELU, 0.0
    if isinstance(m, nn.LeakyReLU):
        return _native.ACT_LEAKY, float(m.negative_slope)
    if isinstance(m, nn.Identity):
        return _native.ACT_IDENTITY, 0.0
    return None


def _hooked(*modules):
    """True when a hook waits on the call of any of ``modules`` (a fused pass would skip it)."""
    return any(len(h) for m in modules for h in (m._forward_pre_hooks, m._forward_hooks,
                                                 m._backward_hooks, m._backward_pre_hooks))


def _layer_drop(module, dropout):
    """The (seed, p) a fused pass applies, or None: the layer dropout acts in training with p > 0 only (eval
    mode and p == 0 take the entries without it)."""
    if dropout is None or not module.training:
        return None
    seed, p = dropout
    p = float(p)
    if p != p or p < 0.0 or p > 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    return (seed, p) if p > 0.0 else None


class GraphNorm(nn.Module):
    """``models/norm.py:7-29`` GraphNorm, fused (see module docstring)."""

    def __init__(self, normalized_shape, eps=1e-05, bias=True, mean_scale=True):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape)) if bias else 0
        self.mean_scale = nn.Parameter(torch.ones(normalized_shape)) if mean_scale else 1

    def forward(self, graphs, feats):
        if feats.dim() != 2:
            raise ValueError("GraphNorm expects [num_nodes, features]")
        off = node_offsets(graphs, feats.device)
        b = self.bias if isinstance(self.bias, torch.Tensor) else None
        ms = self.mean_scale if isinstance(self.mean_scale, torch.Tensor) else None
        return GraphNormFunction.apply(feats, self.weight, b, ms, off, float(self.eps))

    def forward_act(self, graphs, feats, activation, resid=None, dropout=None):
        """``activation(self(graphs, feats)) + resid`` (resid None: no add) in one kernel per
        direction, or None when the activation / operands are not the fused kernel's, or a hook
        waits on either module's call (the caller then runs the three steps itself).  ``dropout`` =
        (seed, p): ``dropout(activation(...)) + resid`` in training, the seed an int or a one-element
        int64 device tensor (a captured step then draws fresh bits on every replay)."""
        code = _act_code(activation)
        hooked = _hooked(self, activation)
        if (code is None or hooked or feats.dim() != 2 or not feats.is_cuda
                or (resid is not None and (resid.dtype != torch.float32 or resid.shape != feats.shape))):
            return None
        off = node_offsets(graphs, feats.device)
        b = self.bias if isinstance(self.bias, torch.Tensor) else None
        ms = self.mean_scale if isinstance(self.mean_scale, torch.Tensor) else None
        return GraphNormActFunction.apply(feats, self.weight, b, ms, off, float(self.eps), code[0], code[1], resid,
                                          _layer_drop(self, dropout))


def _rows(t, N):
    """``t`` [M, N] with unit-stride rows at least N apart (a column slice of a wider tensor stays a view)."""
    return t if t.stride(1) == 1 and t.stride(0) >= N else t.contiguous()


class BatchNormActFunction(torch.autograd.Function):
    """act(BatchNorm1d(X)) + R: ``sir_batch_norm_stats`` (training: the batch statistics and the running
    buffers' update in one launch) and one apply pass; the backward is a reduce pass and an apply pass.
    Saves X and the [N] statistics only — y is recomputed; R's gradient is the incoming gradient itself.
    ``drop`` = (seed, p) or None: the layer dropout between the activation and the add, as
    :class:`GraphNormActFunction` (``sir_batch_norm_act_drop_*``; the statistics pass is the same)."""

    @staticmethod
    def forward(ctx, X, weight, bias, running_mean, running_var, training, momentum, eps, act, slope, R, drop=None):
        M, N = X.shape
        X = _rows(X, N)
        w, b = weight.contiguous(), bias.contiguous()
        Y = torch.empty((M, N), device=X.device, dtype=torch.float32)
        if training:
            mean = torch.empty((N,), device=X.device, dtype=torch.float64)     # the [N] statistics are fp64
            invstd = torch.empty_like(mean)
            if M > 0:
                _native.batch_norm_stats(X, eps, momentum, running_mean, running_var, mean, invstd,
                                         _native.batch_norm_work(M, N, X.device))
        else:
            mean, invstd = running_mean.double(), torch.rsqrt(running_var.double() + eps)
        if M > 0:
            _native.batch_norm_act_fwd(X, mean, invstd, w, b, act, slope, _rows(R, N) if R is not None else None, Y,
                                       drop)
        ctx.save_for_backward(X, w, b, mean, invstd)
        ctx.cfg = (bool(training), act, slope, R is not None)
        ctx.drop = drop
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, w, b, mean, invstd = ctx.saved_tensors
        training, act, slope, has_r = ctx.cfg
        M, N = X.shape
        dY = _rows(dY.float(), N)
        dX = torch.empty((M, N), device=X.device, dtype=torch.float32)
        if M > 0:
            dw = torch.empty((N,), device=X.device, dtype=torch.float32)
            db = torch.empty_like(dw)
            work = _native.batch_norm_work(M, N, X.device)
            _native.batch_norm_act_bwd(X, dY, mean, invstd, w, b, act, slope, training, dX, dw, db, work, ctx.drop)
        else:
            dw = torch.zeros((N,), device=X.device, dtype=torch.float32)
            db = torch.zeros_like(dw)
        return dX, dw, db, None, None, None, None, None, None, None, dY if has_r else None, None


class LayerNormActFunction(torch.autograd.Function):
    """act(LayerNorm(X)) + R in one pass per direction (``sir_layer_norm_act_fwd`` / ``_bwd``).  Saves X and
    the [M] mean / rstd only; R's gradient is the incoming gradient itself.  ``drop`` = (seed, p) or None: the
    layer dropout between the activation and the add, as :class:`GraphNormActFunction`
    (``sir_layer_norm_act_drop_*``)."""

    @staticmethod
    def forward(ctx, X, weight, bias, eps, act, slope, R, drop=None):
        M, N = X.shape
        X = _rows(X, N)
        w, b = weight.contiguous(), bias.contiguous()
        Y = torch.empty((M, N), device=X.device, dtype=torch.float32)
        mean = torch.empty((M,), device=X.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        if M > 0:
            _native.layer_norm_act_fwd(X, w, b, eps, act, slope, _rows(R, N) if R is not None else None, Y, mean, rstd,
                                       drop)
        ctx.save_for_backward(X, w, b, mean, rstd)
        ctx.cfg = (act, slope, R is not None)
        ctx.drop = drop
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, w, b, mean, rstd = ctx.saved_tensors
        act, slope, has_r = ctx.cfg
        M, N = X.shape
        dY = _rows(dY.float(), N)
        dX = torch.empty((M, N), device=X.device, dtype=torch.float32)
        dw, db = _native.layer_norm_act_bwd(X, dY, w, b, mean, rstd, act, slope, dX, ctx.drop)
        return dX, dw, db, None, None, None, dY if has_r else None, None


def _fusable(norm, activation, feats, resid):
    """(code, slope) when ``forward_act`` may run the fused pass on these operands, else None."""
    code = _act_code(activation)
    if (code is None or _hooked(norm, activation) or not feats.is_cuda or not norm._native_ok(feats)
            or (resid is not None and (resid.dtype != torch.float32 or resid.shape != feats.shape
                                       or resid.device != feats.device))):
        return None
    return code


class GraphBatchNorm(nn.BatchNorm1d):
    """``models/norm.py:53-55`` GraphBatchNorm / ``nn.BatchNorm1d``: torch's constructor and state_dict;
    ``forward(graphs, feats)`` or ``forward(feats)``.  A CUDA fp32 [M, N] input on the default-configured
    module (affine, tracked running statistics, a float momentum) runs the native kernels; every other
    configuration or input type runs torch's own forward.  No CPU fallback."""

    def _native_ok(self, feats):
        return (feats.dim() == 2 and feats.dtype == torch.float32 and self.affine and self.track_running_stats
                and self.momentum is not None and self.weight.dtype == torch.float32
                and feats.shape[1] == self.num_features)

    def _run(self, feats, code, resid, drop=None):
        if self.training:
            if feats.shape[0] == 1:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {feats.size()}")
            self.num_batches_tracked.add_(1)            # a device op: no host synchronisation
        return BatchNormActFunction.apply(feats, self.weight, self.bias, self.running_mean, self.running_var,
                                          self.training, float(self.momentum), float(self.eps), code[0], code[1],
                                          resid, drop)

    def forward(self, *args):
        feats = args[-1]
        if not feats.is_cuda:
            raise RuntimeError("sirgcn.GraphBatchNorm needs a ROCm GPU tensor (no CPU fallback)")
        if not self._native_ok(feats):
            return super().forward(feats)
        return self._run(feats, (_native.ACT_IDENTITY, 0.0), None)

    def forward_act(self, graphs, feats, activation, resid=None, dropout=None):
        """``activation(self(graphs, feats)) + resid`` (resid None: no add) in one pass per direction, or
        None when the activation / operands are not the fused kernel's, or a hook waits on either
        module's call (the caller then runs the three steps itself).  ``dropout`` = (seed, p): as
        :meth:`GraphNorm.forward_act`."""
        code = _fusable(self, activation, feats, resid)
        return None if code is None else self._run(feats, code, resid, _layer_drop(self, dropout))


class GraphLayerNorm(nn.LayerNorm):
    """``models/norm.py:58-60`` GraphLayerNorm / ``nn.LayerNorm`` over the feature dimension: as
    :class:`GraphBatchNorm`; native for an elementwise-affine module with N <= 1024."""

    def _native_ok(self, feats):
        return (feats.dim() == 2 and feats.dtype == torch.float32 and self.elementwise_affine
                and self.weight is not None and self.bias is not None and self.weight.dtype == torch.float32
                and len(self.normalized_shape) == 1 and feats.shape[1] == self.normalized_shape[0] <= 1024)

    def _run(self, feats, code, resid, drop=None):
        return LayerNormActFunction.apply(feats, self.weight, self.bias, float(self.eps), code[0], code[1], resid,
                                          drop)

    def forward(self, *args):
        feats = args[-1]
        if not feats.is_cuda:
            raise RuntimeError("sirgcn.GraphLayerNorm needs a ROCm GPU tensor (no CPU fallback)")
        if not self._native_ok(feats):
            return super().forward(feats)
        return self._run(feats, (_native.ACT_IDENTITY, 0.0), None)

    def forward_act(self, graphs, feats, activation, resid=None, dropout=None):
        """As :meth:`GraphBatchNorm.forward_act`."""
        code = _fusable(self, activation, feats, resid)
        return None if code is None else self._run(feats, code, resid, _layer_drop(self, dropout))


class GraphIdentity(nn.Identity):
    """``models/norm.py:63-65``: no norm, called as ``(graphs, feats)`` or ``(feats)``."""

    def forward(self, *args):
        return args[-1]


class GetNorm(nn.Module):
    """``models/norm.py:68-82``: the norm named 'gn' (GraphNorm, ``with_graph`` only), 'bn', 'ln' or 'none' as
    ``self.norm`` (so the reference's ``norm.*`` state_dict keys), called as ``(graphs, feats)`` when
    ``with_graph`` else ``(feats)``.  'cn' (ContraNorm) is not built."""

    def __init__(self, norm, with_graph, *args, **kwargs):
        super().__init__()
        norm_list = {"bn": GraphBatchNorm, "ln": GraphLayerNorm, "none": GraphIdentity}
        if with_graph:
            norm_list["gn"] = GraphNorm
        if norm == "cn":
            raise NotImplementedError("norm = cn (ContraNorm) is not built by sirgcn")
        if norm not in norm_list:
            raise NotImplementedError(f"norm = {norm} not implemented")
        self.norm = norm_list[norm](*args, **kwargs)

    def forward(self, *args):
        return self.norm(*args)

    def forward_act(self, graphs, feats, activation, resid=None, dropout=None):
        """The inner norm's fused ``forward_act`` when it has one and no hook waits on this wrapper."""
        fuse = getattr(self.norm, "forward_act", None)
        if fuse is None or _hooked(self):
            return None
        if dropout is None:
            return fuse(graphs, feats, activation, resid)
        return fuse(graphs, feats, activation, resid, dropout=dropout)
