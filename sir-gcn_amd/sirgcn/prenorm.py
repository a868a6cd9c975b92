"""The pre-norm residual block of the reference's heterophilous configs (roman-empire, amazon-ratings,
minesweeper, tolokers, questions: ``heterophilous-datasets/model.py:12-55``, its only AMP results) on the MI355X.

The block puts the norm first and the dropout BEFORE the activation, which ``SIRStack`` cannot express::

    r = h
    h = norm(h)                   # GetNorm(norm, False, H)
    h = conv(graph, h)            # SIRConv, feat_dropout on Q / K
    h = GELU(drop(h))
    h = drop(linears[i](h))
    h = h + r                     # if residual

:func:`drop_act` is ``act(dropout(y)) + resid`` in one native pass per direction (``sir_drop_act_fwd`` /
``_bwd``): a hashed mask that is never stored (the bits ``sir_dropout_apply`` writes for an [M, N] block), recomputed
by the backward from ``y``, the only tensor it saves.  It replaces the dropout, the activation and the add of
torch — three launches forward, three or more backward and two stored masks per layer.

:class:`PreNormSIRModel` is the drop-in for the reference's ``SIRModel``: its constructor, attribute names and
``state_dict`` keys, with the three sites of the loop (input, after the conv, after the Linear) on :func:`drop_act`,
the Linears on the native GEMMs and every seed of a training step from one device draw.
"""
import torch
from torch import nn

from . import _native, linalg
from .conv import SIRConv, activation_code
from .norm import GetNorm, _hooked
from .resact import _ok

_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
SITE_BIT = 1 << 62        # set in every site's seed word; the convs' words stay below it


def _has_code(activation):
    """True when ``activation`` is one of the five the kernels apply (``sirgcn.activation_code``)."""
    try:
        activation_code(activation)
    except NotImplementedError:
        return False
    return True


def _dropout(dropout, training=True):
    """The (seed, p) a pass applies, or None (the convention of the norms' ``forward_act``): the dropout acts in
    training with p > 0 only."""
    if dropout is None or not training:
        return None
    seed, p = dropout
    p = float(p)
    if p != p or p < 0.0 or p > 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    return (seed, p) if p > 0.0 else None


class DropActFunction(torch.autograd.Function):
    """``act(dropout(Y)) + R`` (``sir_drop_act_fwd`` / ``_bwd``).  Saves Y only: the backward recomputes the mask and
    the dropout's output; R's gradient is the incoming gradient itself.  ``drop`` = (seed, p) or None, its seed an
    int or a one-element int64 device tensor, kept on ``ctx``."""

    @staticmethod
    def forward(ctx, Y, R, act, slope, drop=None):
        out = torch.empty(Y.shape, device=Y.device, dtype=R.dtype if R is not None else Y.dtype)
        _native.drop_act_fwd(Y, R, act, slope, out, drop)
        ctx.save_for_backward(Y)
        ctx.act, ctx.slope, ctx.drop, ctx.has_r = act, slope, drop, R is not None
        return out

    @staticmethod
    def backward(ctx, D):
        Y, = ctx.saved_tensors
        dY = None
        if ctx.needs_input_grad[0]:
            if not _ok(D, (D.dtype,)):
                D = D.contiguous()
            dY = torch.empty(Y.shape, device=Y.device, dtype=Y.dtype)
            _native.drop_act_bwd(D, Y, ctx.act, ctx.slope, dY, ctx.drop)
        return dY, D if ctx.has_r else None, None, None, None


def _composed(y, activation, resid, drop):
    """The same values from torch ops on the explicit mask ``sir_dropout_apply`` writes (any shape the native pass
    does not take, an activation without a code, a hooked activation module)."""
    if drop is not None:
        rows = (y.numel() // y.shape[-1] if y.shape[-1] else 0, y.shape[-1]) if y.dim() else (1, 1)
        m = _native.dropout_apply(torch.ones(rows, device=y.device, dtype=torch.float32), drop).view(y.shape)
        y = torch.where(m != 0, y * m, torch.zeros((), device=y.device, dtype=torch.float32)).to(y.dtype)
    if activation is not None:
        y = activation(y)
    return y if resid is None else y + resid


def drop_act(y, activation, resid=None, dropout=None, training=True):
    """``activation(dropout(y)) + resid`` — the dropout before the activation, ``resid`` optional.

    ``dropout`` = (seed, p) or None; the seed is an int or a one-element int64 device tensor (a captured step then
    draws a fresh mask on every replay).  p == 0, None and ``training=False`` give ``activation(y) + resid``; a p
    outside [0, 1] raises ``ValueError``.  ``activation`` is any form :func:`sirgcn.activation_code` maps (modules,
    ``F.gelu``, ``torch.relu``, None ...).  One native pass per direction when y is a CUDA fp32 / bf16 / fp16 [M, N]
    matrix with N % 4 == 0 and aligned unit-stride rows, resid is fp32 or y's 16-bit type, and no hook waits on
    the activation module; otherwise the same result from torch ops on the same mask.  No CPU fallback."""
    if not y.is_cuda or (resid is not None and not resid.is_cuda):
        raise RuntimeError("sirgcn.drop_act needs a ROCm GPU tensor (no CPU fallback)")
    drop = _dropout(dropout, training)
    code = activation_code(activation) if _has_code(activation) else None
    if isinstance(activation, nn.Module) and _hooked(activation):
        code = None
    # (an empty matrix has no row layout to speak of — torch hands its gradient over with any strides)
    native = (code is not None and y.dim() == 2 and y.shape[1] % 4 == 0 and y.shape[0] > 0 and _ok(y, _DTYPES)
              and (resid is None or (resid.shape == y.shape and resid.device == y.device
                                     and _ok(resid, (torch.float32, y.dtype)))))
    if not native:
        return _composed(y, activation, resid, drop)
    return DropActFunction.apply(y, resid, code[0], code[1], drop)


class PreNormSIRModel(nn.Module):
    """``heterophilous-datasets/model.py:12-55`` ``SIRModel``: the reference's constructor, attribute names and
    ``state_dict`` keys (a reference checkpoint loads), ``forward(graph, feats)`` on a DGLGraph or a
    ``sirgcn.Graph``.  After a training step with any dropout on, ``site_seeds`` holds the 2 * num_layers + 1
    seed words of its sites (input; per layer: after the conv, after the Linear), each with bit 62 set."""

    # the three sites of the loop on sirgcn.drop_act; False: torch's nn.Dropout, activation and add (the route the
    # fused one is measured against, tools/prenorm_bench.py)
    fused_tail = True

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers=1, input_dropout=0, dropout=0, norm='none',
                 residual=False, feat_dropout=0, agg_type='mean', **kwargs):
        super().__init__()
        self.num_layers = num_layers
        self.residual = residual
        self.input_linear = nn.Linear(input_dim, hidden_dim)
        self.input_drop = nn.Dropout(input_dropout)
        self.drop = nn.Dropout(dropout)
        self.activation = nn.GELU()

        self.norms = nn.ModuleList()
        self.convs = nn.ModuleList()
        self.linears = nn.ModuleList()

        for _ in range(num_layers):
            self.norms.append(GetNorm(norm, False, hidden_dim))
            self.convs.append(SIRConv(hidden_dim, hidden_dim, hidden_dim, self.activation, feat_dropout,
                                      agg_type=agg_type))
            self.linears.append(nn.Linear(hidden_dim, hidden_dim))

        self.output_norm = GetNorm(norm, False, hidden_dim)
        self.output_linear = nn.Linear(hidden_dim, output_dim)
        self.site_seeds = None

    def _draw(self, device):
        """Every seed word of this step in ONE device draw: the convs' (below 2^62, handed over as ``step_seed``),
        then the sites' (bit 62 set: a site hashes the (row, col) domain of a conv's Q dropout)."""
        self.site_seeds = None
        if not self.training:
            return
        drawing = [c for c in self.convs if hasattr(c, "step_seed") and c.dropout.p > 0]
        n_site = 2 * self.num_layers + 1 if self.fused_tail and (self.input_drop.p > 0 or self.drop.p > 0) else 0
        if not (drawing or n_site):
            return
        seeds = torch.randint(0, 2 ** 62, (len(drawing) + n_site,), device=device, dtype=torch.int64)
        for j, c in enumerate(drawing):
            c.step_seed = seeds[j:j + 1]
        if n_site:
            self.site_seeds = seeds[len(drawing):].bitwise_or_(SITE_BIT)

    def _site(self, k, y, activation, resid, drop_module):
        """Site k of the step: ``activation(drop_module(y)) + resid``."""
        p = drop_module.p if self.training else 0
        if self.fused_tail and _has_code(activation) and not _hooked(drop_module) \
                and (self.site_seeds is not None or not p > 0):
            return drop_act(y, activation, resid, (self.site_seeds[k:k + 1], p) if p > 0 else None)
        y = drop_module(y)
        if activation is not None:
            y = activation(y)
        return y if resid is None else y + resid

    @staticmethod
    def _linear(lin, x):
        return linalg.linear(x, lin.weight, lin.bias)

    def forward(self, graph, feats):
        if not feats.is_cuda:
            raise RuntimeError("sirgcn.PreNormSIRModel needs a ROCm GPU tensor (no CPU fallback)")
        self._draw(feats.device)
        feats = self._site(0, self._linear(self.input_linear, feats), self.activation, None, self.input_drop)

        for i in range(self.num_layers):
            feats_resid = feats
            feats = self.norms[i](feats)
            feats = self.convs[i](graph, feats)
            feats = self._site(2 * i + 1, feats, self.activation, None, self.drop)
            feats = self._linear(self.linears[i], feats)
            feats = self._site(2 * i + 2, feats, None, feats_resid if self.residual else None, self.drop)

        feats = self.output_norm(feats)
        feats = self._linear(self.output_linear, feats)

        return feats.squeeze(1)
