"""Multi-layer SIRConv stacks: the layer loops of the reference's models, i.e. the callers of the
hot path for BASELINE configs 1, 2, 3 and 5.

The reference models wrap SIRConv in embeddings and prediction heads (out of scope) and end
with a graph readout (``sirgcn.readout``: SumPooling / AvgPooling / MaxPooling);
what reaches the hot path is their per-layer loop, restated here with the conv / norm classes as
parameters so that the SAME loop runs on the reference's own ``models/conv.py`` / ``models/norm.py``
(``tests/golden/make_golden.py`` builds the stack fixtures that way) and on this package's
MI355X modules (tests, ``bench.py --workload``):

* ``order="arxiv"`` — ``ogbn-arxiv/model.py:65-73`` and ``ogbg-molhiv/model.py:76-84``:
  ``resid = h; h = conv(g, h); h = norm(g, h); h = act(h); h = h + resid``;
* ``order="zinc"`` — ``zinc/model.py:50-56`` (identity residual): ``h = conv(g, h) + h;
  h = norm(g, h); h = act(h)``;
* ``order="plain"`` — ``dictionary-lookup/model.py:30-32``: ``h = conv(g, h)`` (the
  ``Sequential`` sigma lives inside the conv).

``norm_cls`` (e.g. GraphNorm, ``models/norm.py:7-29``) is called as ``norm(graph, feats)``.

``dropout`` is the layer's ``nn.Dropout`` of the node-level models, at the reference's position: after the
activation and before the residual add (``ogbn-arxiv/model.py:49,70``), after the activation in zinc order
(``zinc/model.py:24,56``).  A norm whose ``forward_act`` takes ``dropout`` (this package's three) runs it inside
its fused pass from a hashed mask that is never stored; otherwise the stack applies ``self.dropout`` itself.

``edge_dropout`` is the graph-level models' DropEdge (``self.edge_drop`` of ``zinc/model.py:25,50-54``,
``sbm-dataset/model.py:42``): every layer's conv runs on its own dropped graph — in eval mode too, as the
reference's does — while the norm sees the original graph (``sirgcn.dropedge``).
"""
import functools
import inspect

from torch import nn

from .dropedge import DropEdge


def _resid_act(y, resid, activation, order, r_link=None, out_link=None):
    """sirgcn.resact.resid_act for GPU tensors (imported lazily: the stack also runs the reference's
    own modules on the CPU, where it returns None)."""
    if not (getattr(y, "is_cuda", False) and getattr(resid, "is_cuda", False)):
        return None
    from .resact import resid_act
    return resid_act(y, resid, activation, order, r_link, out_link)


@functools.lru_cache(maxsize=None)
def _takes_dropout(fn):
    """True when the ``forward_act`` function ``fn`` has a ``dropout`` parameter."""
    try:
        params = inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False
    return "dropout" in params or any(q.kind is inspect.Parameter.VAR_KEYWORD for q in params.values())


def _new_link():
    from .resact import GradLink
    return GradLink()


class SIRStack(nn.Module):
    # the fused residual pass (no norm): each layer's residual gradient handed to the previous layer's
    # backward (sirgcn.resact.GradLink) instead of an autograd add.  The parameters' and the
    # stack input's gradients are the same bits either way; a hook on (or torch.autograd.grad of) an
    # intermediate layer output sees only its conv-input part — set False for that.
    link_residual_grads = True

    def __init__(self, conv_cls, hidden, num_layers, activation, agg_type="sum", order="arxiv",
                 norm_cls=None, conv_activation=None, feat_dropout=0, dropout=0, edge_dropout=0):
        super().__init__()
        if order not in ("arxiv", "zinc", "plain"):
            raise ValueError(order)
        self.order = order
        self.activation = activation
        sigma = conv_activation if conv_activation is not None else activation
        # feat_dropout: the conv's own Dropout on Q and K, passed positionally as the reference's
        # models do (ogbn-arxiv/model.py:57, ogbg-molhiv/model.py:66)
        self.convs = nn.ModuleList([conv_cls(hidden, hidden, hidden, sigma, feat_dropout, agg_type=agg_type)
                                    for _ in range(num_layers)])
        self.norms = nn.ModuleList([norm_cls(hidden) for _ in range(num_layers)]) if norm_cls else None
        # the layer dropout (the reference's attribute); fused into the norm pass when the norm offers it
        self.dropout = nn.Dropout(dropout)
        self.layer_seeds = None      # the layers' seed words of the last fused-dropout step (one per layer)
        # DropEdge before every conv (a plain callable: no parameters, no state_dict entry); p = 0 hands the
        # graph through untouched
        self.edge_drop = DropEdge(edge_dropout)

    def forward(self, graph, feats):
        p_drop = self.dropout.p if self.training else 0
        self.layer_seeds = None
        if self.training and getattr(feats, "is_cuda", False):
            # the dropout seeds of every layer in ONE device draw (sirgcn SIRConv's step_seed): one
            # RNG launch per step instead of one per layer (small batches are launch-bound)
            drawing = [c for c in self.convs if hasattr(c, "step_seed") and c.dropout.p > 0]
            # ... and one more word per layer for its fused layer dropout.  A layer's word is never a conv's:
            # the conv's Q dropout hashes the same (row, col) domain, so the convs' words stay below 2^62
            # and the layers' get bit 62 set.
            n_layer = len(self.convs) if p_drop > 0 and self.norms is not None and self.order != "plain" else 0
            if drawing or n_layer:
                import torch
                seeds = torch.randint(0, 2 ** 62, (len(drawing) + n_layer,), device=feats.device, dtype=torch.int64)
                for j, c in enumerate(drawing):
                    c.step_seed = seeds[j:j + 1]
                if n_layer:
                    self.layer_seeds = seeds[len(drawing):].bitwise_or_(1 << 62)
        link = None          # the GradLink of feats when a fused residual pass produced it
        for i, conv in enumerate(self.convs):
            graph_ = self.edge_drop(graph)       # the conv's graph; the norm below keeps the original
            if self.order == "plain":
                feats = conv(graph_, feats)
                continue
            resid = feats
            feats = conv(graph_, feats)
            if self.norms is None and not p_drop > 0:
                # + resid and the activation in one pass when the operands allow (sirgcn.resact);
                # the residual gradient of each layer's input handed to the layer that produced it
                # (resact.GradLink) instead of an autograd add
                out_link = _new_link() if self.link_residual_grads and getattr(feats, "is_cuda", False) else None
                fused = _resid_act(feats, resid, self.activation, self.order, link, out_link)
                if fused is not None:
                    feats = fused
                    link = out_link
                    continue
            link = None
            if self.order == "zinc":
                feats = feats + resid
            if self.norms is not None:
                # norm -> act (-> + resid) as one op when the norm offers it (sirgcn.GraphNorm:
                # one kernel per direction; None: not for this activation / these operands)
                fuse = getattr(self.norms[i], "forward_act", None)
                r = resid if self.order == "arxiv" else None
                if not p_drop > 0:
                    out = fuse(graph, feats, self.activation, r) if fuse else None
                elif fuse and self.layer_seeds is not None and _takes_dropout(getattr(fuse, "__func__", fuse)):
                    out = fuse(graph, feats, self.activation, r, dropout=(self.layer_seeds[i:i + 1], p_drop))
                else:
                    out = None          # no fused dropout: norm, activation, self.dropout and the add below
                if out is not None:
                    feats = out
                    continue
                feats = self.norms[i](graph, feats)
            feats = self.activation(feats)
            if p_drop > 0:
                feats = self.dropout(feats)
            if self.order == "arxiv":
                feats = feats + resid
        return feats
