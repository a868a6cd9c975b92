"""Drop-in ``SIREConv`` (SIR-GCN with edge features), briangodwinlim/SIR-GCN ``models/conv.py:70-134``.

    h_u^* = sum_{v in N(u)} W_R sigma(W_Q h_u + W_E h_{u,v} + W_K h_v)

Same constructor ``SIREConv(input_dim, edge_dim, hidden_dim, output_dim, activation, dropout=0,
inner_bias=True, outer_bias=True, agg_type='sum')`` (``conv.py:94``), attributes (``linear_edge``
has no bias, ``conv.py:99``; callers may swap it for an ``nn.Embedding``, ``zinc/model.py:12-15``)
and ``forward(graph, nfeat, efeat)`` (``conv.py:114``).

Two routes, chosen per call:

* **fused** (``SIREConv.fused``, sum / mean / sym with ReLU or LeakyReLU, fp32, ``H % 4 == 0``,
  ``H <= 1024``, no autocast): the edge term is one extra gathered row per edge inside the row-CSR
  edge kernel (``sir_edge_e_agg_fwd``): ``z_e = (Q[v] + K[u]) + e_uv`` in the reference's operand order
  (``conv.py:108``), sigma, the norm product and the sum in registers — no ``[E, H]`` tensor besides
  the edge term itself.  The forward stores the sign of ``z_e`` (:class:`EdgeAggregateE`); the backward
  takes dQ / dK from SIRConv's sign-mask passes unchanged and the edge term's gradient from
  ``sir_edge_e_bwd``.  Q, K and the edge term come from the module's own ``linear_query``,
  ``linear_key``, ``linear_edge`` and ``dropout``, so any edge encoder keeps working:

  - *stream form*: ``Eh = dropout(linear_edge(efeat))`` is read in the caller's edge order through
    the plan's edge ids (no ``index_select`` copy), and its gradient comes back in that order;
  - *table form* (``linear_edge`` is a plain ``nn.Embedding``, ``efeat`` a 1-D integer tensor, dropout
    inactive): the kernel gathers rows of ``linear_edge.weight`` by the edge's type id — the forward
    holds no ``[E, H]`` tensor at all.  The ids are validated on the host with one min / max check
    (ONE device synchronisation per call); an id outside the table raises ``ValueError``.  The
    backward writes the per-edge gradient once and reduces it per type in a fixed order
    (``sir_segment_sum`` over a row CSR of the ids: deterministic, no atomics).

* **edge-materialised** (everything else: ``agg_type='max'``, tanh / GELU / other callables, fp64,
  autocast, ``H % 4 != 0``, or ``fused = False``): node gathers by ``sir_edge_gather_add``, the edge
  term permuted once into destination-CSR order, sigma (any callable) by torch, then
  ``sir_segment_sum`` / ``sir_segment_max`` and their backward kernels (``sirgcn.generic``).
"""
import torch
from torch import nn

from . import _native
from .conv import activation_code, edge_backward, _partial
from .generic import EdgeGatherAdd, EdgeMax, EdgeSum
from .graph import DEFAULT_CHUNK, build_row_csr, get_plan


def _eid32(plan):
    """``plan.dst.eid`` (destination-CSR position -> the caller's edge id) as int32, cached on the plan."""
    e = getattr(plan, "_dst_eid32", None)
    if e is None:
        e = plan.dst.eid.to(torch.int32).contiguous()
        plan._dst_eid32 = e
    return e


class EdgeAggregateE(torch.autograd.Function):
    """S = update_all of ``conv.py:109-113,128-131`` on packed ``QK = [Q | K]`` ([V, 2H]) and edge rows
    ``Eh`` ([R, H]): ``S[v] = sum_p c_p sigma((Q[v] + K[u]) + Eh[eidx[p]])``, ``eidx`` int32 per
    destination-CSR position (the plan's edge ids for an ``[E, H]`` stream in the caller's order, or type
    ids into a table with ``table=True``).  Saves only the sign mask and ``eidx`` — neither QK nor Eh.
    Backward: dQ / dK from the sign-mask passes of SIRConv (:func:`sirgcn.conv.edge_backward`), the edge
    term from ``sir_edge_e_bwd``: in ``eidx`` order for a stream; for a table one row per edge in CSR order,
    then summed per type in a fixed order (``sir_segment_sum``)."""

    @staticmethod
    def forward(ctx, QK, Eh, eidx, plan, H, agg, act, slope, grad_on=True, table=False):
        if QK.device.type != "cuda":
            raise RuntimeError("SIREConv native path needs a ROCm GPU tensor (no CPU fallback)")
        if QK.dtype != torch.float32 or Eh.dtype != torch.float32:
            raise RuntimeError("EdgeAggregateE takes fp32 rows")
        QK = QK.contiguous()
        Eh = Eh.contiguous()
        V = QK.shape[0]
        ctx.plan, ctx.H, ctx.agg, ctx.act, ctx.slope, ctx.V = plan, H, agg, act, slope, V
        ctx.table, ctx.R = table, Eh.shape[0]
        ctx.empty = plan.num_edges == 0
        if ctx.empty:                       # no edge: every row is the empty sum
            return torch.zeros((V, H), device=QK.device, dtype=torch.float32)
        in_norm, out_norm = plan.norms(agg)
        S = torch.empty((V, H), device=QK.device, dtype=torch.float32)
        nw = _native.mask_words(H, act)
        if not nw:
            raise RuntimeError("EdgeAggregateE needs ReLU / LeakyReLU, H % 4 == 0 and H <= 1024")
        mask = None
        if grad_on and any(ctx.needs_input_grad[:2]):       # inference / eval under no_grad: no mask
            mask = torch.empty((plan.num_edges * nw,), device=QK.device, dtype=torch.int64)
        _native.edge_e_agg_fwd(plan.dst, QK[:, :H], QK[:, H:], Eh, eidx, in_norm, out_norm, agg, act, slope, S,
                               _partial(plan, H, QK.device), mask)
        if mask is not None:
            ctx.save_for_backward(mask, eidx)
        return S

    @staticmethod
    def backward(ctx, dS):
        plan, H, agg, act, slope, V = ctx.plan, ctx.H, ctx.agg, ctx.act, ctx.slope, ctx.V
        need_qk, need_e = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dev = dS.device
        if ctx.empty:
            dQK = torch.zeros((V, 2 * H), device=dev, dtype=torch.float32) if need_qk else None
            dEh = torch.zeros((ctx.R, H), device=dev, dtype=torch.float32) if need_e else None
            return dQK, dEh, None, None, None, None, None, None, None, None
        mask, eidx = ctx.saved_tensors
        G = dS.contiguous().float()
        if agg == "mean":       # both passes and the edge term read g = G / deg (as edge_backward's MEAN)
            G = torch.div(G, plan.in_degree_f(), out=torch.empty_like(G))
            agg = "sum"
        dQK = dEh = None
        if need_qk:
            dQK = torch.empty((V, 2 * H), device=dev, dtype=torch.float32)
            edge_backward(plan, H, agg, act, slope, G, None, None, mask, dQK)
        if need_e:
            in_norm, out_norm = plan.norms(agg)
            if not ctx.table:
                dEh = torch.empty((ctx.R, H), device=dev, dtype=torch.float32)     # eidx is a permutation
                _native.edge_e_bwd(plan.dst, mask, G, in_norm, out_norm, agg, act, slope, eidx, dEh)
            else:
                dE = torch.empty((plan.num_edges, H), device=dev, dtype=torch.float32)
                _native.edge_e_bwd(plan.dst, mask, G, in_norm, out_norm, agg, act, slope, None, dE)
                # per-type sums in ascending CSR position, split rows combined in slot order
                ids = eidx.to(torch.int64)
                csr = build_row_csr(ids, ids, ctx.R)
                dEh = torch.empty((ctx.R, H), device=dev, dtype=torch.float32)
                part = torch.empty((csr.n_slots * H,), device=dev, dtype=torch.float32) if csr.n_slots else None
                _native.segment_sum(csr, dE, dEh, perm=csr.eid.to(torch.int32).contiguous(), partial=part)
        return dQK, dEh, None, None, None, None, None, None, None, None


class SIREConv(nn.Module):
    fused = True        # class switch: False runs every input on the edge-materialised path

    def __init__(self, input_dim, edge_dim, hidden_dim, output_dim, activation, dropout=0, inner_bias=True,
                 outer_bias=True, agg_type='sum'):
        super().__init__()
        if agg_type not in ("sum", "mean", "sym", "max"):
            raise AttributeError(f"module 'dgl.function' has no attribute '{agg_type}'")
        self.activation = activation
        self.dropout = nn.Dropout(dropout)
        self.linear_query = nn.Linear(input_dim, hidden_dim, bias=inner_bias)
        self.linear_key = nn.Linear(input_dim, hidden_dim, bias=False)
        self.linear_edge = nn.Linear(edge_dim, hidden_dim, bias=False)
        self.linear_relation = nn.Linear(hidden_dim, output_dim, bias=outer_bias)
        self._agg_type = agg_type
        self.chunk = DEFAULT_CHUNK

    def _fused_code(self, H, Q, K):
        """(act, slope) of the fused route for these Q / K, or None for the edge-materialised path."""
        if not self.fused or self._agg_type not in ("sum", "mean", "sym") or torch.is_autocast_enabled():
            return None
        try:
            act, slope = activation_code(self.activation)
        except NotImplementedError:
            return None
        if act not in (_native.ACT_RELU, _native.ACT_LEAKY) or _native.mask_words(H, act) <= 0:
            return None
        if Q.dtype != torch.float32 or K.dtype != torch.float32 or Q.shape != K.shape:
            return None
        return act, slope

    def _table_ids(self, efeat):
        """The edge-type ids when ``linear_edge`` is a plain embedding lookup the kernel can gather itself."""
        le = self.linear_edge
        if type(le) is not nn.Embedding or le.padding_idx is not None or le.max_norm is not None or le.sparse:
            return None
        if efeat.dim() != 1 or efeat.dtype.is_floating_point or efeat.dtype.is_complex or efeat.dtype == torch.bool:
            return None
        if (self.training and self.dropout.p > 0) or le.weight.dtype != torch.float32:
            return None             # Dropout draws per edge, not per table row
        if efeat.numel():
            lo, hi = torch.stack(torch.aminmax(efeat)).tolist()      # the one host synchronisation
            if lo < 0 or hi >= le.num_embeddings:
                raise ValueError(f"edge type id out of range [0, {le.num_embeddings}): min {lo}, max {hi}")
        return efeat

    def forward(self, graph, nfeat, efeat):
        if isinstance(nfeat, tuple):         # expand_as_pair (conv.py:126)
            nfeat_key, nfeat_query = nfeat
        else:
            nfeat_key = nfeat_query = nfeat
        if nfeat_query.device.type != "cuda":
            raise RuntimeError("SIREConv native path needs a ROCm GPU tensor (no CPU fallback)")
        plan = get_plan(graph, nfeat_query.device, self.chunk)
        if plan.num_nodes != nfeat_query.shape[0]:
            raise ValueError(f"nfeat has {nfeat_query.shape[0]} rows, graph has {plan.num_nodes} nodes")
        if efeat.shape[0] != plan.num_edges:
            raise ValueError(f"efeat has {efeat.shape[0]} rows, graph has {plan.num_edges} edges")
        H = self.linear_query.out_features
        K = self.dropout(self.linear_key(nfeat_key))                     # conv.py:127
        Q = self.dropout(self.linear_query(nfeat_query))                 # conv.py:128
        code = self._fused_code(H, Q, K)
        grad_on = torch.is_grad_enabled()
        if code is not None:
            ids = self._table_ids(efeat)
            if ids is not None:              # table form: the kernel gathers linear_edge.weight rows
                eidx = ids.index_select(0, plan.dst.eid).to(torch.int32)
                S = EdgeAggregateE.apply(torch.cat([Q, K], 1), self.linear_edge.weight, eidx, plan, H,
                                         self._agg_type, code[0], code[1], grad_on, True)
                return self.linear_relation(S)                           # conv.py:133
        Ee = self.dropout(self.linear_edge(efeat))                       # conv.py:129
        if code is not None and Ee.dtype == torch.float32 and Ee.dim() == 2 and Ee.shape[1] == H:
            S = EdgeAggregateE.apply(torch.cat([Q, K], 1), Ee, _eid32(plan), plan, H, self._agg_type,
                                     code[0], code[1], grad_on, False)
            return self.linear_relation(S)                               # conv.py:133
        Z = EdgeGatherAdd.apply(torch.cat([Q, K], 1), plan, H)           # eq[v] + ek[u], dst-CSR order
        Z = Z + Ee.index_select(0, plan.dst.eid).to(Z.dtype)             # (...) + e_uv (conv.py:108)
        A = self.activation(Z)
        if self._agg_type == "max":
            return EdgeMax.apply(self.linear_relation(A), plan)           # conv.py:110, no post-projection
        S = EdgeSum.apply(A, plan, self._agg_type)                       # conv.py:108 norms, 131 update_all
        return self.linear_relation(S)                                   # conv.py:133

    def extra_repr(self):
        return f"agg_type={self._agg_type!r}"
