"""Exact-arithmetic GPU tests: every kernel on dyadic inputs (tests/exact_cases.py), compared with the fp64
oracle by ``torch.equal`` — no tolerance, no tie conditioning.

On these inputs every intermediate is an fp32 number whatever the summation order, the split-row plan or the
MFMA tiling (tests/test_exact_inputs_cpu.py holds the inputs to that), so the tests see what a relative-L2
bound on randn data cannot: sigma' at z == 0 exactly (ReLU'(0) = 0, LeakyReLU'(0) = slope, sign bit = z > 0;
a share of all z by construction), exact ties for the maximum (the FIRST edge wins, as DGL's fn.max), the
16-bit kernels at every mask layout, and a single dropped or doubled term.  Outputs are pre-filled with NaN,
so an unwritten element fails."""
import numpy as np
import pytest
import torch
from torch import nn

import exact_cases as xc
import oracle

from sirgcn import SIRConv, _native, edgemlp
from sirgcn.conv import EdgeAggregate, edge_backward
from sirgcn.econv import EdgeAggregateE
from sirgcn.edgemlp import EdgeMaxLinear, EdgeMLPSum
from sirgcn.generic import EdgeGatherAdd, EdgeMax, EdgeSum
from sirgcn.graph import Graph, GraphPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ACT = {"relu": (_native.ACT_RELU, 0.0), "leaky": (_native.ACT_LEAKY, xc.SLOPE)}
ACT_MODULE = {"relu": nn.ReLU, "leaky": lambda: nn.LeakyReLU(xc.SLOPE)}
GRAPH_AGG = xc.GRAPH_AGG
NAN = float("nan")
_PLANS = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _plan(graph, chunk):
    if (graph, chunk) not in _PLANS:
        src, dst, V = xc.GRAPHS[graph]
        _PLANS[graph, chunk] = GraphPlan(src, dst, V, DEV, chunk=chunk)
    return _PLANS[graph, chunk]


def _graphs(agg):
    return xc.graphs_of(agg)


def _want(t64, dtype=torch.float32):
    """The fp64 oracle result in the kernel's output type: exact for fp32 (the CPU self-check), rounded once
    for 16-bit storage."""
    return t64.float().to(dtype).to(DEV)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: "
                             f"got {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}")


def _same_mask(mask, want, what):
    got = mask.cpu().numpy().view(np.uint64).reshape(want.shape)
    assert np.array_equal(got, want), f"{what}: sign mask differs from z > 0 in the documented layout " \
                                      f"({int((got != want).sum())} words)"


def _mean_g(plan, G, agg):
    """MEAN's g = G / deg, rounded to the storage type (include/sirconv.h; exact on these inputs)."""
    return torch.div(G, plan.in_degree_f(), out=torch.empty_like(G)) if agg == "mean" else G


# ----------------------------------------------------------------------------- sum / mean / sym edge kernels
def _backward_modes(mask):
    """(name, mask, one-launch) of every backward form: recompute (two passes), and with a sign mask the
    one-launch and the two-pass form."""
    modes = [("recompute", None, True)]
    if mask is not None:
        modes += [("sign-mask one-launch", mask, True), ("sign-mask two-pass", mask, False)]
    return modes


def _edge_backward(plan, H, agg, act, G, Q, K, mask, dual, dtype, drop=None):
    code, slope = ACT[act]
    dQK = torch.full((G.shape[0], 2 * H), NAN, device=DEV, dtype=dtype)
    EdgeAggregate.dual = dual
    try:            # the sign-mask forms get no Q / K, as in the product
        edge_backward(plan, H, agg, code, slope, G, None if mask is not None else Q, None if mask is not None else K,
                      mask, dQK, drop)
    finally:
        EdgeAggregate.dual = True
    return dQK


def _edge_forward(plan, H, agg, act, Q, K, dtype):
    code, slope = ACT[act]
    nw = _native.mask_words(H, code)
    assert (nw > 0) == (H % 4 == 0), "sign-mask availability changed: revisit the cases"
    E = plan.dst.col.numel()
    in_norm, out_norm = plan.norms(agg)
    S = torch.full((Q.shape[0], H), NAN, device=DEV, dtype=dtype)
    mask = torch.full((E * nw,), -1, device=DEV, dtype=torch.int64) if nw else None
    part = torch.full((max(plan.dst.n_slots, plan.src.n_slots, 1) * H,), NAN, device=DEV)
    _native.edge_agg_fwd(plan.dst, Q, K, in_norm, out_norm, agg, code, slope, S, part, mask)
    return S, mask


EDGE_CASES = [(d, H) for d in DTYPES for H in xc.EDGE_H] + [("f32", H) for H in xc.EDGE_H_SCALAR]


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("dt,H", EDGE_CASES, ids=[f"{d}-{H}" for d, H in EDGE_CASES])
def test_edge_kernels_exact(dt, H, agg, act):
    """sir_edge_agg_fwd and every backward form (sign-mask one-launch / two-pass, recompute) at chunk 4 / 64 /
    256: S, dQ, dK equal the fp64 oracle (rounded once for 16-bit storage), the mask equals z > 0."""
    dtype = DTYPES[dt]
    for graph in _graphs(agg):
        Q, K, G, _ = (t.to(DEV, dtype) for t in xc.edge_inputs(graph, H))
        wS, wdQ, wdK = (_want(t, dtype) for t in xc.edge_expected(graph, H, agg, act))
        want_mask = xc.expected_mask(graph, H) if H % 4 == 0 else None
        for chunk in (4, 64, 256):
            plan = _plan(graph, chunk)
            what = f"{graph} {dt} H={H} {agg} {act} chunk={chunk}"
            S, mask = _edge_forward(plan, H, agg, act, Q, K, dtype)
            _same(S, wS, what + " S")
            if mask is not None:
                _same_mask(mask, want_mask, what)
            for name, m, dual in _backward_modes(mask):
                dQK = _edge_backward(plan, H, agg, act, G, Q, K, m, dual, dtype)
                _same(dQK[:, :H], wdQ, f"{what} {name} dQ")
                _same(dQK[:, H:], wdK, f"{what} {name} dK")


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("H", xc.EDGE_H_UNALIGNED)
def test_edge_kernels_exact_unaligned_leading_dimension(H, agg, act):
    """Q and K as column blocks of one [V, 2 H + 1] buffer (NaN in the spare column): rows of H % 4 == 0 values
    that are not 16-B aligned take the scalar kernels with every lane's every slot full (H = 64, 128, 256: one,
    two, four values per lane).  The forward and both recompute backward passes equal the fp64 oracle."""
    code, slope = ACT[act]
    for graph in _graphs(agg):
        Q, K, G, _ = (t.to(DEV) for t in xc.edge_inputs(graph, H))
        buf = torch.full((Q.shape[0], 2 * H + 1), NAN, device=DEV)
        buf[:, :H], buf[:, H + 1:] = Q, K
        Qv, Kv = buf[:, :H], buf[:, H + 1:]
        assert Qv.stride(0) % 4 != 0 and Kv.data_ptr() % 16 != 0
        wS, wdQ, wdK = (_want(t) for t in xc.edge_expected(graph, H, agg, act))
        for chunk in (4, 64, 256):
            plan = _plan(graph, chunk)
            what = f"{graph} unaligned H={H} {agg} {act} chunk={chunk}"
            in_norm, out_norm = plan.norms(agg)
            S = torch.full((Q.shape[0], H), NAN, device=DEV)
            part = torch.full((max(plan.dst.n_slots, plan.src.n_slots, 1) * H,), NAN, device=DEV)
            _native.edge_agg_fwd(plan.dst, Qv, Kv, in_norm, out_norm, agg, code, slope, S, part, None)
            _same(S, wS, what + " S")
            dQK = _edge_backward(plan, H, agg, act, G, Qv, Kv, None, True, torch.float32)
            _same(dQK[:, :H], wdQ, what + " recompute dQ")
            _same(dQK[:, H:], wdK, what + " recompute dK")


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("H", [76, 256])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_edge_backward_dropout_exact(dt, H, agg, act):
    """The backward passes with the feature dropout of the forward's QK, p = 0.5 (scale 2: exact): dQ, dK equal
    the oracle result times the explicit mask of sir_dropout_apply on ones."""
    dtype = DTYPES[dt]
    drop = (0x5EED_0000 + H, 0.5)
    for graph in _graphs(agg):
        Q, K, G, _ = (t.to(DEV, dtype) for t in xc.edge_inputs(graph, H))
        _, dQ, dK = xc.edge_expected(graph, H, agg, act)
        keep = _native.dropout_apply(torch.ones(Q.shape[0], 2 * H, device=DEV, dtype=dtype), drop)
        assert set(keep.unique().tolist()) == {0.0, 2.0}
        want = _want(torch.cat([dQ, dK], 1) * keep.cpu().double(), dtype)
        for chunk in (4, 256):
            plan = _plan(graph, chunk)
            _, mask = _edge_forward(plan, H, agg, act, Q, K, dtype)
            for name, m, dual in _backward_modes(mask):
                dQK = _edge_backward(plan, H, agg, act, G, Q, K, m, dual, dtype, drop)
                _same(dQK, want, f"{graph} {dt} H={H} {agg} {act} chunk={chunk} {name} dropout dQK")


# ----------------------------------------------------------------------------- SIREConv fused kernels
@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("H", xc.SIRE_H)
def test_sire_kernels_exact(H, agg, act):
    """sir_edge_e_agg_fwd -> edge_backward in sign-mask mode -> sir_edge_e_bwd with the three eidx forms (NULL:
    Eh in CSR order; a permutation: Eh in the caller's order; a table of 5 rows) against
    oracle.sire_reference_step in fp64: S, dQ, dK, dE and the mask."""
    code, slope = ACT[act]
    for graph in _graphs(agg):
        Q, K, G, Eh = (t.to(DEV) for t in xc.edge_inputs(graph, H))
        T, ids = xc.sire_table(graph, H)
        V, E = Q.shape[0], Eh.shape[0]
        nw = _native.mask_words(H, code)
        for chunk in (64, 256):
            plan = _plan(graph, chunk)
            eid = plan.dst.eid
            eid32 = eid.to(torch.int32)
            in_norm, out_norm = plan.norms(agg)
            forms = {"null": (Eh[eid].contiguous(), None, None), "perm": (Eh, eid32, None),
                     "table": (T.to(DEV), ids.to(DEV)[eid].to(torch.int32), (T, ids))}
            for form, (rows, eidx, table) in forms.items():
                what = f"{graph} H={H} {agg} {act} chunk={chunk} eidx={form}"
                want = xc.sire_expected(graph, H, agg, act, table)
                S = torch.full((V, H), NAN, device=DEV)
                mask = torch.full((E * nw,), -1, device=DEV, dtype=torch.int64)
                part = torch.full((max(plan.dst.n_slots, 1) * H,), NAN, device=DEV)
                _native.edge_e_agg_fwd(plan.dst, Q, K, rows, eidx, in_norm, out_norm, agg, code, slope, S, part, mask)
                _same(S, _want(want["S"]), what + " S")
                _same_mask(mask, xc.expected_mask(graph, H, True, None if table is None else T[ids]), what)
                # the backward as EdgeAggregateE runs it: MEAN on g = G / deg with the SUM kernels
                g, bagg = _mean_g(plan, G, agg), ("sum" if agg == "mean" else agg)
                dQK = torch.full((V, 2 * H), NAN, device=DEV)
                edge_backward(plan, H, bagg, code, slope, g, None, None, mask, dQK)
                _same(dQK[:, :H], _want(want["dQ"]), what + " dQ")
                _same(dQK[:, H:], _want(want["dK"]), what + " dK")
                b_in, b_out = plan.norms(bagg)
                dE = torch.full((E, H), NAN, device=DEV)
                # a stream's gradient lands in eidx order; a table's is written per edge in CSR order
                _native.edge_e_bwd(plan.dst, mask, g, b_in, b_out, bagg, code, slope, eidx if form == "perm" else None, dE)
                wdE = _want(want["dE"])
                _same(dE, wdE if form == "perm" else wdE[eid], what + " dE")
                if form == "table":         # and the per-type sum of the autograd wrapper
                    QK = torch.cat([Q, K], 1).requires_grad_(True)
                    Tr = T.to(DEV).requires_grad_(True)
                    S2 = EdgeAggregateE.apply(QK, Tr, eidx, plan, H, agg, code, slope, True, True)
                    S2.backward(G)
                    _same(S2.detach(), _want(want["S"]), what + " S (autograd)")
                    _same(QK.grad, torch.cat([_want(want["dQ"]), _want(want["dK"])], 1), what + " dQK (autograd)")
                    wdT = torch.zeros(T.shape, dtype=torch.float64).index_add_(0, ids, want["dE"])
                    _same(Tr.grad, _want(wdT), what + " dT")


# ----------------------------------------------------------------------------- per-edge Linear forms
@pytest.mark.parametrize("graph,agg", GRAPH_AGG)
@pytest.mark.parametrize("H,F", xc.SEQ_SHAPES)
def test_seq_sigma_kernels_exact(H, F, graph, agg):
    """sir_edge_mlp_fwd / _bwd_dst / _bwd_src (sigma = ReLU, Linear(H, F), ReLU): out, dQ, dK and the summed
    per-wave partials (dW, db) equal the fp64 oracle."""
    Q, K, W, b, G = (t.to(DEV) for t in xc.mlp_inputs(graph, H, F))
    want = {k: _want(v) for k, v in xc.seq_expected(graph, H, F, agg).items()}
    for chunk in (4, 64, 256):
        what = f"seq {graph} {agg} H={H} F={F} chunk={chunk}"
        QK = torch.cat([Q, K], 1).requires_grad_(True)
        Wr, br = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        S = EdgeMLPSum.apply(QK, Wr, br, _plan(graph, chunk), H, agg, _native.ACT_RELU, 0.0, _native.ACT_RELU)
        S.backward(G)
        _same(S.detach(), want["S"], what + " S")
        _same(QK.grad[:, :H], want["dQ"], what + " dQ")
        _same(QK.grad[:, H:], want["dK"], what + " dK")
        _same(Wr.grad, want["dW"], what + " dW")
        _same(br.grad, want["db"], what + " db")


def _max_forward(plan, Q, K, W, b, act, dtype):
    """The max forward at kernel level (fp32 kernels, or the 16-bit ``_st`` forms on Q, K of ``dtype``):
    Y and the arg edges as dst-CSR positions."""
    code, slope = ACT[act]
    V, O = Q.shape[0], W.shape[0]
    Y = torch.full((V, O), NAN, device=DEV)
    arg = torch.full((V, O), -2, device=DEV, dtype=torch.int32)
    if dtype == torch.float32:
        edgemlp._fwd(plan, Q, K, W, b, "max", code, slope, _native.ACT_IDENTITY, Y, arg)
    else:
        edgemlp._fwd_st(plan, Q.to(dtype), K.to(dtype), W, b, code, slope, Y, arg)
    return Y, arg


def _edge_ids(plan, arg):
    """dst-CSR positions -> the caller's edge ids (-1 stays)."""
    pos = arg.long()
    return torch.where(pos >= 0, plan.dst.eid[pos.clamp_min(0)], pos)


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("graph", list(xc.GRAPHS))
@pytest.mark.parametrize("H,O", xc.MAX_SHAPES)
def test_max_forward_exact_first_edge_wins(H, O, graph, act, monkeypatch):
    """The max forward (per-item kernel at chunk 4 / 64 / 256, the stream kernel at H = 256; fp32 and the two
    16-bit forms): Y and arg equal oracle.max_first_wins — an exact tie goes to the first edge, an empty row
    gives 0 / -1."""
    Q, K, W, b, _ = (t.to(DEV) for t in xc.mlp_inputs(graph, H, O))
    want = xc.max_expected(graph, H, O, act)
    wY, warg = _want(want["Y"]), want["arg"].to(DEV)
    empty = torch.bincount(xc.GRAPHS[graph][1], minlength=Q.shape[0]) == 0
    assert bool(empty.any()) and bool((warg[empty] == -1).all()) and bool((wY[empty] == 0).all())
    for dt, dtype in DTYPES.items():
        runs = [(False, c) for c in (4, 64, 256)] + ([(True, 256)] if H == 256 and O <= 256 else [])
        for stream, chunk in runs:
            monkeypatch.setattr(edgemlp, "STREAM", stream)
            plan = _plan(graph, chunk)
            what = f"max {graph} {act} H={H} O={O} {dt} {'stream' if stream else f'chunk={chunk}'}"
            Y, arg = _max_forward(plan, Q, K, W, b, act, dtype)
            _same(Y, wY, what + " Y")
            _same(_edge_ids(plan, arg), warg, what + " arg")


# route switches of EdgeMaxLinear (as test_max_backward_routes_agree / test_max_hybrid_backward_matches_materialised)
MAX_ROUTES = {
    "routed": (dict(fused_bwd=None, sparse_bwd=True), edgemlp.max_bwd_sparse),
    "fused": (dict(fused_bwd=True), lambda H, O, V: edgemlp.max_bwd_fused(H, O)),
    "hybrid dw_qk": (dict(fused_bwd=None, sparse_bwd=False, hybrid_bwd=True, dw_qk=True), edgemlp.max_bwd_sparse),
    "hybrid dw_rows": (dict(fused_bwd=None, sparse_bwd=False, hybrid_bwd=True, dw_qk=False), edgemlp.max_bwd_sparse),
    "materialised dw_rows": (dict(fused_bwd=False, dw_rows=True), lambda H, O, V: True),
    "materialised dw gemm": (dict(fused_bwd=False, dw_rows=False), lambda H, O, V: True),
}


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("graph", list(xc.GRAPHS))
@pytest.mark.parametrize("H,O", xc.MAX_SHAPES)
def test_max_backward_routes_exact(H, O, graph, act, monkeypatch):
    """Every max backward route within its limits — routed (sir_edge_max_bwd_sparse + its dW pass), fused
    (sir_edge_max_bwd_dst / _src), hybrid (routed dQ / dK + sir_max_dw_qk or sir_max_dw_rows), edge-materialised
    (sir_edge_gather_act sign words at H = 256, sir_gemm_nt_dact, sir_max_dw_rows or the TN GEMM): dQ, dK, dW_R,
    db_R equal the fp64 oracle, hence each other."""
    code, slope = ACT[act]
    Q, K, W, b, dY = (t.to(DEV) for t in xc.mlp_inputs(graph, H, O))
    want = {k: _want(v) for k, v in xc.max_expected(graph, H, O, act).items() if k != "arg"}
    V = Q.shape[0]
    monkeypatch.setattr(edgemlp, "STREAM", False)
    ran = 0
    for chunk in (4, 256):
        plan = _plan(graph, chunk)
        _, arg = _max_forward(plan, Q, K, W, b, act, torch.float32)
        for route, (switches, applies) in MAX_ROUTES.items():
            if not applies(H, O, V):
                continue
            for k, v in switches.items():
                monkeypatch.setattr(EdgeMaxLinear, k, v)
            what = f"max {graph} {act} H={H} O={O} chunk={chunk} {route}"
            dQK = torch.full((V, 2 * H), NAN, device=DEV)
            dW, db = edgemlp.max_linear_backward(plan, Q, K, W, arg, dY, code, slope, dQK[:, :H], dQK[:, H:])
            _same(dQK[:, :H], want["dQ"], what + " dQ")
            _same(dQK[:, H:], want["dK"], what + " dK")
            _same(dW.contiguous(), want["dW"], what + " dW_R")
            _same(db.contiguous(), want["db"], what + " db_R")
            ran += 1
    assert ran >= 4


@pytest.mark.parametrize("graph,agg", GRAPH_AGG)
@pytest.mark.parametrize("F", xc.HELPER_F)
def test_edge_materialised_helpers_exact(F, graph, agg):
    """sirgcn.generic on integers: sir_edge_gather_add, sir_segment_sum (plain, with norms / mean, and the
    ``perm`` form of the source side), sir_edge_broadcast, sir_segment_max / _bwd."""
    src, dst, V = xc.GRAPHS[graph]
    E = src.numel()
    Q, K, dS = (xc.ints((V, F), 4, 300 + F + i) for i in range(3))
    M, dZ = xc.ints((E, F), 4, 310 + F), xc.ints((E, F), 4, 311 + F)      # caller's edge order
    ind = torch.bincount(dst, minlength=V).clamp(min=1).double()[:, None]
    in_norm, out_norm = oracle.degree_norms(torch.bincount(dst, minlength=V), torch.bincount(src, minlength=V), agg)
    c = (out_norm[src] * in_norm[dst]).double()[:, None]
    wS = torch.zeros(V, F, dtype=torch.float64).index_add_(0, dst, c * M.double())
    wdM = c * dS.double()[dst]
    if agg == "mean":
        wS, wdM = wS / ind, wdM / ind[dst]
    wY, warg = oracle.max_first_wins(dst, V, M.double())
    wdMax = torch.zeros(E, F, dtype=torch.float64)
    r, f = torch.nonzero(warg >= 0, as_tuple=True)
    wdMax[warg[r, f], f] = dS.double()[r, f]
    for chunk in (4, 256):
        plan = _plan(graph, chunk)
        eid = plan.dst.eid
        what = f"generic {graph} {agg} F={F} chunk={chunk}"
        QK = torch.cat([Q, K], 1).to(DEV).requires_grad_(True)
        Z = EdgeGatherAdd.apply(QK, plan, F)
        _same(Z.detach(), (Q[dst] + K[src]).to(DEV)[eid], what + " gather_add")
        Z.backward(dZ.to(DEV)[eid])
        _same(QK.grad[:, :F], _want(torch.zeros(V, F, dtype=torch.float64).index_add_(0, dst, dZ.double())),
              what + " segment_sum (dQ)")
        _same(QK.grad[:, F:], _want(torch.zeros(V, F, dtype=torch.float64).index_add_(0, src, dZ.double())),
              what + " segment_sum perm (dK)")
        Mc = M.to(DEV)[eid].requires_grad_(True)
        S = EdgeSum.apply(Mc, plan, agg)
        S.backward(dS.to(DEV))
        _same(S.detach(), _want(wS), what + " segment_sum")
        _same(Mc.grad, _want(wdM)[eid], what + " edge_broadcast")
        if agg == "sum":
            Mx = M.to(DEV)[eid].requires_grad_(True)
            Y = EdgeMax.apply(Mx, plan)
            Y.backward(dS.to(DEV))
            _same(Y.detach(), _want(wY), what + " segment_max")
            _same(Mx.grad, _want(wdMax)[eid], what + " segment_max_bwd")


# ----------------------------------------------------------------------------- one layer through the GEMMs
@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("agg", xc.LAYER_AGGS)
@pytest.mark.parametrize("H,O", xc.LAYER_SHAPES)
def test_layer_step_exact(H, O, agg, act):
    """SIRConv(8, H, O) on graph A, fp32, the fused path: integer X, weights and dY whose every GEMM operand is
    exact under the split-fp16 rule (hi + lo with lo = 0 for the integer weights, so the dropped lo * lo term is
    0; tests/test_exact_inputs_cpu.py::test_layer_inputs).  Y and every gradient equal
    oracle.reference_cpu_step in fp64."""
    src, dst, V = xc.GRAPHS["A"]
    X, W_Q, b_Q, W_K, W_R, b_R, dY = (t.to(DEV) for t in xc.layer_inputs(H, O))
    want = xc.layer_expected(H, O, agg, act)
    m = SIRConv(xc.LAYER_D, H, O, ACT_MODULE[act](), 0, agg_type=agg).to(DEV)
    with torch.no_grad():
        for p, v in ((m.linear_query.weight, W_Q), (m.linear_query.bias, b_Q), (m.linear_key.weight, W_K),
                     (m.linear_relation.weight, W_R), (m.linear_relation.bias, b_R)):
            p.copy_(v)
    g = Graph(src, dst, V)
    for chunk in (64, 256):
        m.chunk = chunk
        m.zero_grad(set_to_none=True)
        Xr = X.clone().requires_grad_(True)
        Y = m(g, Xr)
        Y.backward(dY)
        got = {"Y": Y.detach(), "dX": Xr.grad, "dW_Q": m.linear_query.weight.grad, "db_Q": m.linear_query.bias.grad,
               "dW_K": m.linear_key.weight.grad, "dW_R": m.linear_relation.weight.grad,
               "db_R": m.linear_relation.bias.grad}
        for k in xc.LAYER_OUTPUTS:
            _same(got[k].contiguous(), _want(want[k]), f"layer {agg} {act} H={H} O={O} chunk={chunk} {k}")


@pytest.mark.parametrize("M", xc.GEMM_M)
def test_small_gemms_exact_on_integers(M):
    """sir_gemm_nt with bias, sir_gemm_nt_direct2, sir_gemm_tn with colsum_a, sir_gemm_nt16 and sir_gemm_tn16 on
    integer operands at the smallest ragged shapes: the integer result, exactly."""
    for K in xc.GEMM_KN:
        for N in xc.GEMM_KN:
            what = f"M={M} K={K} N={N}"
            A, W, b = xc.gemm_inputs(M, K, N)
            _, W2, _ = xc.gemm_inputs(M + 1, K, N)
            B = xc.ints((M, N), 4, 17 + M + K + N)                        # TN: contraction over the M rows
            wC = A.double() @ W.double().t()
            A, W, W2, b, B = (t.to(DEV) for t in (A, W, W2, b, B))
            _same(_native.gemm_nt(A, _native.gemm_pack(W), b), _want(wC + b.cpu().double()), what + " gemm_nt")
            w2 = torch.cat([wC + b.cpu().double(), A.cpu().double() @ W2.cpu().double().t()], 1)
            _same(_native.gemm_nt_direct2(A, W, W2, False, b), _want(w2), what + " gemm_nt_direct2")
            wT = A.cpu().double().t() @ B.cpu().double()
            C, cs = _native.gemm_tn(A, B, colsum=True)
            _same(C, _want(wT), what + " gemm_tn")
            _same(cs, _want(A.cpu().double().sum(0)), what + " gemm_tn colsum_a")
            for dt in (torch.bfloat16, torch.float16):
                if K in (128, 256, 512) and N % 8 == 0:         # the 16-bit NT kernel's shapes
                    C16 = _native.gemm_nt16(A.to(dt), _native.gemm_pack16(W, dt), b, torch.float32)
                    _same(C16, _want(wC + b.cpu().double()), f"{what} gemm_nt16 {dt}")
                C, cs = _native.gemm_tn16(A.to(dt), B.to(dt), colsum=True)
                _same(C, _want(wT), f"{what} gemm_tn16 {dt}")
                _same(cs, _want(A.cpu().double().sum(0)), f"{what} gemm_tn16 colsum {dt}")
