"""Poison tests on the GPU (inputs and checkers: tests/poison_cases.py; their self-check:
tests/test_poison_inputs_cpu.py).

Part A, isolation: every operand is a view into a NaN-filled allocation (leading dimension > width, rows
past the last, where the ABI allows a misaligned base), the rows of node matrices and edge tables the result
does not depend on hold NaN, workspaces are NaN-filled, outputs are views into sentinel-filled buffers.  On
the dyadic inputs of tests/exact_cases.py the logical output equals the fp64 oracle (``torch.equal``), holds
no sentinel, and no sentinel outside it changed.

Part B, propagation: +inf / -inf / NaN where the result depends on them, against the fp64 reference on the
same inputs — finite and equal where it is finite, non-finite where it is not (never silently finite), the
same class where the kernel only selects, adds and scales; the maximum follows torch.max's order with the
first edge as arg, whatever the chunk, the route or the readout's slab cut (include/sirconv.h, "Non-finite
values")."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import exact_cases as xc
import oracle
import poison_cases as pc
import test_exact_gpu as xg

from sirgcn import _native, edgemlp

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = xg.DTYPES
NAN, INF = pc.NAN, pc.INF


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


@contextlib.contextmanager
def _abi_args(name):
    """Record the integer arguments of every call of the exported function ``name`` (leading dimensions
    among them): what reached the ABI, not what a Python layer was given."""
    lib = _native.load()
    orig, seen = getattr(lib, name), []

    def rec(*a):
        seen.append([x.value if isinstance(x, ctypes.c_void_p) else x for x in a])
        return orig(*a)
    setattr(lib, name, rec)
    try:
        yield seen
    finally:
        setattr(lib, name, orig)


def _reached(args, *views):
    """Every view's base pointer is an argument of the recorded call and the argument after it (its leading
    dimension, in every signature of include/sirconv.h) is the view's row stride."""
    for k, v in enumerate(views):
        at = [i for i, x in enumerate(args) if isinstance(x, int) and not isinstance(x, bool) and x == v.data_ptr()]
        assert at, f"operand {k} did not reach the ABI by its own pointer (copied?)"
        assert any(i + 1 < len(args) and args[i + 1] == v.stride(0) for i in at), \
            f"operand {k} reached the ABI with another leading dimension than {v.stride(0)}"


def _slope(act):
    return xg.ACT[act]


def _g_over_deg(G, plan):
    """MEAN's g = G / deg in fp32, rounded once to G's type (include/sirconv.h), contiguous."""
    return torch.div(G, plan.in_degree_f(), out=torch.zeros(G.shape, dtype=G.dtype, device=G.device))


def _eq_nan(got, want, what):
    """Equality that treats NaN as a value (payloads aside)."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got != want))
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {list(i)}: "
                             f"got {got[i].item()!r}, want {want[i].item()!r}")


# ----------------------------------------------------------------------------- Part A: edge passes
EDGE_H = (4, 60, 128, 256, 776)
EDGE_CASES = [(d, H) for d in DTYPES for H in EDGE_H] + [("f32", H) for H in (3, 30)]


def _edge_backward_forms(plan, graph, H, agg, act, dtype, pad, mis, mask, what):
    """Every backward form on poisoned operands and sentinel outputs: recompute (two passes), sign-mask two-pass
    and one-launch.  dQ, dK equal the oracle; returns nothing."""
    code, slope = _slope(act)
    V = xc.GRAPHS[graph][2]
    Q, K, G = pc.edge_operands(graph, H, dtype, DEV, pad, mis)
    in_norm, out_norm = plan.norms(agg)
    _, wdQ, wdK = (xg._want(t, dtype) for t in xc.edge_expected(graph, H, agg, act))
    no_in, _ = pc.unreferenced(graph)
    n_part = max(plan.dst.n_slots, plan.src.n_slots, 1) * H
    forms = [("recompute", None, False)]
    if mask is not None:
        forms += [("sign-mask two-pass", mask, False), ("sign-mask one-launch", mask, True)]
    for name, m, dual in forms:
        w = f"{what} {name}"
        dQ, dK = pc.Out((V, H), dtype, DEV, pad, 2, mis), pc.Out((V, H), dtype, DEV, pad, 2, mis)
        part, part_s = pc.Out((1, n_part), torch.float32, DEV, 0, 0), pc.Out((1, n_part), torch.float32, DEV, 0, 0)
        if dual:
            g, bagg = G, agg
            if agg == "mean":       # as conv.edge_backward: the one-launch form runs SUM on g = G / deg
                gd = _g_over_deg(G, plan)
                gd[no_in.to(DEV)] = NAN
                g, bagg = pc.embed(gd, pad, 2, mis)[0], "sum"
            b_in, b_out = plan.norms(bagg)
            with _abi_args("sir_edge_agg_bwd") as seen:
                _native.edge_agg_bwd(plan.dst, plan.src, g, m, b_in, b_out, bagg, code, slope, dQ.view, dK.view,
                                     part.view[0], part_s.view[0])
            _reached(seen[-1], g, dQ.view, dK.view)
            part_s.check_outside(w + " partial_s")
        else:
            Gm = pc.Out((V, H), dtype, DEV, pad, 2, mis) if agg == "mean" else None
            qk = (None, None) if m is not None else (Q, K)
            with _abi_args("sir_edge_agg_bwd_dst") as seen:
                _native.edge_agg_bwd_dst(plan.dst, qk[0], qk[1], G, in_norm, out_norm, agg, code, slope, dQ.view,
                                         None if Gm is None else Gm.view, part.view[0], m)
            _reached(seen[-1], G, dQ.view, *([] if m is not None else [Q, K]), *([] if Gm is None else [Gm.view]))
            if Gm is not None:      # G / deg, rounded once; the rows of nodes without in-edges are don't-care
                Gm.check_outside(w + " Gm")
                rows = (~no_in).to(DEV)
                wGm = _g_over_deg(G, plan)
                xg._same(Gm.view[rows], wGm[rows], w + " Gm")
            _native.edge_agg_bwd_src(plan.src, qk[1], qk[0], G if Gm is None else Gm.view, out_norm, in_norm, agg, code,
                                     slope, dK.view, part.view[0], m)
        dQ.check(wdQ, w + " dQ")
        dK.check(wdK, w + " dK")
        part.check_outside(w + " partial")


@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("dt,H", EDGE_CASES, ids=[f"{d}-{H}" for d, H in EDGE_CASES])
def test_edge_passes_ignore_poison(dt, H, agg):
    """sir_edge_agg_fwd, _bwd_dst, _bwd_src (recompute and sign-mask) and sir_edge_agg_bwd at chunk 4 / 256:
    NaN in the pad columns and rows of Q, K, G, in Q[v] / G[v] of rows without in-edges and K[u] of nodes without
    out-edges, in the partial workspaces and (as sentinel) around S, the mask, dQ, dK, Gm.  H = 3, 30: the scalar
    path with a leading dimension that is no multiple of 4 and a base 4 bytes past a 16-byte boundary."""
    dtype = DTYPES[dt]
    pad, mis = (3, 1) if H % 4 else (4, 0)
    for graph in xg._graphs(agg):
        for act in xc.ACT_NAMES:
            nw = _native.mask_words(H, _slope(act)[0])
            for chunk in (4, 256):
                plan = xg._plan(graph, chunk)
                what = f"{graph} {dt} H={H} {agg} {act} chunk={chunk}"
                with _abi_args("sir_edge_agg_fwd") as seen:
                    S, mask = pc.check_edge_forward(_native, plan, graph, H, agg, act, dtype, DEV, pad, mis, nw)
                _reached(seen[-1], S.view)
                assert seen[-1].count(H + pad) >= 3, "Q, K, S must reach the ABI with their leading dimension"
                m = None
                if mask is not None:
                    xg._same_mask(mask.view, xc.expected_mask(graph, H), what)
                    m = mask.view.reshape(-1)
                _edge_backward_forms(plan, graph, H, agg, act, dtype, pad, mis, m, what)


@pytest.mark.parametrize("agg", ["sum", "sym"])
@pytest.mark.parametrize("dt,H", [("f32", 60), ("f32", 256), ("bf16", 128), ("f32", 30)])
def test_edge_forward_accumulate_ignores_poison(dt, H, agg):
    """SIR_AGG_ACCUMULATE: S[v] = S[v] + the sum, on an S that holds integers inside a sentinel allocation."""
    dtype = DTYPES[dt]
    pad, mis = (3, 1) if H % 4 else (4, 0)
    code, slope = _slope("leaky")
    for graph in xg._graphs(agg):
        V = xc.GRAPHS[graph][2]
        seed = xc.ints((V, H), 4, 77 + H)
        want = xg._want(seed.double() + xc.edge_expected(graph, H, agg, "leaky")[0], dtype)
        for chunk in (4, 256):
            plan = xg._plan(graph, chunk)
            Q, K, _ = pc.edge_operands(graph, H, dtype, DEV, pad, mis)
            S = pc.Out((V, H), dtype, DEV, pad, 2, mis).seed(seed.to(DEV, dtype))
            part = pc.Out((1, max(plan.dst.n_slots, 1) * H), torch.float32, DEV, 0, 0)
            in_norm, out_norm = plan.norms(agg)
            _native.edge_agg_fwd(plan.dst, Q, K, in_norm, out_norm, agg, code, slope, S.view, part.view[0], None,
                                 accumulate=True)
            S.check(want, f"accumulate {graph} {dt} H={H} {agg} chunk={chunk}")
            part.check_outside("accumulate partial")


# ----------------------------------------------------------------------------- Part A: SIREConv kernels
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("H", [4, 132, 256])
def test_sire_kernels_ignore_poison(H, agg):
    """sir_edge_e_agg_fwd / sir_edge_e_bwd with the edge term as a stream (eidx a permutation) and as an
    nn.Embedding-style table whose rows 5.. no edge references: those rows, the pads of Q, K, Eh, G and the
    partial workspace hold NaN; S, the mask and dE sit in sentinel allocations."""
    act = "leaky"
    code, slope = _slope(act)
    pad = 4
    for graph in xg._graphs(agg):
        V = xc.GRAPHS[graph][2]
        Q, K, G = pc.edge_operands(graph, H, torch.float32, DEV, pad)
        Eh = xc.edge_inputs(graph, H)[3]
        T, ids = xc.sire_table(graph, H)
        E = Eh.shape[0]
        nw = _native.mask_words(H, code)
        no_in = pc.unreferenced(graph)[0].to(DEV)
        for chunk in (4, 256):
            plan = xg._plan(graph, chunk)
            eid32 = plan.dst.eid.to(torch.int32)
            in_norm, out_norm = plan.norms(agg)
            Tpad = torch.cat([T, torch.full((3, H), NAN)])
            forms = {"perm": (pc.embed(Eh.to(DEV), pad)[0], eid32, None),
                     "table": (pc.embed(Tpad.to(DEV), pad, 0)[0], ids.to(DEV)[plan.dst.eid].to(torch.int32), (T, ids))}
            for form, (rows, eidx, table) in forms.items():
                what = f"sire {graph} H={H} {agg} chunk={chunk} eidx={form}"
                want = xc.sire_expected(graph, H, agg, act, table)
                S = pc.Out((V, H), torch.float32, DEV, pad)
                mask = pc.Out((E, nw), torch.int64, DEV, 0, 0)
                part = pc.Out((1, max(plan.dst.n_slots, 1) * H), torch.float32, DEV, 0, 0)
                with _abi_args("sir_edge_e_agg_fwd") as seen:
                    _native.edge_e_agg_fwd(plan.dst, Q, K, rows, eidx, in_norm, out_norm, agg, code, slope, S.view,
                                           part.view[0], mask.view.reshape(-1))
                _reached(seen[-1], Q, K, rows, S.view)
                S.check(xg._want(want["S"]), what + " S")
                part.check_outside(what + " partial")
                mask.check_written(what + " mask")
                mask.check_outside(what + " mask")
                xg._same_mask(mask.view, xc.expected_mask(graph, H, True, None if table is None else T[ids]), what)
                g, bagg = G, ("sum" if agg == "mean" else agg)
                if agg == "mean":
                    gd = _g_over_deg(G, plan)
                    gd[no_in] = NAN
                    g = pc.embed(gd, pad)[0]
                b_in, b_out = plan.norms(bagg)
                dE = pc.Out((E, H), torch.float32, DEV, pad)
                _native.edge_e_bwd(plan.dst, mask.view.reshape(-1), g, b_in, b_out, bagg, code, slope,
                                   eidx if form == "perm" else None, dE.view)
                wdE = xg._want(want["dE"])
                dE.check(wdE if form == "perm" else wdE[plan.dst.eid], what + " dE")


# ----------------------------------------------------------------------------- Part A: edge-materialised helpers
@pytest.mark.parametrize("graph,agg", xg.GRAPH_AGG)
@pytest.mark.parametrize("F", [3, 64, 256])
def test_edge_materialised_helpers_ignore_poison(F, graph, agg):
    """sir_edge_gather_add, _gather_act (with the sign words at F = 256), sir_segment_sum (plain, norms / mean,
    ``perm``), sir_edge_broadcast, sir_segment_max / _max_bwd on embedded operands (F = 3: a leading dimension
    that is no multiple of 4 and a misaligned base), NaN workspaces, sentinel outputs."""
    src, dst, V = xc.GRAPHS[graph]
    E = src.numel()
    pad, mis = (3, 1) if F % 4 else (4, 0)
    no_in, no_out = pc.unreferenced(graph)
    Q, K, dS = (xc.ints((V, F), 4, 300 + F + i) for i in range(3))
    M, dZ = xc.ints((E, F), 4, 310 + F), xc.ints((E, F), 4, 311 + F)
    ind = torch.bincount(dst, minlength=V).clamp(min=1).double()[:, None]
    in_norm, out_norm = oracle.degree_norms(torch.bincount(dst, minlength=V), torch.bincount(src, minlength=V), agg)
    c = (out_norm[src] * in_norm[dst]).double()[:, None]
    wS = torch.zeros(V, F, dtype=torch.float64).index_add_(0, dst, c * M.double())
    wdM = c * dS.double()[dst]
    if agg == "mean":
        wS, wdM = wS / ind, wdM / ind[dst]
    wY, warg = oracle.max_first_wins(dst, V, M.double())
    emb = lambda t: pc.embed(t.to(DEV), pad, 2, mis)[0]
    out = lambda rows, dtype=torch.float32: pc.Out((rows, F), dtype, DEV, pad, 2, mis)
    ws = lambda n, dtype=torch.float32: pc.Out((1, max(n, 1) * F), dtype, DEV, 0, 0)
    code, slope = _slope("leaky")
    for chunk in (4, 256):
        plan = xg._plan(graph, chunk)
        eid = plan.dst.eid
        p_in, p_out = plan.norms(agg)
        what = f"generic {graph} {agg} F={F} chunk={chunk}"
        Qp, Kp = emb(pc.poison_rows(Q, no_in)), emb(pc.poison_rows(K, no_out))
        Z = out(E)
        with _abi_args("sir_edge_gather_add") as seen:
            _native.edge_gather_add(plan.dst, Qp, Kp, Z.view)
        _reached(seen[-1], Qp, Kp, Z.view)
        wZ = (Q[dst] + K[src])[eid.cpu()]
        Z.check(wZ.to(DEV), what + " gather_add")
        A = out(E)
        smask = pc.Out((E, 4), torch.int64, DEV, 0, 0) if F == 256 else None
        _native.edge_gather_act(plan.dst, Qp, Kp, code, slope, A.view, None if smask is None else smask.view)
        wA = oracle.act_fwd(wZ.double(), "leaky", xc.SLOPE)
        A.check(xg._want(wA), what + " gather_act")
        if smask is not None:       # bit l of word x = A[e][4 l + x] > 0
            smask.check_outside(what + " sign words")
            pos = (wA > 0).numpy().reshape(E, 64, 4)
            words = (pos.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, :, None]).sum(1, dtype=np.uint64)
            assert np.array_equal(smask.view.cpu().numpy().view(np.uint64), words), what + " sign words"
        n_slots = max(plan.dst.n_slots, plan.src.n_slots)
        dZe = emb(dZ.to(DEV)[eid].cpu())
        for csr, perm, by, name in ((plan.dst, None, dst, "segment_sum (dQ)"), (plan.src, plan.src.perm, src, "segment_sum perm (dK)")):
            o, part = out(V), ws(n_slots)
            _native.segment_sum(csr, dZe, o.view, perm=perm, partial=part.view[0])
            o.check(xg._want(torch.zeros(V, F, dtype=torch.float64).index_add_(0, by, dZ.double())), f"{what} {name}")
            part.check_outside(f"{what} {name} partial")
        Me = emb(M.to(DEV)[eid].cpu())
        S, part = out(V), ws(plan.dst.n_slots)
        _native.segment_sum(plan.dst, Me, S.view, p_in, p_out, agg == "mean", partial=part.view[0])
        S.check(xg._want(wS), what + " segment_sum")
        part.check_outside(what + " segment_sum partial")
        dM = out(E)
        _native.edge_broadcast(plan.dst, emb(pc.poison_rows(dS, no_in)), dM.view, p_in, p_out, agg == "mean")
        dM.check(xg._want(wdM)[eid], what + " edge_broadcast")
        if agg == "sum":
            Y, arg = out(V), out(V, torch.int32)
            pval, parg = ws(plan.dst.n_slots), ws(plan.dst.n_slots, torch.int32)
            _native.segment_max(plan.dst, Me, Y.view, arg.view, pval.view[0], parg.view[0])
            Y.check(xg._want(wY), what + " segment_max")
            arg.check_written(what + " segment_max arg")
            arg.check_outside(what + " segment_max arg")
            pval.check_outside(what + " pval")
            parg.check_outside(what + " parg")
            xg._same(xg._edge_ids(plan, arg.view.contiguous()), warg.to(DEV), what + " segment_max arg")
            dMx = out(E)
            _native.segment_max_bwd(plan.dst, arg.view, emb(pc.poison_rows(dS, no_in)), dMx.view)
            wdMax = torch.zeros(E, F, dtype=torch.float64)
            r, f = torch.nonzero(warg >= 0, as_tuple=True)
            wdMax[warg[r, f], f] = dS.double()[r, f]
            dMx.check(xg._want(wdMax)[eid], what + " segment_max_bwd")


# ----------------------------------------------------------------------------- Part A: fused edge MLP
def _mlp_operands(graph, H, F, pad=4):
    Q, K, W, b, G = xc.mlp_inputs(graph, H, F)
    no_in, no_out = pc.unreferenced(graph)
    Qp = pc.embed(pc.poison_rows(Q, no_in).to(DEV), pad)[0]
    Kp = pc.embed(pc.poison_rows(K, no_out).to(DEV), pad)[0]
    return Qp, Kp, W.to(DEV), b.to(DEV), G


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("graph", ["A", "B"])
@pytest.mark.parametrize("H,O", [(64, 64), (100, 200), (256, 40)])
def test_max_forward_ignores_poison(H, O, graph, act, monkeypatch):
    """sir_edge_mlp_fwd / _fwd_stream and the 16-bit _fwd_st / _fwd_stream_st (max): embedded Q, K with NaN pads
    and NaN rows of the nodes the result does not depend on, NaN-filled partials, Y and arg in sentinel
    allocations — Y, arg equal the first-wins oracle."""
    Qp, Kp, W, b, _ = _mlp_operands(graph, H, O)
    V = Qp.shape[0]
    want = xc.max_expected(graph, H, O, act)
    wY, warg = xg._want(want["Y"]), want["arg"].to(DEV)
    code, slope = _slope(act)
    for dt, dtype in DTYPES.items():
        runs = [(False, c) for c in (4, 256)] + ([(True, 256)] if H == 256 else [])
        for stream, chunk in runs:
            monkeypatch.setattr(edgemlp, "STREAM", stream)
            plan = xg._plan(graph, chunk)
            what = f"max {graph} {act} H={H} O={O} {dt} {'stream' if stream else f'chunk={chunk}'}"
            Y, arg = pc.Out((V, O), torch.float32, DEV), pc.Out((V, O), torch.int32, DEV)
            name = "sir_edge_mlp_fwd" + ("_stream" if stream else "") + ("" if dt == "f32" else "_st")
            with pc.poisoned_empty(), _abi_args(name) as seen:
                if dt == "f32":
                    qk = (Qp, Kp)
                    edgemlp._fwd(plan, Qp, Kp, W, b, "max", code, slope, _native.ACT_IDENTITY, Y.view, arg.view)
                else:
                    qk = (pc.embed(Qp.to(dtype), 4)[0], pc.embed(Kp.to(dtype), 4)[0])
                    edgemlp._fwd_st(plan, qk[0], qk[1], W, b, code, slope, Y.view, arg.view)
            _reached(seen[-1], qk[0], qk[1], Y.view, arg.view)
            Y.check(wY, what + " Y")
            arg.check_written(what + " arg")
            arg.check_outside(what + " arg")
            xg._same(xg._edge_ids(plan, arg.view.contiguous()), warg, what + " arg")


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("graph", ["A", "B"])
@pytest.mark.parametrize("H,O", [(64, 64), (100, 200), (256, 40)])
def test_max_backward_routes_ignore_poison(H, O, graph, act, monkeypatch):
    """Every max backward route within its limits (sir_edge_max_bwd_sparse, sir_edge_max_bwd_dst / _src,
    sir_max_dw_qk, sir_max_dw_rows, the edge-materialised helpers with sir_gemm_nt_dact and the TN GEMM): Q, K
    embedded with NaN pads and NaN rows of the nodes the result does not depend on, NaN in dY of the rows
    without edges, every float workspace the Python layer allocates NaN-filled, dQ / dK in sentinel allocations."""
    code, slope = _slope(act)
    Qp, Kp, W, b, dY = _mlp_operands(graph, H, O)
    V = Qp.shape[0]
    dYp = pc.poison_rows(dY, pc.unreferenced(graph)[0]).to(DEV)
    want = {k: xg._want(v) for k, v in xc.max_expected(graph, H, O, act).items() if k != "arg"}
    monkeypatch.setattr(edgemlp, "STREAM", False)
    ran = 0
    for chunk in (4, 256):
        plan = xg._plan(graph, chunk)
        _, arg = xg._max_forward(plan, Qp, Kp, W, b, act, torch.float32)
        for route, (switches, applies) in xg.MAX_ROUTES.items():
            if not applies(H, O, V):
                continue
            for k, v in switches.items():
                monkeypatch.setattr(edgemlp.EdgeMaxLinear, k, v)
            what = f"max {graph} {act} H={H} O={O} chunk={chunk} {route}"
            dQ, dK = pc.Out((V, H), torch.float32, DEV), pc.Out((V, H), torch.float32, DEV)
            with pc.poisoned_empty() as filled:
                dW, db = edgemlp.max_linear_backward(plan, Qp, Kp, W, arg, dYp, code, slope, dQ.view, dK.view)
            assert len(filled) >= 2, "the route's workspaces were not allocated through torch.empty"
            dQ.check(want["dQ"], what + " dQ")
            dK.check(want["dK"], what + " dK")
            xg._same(dW.contiguous(), want["dW"], what + " dW_R")
            xg._same(db.contiguous(), want["db"], what + " db_R")
            ran += 1
    assert ran >= 4


@pytest.mark.parametrize("graph,agg", xg.GRAPH_AGG)
@pytest.mark.parametrize("H,F", xc.SEQ_SHAPES[:2] + ((256, 256),))     # H = 256: sir_edge_mlp_fwd_stream
def test_seq_sigma_kernels_ignore_poison(H, F, graph, agg):
    """sir_edge_mlp_fwd (sum family) / _bwd_dst / _bwd_src through EdgeMLPSum (which copies QK to a contiguous
    tensor: no leading dimension to embed): NaN in Q[v], dS[v] of rows without in-edges and K[u] of nodes without
    out-edges, S, dQK, Gm and every workspace (pval, partial, wpart, the col-sum's) NaN-filled before the call."""
    Q, K, W, b, G = xc.mlp_inputs(graph, H, F)
    no_in, no_out = pc.unreferenced(graph)
    want = {k: xg._want(v) for k, v in xc.seq_expected(graph, H, F, agg).items()}
    for chunk in (4, 256):
        what = f"seq {graph} {agg} H={H} F={F} chunk={chunk}"
        QK = torch.cat([pc.poison_rows(Q, no_in), pc.poison_rows(K, no_out)], 1).to(DEV).requires_grad_(True)
        Wr, br = W.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with pc.poisoned_empty() as filled:
            S = edgemlp.EdgeMLPSum.apply(QK, Wr, br, xg._plan(graph, chunk), H, agg, _native.ACT_RELU, 0.0,
                                         _native.ACT_RELU)
            S.backward(pc.poison_rows(G, no_in).to(DEV))
        V = QK.shape[0]
        assert (V, F) in filled and (V, 2 * H) in filled and len(filled) >= 5, "S, dQK, wpart, partial, col-sum"
        xg._same(S.detach(), want["S"], what + " S")
        xg._same(QK.grad[:, :H], want["dQ"], what + " dQ")
        xg._same(QK.grad[:, H:], want["dK"], what + " dK")
        xg._same(Wr.grad, want["dW"], what + " dW")
        xg._same(br.grad, want["db"], what + " db")


# ----------------------------------------------------------------------------- Part B: edge passes
def _bits_equal(a, b, what):
    """Bit identity of two results, a NaN matching a NaN: which of the NaN encodings a rounding to 16 bits
    yields is not part of any contract (the kernels' and torch's differ), its position is."""
    ba, bb = pc.bits(a.contiguous()), pc.bits(b.contiguous())
    bad = (ba != bb) & ~(torch.isnan(a) & torch.isnan(b))
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ in their bits, first at {list(i)}: "
                             f"{a[i].item()!r} vs {b[i].item()!r}")


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("site", list(pc.SITES))
def test_edge_passes_propagate_nonfinite(site, agg, act):
    """+inf, -inf, NaN in Q / K (an unsplit row, a hub row split at chunk 4, +inf meeting -inf in one sum) and
    in G (sigma' = 0 with t = inf): S, dQ, dK have the reference's value where it is finite and its class where
    it is not; with a non-finite z the rows of dQ / dK the poisoned edges touch are exempt (include/sirconv.h).
    The backward forms stay bit-identical to each other."""
    code, slope = _slope(act)
    for dt, H in (("f32", 12), ("f32", 256), ("bf16", 12), ("f32", 7)):
        dtype = DTYPES[dt]
        Q, K, G = (t.to(DEV, dtype) for t in pc.edge_case(H, site))
        wS, wdQ, wdK, ex_q, ex_k = pc.edge_case_expected(H, site, agg, act)
        rq, rk = (~ex_q).to(DEV), (~ex_k).to(DEV)
        per_chunk = []
        for chunk in (4, 256):
            plan = xg._plan("A", chunk)
            what = f"{site} {dt} H={H} {agg} {act} chunk={chunk}"
            S, mask = xg._edge_forward(plan, H, agg, act, Q, K, dtype)
            pc.check_propagation(S, wS, what + " S")
            got = []
            for name, m, dual in xg._backward_modes(mask):
                dQK = xg._edge_backward(plan, H, agg, act, G, Q, K, m, dual, dtype)
                pc.check_propagation(dQK[:, :H], wdQ, f"{what} {name} dQ", rows=rq)
                pc.check_propagation(dQK[:, H:], wdK, f"{what} {name} dK", rows=rk)
                got.append(dQK)
            if site == "G":             # finite z: nothing is exempt, and every form gives the same bits
                for other in got[1:]:
                    _bits_equal(got[0], other, what + " backward forms")
            elif len(got) == 3:
                _bits_equal(got[1], got[2], what + " one-launch vs two-pass")
            per_chunk.append((S, got[0]))
        if site == "G":
            _bits_equal(per_chunk[0][1], per_chunk[1][1], f"{site} {dt} H={H} {agg} {act}: chunk 4 vs 256")


# ----------------------------------------------------------------------------- Part B: the maximum
def _max_want(dst, V, M64):
    Y, arg = pc.max_nan_wins(dst, V, M64)
    return Y.float().to(DEV), arg.to(DEV)


@pytest.mark.parametrize("kind", ["inf", "nan"])
@pytest.mark.parametrize("graph", ["A", "B"])
@pytest.mark.parametrize("F", [3, 64])
def test_segment_max_nonfinite(F, graph, kind):
    """sir_segment_max with +-inf / NaN among the candidates at chunk 4 / 64 / 256: torch.max's order, the first
    of equals and the first NaN as arg; a row of -inf gives -inf and its first edge; sir_segment_max_bwd routes
    dY to exactly that edge."""
    src, dst, V = xc.GRAPHS[graph]
    M = pc.max_messages_case(graph, F, kind)
    E = M.shape[0]
    wY, warg = _max_want(dst, V, M.double())
    dY = xc.ints((V, F), 4, 99 + F).to(DEV)
    wdM = torch.zeros(E, F)
    r, f = torch.nonzero(warg.cpu() >= 0, as_tuple=True)
    wdM[warg.cpu()[r, f], f] = dY.cpu()[r, f]
    for chunk in (4, 64, 256):
        plan = xg._plan(graph, chunk)
        what = f"segment_max {kind} {graph} F={F} chunk={chunk}"
        Y = torch.full((V, F), 7.0, device=DEV)
        arg = torch.full((V, F), -2, device=DEV, dtype=torch.int32)
        n = plan.dst.n_slots
        pval = torch.full((max(n, 1) * F,), NAN, device=DEV)
        parg = torch.full((max(n, 1) * F,), -2, device=DEV, dtype=torch.int32)
        _native.segment_max(plan.dst, M.to(DEV)[plan.dst.eid].contiguous(), Y, arg, pval, parg)
        _eq_nan(Y, wY, what + " Y")
        xg._same(xg._edge_ids(plan, arg), warg, what + " arg")
        dM = torch.full((E, F), NAN, device=DEV)
        _native.segment_max_bwd(plan.dst, arg, dY, dM)
        xg._same(dM, wdM.to(DEV)[plan.dst.eid], what + " dM")


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("graph", ["A", "B"])
@pytest.mark.parametrize("H,O", [(64, 64), (100, 200), (256, 40)])
def test_max_forward_nonfinite(H, O, graph, act, monkeypatch):
    """The fused edge-MLP max forward (fp32 per-item kernels at chunk 4 / 64 / 256, the stream kernel at H = 256,
    the 16-bit forms) with every message of a column -inf, +inf or NaN and with NaN rows of Q / K: the value and
    the arg edge equal the edge-materialised route's (sir_segment_max on the reference messages) and the oracle's
    — a row with edges always takes an edge (all -inf: -inf and the first edge, all NaN: NaN and the first
    edge), whatever the chunk."""
    src, dst, V = xc.GRAPHS[graph]
    Q, K, W, b, wY64, warg = pc.mlp_max_case(graph, H, O, act)
    wY, warg = wY64.float().to(DEV), warg.to(DEV)
    has = torch.bincount(dst, minlength=V) > 0
    clean = has & torch.isfinite(wY64[:, 3:]).all(1)           # rows no NaN of Q / K reaches
    assert bool((warg.cpu()[has] >= 0).all()) and bool(clean.any()) and bool((wY64[clean][:, 0] == -INF).all())
    assert bool((wY64[clean][:, 1] == INF).all()) and bool(torch.isnan(wY64[has][:, 2]).all())
    assert pc.rows_share(wY64[:, 3:]) <= 0.25 and bool(torch.isnan(wY64[:, 3:]).all(1).any())
    code, slope = _slope(act)
    Qd, Kd, Wd, bd = (t.to(DEV) for t in (Q, K, W, b))
    # the edge-materialised route on the same messages (fp64 reference messages, exact in fp32)
    M32 = (oracle.act_fwd(Q.double()[dst] + K.double()[src], act, xc.SLOPE) @ W.double().t() + b.double()).float()
    for dt, dtype in DTYPES.items():
        runs = [(False, c) for c in (4, 64, 256)] + ([(True, 256)] if H == 256 else [])
        for stream, chunk in runs:
            monkeypatch.setattr(edgemlp, "STREAM", stream)
            plan = xg._plan(graph, chunk)
            what = f"max non-finite {graph} {act} H={H} O={O} {dt} {'stream' if stream else f'chunk={chunk}'}"
            Y, arg = xg._max_forward(plan, Qd, Kd, Wd, bd, act, dtype)
            _eq_nan(Y, wY, what + " Y")
            xg._same(xg._edge_ids(plan, arg), warg, what + " arg")
            if dt == "f32" and not stream:
                Ym = torch.full((V, O), 7.0, device=DEV)
                am = torch.full((V, O), -2, device=DEV, dtype=torch.int32)
                n = plan.dst.n_slots
                _native.segment_max(plan.dst, M32.to(DEV)[plan.dst.eid].contiguous(), Ym, am,
                                    torch.empty(max(n, 1) * O, device=DEV),
                                    torch.empty(max(n, 1) * O, device=DEV, dtype=torch.int32))
                _eq_nan(Y, Ym, what + " fused vs edge-materialised Y")
                xg._same(arg, am, what + " fused vs edge-materialised arg")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("F", [5, 64])
def test_readout_max_nonfinite(F, dt):
    """sir_graph_pool_fwd (max) with +-inf / NaN among a graph's rows, on a graph of more than one slab (a NaN
    on either side of the slab boundary, another one in the last slab), short graphs and an empty one: value and
    arg as torch.max's order gives them, the first NaN's row as arg; sum / mean keep the IEEE class; the backward
    routes dP to exactly the arg row."""
    dtype = DTYPES[dt]
    R = _native.POOL_SLAB_ROWS
    ns = [R + 9, 0, 5, 2 * R + 1, 20]
    V, B = sum(ns), len(ns)
    off = torch.tensor([0] + ns).cumsum(0)
    X = xc.ints((V, F), 4, 600 + F)
    gid = torch.repeat_interleave(torch.arange(B), torch.tensor(ns))
    g0 = int(off[3])
    X[R - 1, 0], X[R, 0] = NAN, NAN             # graph 0: the last row of slab 0 and the first of slab 1
    X[R + 3, 1], X[2, 1] = INF, INF             # the first +inf wins
    X[:ns[0], 2] = -INF                          # every row -inf: -inf and row 0
    X[g0 + 2 * R, 0] = NAN                       # graph 3: a NaN in its last slab only
    X[g0 + R + 1, 1], X[g0 + 7, 1] = -INF, INF
    X[int(off[2]):int(off[3]), 3] = NAN          # a short graph, all NaN
    X[int(off[4]) + 4, 4] = -INF
    X16 = X.to(dtype)
    wY, warg = pc.max_nan_wins(gid, B, X16.double())
    warg = torch.where(warg >= 0, warg - off[:-1, None], warg)         # row within its graph
    Xd = X16.to(DEV)
    offd = off.to(DEV)
    P = torch.full((B, F), 7.0, device=DEV, dtype=dtype)
    arg = torch.full((B, F), -2, device=DEV, dtype=torch.int32)
    with pc.poisoned_empty():
        _native.graph_pool_fwd(offd, Xd, _native.POOL_MAX, P, arg)
    _eq_nan(P, wY.to(dtype).to(DEV), f"readout max {dt} F={F} P")
    live = torch.tensor(ns) > 0
    xg._same(arg[live.to(DEV)].long(), warg[live].to(DEV), f"readout max {dt} F={F} arg")
    dP = xc.ints((B, F), 4, 601).to(DEV, dtype)
    dX = torch.full((V, F), NAN, device=DEV, dtype=dtype)
    _native.graph_pool_bwd(offd, dP, _native.POOL_MAX, dX, arg)
    wdX = torch.zeros(V, F, dtype=dtype)
    for bi in torch.nonzero(live).flatten().tolist():
        wdX[off[bi] + warg[bi], torch.arange(F)] = dP.cpu()[bi]
    xg._same(dX, wdX.to(DEV), f"readout max {dt} F={F} dX")
    if dt == "f32":     # sum / mean: the class IEEE arithmetic gives (exact otherwise: integers, power-of-two-free n aside)
        n = torch.tensor(ns, dtype=torch.float64).clamp(min=1)[:, None]
        tot = torch.zeros(B, F, dtype=torch.float64).index_add_(0, gid, X.double())
        for op, code, ref in (("sum", _native.POOL_SUM, tot), ("mean", _native.POOL_MEAN, tot / n)):
            Ps = torch.full((B, F), 7.0, device=DEV)
            with pc.poisoned_empty():
                _native.graph_pool_fwd(offd, Xd, code, Ps)
            # the mean is one fp32 division of the exact integer sum: fp32(sum / n) is its correctly rounded value
            pc.check_propagation(Ps, ref, f"readout {op} F={F}")


# ----------------------------------------------------------------------------- GEMMs
def _tn_call(fn, A, B, C, cs, dt=None):
    """sir_gemm_tn / sir_gemm_tn16 with a NaN-filled workspace of the queried size and a sentinel tail."""
    lib = _native.load()
    R, M = A.shape
    N = B.shape[1]
    nbytes = int(lib.sir_gemm_tn_workspace(R, M, N))
    ws = pc.Out((1, max(nbytes // 4, 1)), torch.float32, DEV, 0, 0)
    P, st = _native._ptr, _native._stream(A.device)
    args = [P(A), A.stride(0), P(B), B.stride(0), R, M, N] + ([_native._DT16[dt]] if dt is not None else []) + \
           [P(C), C.stride(0), P(cs), P(ws.view), 4 * ws.view.numel(), st]
    _native._check(getattr(lib, fn)(*args), lib)
    ws.check_outside(fn + " workspace")


GEMM_SHAPES = [(M, K, N) for M in (1, 513) for K in (128, 256, 100) for N in (40, 260)]
# SIR_GEMM_SMALL_ROWS moves the row threshold per call (tests/test_gemm_gpu.py): "small" = the one-wave kernels
# (k_gemm_nt_s / k_gemm_tn_s), "block" = the block-tiled ones at every M: the persistent k_gemm_nt_p with its fused
# dact epilogue at N = 260, K = 128 / 256, k_gemm_nt (K = 100: the kfull = false form; N = 40: the 128-wide tiles)
# with the k_gate_dact post-pass, and the block TN kernels with their running column scales
GEMM_ROUTES = {"small": "1000000000", "block": "0"}


@pytest.mark.parametrize("route", list(GEMM_ROUTES))
@pytest.mark.parametrize("M,K,N", GEMM_SHAPES)
def test_gemms_ignore_poison(M, K, N, route, monkeypatch):
    """sir_gemm_nt on the one-wave, the persistent and the block route, _nt_dact (fused epilogue and post-pass),
    _nt_direct, _nt_direct2, sir_gemm_tn, sir_gemm_tn16 (one-wave and block) and sir_gemm_nt16 with Acopy, on
    integers: A / B with NaN pad columns (lda > K, ldb > N) and NaN rows past M / R, C (and colsum, Acopy) in
    sentinel allocations, the TN workspace NaN-filled with a sentinel tail."""
    monkeypatch.setenv("SIR_GEMM_SMALL_ROWS", GEMM_ROUTES[route])
    what = f"{route} M={M} K={K} N={N}"
    A, W, b = xc.gemm_inputs(M, K, N)
    _, W2, _ = xc.gemm_inputs(M + 1, K, N)
    B = xc.ints((M, N), 4, 17 + M + K + N)
    gate = xc.ints((M, N), 2, 23 + M + K + N)
    wC = A.double() @ W.double().t()
    emb = lambda t, pad=4: pc.embed(t.to(DEV), pad)[0]
    out = lambda r, c, dtype=torch.float32, pad=4: pc.Out((r, c), dtype, DEV, pad)
    Ae, bd = emb(A), b.to(DEV)
    packed = _native.gemm_pack(emb(W))
    C = out(M, N)
    with _abi_args("sir_gemm_nt") as seen:
        _native.gemm_nt(Ae, packed, bd, out=C.view)
    _reached(seen[-1], Ae, C.view)
    C.check(xg._want(wC + b.double()), what + " gemm_nt")
    code, slope = _slope("leaky")
    ge = emb(gate)
    C = out(M, N)
    _native.gemm_nt_dact(Ae, packed, ge, code, slope, out=C.view)
    C.check(xg._want(torch.where(gate.double() > 0, wC, wC * xc.SLOPE)), what + " gemm_nt_dact")
    C = out(M, N)
    _native.gemm_nt_direct(Ae, emb(W), False, bd, out=C.view)
    C.check(xg._want(wC + b.double()), what + " gemm_nt_direct")
    C = out(M, 2 * N)
    _native.gemm_nt_direct2(Ae, emb(W), emb(W2), False, bd, out=C.view)
    C.check(xg._want(torch.cat([wC + b.double(), A.double() @ W2.double().t()], 1)), what + " gemm_nt_direct2")
    wT = A.double().t() @ B.double()
    Be = emb(B)
    C, cs = out(K, N), pc.Out((1, K), torch.float32, DEV, 0, 0)
    _tn_call("sir_gemm_tn", Ae, Be, C.view, cs.view[0])
    C.check(xg._want(wT), what + " gemm_tn")
    cs.check(xg._want(A.double().sum(0))[None], what + " gemm_tn colsum_a")
    for dt in (torch.bfloat16, torch.float16):
        A16, B16 = emb(A.to(dt), 8), emb(B.to(dt), 8)
        C, cs = out(K, N), pc.Out((1, K), torch.float32, DEV, 0, 0)
        _tn_call("sir_gemm_tn16", A16, B16, C.view, cs.view[0], dt)
        C.check(xg._want(wT), f"{what} gemm_tn16 {dt}")
        cs.check(xg._want(A.double().sum(0))[None], f"{what} gemm_tn16 colsum {dt}")
        if K in (128, 256) and N % 8 == 0:
            C, Ac = out(M, N), out(M, K, dt, 8)
            _native.gemm_nt16(Ae, _native.gemm_pack16(emb(W), dt), bd, torch.float32, acopy=Ac.view, out=C.view)
            C.check(xg._want(wC + b.double()), f"{what} gemm_nt16 {dt}")
            Ac.check(A.to(dt).to(DEV), f"{what} gemm_nt16 Acopy {dt}")


@pytest.mark.parametrize("route", list(GEMM_ROUTES))
@pytest.mark.parametrize("M,K,N", [(513, 256, 40), (33, 100, 260), (513, 128, 260)])
def test_gemms_keep_nonfinite_rows_apart(M, K, N, route, monkeypatch):
    """A NaN / Inf in one data row of a GEMM makes exactly the rows (NT) or the row and the column (TN) of C
    non-finite that the reference marks — a row scale may turn Inf into NaN, never into a number — and reaches
    no other row: everything else equals the integer result."""
    monkeypatch.setenv("SIR_GEMM_SMALL_ROWS", GEMM_ROUTES[route])
    what = f"{route} M={M} K={K} N={N}"
    A, W, b, B = pc.gemm_nonfinite_case(M, K, N)
    ref = A.double() @ W.double().t() + b.double()
    assert pc.rows_share(ref) <= 0.25 and int((~torch.isfinite(ref)).any(1).sum()) == 3
    Ad, Bd, bd = A.to(DEV), B.to(DEV), b.to(DEV)
    for name, C in (("gemm_nt", _native.gemm_nt(Ad, _native.gemm_pack(W.to(DEV)), bd)),
                    ("gemm_nt_direct", _native.gemm_nt_direct(Ad, W.to(DEV), False, bd))):
        pc.check_propagation(C, ref, f"{what} {name}", same_class=False)
    refT = A.double().t() @ B.double()
    bad = ~torch.isfinite(refT)           # whole rows (a bad A column) and whole columns (a bad B column), nothing else
    rows, cols = bad.all(1), bad.all(0)
    assert 0 < float(rows.float().mean()) <= 0.25 and 0 < float(cols.float().mean()) <= 0.25
    assert torch.equal(bad, rows[:, None] | cols[None, :])
    C, cs = _native.gemm_tn(Ad, Bd, colsum=True)
    pc.check_propagation(C, refT, what + " gemm_tn", same_class=False)
    pc.check_propagation(cs, A.double().sum(0), what + " gemm_tn colsum_a", same_class=False)
    for dt in (torch.bfloat16, torch.float16):
        C, cs = _native.gemm_tn16(Ad.to(dt), Bd.to(dt), colsum=True)
        pc.check_propagation(C, refT, f"{what} gemm_tn16 {dt}", same_class=False)
        pc.check_propagation(cs, A.double().sum(0), f"{what} gemm_tn16 colsum {dt}", same_class=False)


# ----------------------------------------------------------------------------- norms
def test_node_norms_ignore_poison():
    """sir_batch_norm_stats / _act_fwd / _act_bwd and sir_layer_norm_act_fwd / _bwd through GraphBatchNorm /
    GraphLayerNorm on an X embedded in NaN (misaligned base and ld, and aligned), every float allocation of the
    Python layer (outputs, work, partials) NaN-filled: inside the bound of the kernels' own parity test
    (tests/test_nodenorm_gpu.py, imported) and bit-equal to the same step on clean contiguous operands."""
    import test_nodenorm_gpu as nt
    from sirgcn import GraphBatchNorm, GraphLayerNorm
    R = nt.R
    for aligned, wrap in ((False, lambda x: pc.embed(x, 3, 2, 1)[0]), (True, lambda x: pc.embed(x, 4, 2, 0)[0])):
        with pc.poisoned_empty():
            nt._bn_case(R + 1, 75, wrap=wrap)
            nt._bn_case(3 * R + 7, 128, wrap=wrap)
            nt._ln_case(67, 75, wrap=wrap)
            nt._ln_case(67, 128, wrap=wrap)
        for cls, M, N in ((GraphBatchNorm, R + 1, 75), (GraphBatchNorm, 3 * R + 7, 128), (GraphLayerNorm, 67, 75),
                          (GraphLayerNorm, 1000, 128)):
            if N % 4 == 0 and not aligned:      # the scalar kernels of a misaligned view sum in another order
                continue
            xs, dys, gamma, beta = nt._data(M, N)
            X, dY = xs[0].to(DEV), dys[0].to(DEV)
            clean = nt._step(nt._init(cls(N), gamma, beta).to(DEV), X, dY)
            with pc.poisoned_empty():
                seen = []
                orig = _native._ld
                _native._ld = lambda t, H: seen.append(orig(t, H)) or seen[-1]
                try:
                    got = nt._step(nt._init(cls(N), gamma, beta).to(DEV), wrap(X), dY)
                finally:
                    _native._ld = orig
            assert wrap(X).stride(0) in seen, "the embedded X must reach the ABI with its leading dimension"
            for a, c, name in zip(got, clean, ("Y", "dX", "dweight", "dbias")):
                assert torch.equal(a, c), f"{cls.__name__} {M}x{N} {name}: embedded differs from contiguous"


@pytest.mark.parametrize("F", [6, 128, 300])
def test_graph_norm_ignores_poison(F):
    """sir_graph_norm_fwd / _bwd and the _act_ forms on embedded X, dY, R and sentinel Y, dX, mean, std, partials:
    bit-equal to the call on clean contiguous operands, inside the golden test's bound (1e-5, conftest.assert_parity)
    of the fp64 oracle, nothing outside the logical outputs written."""
    from conftest import assert_parity
    gen = torch.Generator().manual_seed(F)
    ns = [int(v) for v in torch.randint(1, 60, (12,), generator=gen)] + [0, 3]
    V, B = sum(ns), len(ns)
    off = torch.tensor([0] + ns).cumsum(0).to(DEV)
    X, dY, Rr = (torch.randn(V, F, generator=gen) for _ in range(3))
    w, b, ms = (torch.rand(F, generator=gen) + 0.5 for _ in range(3))
    eps = 1e-5
    pad, mis = (3, 1) if F % 4 else (4, 0)
    code, slope = _native.ACT_LEAKY, 0.2

    def run(embedded, fused):
        if embedded:
            e = lambda t: pc.embed(t.to(DEV), pad, 2, mis)[0]
            o = lambda r, c, p=pad, m=mis: pc.Out((r, c), torch.float32, DEV, p, 2 if p else 0, m)
        else:
            e = lambda t: t.to(DEV)
            o = lambda r, c, p=0, m=0: pc.Out((r, c), torch.float32, DEV, 0, 0, 0)
        Xe, dYe, Re = e(X), e(dY), e(Rr)
        Y, dX = o(V, F), o(V, F)
        mean, std = o(B, F, 0, 0), o(B, F, 0, 0)
        parts = [o(B, F, 0, 0) for _ in range(3)]
        wd, bd, msd = w.to(DEV), b.to(DEV), ms.to(DEV)
        if fused:
            _native.graph_norm_act_fwd(off, Xe, wd, bd, msd, eps, code, slope, Re, Y.view, mean.view, std.view)
            _native.graph_norm_act_bwd(off, Xe, dYe, wd, bd, msd, mean.view, std.view, code, slope, dX.view,
                                       parts[0].view, parts[2].view, parts[1].view)
        else:
            _native.graph_norm_fwd(off, Xe, wd, bd, msd, eps, Y.view, mean.view, std.view)
            _native.graph_norm_bwd(off, Xe, dYe, wd, msd, mean.view, std.view, dX.view, parts[0].view, parts[2].view,
                                   parts[1].view)
        outs = [Y, dX, mean, std] + parts
        for k, t in enumerate(outs):
            t.check_outside(f"graph norm F={F} fused={fused} output {k}")
        live = (torch.tensor(ns) > 0).to(DEV)
        for t in (Y, dX):
            t.check_written(f"graph norm F={F} fused={fused}")
        return [t.view.clone() for t in (Y, dX)] + [t.view[live].clone() for t in [mean, std] + parts]

    for fused in (False, True):
        clean, got = run(False, fused), run(True, fused)
        for k, (a, c) in enumerate(zip(got, clean)):
            assert torch.equal(a, c), f"graph norm F={F} fused={fused} output {k}: embedded differs from contiguous"
    Y, dX, mean, std, pw, pb, pms = run(True, False)
    ref = {}
    for dt in (torch.float32, torch.float64):
        a = [t.to(dt) for t in (X, dY, w, b, ms)]
        nz = [n for n in ns if n > 0]           # an empty graph has no rows and no share in any sum
        Yr, mr, sr = oracle.graph_norm_fwd(a[0], nz, a[2], a[3], a[4], eps)
        ref[dt] = (Yr,) + tuple(oracle.graph_norm_bwd(a[0], a[1], nz, a[2], a[4], mr, sr))
    r32, r64 = ref[torch.float32], ref[torch.float64]
    assert_parity(Y.cpu(), r32[0], r64[0], 1e-5, "Y")
    assert_parity(dX.cpu(), r32[1], r64[1], 1e-5, "dX")
    assert_parity(pw.sum(0).cpu(), r32[2], r64[2], 1e-5, "dweight")
    assert_parity(pb.sum(0).cpu(), r32[3], r64[3], 1e-5, "dbias")
    assert_parity(pms.sum(0).cpu(), r32[4], r64[4], 1e-5, "dmean_scale")


# ----------------------------------------------------------------------------- readout, resid-act, dropout, col-sum
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("F", [5, 64, 300])
def test_readout_ignores_poison(F, dt):
    """sir_graph_pool_fwd / _bwd (sum, mean, max) on the exact inputs of tests/readout_cases.py (graphs around
    and above one slab, empty graphs): X and dP embedded in NaN, P, dX and arg in sentinel allocations, the slab
    workspace NaN-filled.  Sum and max equal the oracle; the mean (a division) equals the call on clean operands."""
    import readout_cases as rc
    dtype = DTYPES[dt]
    ns, X, dP = rc.exact_inputs(_native.POOL_SLAB_ROWS)
    X, dP = X[:, :F].contiguous().to(dtype), dP[:, :F].contiguous().to(dtype)
    V, B = sum(ns), len(ns)
    off = rc.offsets(ns).to(DEV)
    pad, mis = ((3, 1) if dt == "f32" else (4, 0)) if F % 4 else (4, 0)
    live = (torch.tensor(ns) > 0).to(DEV)
    for op, code in (("sum", _native.POOL_SUM), ("mean", _native.POOL_MEAN), ("max", _native.POOL_MAX)):
        what = f"readout {op} {dt} F={F}"
        Xe, dPe = pc.embed(X.to(DEV), pad, 2, mis)[0], pc.embed(dP.to(DEV), pad, 2, mis)[0]
        P, dX = pc.Out((B, F), dtype, DEV, pad, 2, mis), pc.Out((V, F), dtype, DEV, pad, 2, mis)
        arg = pc.Out((B, F), torch.int32, DEV, 0, 0) if op == "max" else None
        a = None if arg is None else arg.view
        with pc.poisoned_empty(), _abi_args("sir_graph_pool_fwd") as seen:
            _native.graph_pool_fwd(off, Xe, code, P.view, a)
        _reached(seen[-1], Xe, P.view)
        _native.graph_pool_bwd(off, dPe, code, dX.view, a)
        if op == "mean":
            Pc = torch.empty((B, F), device=DEV, dtype=dtype)
            dXc = torch.empty((V, F), device=DEV, dtype=dtype)
            _native.graph_pool_fwd(off, X.to(DEV), code, Pc)
            _native.graph_pool_bwd(off, dP.to(DEV), code, dXc)
            wP, wdX = Pc, dXc
        else:
            wP64, warg = rc.pool_ref(X.double(), ns, op)
            wP, wdX = wP64.to(dtype).to(DEV), rc.pool_bwd_ref(dP.double(), warg, ns, op).to(dtype).to(DEV)
        P.check(wP, what + " P")
        dX.check(wdX, what + " dX")
        if arg is not None:
            arg.check_outside(what + " arg")
            xg._same(arg.view[live], warg.to(DEV)[live], what + " arg")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("order", [0, 1])
def test_resid_act_ignores_poison_and_propagates(order, dt):
    """sir_resid_act_fwd / _bwd on integers embedded in NaN, with +inf / -inf / NaN in Y, R and D: the output has
    the class IEEE arithmetic gives (ReLU(-inf) = 0, ReLU(NaN) = NaN), sigma' = 0 with an infinite gradient is 0,
    nothing outside the logical outputs is written."""
    dtype = DTYPES[dt]
    Y, R, D, D2 = pc.resid_case()
    M, N = Y.shape
    Y = Y.to(dtype)
    for act in ("relu", "leaky"):
        code, slope = _slope(act)
        what = f"resid_act order={order} {dt} {act}"
        Ye, Re, De, D2e = (pc.embed(t.to(DEV), 4)[0] for t in (Y, R, D, D2))
        out = pc.Out((M, N), torch.float32, DEV)
        _native.resid_act_fwd(Ye, Re, code, slope, order, out.view)
        z = Y.double() + R.double() if order == 0 else Y.double()
        ref = oracle.act_fwd(z, act, xc.SLOPE) + (0 if order == 0 else R.double())
        out.check_written(what)
        out.check_outside(what)
        pc.check_propagation(out.view, ref, what + " out")
        dYo, dRo = pc.Out((M, N), dtype, DEV), pc.Out((M, N), torch.float32, DEV)
        _native.resid_act_bwd(De, Ye, Re if order == 0 else None, code, slope, order, dYo.view, dRo.view, D2=D2e)
        g = D.double() + D2.double()
        rdY = oracle.act_bwd(z, g, act, xc.SLOPE)
        rows = torch.isfinite(z).all(1).to(DEV)            # a NaN z: deviation 2 of include/sirconv.h
        for o, r, name in ((dYo, rdY, "dY"), (dRo, rdY if order == 0 else g, "dR")):
            o.check_written(f"{what} {name}")
            o.check_outside(f"{what} {name}")
            pc.check_propagation(o.view, r, f"{what} {name}", rows=rows if name == "dY" or order == 0 else None)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_dropout_ignores_poison_and_propagates(dt):
    """sir_dropout_apply in place on a block embedded in a sentinel allocation: a dropped element is 0 whatever it
    held (nn.Dropout gives NaN * 0 = NaN: the documented deviation), a kept one is scaled and keeps its class;
    the pads stay untouched."""
    dtype = DTYPES[dt]
    M, N = 61, 76
    drop = (0xD20F, 0.5)
    keep = _native.dropout_apply(torch.ones(M, N, device=DEV, dtype=dtype), drop).float().cpu()
    assert set(keep.unique().tolist()) == {0.0, 2.0}
    X = xc.ints((M, N), 4, 900)
    for k, val in enumerate((INF, -INF, NAN)):       # each class at a dropped and at a kept element
        d, kp = torch.nonzero(keep == 0)[k + 3], torch.nonzero(keep == 2)[k + 3]
        X[d[0], d[1]] = val
        X[kp[0], kp[1]] = val
    buf = pc.Out((M, N), dtype, DEV).seed(X.to(DEV, dtype))
    _native.dropout_apply(buf.view, drop)
    ref = torch.where(keep == 0, torch.zeros(M, N, dtype=torch.float64), X.double() * 2)
    assert pc.nonfinite_share(ref) <= 0.25 and {1, 2, 3} <= set(pc.classes(ref).unique().tolist())
    buf.check_outside(f"dropout {dt}")
    pc.check_propagation(buf.view, ref, f"dropout {dt}")


def test_col_sum_ignores_poison_and_propagates():
    """sir_col_sum on a tall view embedded in NaN with a NaN-filled workspace: the integer column sums; a NaN, an
    Inf, and +inf meeting -inf each stay in their own column with the IEEE class."""
    for n, m in ((5, 16), (3001, 76)):
        X = xc.ints((n, m), 4, 950 + n)
        Xe = pc.embed(X.to(DEV), 4)[0]
        with pc.poisoned_empty():
            got = _native.col_sum(Xe)
        xg._same(got, xg._want(X.double().sum(0)), f"col_sum {n}x{m}")
        X = pc.col_sum_case(n, m)
        ref = X.double().sum(0)
        assert pc.nonfinite_share(ref) <= 0.25 and {1, 2} <= set(pc.classes(ref).unique().tolist())
        with pc.poisoned_empty():
            got = _native.col_sum(pc.embed(X.to(DEV), 4)[0])
        pc.check_propagation(got, ref, f"col_sum {n}x{m} non-finite")


# ----------------------------------------------------------------------------- Part B: the remaining families
@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("H", [4, 132])
def test_sire_kernels_propagate_nonfinite(H, agg, act):
    """sir_edge_e_agg_fwd with +inf / -inf / NaN in Eh (an edge into an unsplit row, one into a hub row, +inf and
    -inf meeting in one hub row): S has the reference's value and class.  sir_edge_e_bwd with +inf / -inf / NaN in G
    and a finite z: dE has the reference's value and class (sigma' = 0 with t = inf is 0); with the non-finite Eh,
    dE of every edge the poison does not sit on is exact."""
    code, slope = _slope(act)
    src, dst, V = xc.GRAPHS["A"]
    Q, K, G, Eh = (t.clone() for t in xc.edge_inputs("A", H))
    order = xc.csr_order("A")
    first = lambda v, k=0: int(order[(dst[order] == v).nonzero()[k]])        # the k-th in-edge of node v
    sites = [(first(0), 0, INF), (first(0), 1, -INF), (first(0), 2, NAN), (first(11), 0, INF), (first(11, 9), 1, -INF),
             (first(11, 15), 2, NAN), (first(12, 1), 3, INF), (first(12, 14), 3, -INF)]
    Ep = Eh.clone()
    for e, c, val in sites:
        Ep[e, c] = val
    Gp = pc.inject(G, pc.SITES["G"][1])
    ind = torch.bincount(dst, minlength=V)
    in_norm, out_norm = oracle.degree_norms(ind, torch.bincount(src, minlength=V), agg)
    c = (out_norm[src] * in_norm[dst]).double()[:, None] if agg == "sym" else 1.0
    div = ind.clamp(min=1).double()[:, None] if agg == "mean" else 1.0

    def ref(E_, G_):
        z = Q.double()[dst] + K.double()[src] + E_.double()
        S = torch.zeros(V, H, dtype=torch.float64).index_add_(0, dst, c * oracle.act_fwd(z, act, xc.SLOPE)) / div
        dE = oracle.act_bwd(z, (G_.double() / div)[dst] * c, act, xc.SLOPE)
        return S, dE
    wS, _ = ref(Ep, G)
    _, wdE_g = ref(Eh, Gp)
    _, wdE_e = ref(Ep, G)
    assert pc.nonfinite_share(wS) <= 0.25 and pc.nonfinite_share(wdE_g) <= 0.25
    assert {1, 2} <= set(pc.classes(wS).unique().tolist()) and {1, 2, 3} <= set(pc.classes(wdE_g).unique().tolist())
    clean_edges = torch.ones(Eh.shape[0], dtype=torch.bool)
    clean_edges[[e for e, _, _ in sites]] = False
    Qd, Kd = Q.to(DEV), K.to(DEV)
    nw = _native.mask_words(H, code)
    for chunk in (4, 256):
        plan = xg._plan("A", chunk)
        eid = plan.dst.eid
        eid32 = eid.to(torch.int32)
        p_in, p_out = plan.norms(agg)
        bagg = "sum" if agg == "mean" else agg
        b_in, b_out = plan.norms(bagg)
        what = f"sire non-finite H={H} {agg} {act} chunk={chunk}"
        for E_, G_, name in ((Ep, G, "Eh"), (Eh, Gp, "G")):
            S = torch.full((V, H), 7.0, device=DEV)
            mask = torch.full((Eh.shape[0] * nw,), -1, device=DEV, dtype=torch.int64)
            part = torch.full((max(plan.dst.n_slots, 1) * H,), NAN, device=DEV)
            _native.edge_e_agg_fwd(plan.dst, Qd, Kd, E_.to(DEV), eid32, p_in, p_out, agg, code, slope, S, part, mask)
            if name == "Eh":
                pc.check_propagation(S, wS, what + " S")
            g = xg._mean_g(plan, G_.to(DEV), agg)
            dE = torch.full(Eh.shape, 7.0, device=DEV)
            _native.edge_e_bwd(plan.dst, mask, g, b_in, b_out, bagg, code, slope, eid32, dE)
            if name == "G":
                pc.check_propagation(dE, wdE_g, what + " dE (G)")
            else:
                pc.check_propagation(dE, wdE_e, what + " dE (Eh)", rows=clean_edges.to(DEV))


@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("F", [3, 64, 256])
def test_edge_materialised_helpers_propagate_nonfinite(F, agg):
    """sir_edge_gather_add / _gather_act (ReLU(-inf) = 0, ReLU(NaN) = NaN, LeakyReLU(-inf) = -inf), sir_segment_sum
    (norms / mean; +inf and -inf meeting in a row) and sir_edge_broadcast with +inf / -inf / NaN in their operands:
    the reference's value where it is finite, its class where it is not."""
    src, dst, V = xc.GRAPHS["A"]
    E = src.numel()
    Q, K, dS = (xc.ints((V, F), 4, 300 + F + i) for i in range(3))
    Q, dS = pc.inject(Q, pc.SITES["Q"][1]), pc.inject(dS, pc.SITES["G"][1])
    K = pc.inject(K, [(5, 1, INF), (6, 1, -INF)])
    M = xc.ints((E, F), 4, 310 + F)
    order = xc.csr_order("A")
    e11 = order[(dst[order] == 11).nonzero().flatten()]
    for e, c, val in ((e11[2], 0, INF), (e11[13], 0, -INF), (e11[5], 1, NAN), (e11[7], 2, -INF), (order[0], 0, INF)):
        M[e, c] = val
    ind = torch.bincount(dst, minlength=V)
    in_norm, out_norm = oracle.degree_norms(ind, torch.bincount(src, minlength=V), agg)
    c = (out_norm[src] * in_norm[dst]).double()[:, None]
    div = ind.clamp(min=1).double()[:, None] if agg == "mean" else torch.ones(V, 1, dtype=torch.float64)
    wZ = Q.double()[dst] + K.double()[src]
    wS = torch.zeros(V, F, dtype=torch.float64).index_add_(0, dst, c * M.double()) / div
    wdM = c * (dS.double() / div)[dst]
    for r in (wZ, wS, wdM):
        assert pc.nonfinite_share(r) <= 0.25
    assert {1, 2, 3} <= set(pc.classes(wZ).unique().tolist()) and bool(torch.isnan(wS[11, 0]))
    for chunk in (4, 256):
        plan = xg._plan("A", chunk)
        eid = plan.dst.eid.cpu()
        p_in, p_out = plan.norms(agg)
        what = f"generic non-finite {agg} F={F} chunk={chunk}"
        Z = torch.full((E, F), 7.0, device=DEV)
        _native.edge_gather_add(plan.dst, Q.to(DEV), K.to(DEV), Z)
        pc.check_propagation(Z, wZ[eid], what + " gather_add")
        for act in xc.ACT_NAMES:
            A = torch.full((E, F), 7.0, device=DEV)
            _native.edge_gather_act(plan.dst, Q.to(DEV), K.to(DEV), *_slope(act), A)
            pc.check_propagation(A, oracle.act_fwd(wZ, act, xc.SLOPE)[eid], f"{what} gather_act {act}")
        S = torch.full((V, F), 7.0, device=DEV)
        part = torch.full((max(plan.dst.n_slots, 1) * F,), NAN, device=DEV)
        _native.segment_sum(plan.dst, M[eid].to(DEV), S, p_in, p_out, agg == "mean", partial=part)
        pc.check_propagation(S, wS, what + " segment_sum")
        dM = torch.full((E, F), 7.0, device=DEV)
        _native.edge_broadcast(plan.dst, dS.to(DEV), dM, p_in, p_out, agg == "mean")
        pc.check_propagation(dM, wdM[eid], what + " edge_broadcast")


@pytest.mark.parametrize("graph,agg", xg.GRAPH_AGG)
@pytest.mark.parametrize("H,F", xc.SEQ_SHAPES[:2])
def test_seq_sigma_forward_keeps_nonfinite_rows_apart(H, F, graph, agg, monkeypatch):
    """sir_edge_mlp_fwd (sum family; ReLU, Linear, ReLU) with one NaN in Q of a hub row and of a short row and one
    in K of a sender: S is non-finite in exactly the rows the reference marks (every row those edges reach) and
    equals the oracle in every other row."""
    src, dst, V = xc.GRAPHS[graph]
    Q, K, W, b, wS = pc.seq_nan_case(graph, H, F, agg)
    bad = ~torch.isfinite(wS)
    assert 0 < pc.rows_share(wS) <= 0.25 and torch.equal(bad, bad.any(1, keepdim=True).expand_as(bad))
    for chunk in (4, 256):
        QK = torch.cat([Q, K], 1).to(DEV)
        S = edgemlp.EdgeMLPSum.apply(QK, W.to(DEV), b.to(DEV), xg._plan(graph, chunk), H, agg, _native.ACT_RELU, 0.0,
                                     _native.ACT_RELU)
        pc.check_propagation(S, wS, f"seq non-finite {graph} {agg} H={H} F={F} chunk={chunk}", same_class=False)


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("graph", ["A", "B"])
@pytest.mark.parametrize("H,O", [(64, 64), (100, 200), (256, 40)])
def test_max_backward_routes_follow_a_nonfinite_arg(H, O, graph, act, monkeypatch):
    """Output columns whose every message is -inf, +inf or NaN (through the bias; Q, K finite): the forward takes
    the first edge, and every backward route sends dY of those columns to exactly that edge — dQ, dK, dW_R, db_R
    equal the fp64 evaluation on the oracle's arg edges."""
    code, slope = _slope(act)
    src, dst, V = xc.GRAPHS[graph]
    Q, K, W, b, dY, warg, want = pc.max_bias_case(graph, H, O, act)
    Qd, Kd, Wd, bd, dYd = (t.to(DEV) for t in (Q, K, W, b, dY))
    monkeypatch.setattr(edgemlp, "STREAM", False)
    ran = 0
    for chunk in (4, 256):
        plan = xg._plan(graph, chunk)
        _, arg = xg._max_forward(plan, Qd, Kd, Wd, bd, act, torch.float32)
        xg._same(xg._edge_ids(plan, arg), warg.to(DEV), f"max bias {graph} {act} H={H} O={O} chunk={chunk} arg")
        for route, (switches, applies) in xg.MAX_ROUTES.items():
            if not applies(H, O, V):
                continue
            for k, v in switches.items():
                monkeypatch.setattr(edgemlp.EdgeMaxLinear, k, v)
            what = f"max bias {graph} {act} H={H} O={O} chunk={chunk} {route}"
            dQK = torch.full((V, 2 * H), NAN, device=DEV)
            dW, db = edgemlp.max_linear_backward(plan, Qd, Kd, Wd, arg, dYd, code, slope, dQK[:, :H], dQK[:, H:])
            xg._same(dQK[:, :H], xg._want(want["dQ"]), what + " dQ")
            xg._same(dQK[:, H:], xg._want(want["dK"]), what + " dK")
            xg._same(dW.contiguous(), xg._want(want["dW"]), what + " dW_R")
            xg._same(db.contiguous(), xg._want(want["db"]), what + " db_R")
            ran += 1
    assert ran >= 4


def _norm_propagation(got, ref32, ref64, bad, what):
    """A norm's output with non-finite inputs: the reference is non-finite only inside ``bad`` (the cells the
    poisoned statistic reaches), the kernel is non-finite wherever the reference is, finite everywhere outside
    ``bad`` and there inside the bound of the kernels' own parity tests (1e-5, conftest.assert_parity)."""
    from conftest import assert_parity
    g = got.detach().cpu()
    assert not bool((~torch.isfinite(ref64) & ~bad).any()), what + ": the reference leaks"
    assert float(bad.float().mean()) <= 0.25 and bool((~torch.isfinite(ref64)).any()), what
    silent = ~torch.isfinite(ref64) & torch.isfinite(g)
    assert not bool(silent.any()), f"{what}: {int(silent.sum())} elements are finite where the reference is not"
    assert bool(torch.isfinite(g[~bad]).all()), f"{what}: a non-finite value left its row / column"
    z = lambda t: torch.where(bad, torch.zeros((), dtype=t.dtype), t)
    assert_parity(z(g), z(ref32), z(ref64), 1e-5, what)


@pytest.mark.parametrize("kind", ["batch", "layer", "graph"])
def test_fused_norms_propagate_nonfinite(kind):
    """ReLU(norm(X)) + R through the fused passes (sir_batch_norm_stats / _act_fwd / _act_bwd,
    sir_layer_norm_act_fwd / _bwd, sir_graph_norm_act_fwd / _bwd) with a NaN and an Inf in X: Y and dX are
    non-finite wherever torch's composition is (ReLU(NaN) is NaN), the poison stays in its column (BatchNorm), its
    row (LayerNorm) or its (graph, column) cell (GraphNorm), and everything else is inside the parity bound."""
    import test_nodenorm_gpu as nt
    from torch import nn
    from sirgcn import Graph, GraphBatchNorm, GraphLayerNorm, GraphNorm, batch
    M, N = 3 * nt.R + 7, 76
    xs, dys, gamma, beta = nt._data(M, N, seed=3)
    X, dY = xs[0].clone(), dys[0]
    Rr = torch.randn(M, N, generator=torch.Generator().manual_seed(5))
    X[5, 3], X[M - 2, 40] = NAN, INF
    bad = torch.zeros(M, N, dtype=torch.bool)
    ns = [40, M - 40 - 60, 0, 60]
    if kind == "batch":
        bad[:, [3, 40]] = True
    elif kind == "layer":
        bad[[5, M - 2]] = True
    else:
        bad[:40, 3] = True
        bad[M - 60:, 40] = True
    graphs = batch([Graph(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), n) for n in ns])
    cls = {"batch": GraphBatchNorm, "layer": GraphLayerNorm, "graph": GraphNorm}[kind]
    mod = nt._init(cls(N), gamma, beta).to(DEV)
    Xr = X.to(DEV).requires_grad_(True)
    Y = mod.forward_act(graphs, Xr, nn.ReLU(), Rr.to(DEV))
    assert Y is not None, "the fused pass was refused"
    Y.backward(dY.to(DEV))
    refs = []
    for dt in (torch.float32, torch.float64):
        x = X.detach().clone().to(dt).requires_grad_(True)
        if kind == "graph":
            nz = [n for n in ns if n > 0]
            y = oracle.graph_norm_fwd(x, nz, gamma.to(dt), beta.to(dt), torch.ones(N, dtype=dt), 1e-5)[0]
        else:
            ref = nt._init((nn.BatchNorm1d if kind == "batch" else nn.LayerNorm)(N), gamma, beta).to(dt)
            y = ref(x)
        y = torch.relu(y) + Rr.to(dt)
        y.backward(dY.to(dt))
        refs.append((y.detach(), x.grad))
    _norm_propagation(Y, refs[0][0], refs[1][0], bad, f"{kind} norm Y")
    _norm_propagation(Xr.grad, refs[0][1], refs[1][1], bad, f"{kind} norm dX")
