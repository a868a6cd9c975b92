"""GPU checks of the fused SIREConv route: sir_edge_e_agg_fwd / sir_edge_e_bwd at kernel level (bitwise
against the edge-materialised composition and the documented mask layout, fp64 oracle on split rows),
the eidx forms, the module against its own edge-materialised path, routing, determinism, bad ids and
the peak-memory bound that the fused route exists for.

Q, K and Eh of the kernel-level tests are drawn directly (no GEMM): every expected value is formed from the
same fp32 numbers, so no sigma' near-tie can arise."""
import numpy as np
import pytest
import torch
from torch import nn

import oracle
from conftest import assert_close, assert_parity
import width_cases as wc
from exact_cases import encode_mask as _encode_mask

from sirgcn import SIREConv, _native
from sirgcn.conv import edge_backward
from sirgcn.econv import EdgeAggregateE
from sirgcn.graph import Graph, GraphPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, NE = 67, 700
HS = wc.ECONV_HS
AGGS = ["sum", "mean", "sym"]
ACTS = {"relu": (nn.ReLU(), _native.ACT_RELU, 0.0), "leaky": (nn.LeakyReLU(0.2), _native.ACT_LEAKY, 0.2)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _edges():
    """67 nodes, 700 edges in shuffled order: node 0 has 300 in-edges (plus random ones), node 1 has 300
    out-edges, duplicates and self-loops, the last node has no edge at all."""
    gen = torch.Generator().manual_seed(1234)
    n = V - 1
    rs, rd = torch.randint(0, n, (90,), generator=gen), torch.randint(0, n, (90,), generator=gen)
    src = torch.cat([rs, rs[:4], torch.tensor([5, 5, 9, 0, 1, 1]), torch.randint(0, n, (300,), generator=gen),
                     torch.ones(300, dtype=torch.int64)])
    dst = torch.cat([rd, rd[:4], torch.tensor([5, 5, 9, 0, 1, 1]), torch.zeros(300, dtype=torch.int64),
                     torch.randint(0, n, (300,), generator=gen)])
    assert src.numel() == NE
    p = torch.randperm(NE, generator=gen)
    return src[p].contiguous(), dst[p].contiguous()


SRC, DST = _edges()
_PLANS = {}
_INPUTS = {}
_ORACLE = {}


def _plan(chunk):
    if chunk not in _PLANS:
        _PLANS[chunk] = GraphPlan(SRC, DST, V, DEV, chunk=chunk)
    return _PLANS[chunk]


def _inputs(H):
    """Q, K [V, H], Eh [E, H] (caller's edge order), dS [V, H] — CPU fp32, drawn once per H."""
    if H not in _INPUTS:
        gen = torch.Generator().manual_seed(100 + H)
        _INPUTS[H] = tuple(torch.randn(s, H, generator=gen) for s in (V, V, NE, V))
    return _INPUTS[H]


def _oracle_step(H, agg, act, dtype):
    """oracle.sire_reference_step with identity projections: X = [Q | K], W_Q = [I 0], W_K = [0 I], W_E = I,
    W_R = I, zero biases -> Y = S, dX = [dQ | dK], defeat = dE.  Computed once per case and shared."""
    key = (H, agg, act, dtype)
    if key not in _ORACLE:
        Q, K, Eh, dS = (t.to(dtype) for t in _inputs(H))
        eye, zero = torch.eye(H, dtype=dtype), torch.zeros(H, H, dtype=dtype)
        r = oracle.sire_reference_step(SRC, DST, V, torch.cat([Q, K], 1), Eh, torch.cat([eye, zero], 1),
                                       torch.zeros(H, dtype=dtype), torch.cat([zero, eye], 1), eye, eye,
                                       torch.zeros(H, dtype=dtype), dS, agg, act, ACTS[act][2])
        _ORACLE[key] = {"S": r["Y"], "dQ": r["dX"][:, :H], "dK": r["dX"][:, H:], "dE": r["defeat"]}
    return _ORACLE[key]


def _csr_rows(plan):
    rp = plan.dst.rowptr.long()
    return torch.repeat_interleave(torch.arange(V, device=DEV), rp[1:] - rp[:-1])


def _z(plan, Q, K, Eh):
    """z per destination-CSR position, in the kernel's operand order."""
    return (Q[_csr_rows(plan)] + K[plan.dst.col.long()]) + Eh[plan.dst.eid]


def _split_rows(plan):
    rows = torch.zeros(V, dtype=torch.bool)
    if plan.dst.n_splits:
        rows[plan.dst.splits[:, 0].long().cpu()] = True
    return rows


def _fwd(plan, Q, K, Eh, eidx, agg, act, want_mask=True):
    H = Q.shape[1]
    code, slope = ACTS[act][1], ACTS[act][2]
    in_norm, out_norm = plan.norms(agg)
    S = torch.full((V, H), float("nan"), device=DEV)
    nw = _native.mask_words(H, code)
    mask = torch.full((NE * nw,), -1, device=DEV, dtype=torch.int64) if want_mask else None
    n = max(plan.dst.n_slots, 1)
    partial = torch.empty((n * H,), device=DEV)
    _native.edge_e_agg_fwd(plan.dst, Q, K, Eh, eidx, in_norm, out_norm, agg, code, slope, S, partial, mask)
    return S, mask


def _legacy_S(plan, Q, K, Eh, agg, act):
    H = Q.shape[1]
    Z = torch.empty((NE, H), device=DEV)
    _native.edge_gather_add(plan.dst, Q, K, Z)
    A = ACTS[act][0](Z + Eh.index_select(0, plan.dst.eid))
    in_norm, out_norm = plan.norms(agg)
    S = torch.empty((V, H), device=DEV)
    n = max(plan.dst.n_slots, 1)
    _native.segment_sum(plan.dst, A, S, in_norm, out_norm, agg == "mean", partial=torch.empty((n * H,), device=DEV))
    return S


@pytest.mark.parametrize("chunk", [64, 256])
@pytest.mark.parametrize("H", HS)
def test_forward_and_mask_kernel_level(H, chunk):
    plan = _plan(chunk)
    Q, K, Eh, _ = (t.to(DEV) for t in _inputs(H))
    eid32 = plan.dst.eid.to(torch.int32)
    split = _split_rows(plan)
    assert split[0] and not split[V - 1] and plan.dst.n_splits >= 1
    zpos = (_z(plan, Q, K, Eh) > 0).cpu().numpy()
    want_mask = _encode_mask(zpos, H)
    for agg in AGGS:
        for act in ACTS:
            S, mask = _fwd(plan, Q, K, Eh, eid32, agg, act)
            S = S.cpu()
            ref = _legacy_S(plan, Q, K, Eh, agg, act).cpu()
            what = f"H={H} chunk={chunk} {agg} {act}"
            assert torch.equal(S[~split], ref[~split]), f"{what}: unsplit rows differ, max {(S - ref)[~split].abs().max()}"
            assert torch.equal(S[V - 1], torch.zeros(H)), what
            o32, o64 = _oracle_step(H, agg, act, torch.float32), _oracle_step(H, agg, act, torch.float64)
            assert_parity(S[split], o32["S"][split], o64["S"][split], 1e-5, what + " split rows")
            assert_parity(S, o32["S"], o64["S"], 1e-5, what + " S")
            got = mask.cpu().numpy().view(np.uint64).reshape(NE, -1)
            assert np.array_equal(got, want_mask), f"{what}: sign mask differs from the documented layout"
            # no mask requested: same S
            S2, _ = _fwd(plan, Q, K, Eh, eid32, agg, act, want_mask=False)
            assert torch.equal(S2.cpu(), S), what


@pytest.mark.parametrize("H", HS)
def test_backward_kernel_level(H):
    plan = _plan(64)
    Q, K, Eh, dS = (t.to(DEV) for t in _inputs(H))
    eid32 = plan.dst.eid.to(torch.int32)
    rows, cols = _csr_rows(plan), plan.dst.col.long()
    zpos = _z(plan, Q, K, Eh) > 0
    for agg in AGGS:
        for act in ACTS:
            code, slope = ACTS[act][1], ACTS[act][2]
            what = f"H={H} {agg} {act}"
            QK = torch.cat([Q, K], 1).requires_grad_(True)
            Er = Eh.clone().requires_grad_(True)
            S = EdgeAggregateE.apply(QK, Er, eid32, plan, H, agg, code, slope, True, False)
            S.backward(dS)
            # the edge term's gradient, bit for bit: where(z > 0, t, t * slope or 0) in the kernel's operand order
            g = dS / plan.in_degree_f() if agg == "mean" else dS
            t = g[rows]
            if agg == "sym":
                in_norm, out_norm = plan.norms("sym")
                t = t * (out_norm[cols] * in_norm[rows])[:, None]
            neg = torch.zeros_like(t) if act == "relu" else t * slope
            want = torch.empty_like(Eh)
            want[plan.dst.eid] = torch.where(zpos, t, neg)
            assert torch.equal(Er.grad, want), f"{what}: dE max diff {(Er.grad - want).abs().max()}"
            o32, o64 = _oracle_step(H, agg, act, torch.float32), _oracle_step(H, agg, act, torch.float64)
            assert_parity(QK.grad[:, :H].cpu(), o32["dQ"], o64["dQ"], 1e-5, what + " dQ")
            assert_parity(QK.grad[:, H:].cpu(), o32["dK"], o64["dK"], 1e-5, what + " dK")
            assert_parity(Er.grad.cpu(), o32["dE"], o64["dE"], 1e-5, what + " dE")
            # Eh = 0: z = Q + K, and the mask hand-over gives the recompute-mode passes' bits
            QK0 = torch.cat([Q, K], 1).requires_grad_(True)
            S0 = EdgeAggregateE.apply(QK0, torch.zeros_like(Eh), eid32, plan, H, agg, code, slope, True, False)
            S0.backward(dS)
            ref = torch.empty((V, 2 * H), device=DEV)
            edge_backward(plan, H, agg, code, slope, dS, Q, K, None, ref)
            assert torch.equal(QK0.grad, ref), f"{what}: dQK differs from the recompute mode at Eh = 0"


@pytest.mark.parametrize("H", [32, 256])
def test_eidx_forms(H):
    plan = _plan(64)
    Q, K, _, dS = (t.to(DEV) for t in _inputs(H))
    gen = torch.Generator().manual_seed(7)
    R = 4
    T = torch.randn(R, H, generator=gen).to(DEV)
    ids = torch.randint(0, R, (NE,), generator=gen).to(DEV)
    Eh = T[ids]                                              # the same row values in all three forms
    eid32 = plan.dst.eid.to(torch.int32)
    tid32 = ids[plan.dst.eid].to(torch.int32)
    for agg in AGGS:
        what = f"H={H} {agg}"
        S_perm, m_perm = _fwd(plan, Q, K, Eh, eid32, agg, "leaky")
        S_null, m_null = _fwd(plan, Q, K, Eh[plan.dst.eid].contiguous(), None, agg, "leaky")
        S_tab, m_tab = _fwd(plan, Q, K, T, tid32, agg, "leaky")
        assert torch.equal(S_perm, S_null) and torch.equal(S_perm, S_tab), what
        assert torch.equal(m_perm, m_null) and torch.equal(m_perm, m_tab), what
        # table-form gradient: the fp64 sum over the edges of each type
        QK = torch.cat([Q, K], 1).requires_grad_(True)
        Tr = T.clone().requires_grad_(True)
        S = EdgeAggregateE.apply(QK, Tr, tid32, plan, H, agg, _native.ACT_LEAKY, 0.2, True, True)
        assert torch.equal(S, S_perm), what
        S.backward(dS)
        ref = {}
        for dt in (torch.float32, torch.float64):
            r = oracle.sire_reference_step(SRC, DST, V, torch.cat([Q, K], 1).cpu().to(dt), Eh.cpu().to(dt),
                                           torch.cat([torch.eye(H), torch.zeros(H, H)], 1).to(dt), torch.zeros(H, dtype=dt),
                                           torch.cat([torch.zeros(H, H), torch.eye(H)], 1).to(dt), torch.eye(H, dtype=dt),
                                           torch.eye(H, dtype=dt), torch.zeros(H, dtype=dt), dS.cpu().to(dt), agg,
                                           "leaky", 0.2)
            ref[dt] = torch.zeros(R, H, dtype=dt).index_add(0, ids.cpu(), r["defeat"])
        assert_parity(Tr.grad.cpu(), ref[torch.float32], ref[torch.float64], 1e-5, what + " dT")
        # a stream-form backward on the same values gives the same dQ / dK bits (same mask)
        QK2 = torch.cat([Q, K], 1).requires_grad_(True)
        EdgeAggregateE.apply(QK2, Eh, eid32, plan, H, agg, _native.ACT_LEAKY, 0.2, True, False).backward(dS)
        assert torch.equal(QK.grad, QK2.grad), what


def _module(H, agg, act=None, d=16, de=6, dropout=0.0, dtype=torch.float32, seed=3):
    torch.manual_seed(seed)
    m = SIREConv(d, de, H, 24, act if act is not None else nn.LeakyReLU(0.2), dropout, agg_type=agg).to(DEV, dtype)
    m.chunk = 64
    return m


def _step(m, fused, X, Ef, dY, seed=None, tuple_feat=False):
    """One forward + backward of ``m`` on the fused or the edge-materialised route; every output, detached."""
    m.fused = fused
    m.zero_grad(set_to_none=True)
    Xk = X.clone().requires_grad_(True)
    Xq = X.flip(0).clone().requires_grad_(True) if tuple_feat else Xk
    E = Ef.clone().requires_grad_(True) if Ef.dtype.is_floating_point else Ef
    if seed is not None:
        torch.manual_seed(seed)
    Y = m(Graph(SRC, DST, V), (Xk, Xq) if tuple_feat else Xk, E)
    Y.backward(dY)
    out = {"Y": Y.detach(), "dX": Xk.grad}
    if tuple_feat:
        out["dXq"] = Xq.grad
    if E.requires_grad:
        out["defeat"] = E.grad
    for name, p in m.named_parameters():
        out["d" + name] = p.grad
    del m.fused
    return {k: v.clone() for k, v in out.items()}


def _module_data(d=16, de=6, O=24, dtype=torch.float32):
    gen = torch.Generator().manual_seed(11)
    return (torch.randn(V, d, generator=gen).to(DEV, dtype), torch.randn(NE, de, generator=gen).to(DEV, dtype),
            torch.randn(V, O, generator=gen).to(DEV, dtype))


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("H", [32, 256])
def test_module_fused_vs_edge_materialised(H, agg):
    X, Ef, dY = _module_data()
    m = _module(H, agg)
    a, b = _step(m, True, X, Ef, dY), _step(m, False, X, Ef, dY)
    assert set(a) == set(b) and "defeat" in a and "dlinear_edge.weight" in a
    for k in a:
        assert_close(a[k], b[k], 1e-5, f"H={H} {agg} {k}")


@pytest.mark.parametrize("variant", ["dropout", "tuple"])
def test_module_fused_vs_edge_materialised_variants(variant):
    X, Ef, dY = _module_data()
    if variant == "dropout":        # training mode, fixed seed: both routes draw the same three masks
        m = _module(256, "sum", dropout=0.2).train()
        a, b = _step(m, True, X, Ef, dY, seed=5), _step(m, False, X, Ef, dY, seed=5)
    else:
        m = _module(32, "sym")
        a, b = _step(m, True, X, Ef, dY, tuple_feat=True), _step(m, False, X, Ef, dY, tuple_feat=True)
    assert set(a) == set(b)
    for k in a:
        assert_close(a[k], b[k], 1e-5, f"{variant} {k}")


@pytest.mark.parametrize("case", ["fp64", "tanh", "max", "H30", "autocast"])
def test_routing_keeps_the_edge_materialised_path(case, monkeypatch):
    """Inputs outside the fused route run the same code whatever ``fused`` says: the new kernels are never
    called and the results are the bits ``fused = False`` gives."""
    def boom(*a, **k):
        raise AssertionError("the fused kernels must not run for this input")
    monkeypatch.setattr(_native, "edge_e_agg_fwd", boom)
    dtype = torch.float64 if case == "fp64" else torch.float32
    X, Ef, dY = _module_data(dtype=dtype)
    m = _module(30 if case == "H30" else 32, "max" if case == "max" else "sum",
                act=nn.Tanh() if case == "tanh" else None, dtype=dtype)
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if case == "autocast" else torch.autocast("cuda", enabled=False)
    outs = []
    for fused in (True, False):
        m.fused = fused
        Xr = X.clone().requires_grad_(True)
        with ctx:
            Y = m(Graph(SRC, DST, V), Xr, Ef)
        Y.float().backward(dY.float()[:, :Y.shape[1]])
        outs.append((Y.detach().clone(), Xr.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_fused_route_is_taken(monkeypatch):
    """The default module on fp32 ReLU-family inputs runs the new kernels (and ``fused = False`` does not)."""
    calls = []
    real = _native.edge_e_agg_fwd
    monkeypatch.setattr(_native, "edge_e_agg_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    X, Ef, dY = _module_data()
    m = _module(32, "sum")
    assert SIREConv.fused is True
    m(Graph(SRC, DST, V), X, Ef)
    assert len(calls) == 1
    m.fused = False
    m(Graph(SRC, DST, V), X, Ef)
    assert len(calls) == 1


def _table_module(H, R=4):
    m = _module(H, "sum", d=16)
    torch.manual_seed(4)
    m.linear_edge = nn.Embedding(R, H).to(DEV)
    return m


def test_determinism_stream_and_table():
    X, Ef, dY = _module_data()
    m = _module(256, "sym")
    a, b = _step(m, True, X, Ef, dY), _step(m, True, X, Ef, dY)
    for k in a:
        assert torch.equal(a[k], b[k]), f"stream {k}"
    mt = _table_module(256)
    ids = torch.randint(0, 4, (NE,), generator=torch.Generator().manual_seed(2)).to(DEV)
    a, b = _step(mt, True, X, ids, dY), _step(mt, True, X, ids, dY)
    assert "dlinear_edge.weight" in a
    for k in a:
        assert torch.equal(a[k], b[k]), f"table {k}"
    # and the table form agrees with the edge-materialised embedding lookup
    c = _step(mt, False, X, ids, dY)
    for k in a:
        assert_close(a[k], c[k], 1e-5, f"table vs edge-materialised {k}")


def test_no_grad_allocates_no_mask(monkeypatch):
    seen = []
    real = _native.edge_e_agg_fwd
    monkeypatch.setattr(_native, "edge_e_agg_fwd", lambda *a, **k: (seen.append(a[-1] if len(a) > 12 else k.get("mask_out")), real(*a, **k))[1])
    X, Ef, _ = _module_data()
    m = _module(32, "mean")
    with torch.no_grad():
        m(Graph(SRC, DST, V), X, Ef)
    m.eval()
    with torch.no_grad():
        m(Graph(SRC, DST, V), X, Ef)
    assert seen == [None, None]


def test_bad_table_id_raises(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("no kernel may be launched with an id outside the table")
    monkeypatch.setattr(_native, "edge_e_agg_fwd", boom)
    X, _, _ = _module_data()
    m = _table_module(32)
    ids = torch.zeros(NE, dtype=torch.int64, device=DEV)
    ids[17] = 4
    with pytest.raises(ValueError, match="out of range"):
        m(Graph(SRC, DST, V), X, ids)
    ids[17] = -1
    with pytest.raises(ValueError, match="out of range"):
        m(Graph(SRC, DST, V), X, ids)


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_peak_memory_of_one_step():
    """E = 50 000, V = 1 000, H = 256, de = 16, sum, LeakyReLU, no dropout: one forward + backward of the fused
    route stays at or under 2.25 E H 4 bytes (Eh, then dEh, the 32-byte-per-edge mask, the index arrays and
    the V-sized tensors); the edge-materialised route holds at least five [E, H] buffers.  The table form's
    forward alone stays under 1.25 E H 4."""
    Vm, Em, H, de = 1000, 50000, 256, 16
    gen = torch.Generator().manual_seed(21)
    g = Graph(torch.randint(0, Vm, (Em,), generator=gen), torch.randint(0, Vm, (Em,), generator=gen), Vm)
    X = torch.randn(Vm, 16, generator=gen).to(DEV)
    Ef = torch.randn(Em, de, generator=gen).to(DEV)
    dY = torch.randn(Vm, 24, generator=gen).to(DEV)
    torch.manual_seed(0)
    m = SIREConv(16, de, H, 24, nn.LeakyReLU(0.2), 0, agg_type="sum").to(DEV)
    unit = Em * H * 4

    def step():
        m.zero_grad(set_to_none=True)
        Xr, Er = X.clone().requires_grad_(True), Ef.clone().requires_grad_(True)
        m(g, Xr, Er).backward(dY)

    peaks = {}
    for fused in (True, False):
        m.fused = fused
        step()                      # warm-up: the plan, library workspaces
        peaks[fused] = _peak(step)
    print(f"peak bytes of one step: fused {peaks[True]} ({peaks[True] / unit:.2f} E*H*4), "
          f"edge-materialised {peaks[False]} ({peaks[False] / unit:.2f} E*H*4)")
    assert peaks[True] <= 2.25 * unit, f"fused step peak {peaks[True] / unit:.2f} E*H*4"
    assert peaks[False] > peaks[True]

    m.fused = True
    m.linear_edge = nn.Embedding(4, H).to(DEV)
    ids = torch.randint(0, 4, (Em,), generator=gen).to(DEV)
    fwd = lambda: m(g, X.clone().requires_grad_(True), ids)
    fwd()
    pk = _peak(fwd)
    print(f"peak bytes of the table-form forward: {pk} ({pk / unit:.2f} E*H*4)")
    assert pk < 1.25 * unit
