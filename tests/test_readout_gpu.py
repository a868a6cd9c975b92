"""sirgcn.SumPooling / AvgPooling / MaxPooling / broadcast_nodes on the MI355X (dgl.nn.*Pooling,
dgl.broadcast_nodes) against the restatement of tests/readout_cases.py:
1. exact inputs: P, arg and dX of all three ops equal the fp64 restatement cast to the dtype, bit for bit;
2. random inputs: sum / mean inside the project's parity envelope, every selection / copy / one division exact;
3. layouts: column slices, 1-D and 3-D feats, a transposed dP, B = 1, a batch of empty graphs;
4. broadcast_nodes;  5. run-to-run determinism;  6. a training step captured in a HIP graph replays;
7. the readout at the end of a small molecule model against the torch-composed readout."""
import pytest
import torch
from torch import nn

from conftest import assert_parity

import readout_cases as rc
import sirgcn
from sirgcn import AvgPooling, Graph, GraphNorm, MaxPooling, SIRConv, SumPooling, _native, workloads
from sirgcn.stacks import SIRStack

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = _native.POOL_SLAB_ROWS
POOLS = {"sum": SumPooling, "mean": AvgPooling, "max": MaxPooling}
CODES = {"sum": _native.POOL_SUM, "mean": _native.POOL_MEAN, "max": _native.POOL_MAX}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_GRAPHS = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _graph(ns):
    """The batched graph of ``ns`` nodes per graph (no edges: the readout reads batch_num_nodes only)."""
    key = tuple(ns)
    if key not in _GRAPHS:
        e = torch.zeros(0, dtype=torch.int64)
        _GRAPHS[key] = sirgcn.batch([Graph(e, e, n) for n in ns])
    return _GRAPHS[key]


def _step(op, graph, X, dP):
    """One forward + backward of the pooling module: (P, dX)."""
    Xr = X.detach().requires_grad_(True)
    P = POOLS[op]()(graph, Xr)
    P.backward(dP)
    return P.detach(), Xr.grad


def _ids(ns):
    return torch.repeat_interleave(torch.arange(len(ns)), torch.as_tensor(ns, dtype=torch.int64))


def _composed(graph, X, op):
    """The readout a user writes today from torch ops (sum / mean)."""
    n = torch.as_tensor(graph.batch_num_nodes(), dtype=torch.int64).to(X.device)
    ids = torch.repeat_interleave(torch.arange(n.numel(), device=X.device), n)
    P = torch.zeros(n.numel(), X.shape[1], device=X.device, dtype=X.dtype).index_add_(0, ids, X)
    return P / n.clamp(min=1).to(X.dtype)[:, None] if op == "mean" else P


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("F", [1, 3, 4, 64, 65, 75, 256, 260, 300])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_exact_inputs_bit_for_bit(dt, F):
    dtype = DTYPES[dt]
    ns, X, dP = rc.exact_inputs(R)
    g = _graph(ns)
    off = rc.offsets(ns)
    Xd = X[:, :F].to(dtype).contiguous().to(DEV)
    dPd = dP[:, :F].to(dtype).contiguous().to(DEV)
    for op in rc.OPS:
        want = rc.exact_expected(R, op)
        P, dX = _step(op, g, Xd, dPd)
        assert P.dtype == dtype and dX.dtype == dtype and P.shape == (len(ns), F) and dX.shape == Xd.shape
        assert torch.equal(P.cpu(), want["P"][:, :F].to(dtype)), f"{op} {dt} F={F}: P"
        assert torch.equal(dX.cpu(), want["dX"][:, :F].to(dtype)), f"{op} {dt} F={F}: dX"
        if op == "max":
            Pn = torch.empty_like(P)
            arg = torch.empty(P.shape, device=DEV, dtype=torch.int32)
            _native.graph_pool_fwd(off.to(DEV), Xd, CODES[op], Pn, arg)
            assert torch.equal(Pn, P)
            assert torch.equal(arg.cpu(), want["arg"][:, :F]), f"{dt} F={F}: arg"
            # in a tie the lowest row wins: the gradient sits on one row only, the first maximal one
            dXc, Xc = dX.cpu().float(), Xd.cpu().float()
            for b, n in enumerate(ns):
                seg, xs = dXc[off[b]:off[b + 1]], Xc[off[b]:off[b + 1]]
                if n > 0:
                    assert int((seg != 0).sum(0).max()) <= 1
                    first = (xs == xs.max(0).values).float().argmax(0)
                    hit = seg.gather(0, first[None, :])[0]
                    assert torch.equal(hit, dPd[b].cpu().float())


# ------------------------------------------------------------------ 2. parity on random inputs
@pytest.mark.parametrize("F", [1, 3, 75, 80, 300])
def test_random_inputs_parity(F):
    ns, X, dP, refs = rc.random_case(R, F)
    g = _graph(ns)
    Xd, dPd = X.to(DEV), dP.to(DEV)
    for op in rc.OPS:
        r32, r64 = refs[op]
        P, dX = _step(op, g, Xd, dPd)
        if op == "max":
            assert torch.equal(P.cpu(), r32["P"]), f"max F={F}: P"
        else:
            assert_parity(P, r32["P"], r64["P"], 1e-5, f"readout {op} F={F} P")
        assert torch.equal(dX.cpu(), r32["dX"]), f"{op} F={F}: dX"


# ------------------------------------------------------------------ 3. layout
def _sliced(x, pad=3):
    """x as a column slice of a wider tensor: ld > F, rows not 16-B aligned."""
    wide = torch.zeros(x.shape[0], x.shape[1] + pad, device=x.device, dtype=x.dtype)
    wide[:, 1:1 + x.shape[1]] = x
    v = wide[:, 1:1 + x.shape[1]]
    assert v.stride(0) == x.shape[1] + pad and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("F", [80, 75])
def test_column_slice_input(F, dt, monkeypatch):
    ns, X, dP, _ = rc.random_case(R, F)
    g = _graph(ns)
    Xd, dPd = X.to(DEV).to(DTYPES[dt]), dP.to(DEV).to(DTYPES[dt])
    seen = []
    orig = _native.graph_pool_fwd
    monkeypatch.setattr(_native, "graph_pool_fwd", lambda off, Xa, *a, **k: seen.append(Xa.stride(0)) or orig(off, Xa, *a, **k))
    for op in rc.OPS:
        plain = _step(op, g, Xd, dPd)
        view = _step(op, g, _sliced(Xd), _sliced(dPd))
        assert seen[-2:] == [F, F + 3], "the slice must be passed with its leading dimension, not copied"
        for a, b in zip(plain, view):
            assert torch.equal(a, b), f"{op} {dt} F={F}"


def test_1d_3d_feats_and_transposed_gradient():
    ns, X, dP, refs = rc.random_case(R, 75)
    g = _graph(ns)
    V, B = sum(ns), len(ns)
    X15 = X[:, :15].contiguous().to(DEV)
    for op in rc.OPS:
        P2, dX2 = _step(op, g, X15, dP[:, :15].contiguous().to(DEV))
        P3, dX3 = _step(op, g, X15.reshape(V, 5, 3), dP[:, :15].reshape(B, 5, 3).to(DEV))
        assert P3.shape == (B, 5, 3) and dX3.shape == (V, 5, 3)
        assert torch.equal(P3.reshape(B, 15), P2) and torch.equal(dX3.reshape(V, 15), dX2)
        P1, dX1 = _step(op, g, X15[:, 4].contiguous(), dP[:, 4].contiguous().to(DEV))
        assert P1.shape == (B,) and dX1.shape == (V,)
        assert torch.equal(P1, P2[:, 4]) and torch.equal(dX1, dX2[:, 4])
        # a transposed (non-contiguous) dP
        dPt = dP[:, :15].to(DEV).t().contiguous().t()
        assert not dPt.is_contiguous()
        Pt, dXt = _step(op, g, X15, dPt)
        assert torch.equal(Pt, P2) and torch.equal(dXt, dX2)


def test_single_graph_and_all_graphs_empty():
    F = 75
    g1 = torch.Generator().manual_seed(5)
    for n in (1, 40, R + 5):
        X, dP = torch.randn(n, F, generator=g1), torch.randn(1, F, generator=g1)
        for op in rc.OPS:
            P, dX = _step(op, _graph([n]), X.to(DEV), dP.to(DEV))
            rP, rarg = rc.pool_ref(X, [n], op)
            t64 = rc.pool_ref(X.double(), [n], op)[0]
            if op == "max":
                assert torch.equal(P.cpu(), rP)
            else:
                assert_parity(P, rP, t64, 1e-5, f"B=1 n={n} {op}")
            assert torch.equal(dX.cpu(), rc.pool_bwd_ref(dP, rarg, [n], op))
    empty = _graph([0, 0, 0])
    for dtype in DTYPES.values():
        for op in rc.OPS:
            P, dX = _step(op, empty, torch.zeros(0, F, device=DEV, dtype=dtype), torch.ones(3, F, device=DEV, dtype=dtype))
            assert P.shape == (3, F) and P.dtype == dtype and not P.any() and dX.shape == (0, F)
    arg = torch.zeros(3, F, device=DEV, dtype=torch.int32)
    _native.graph_pool_fwd(rc.offsets([0, 0, 0]).to(DEV), torch.zeros(0, F, device=DEV), _native.POOL_MAX,
                           torch.empty(3, F, device=DEV), arg)
    assert bool((arg == -1).all())
    out = sirgcn.broadcast_nodes(empty, torch.ones(3, F, device=DEV))
    assert out.shape == (0, F)


# ------------------------------------------------------------------ 4. broadcast_nodes
@pytest.mark.parametrize("dt", list(DTYPES))
def test_broadcast_nodes(dt):
    dtype = DTYPES[dt]
    ns, X, dP = rc.exact_inputs(R)
    g = _graph(ns)
    ids = _ids(ns)
    for F in (1, 75, 300):
        G = dP[:, :F].to(dtype).contiguous().to(DEV).requires_grad_(True)
        up = X[:, :F].to(dtype).contiguous().to(DEV)              # the upstream gradient of the broadcast
        out = sirgcn.broadcast_nodes(g, G)
        assert out.shape == (sum(ns), F) and torch.equal(out.detach().cpu(), dP[:, :F].to(dtype)[ids])
        out.backward(up)
        assert torch.equal(G.grad.cpu(), rc.exact_expected(R, "sum")["P"][:, :F].to(dtype))
        # SumPooling(broadcast_nodes(g, P)) = n_b P exactly on dyadic P
        back = SumPooling()(g, out.detach())
        want = (dP[:, :F].double() * torch.tensor(ns, dtype=torch.float64)[:, None]).to(dtype)
        assert torch.equal(back.cpu(), want)
    G3 = dP[:, :15].reshape(len(ns), 5, 3).to(DEV)
    assert torch.equal(sirgcn.broadcast_nodes(g, G3).cpu(), dP[:, :15].reshape(len(ns), 5, 3)[ids])


# ------------------------------------------------------------------ 5. determinism
def test_run_to_run_determinism():
    for F in (300, 75):
        ns, X, dP, _ = rc.random_case(R, F)
        for op in rc.OPS:
            runs = []
            for _ in range(2):
                e = torch.zeros(0, dtype=torch.int64)
                g = sirgcn.batch([Graph(e, e, n) for n in ns])      # a fresh graph: fresh offsets
                runs.append(_step(op, g, X.to(DEV), dP.to(DEV)))
            for a, b in zip(*runs):
                assert torch.equal(a, b), f"{op} F={F}"


# ------------------------------------------------------------------ 6. no host synchronisation
@pytest.mark.parametrize("op", rc.OPS)
def test_training_step_captures_and_replays(op):
    F = 96
    ns = rc.sizes(R)
    g = _graph(ns)
    gen = torch.Generator().manual_seed(13)
    xs = [torch.randn(sum(ns), F, generator=gen) for _ in range(2)]
    dP = torch.randn(len(ns), F, generator=gen).to(DEV)
    pool = POOLS[op]()
    Xs = xs[0].to(DEV).requires_grad_(True)

    def step(Xin):
        P = pool(g, Xin)
        gx, = torch.autograd.grad(P, (Xin,), dP)
        return P, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture (allocations, offsets)
        step(Xs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(Xs)
    with torch.no_grad():
        Xs.copy_(xs[1].to(DEV))                        # a changed input, then two replays
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    want = step(xs[1].to(DEV).requires_grad_(True))
    for a, b in zip(outs, want):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("op", ["sum", "mean"])
def test_molecule_model_readout(op):
    g = workloads.molecule_batch(8, 25)
    V, H = g.num_nodes(), 300
    torch.manual_seed(11)
    stack = SIRStack(SIRConv, H, 2, nn.LeakyReLU(0.2), norm_cls=GraphNorm).to(DEV)
    head = nn.Linear(H, 1).to(DEV)
    X = torch.randn(V, H, device=DEV)
    dOut = torch.randn(g.batch_size, 1, device=DEV)
    w = stack.convs[0].linear_query.weight

    def run(readout, head_):
        stack.zero_grad(set_to_none=True)
        h = stack(g, X)
        hg = readout(h)
        (head_(hg) * dOut.to(hg.dtype)).sum().backward()
        return hg.detach(), w.grad.clone()

    ours = run(lambda h: POOLS[op]()(g, h), head)
    ref32 = run(lambda h: _composed(g, h, op), head)
    head64 = nn.Linear(H, 1).to(DEV).double()
    head64.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    truth = run(lambda h: _composed(g, h.double(), op), head64)
    assert ours[0].dtype == torch.float32 and ours[0].shape == (g.batch_size, H)
    assert_parity(ours[0], ref32[0], truth[0], 1e-5, f"molecule model {op} pooled", factor=4.0)
    assert_parity(ours[1], ref32[1], truth[1], 1e-5, f"molecule model {op} dW_Q", factor=4.0)


def test_other_cuda_dtypes_take_the_torch_composition(monkeypatch):
    ns, X, dP, refs = rc.random_case(R, 3)
    g = _graph(ns)
    monkeypatch.setattr(_native, "graph_pool_fwd", lambda *a, **k: pytest.fail("fp64 must not reach the kernels"))
    monkeypatch.setattr(_native, "graph_pool_bwd", lambda *a, **k: pytest.fail("fp64 must not reach the kernels"))
    Xd, dPd = X.double().to(DEV), dP.double().to(DEV)
    for op in rc.OPS:
        r64 = refs[op][1]
        P, dX = _step(op, g, Xd, dPd)
        assert P.dtype == torch.float64 and dX.dtype == torch.float64
        if op == "max":
            assert torch.equal(P.cpu(), r64["P"]) and torch.equal(dX.cpu(), r64["dX"])
        else:
            assert torch.allclose(P.cpu(), r64["P"], rtol=1e-12, atol=1e-12)
            assert torch.allclose(P, _composed(g, Xd, op), rtol=1e-12, atol=1e-12)
            assert torch.allclose(dX.cpu(), r64["dX"], rtol=1e-14, atol=0)
    out = sirgcn.broadcast_nodes(g, dPd)
    assert torch.equal(out.cpu(), dP.double()[_ids(ns)])
