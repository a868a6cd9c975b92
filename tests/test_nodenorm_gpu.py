"""sirgcn.GraphBatchNorm / GraphLayerNorm / GetNorm on the MI355X (models/norm.py:53-60,68-82):
1. norm-only parity against torch's own CPU modules (fp32 scored inside the fp64 envelope);
2. the fused ``forward_act`` equals the module's own forward + torch's activation and add, bit for bit;
3. SIRStack takes the fused pass through its existing hook, with the same bits as the three steps;
4. routing (which inputs run torch's own forward) and drop-in state_dict / GetNorm;
5. run-to-run determinism;  6. a training step captured in a HIP graph replays (no host sync)."""
import pytest
import torch
from torch import nn

from conftest import assert_parity
import width_cases as wc

import sirgcn
from sirgcn import GetNorm, Graph, GraphBatchNorm, GraphLayerNorm, GraphNorm, SIRConv, _native
from sirgcn.stacks import SIRStack

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = _native.BN_SLAB_ROWS            # the BatchNorm kernels' slab (rows per partial)

BN_SHAPES = [(M, N) for M in (2, R - 1, R, R + 1, 3 * R + 7) for N in (1, 3, 75, 95, 128, 256, 300)]
LN_SHAPES = wc.LN_SHAPES
ACTS = {"relu": nn.ReLU, "leaky": lambda: nn.LeakyReLU(0.2), "identity": nn.Identity}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _data(M, N, steps=1, seed=0):
    """X = randn * std + offset with per-column std in [0.5, 2], offset in [-30, 30]; dY; gamma, beta."""
    g = torch.Generator().manual_seed(1000 * M + N + seed)
    std = 0.5 + 1.5 * torch.rand(N, generator=g)
    off = 60.0 * torch.rand(N, generator=g) - 30.0
    xs = [torch.randn(M, N, generator=g) * std + off for _ in range(steps)]
    dys = [torch.randn(M, N, generator=g) for _ in range(steps)]
    gamma = (0.5 + torch.rand(N, generator=g)) * torch.where(torch.rand(N, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.randn(N, generator=g)
    return xs, dys, gamma, beta


def _init(mod, gamma, beta):
    with torch.no_grad():
        mod.weight.copy_(gamma)
        mod.bias.copy_(beta)
    return mod


def _step(mod, X, dY, graph_arg=False):
    """One forward + backward; (Y, dX, dweight, dbias) detached."""
    Xr = X.detach().requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    Y = mod(None, Xr) if graph_arg else mod(Xr)
    Y.backward(dY)
    return Y.detach(), Xr.grad, mod.weight.grad.clone(), mod.bias.grad.clone()


def _score(ours, ref32, ref64, what):
    for name, a, r, t in zip(("Y", "dX", "dweight", "dbias"), ours, ref32, ref64):
        assert a.dtype == torch.float32 and a.shape == r.shape
        assert_parity(a, r, t, 1e-5, f"{what} {name}")


# ------------------------------------------------------------------ 1. norm-only parity
def _bn_case(M, N, wrap=lambda x: x, graph_arg=True):
    xs, dys, gamma, beta = _data(M, N, steps=4)
    ours = _init(GraphBatchNorm(N), gamma, beta).to(DEV)
    r32 = _init(nn.BatchNorm1d(N), gamma, beta)
    r64 = _init(nn.BatchNorm1d(N).double(), gamma.double(), beta.double())
    for k in range(4):
        if k == 3:
            for m in (ours, r32, r64):
                m.eval()
        o = _step(ours, wrap(xs[k].to(DEV)), dys[k].to(DEV), graph_arg=graph_arg and k % 2 == 0)
        a = _step(r32, xs[k], dys[k])
        b = _step(r64, xs[k].double(), dys[k].double())
        _score(o, a, b, f"bn {M}x{N} step {k}")
        if k >= 2:
            assert_parity(ours.running_mean, r32.running_mean, r64.running_mean, 1e-5, f"bn {M}x{N} running_mean {k}")
            assert_parity(ours.running_var, r32.running_var, r64.running_var, 1e-5, f"bn {M}x{N} running_var {k}")
            assert ours.num_batches_tracked.item() == r32.num_batches_tracked.item() == 3


@pytest.mark.parametrize("M,N", BN_SHAPES)
def test_batch_norm_parity(M, N):
    _bn_case(M, N)


def _ln_case(M, N, wrap=lambda x: x):
    xs, dys, gamma, beta = _data(M, N)
    ours = _init(GraphLayerNorm(N), gamma, beta).to(DEV)
    r32 = _init(nn.LayerNorm(N), gamma, beta)
    r64 = _init(nn.LayerNorm(N).double(), gamma.double(), beta.double())
    for graph_arg in (True, False):
        o = _step(ours, wrap(xs[0].to(DEV)), dys[0].to(DEV), graph_arg=graph_arg)
        _score(o, _step(r32, xs[0], dys[0]), _step(r64, xs[0].double(), dys[0].double()), f"ln {M}x{N}")


@pytest.mark.parametrize("M,N", LN_SHAPES)
def test_layer_norm_parity(M, N):
    _ln_case(M, N)


def _sliced(x, pad=3):
    """x as a column slice of a wider tensor: ld > N, rows not 16-B aligned."""
    wide = torch.zeros(x.shape[0], x.shape[1] + pad, device=x.device)
    wide[:, 1:1 + x.shape[1]] = x
    v = wide[:, 1:1 + x.shape[1]]
    assert v.stride(0) == x.shape[1] + pad and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("N", [128, 75])
def test_column_slice_input(N):
    _bn_case(R + 1, N, wrap=_sliced)
    _ln_case(67, N, wrap=_sliced)


@pytest.mark.parametrize("N", wc.LN_UNALIGNED_N)
def test_layer_norm_unaligned_rows(N):
    """N % 4 == 0 rows behind an unaligned column slice: the scalar kernels with every lane's 1, 2, 4, 8, 16
    values in use (N = 64 .. 1024)."""
    _ln_case(67, N, wrap=_sliced)


def test_empty_batch_eval_and_graph_argument():
    N = 75
    _, _, gamma, beta = _data(4, N)
    for ours, ref in ((GraphBatchNorm(N), nn.BatchNorm1d(N)), (GraphLayerNorm(N), nn.LayerNorm(N))):
        _init(ours, gamma, beta).to(DEV).eval()
        _init(ref, gamma, beta).eval()
        o = _step(ours, torch.zeros(0, N, device=DEV), torch.zeros(0, N, device=DEV))
        r = _step(ref, torch.zeros(0, N), torch.zeros(0, N))
        for a, b in zip(o, r):
            assert a.shape == b.shape and torch.equal(a.cpu(), b)
        # the graph argument is not read: None, an empty graph and no graph give the same bits
        X = torch.randn(40, N, device=DEV)
        empty = Graph(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 0)
        assert torch.equal(ours(None, X), ours(X)) and torch.equal(ours(empty, X), ours(X))


# ------------------------------------------------------------------ 2. fused == composed, bit for bit
def _fused_vs_composed(mod, M, N, act_name, with_resid, training):
    xs, dys, _, _ = _data(M, N, seed=7)
    X, dY = xs[0].to(DEV), dys[0].to(DEV)
    Rr = torch.randn(M, N, device=DEV) if with_resid else None
    act = ACTS[act_name]()
    mod.train(training)
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    out = []
    for fused in (True, False):
        mod.load_state_dict(state)
        mod.zero_grad(set_to_none=True)
        Xr = X.clone().requires_grad_(True)
        Rq = Rr.clone().requires_grad_(True) if with_resid else None
        if fused:
            Y = mod.forward_act(None, Xr, act, Rq)
            assert Y is not None, "the fused pass was refused"
        else:
            Y = act(mod(None, Xr))
            if with_resid:
                Y = Y + Rq
        Y.backward(dY)
        out.append((Y.detach(), Xr.grad, Rq.grad if with_resid else None, mod.weight.grad.clone(),
                    mod.bias.grad.clone(), {k: v.clone() for k, v in mod.state_dict().items()}))
    for name, a, b in zip(("Y", "dX", "dR", "dweight", "dbias"), out[0], out[1]):
        assert (a is None and b is None) or torch.equal(a, b), f"{name} differs ({act_name}, resid {with_resid})"
    for k in state:
        assert torch.equal(out[0][5][k], out[1][5][k]), k
    if with_resid:
        assert torch.equal(out[0][2], dY)


@pytest.mark.parametrize("with_resid", [False, True])
@pytest.mark.parametrize("act_name", ["relu", "leaky", "identity"])
def test_fused_equals_composed_bit_for_bit(act_name, with_resid):
    for M, N in ((3 * R + 7, 128), (R + 1, 75)):
        _, _, gamma, beta = _data(M, N)
        bn = _init(GraphBatchNorm(N), gamma, beta).to(DEV)
        _fused_vs_composed(bn, M, N, act_name, with_resid, training=True)
        _fused_vs_composed(bn, M, N, act_name, with_resid, training=False)
        ln = _init(GraphLayerNorm(N), gamma, beta).to(DEV)
        _fused_vs_composed(ln, M, N, act_name, with_resid, training=True)


# ------------------------------------------------------------------ 3. the stack takes the fused pass
def _small_batched_graph():
    g = torch.Generator().manual_seed(3)
    graphs = []
    for n in (23, 1, 40, 17, 31):
        e = 3 * n
        graphs.append(Graph(torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g), n))
    return sirgcn.batch(graphs)


@pytest.mark.parametrize("norm_cls,order", [(GraphBatchNorm, "arxiv"), (GraphLayerNorm, "zinc")])
def test_stack_takes_the_fused_pass(norm_cls, order, monkeypatch):
    graph = _small_batched_graph()
    V, H = graph.num_nodes(), 32
    torch.manual_seed(5)
    stack = SIRStack(SIRConv, H, 3, nn.LeakyReLU(0.2), "sym", order=order, norm_cls=norm_cls).to(DEV)
    with torch.no_grad():
        for norm in stack.norms:
            norm.weight.uniform_(0.5, 1.5)
            norm.bias.normal_()
    X = torch.randn(V, H, device=DEV)
    dY = torch.randn(V, H, device=DEV)
    state = {k: v.clone() for k, v in stack.state_dict().items()}
    calls = []
    orig = norm_cls.forward_act

    def spy(self, *a, **k):
        out = orig(self, *a, **k)
        calls.append(out is not None)
        return out

    def run():
        stack.load_state_dict(state)
        stack.zero_grad(set_to_none=True)
        Xr = X.clone().requires_grad_(True)
        Y = stack(graph, Xr)
        Y.backward(dY)
        grads = {n: p.grad.clone() for n, p in stack.named_parameters()}
        return Y.detach(), Xr.grad, grads, {k: v.clone() for k, v in stack.state_dict().items()}

    monkeypatch.setattr(norm_cls, "forward_act", spy)
    fused = run()
    assert calls == [True] * 3, f"the fused norm pass did not run in every layer: {calls}"
    monkeypatch.setattr(norm_cls, "forward_act", lambda self, *a, **k: None)
    plain = run()
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])
    assert set(fused[2]) == set(plain[2]) and all(g is not None for g in plain[2].values())
    for k in plain[2]:
        assert torch.equal(fused[2][k], plain[2][k]), k
    for k in plain[3]:
        assert torch.equal(fused[3][k], plain[3][k]), k


# ------------------------------------------------------------------ 4. routing and drop-in
def test_state_dict_round_trip():
    N = 20
    for ours_cls, ref_cls in ((GraphBatchNorm, nn.BatchNorm1d), (GraphLayerNorm, nn.LayerNorm)):
        ref = ref_cls(N)
        with torch.no_grad():
            for p in ref.parameters():
                p.normal_()
            for b in ref.buffers():
                b.copy_(torch.rand_like(b.float()).to(b.dtype) + 3)
        ours = ours_cls(N)
        assert list(ours.state_dict()) == list(ref.state_dict())
        ours.load_state_dict(ref.state_dict())
        back = ref_cls(N)
        back.load_state_dict(ours.state_dict())
        for k, v in ref.state_dict().items():
            assert torch.equal(back.state_dict()[k], v), k
    assert "running_mean" in GraphBatchNorm(N).state_dict() and "num_batches_tracked" in GraphBatchNorm(N).state_dict()


def _torch_bits(ours, ref, X, what):
    ours.to(DEV)
    ref.to(DEV)
    ref.load_state_dict(ours.state_dict())
    assert ours.forward_act(None, X, nn.ReLU(), None) is None, f"{what}: forward_act must refuse"
    a, b = ours(None, X), ref(X)
    assert a.dtype == b.dtype and torch.equal(a, b), what
    for k, v in ref.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), (what, k)


def test_non_native_inputs_run_torchs_own_forward():
    N = 24
    X = torch.randn(50, N, device=DEV) * 2 + 5
    _torch_bits(GraphBatchNorm(N), nn.BatchNorm1d(N), X.bfloat16(), "bn bf16")
    _torch_bits(GraphBatchNorm(N).double(), nn.BatchNorm1d(N).double(), X.double(), "bn fp64")
    _torch_bits(GraphBatchNorm(N, momentum=None), nn.BatchNorm1d(N, momentum=None), X, "bn momentum=None")
    _torch_bits(GraphBatchNorm(N, affine=False), nn.BatchNorm1d(N, affine=False), X, "bn affine=False")
    _torch_bits(GraphBatchNorm(N, track_running_stats=False), nn.BatchNorm1d(N, track_running_stats=False), X,
                "bn track_running_stats=False")
    _torch_bits(GraphBatchNorm(N), nn.BatchNorm1d(N), X.t().reshape(2, N, 25).contiguous(), "bn 3-D")
    _torch_bits(GraphLayerNorm(N).half(), nn.LayerNorm(N).half(), X.half(), "ln fp16")
    _torch_bits(GraphLayerNorm(N, elementwise_affine=False), nn.LayerNorm(N, elementwise_affine=False), X,
                "ln affine=False")
    _torch_bits(GraphLayerNorm(N), nn.LayerNorm(N), X.reshape(5, 10, N), "ln 3-D")
    wide = torch.randn(9, 1028, device=DEV)
    _torch_bits(GraphLayerNorm(1028), nn.LayerNorm(1028), wide, "ln N > 1024")


def test_fused_pass_is_refused_for_gelu_hooks_and_foreign_residuals():
    N = 16
    X = torch.randn(30, N, device=DEV)
    for mod in (GraphBatchNorm(N).to(DEV), GraphLayerNorm(N).to(DEV)):
        assert mod.forward_act(None, X, nn.GELU(), None) is None
        assert mod.forward_act(None, X, nn.ReLU(), X.double()) is None
        assert mod.forward_act(None, X, nn.ReLU(), X[:, :8]) is None
        assert mod.forward_act(None, X.cpu(), nn.ReLU(), None) is None
        act = nn.ReLU()
        h = act.register_forward_hook(lambda *a: None)
        assert mod.forward_act(None, X, act, None) is None
        h.remove()
        h = mod.register_forward_pre_hook(lambda *a: None)
        assert mod.forward_act(None, X, nn.ReLU(), None) is None
        h.remove()
        assert mod.forward_act(None, X, nn.ReLU(), None) is not None
    # under autocast an fp32 input stays on the native path (torch runs both norms in fp32 there too)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for mod in (GraphBatchNorm(N).to(DEV), GraphLayerNorm(N).to(DEV)):
            out = mod.forward_act(None, X, nn.ReLU(), None)
            assert out is not None and out.dtype == torch.float32


def test_cpu_tensor_and_single_row_training_raise():
    N = 8
    for mod in (GraphBatchNorm(N), GraphLayerNorm(N)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod(None, torch.randn(4, N))
    bn = GraphBatchNorm(N).to(DEV)
    for call in (lambda x: bn(x), lambda x: bn(None, x), lambda x: bn.forward_act(None, x, nn.ReLU(), None)):
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            call(torch.randn(1, N, device=DEV))
    assert bn.num_batches_tracked.item() == 0
    bn.eval()
    assert bn(torch.randn(1, N, device=DEV)).shape == (1, N)


def test_get_norm_factory():
    N = 12
    for name, cls in (("bn", GraphBatchNorm), ("ln", GraphLayerNorm), ("gn", GraphNorm), ("none", nn.Identity)):
        m = GetNorm(name, True, N) if name != "none" else GetNorm(name, True)
        assert isinstance(m.norm, cls)
        assert all(k.startswith("norm.") for k in m.state_dict()) and (name == "none" or len(m.state_dict()) >= 2)
    assert set(GetNorm("bn", False, N).state_dict()) == {"norm.weight", "norm.bias", "norm.running_mean",
                                                         "norm.running_var", "norm.num_batches_tracked"}
    assert isinstance(GetNorm("ln", False, N, eps=1e-3).norm, GraphLayerNorm)
    assert GetNorm("ln", False, N, eps=1e-3).norm.eps == 1e-3
    for args in (("cn", True, N), ("cn", False, N)):
        with pytest.raises(NotImplementedError, match="cn"):
            GetNorm(*args)
    with pytest.raises(NotImplementedError):
        GetNorm("gn", False, N)
    # both call forms, and forward_act forwarded to the inner norm
    X = torch.randn(33, N, device=DEV)
    g = Graph(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 33, [20, 13])
    for name in ("bn", "ln", "gn"):
        m = GetNorm(name, True, N).to(DEV)
        inner_state = {k: v.clone() for k, v in m.state_dict().items()}
        fused = m.forward_act(g, X, nn.LeakyReLU(0.2), X)
        m.load_state_dict(inner_state)
        assert fused is not None and torch.equal(fused, nn.functional.leaky_relu(m(g, X), 0.2) + X), name
    m = GetNorm("bn", False, N).to(DEV)
    assert m(X).shape == X.shape
    ident = GetNorm("none", True)
    assert ident(g, X) is X and GetNorm("none", False)(X) is X
    assert ident.forward_act(g, X, nn.ReLU(), None) is None


# ------------------------------------------------------------------ 5. determinism
def test_run_to_run_determinism():
    for cls, M, N in ((GraphBatchNorm, 3 * R + 7, 300), (GraphBatchNorm, 3 * R + 7, 75), (GraphLayerNorm, 1000, 300),
                      (GraphLayerNorm, 1000, 75)):
        xs, dys, gamma, beta = _data(M, N, seed=11)
        X, dY, Rr = xs[0].to(DEV), dys[0].to(DEV), torch.randn(M, N, device=DEV)
        runs = []
        for _ in range(2):
            mod = _init(cls(N), gamma, beta).to(DEV)
            Xr = X.clone().requires_grad_(True)
            Y = mod.forward_act(None, Xr, nn.LeakyReLU(0.2), Rr)
            Y.backward(dY)
            runs.append([Y.detach(), Xr.grad, mod.weight.grad, mod.bias.grad] + [b.clone() for b in mod.buffers()])
        for a, b in zip(*runs):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ 6. no host synchronisation
@pytest.mark.parametrize("cls", [GraphBatchNorm, GraphLayerNorm])
def test_training_step_captures_and_replays(cls):
    M, N = 3 * R + 7, 96
    xs, dys, gamma, beta = _data(M, N, steps=2, seed=13)
    mod = _init(cls(N), gamma, beta).to(DEV)
    ref = _init(cls(N), gamma, beta).to(DEV)
    act = nn.LeakyReLU(0.2)
    Xs = xs[0].to(DEV).requires_grad_(True)
    dY = dys[0].to(DEV)
    Rr = torch.randn(M, N, device=DEV)

    def step(m, Xin):
        Y = m.forward_act(None, Xin, act, Rr)
        gx, gw, gb = torch.autograd.grad(Y, (Xin, m.weight, m.bias), dY)
        return Y, gx, gw, gb

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture (allocations, library load)
        step(_init(cls(N), gamma, beta).to(DEV), Xs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(mod, Xs)
    with torch.no_grad():
        Xs.copy_(xs[1].to(DEV))                       # a changed input, then two replays
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    want = None
    for _ in range(2):                                # the capture pass itself ran nothing: two steps in all
        want = step(ref, xs[1].to(DEV).requires_grad_(True))
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    if cls is GraphBatchNorm:
        assert mod.num_batches_tracked.item() == 2
        for a, b in zip(mod.buffers(), ref.buffers()):
            assert torch.equal(a, b)
