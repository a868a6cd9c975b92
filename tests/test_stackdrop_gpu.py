"""The layer dropout fused into the norm -> activation -> residual pass (``sir_*_norm_act_drop_*``,
``forward_act(..., dropout=(seed, p))``, ``SIRStack(..., dropout=p)``) on the MI355X.

Everything at the kernel level is exact: the mask is the one ``sir_dropout_apply`` writes for an [M, N] block at
col0 = 0, and the fused pass follows torch's autograd order for act -> dropout -> add, so
  forward : out == where(m != 0, a * m, 0) + R     (a = the existing fused pass without residual, m = mask * scale)
  backward: every gradient == autograd through a * m + R on the existing fused function
bit for bit.  The stack is held to the 1e-5 relative bar of the stack parity tests against the hand-composed loop
on explicit masks."""
import copy

import pytest
import torch
from torch import nn

from conftest import assert_close
import width_cases as wc

import sirgcn
from sirgcn import Graph, GraphBatchNorm, GraphLayerNorm, GraphNorm, GetNorm, SIRConv, _native
from sirgcn.norm import BatchNormActFunction, GraphNormActFunction, LayerNormActFunction
from sirgcn.stacks import SIRStack

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x1234_5678_9ABC

# the smallest shapes at which each kernel's partition can go wrong (slab = 128 rows; float4 / scalar columns;
# LayerNorm's every count of vectors per lane, tests/width_cases.py; an empty, a one-node and a multi-chunk graph)
BN_SHAPES = [(2, 4), (129, 75), (257, 256), (130, 300)]
LN_SHAPES = wc.STACKDROP_LN_SHAPES
GN_SIZES = [0, 1, 7, 130, 33]
GN_WIDTHS = [75, 256]
ACTS = {"relu": nn.ReLU, "leaky": lambda: nn.LeakyReLU(0.2), "identity": nn.Identity}
PS = (0.2, 0.5)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _mask(M, N, seed, p):
    """m = keep * scale: the bits sir_dropout_apply writes for an [M, N] block at col0 = 0."""
    return _native.dropout_apply(torch.ones(M, N, device=DEV), (seed, p))


def _gn_graph(sizes=GN_SIZES):
    e = torch.zeros(0, dtype=torch.int64)
    return sirgcn.batch([Graph(e, e, n) for n in sizes])


class _Case:
    """One norm module with data: ``fa(mod, X, R, dropout)`` runs its forward_act, ``params(mod)`` lists the
    parameters whose gradients are compared."""

    def __init__(self, kind, M, N, act_name, seed=0):
        g = torch.Generator().manual_seed(1000 * M + N + seed)
        self.kind, self.M, self.N = kind, M, N
        self.act = ACTS[act_name]()
        self.graph = _gn_graph() if kind == "gn" else None
        std = 0.5 + 1.5 * torch.rand(N, generator=g)
        off = 6.0 * torch.rand(N, generator=g) - 3.0
        self.X = (torch.randn(M, N, generator=g) * std + off).to(DEV)
        self.dY = torch.randn(M, N, generator=g).to(DEV)
        self.R = torch.randn(M, N, generator=g).to(DEV)
        mod = {"bn": GraphBatchNorm, "ln": GraphLayerNorm, "gn": GraphNorm}[kind](N)
        with torch.no_grad():
            mod.weight.copy_((0.5 + torch.rand(N, generator=g)) * torch.where(torch.rand(N, generator=g) < 0.25, -1.0, 1.0))
            mod.bias.copy_(torch.randn(N, generator=g))
            if kind == "gn":
                mod.mean_scale.copy_(0.5 + torch.rand(N, generator=g))
        self.mod = mod.to(DEV).train()

    def params(self, mod):
        return [mod.weight, mod.bias] + ([mod.mean_scale] if self.kind == "gn" else [])

    def fa(self, mod, X, R=None, dropout=None):
        if dropout is None:
            out = mod.forward_act(self.graph, X, self.act, R)
        else:
            out = mod.forward_act(self.graph, X, self.act, R, dropout=dropout)
        assert out is not None, "the fused pass was refused"
        return out

    def step(self, fn, with_resid, mod=None):
        """fn(mod, X, R) -> Y on a copy of the module; (Y, dX, dR, parameter grads..., module copy)."""
        mod = copy.deepcopy(self.mod) if mod is None else mod
        X = self.X.clone().requires_grad_(True)
        R = self.R.clone().requires_grad_(True) if with_resid else None
        Y = fn(mod, X, R)
        Y.backward(self.dY)
        return [Y.detach(), X.grad, R.grad if with_resid else None] + [q.grad for q in self.params(mod)] + [mod]


def _exact(case, p, with_resid, seed=SEED):
    """Forward and backward of the fused dropout against the existing fused pass times the explicit mask."""
    m = _mask(case.M, case.N, seed, p)
    assert 0 < int((m == 0).sum()) < m.numel() or m.numel() < 16
    ref = case.step(lambda mod, X, R: case.fa(mod, X) * m + (R if R is not None else 0), with_resid)
    got = case.step(lambda mod, X, R: case.fa(mod, X, R, dropout=(seed, p)), with_resid)
    a = case.fa(copy.deepcopy(case.mod), case.X)
    want = torch.where(m != 0, a * m, torch.zeros_like(a))
    if with_resid:
        want = want + case.R
    assert torch.equal(got[0], want), "forward"
    names = ["Y", "dX", "dR", "dweight", "dbias", "dmean_scale"]
    for name, u, v in zip(names[1:], got[1:-1], ref[1:-1]):
        assert (u is None and v is None) or torch.equal(u, v), f"{name} (p {p}, resid {with_resid})"
    if with_resid:
        assert torch.equal(got[2], case.dY)
    for (k, u), (_, v) in zip(got[-1].state_dict().items(), ref[-1].state_dict().items()):
        assert torch.equal(u, v), k              # BatchNorm: running_mean / running_var / num_batches_tracked
    if case.kind == "bn":
        assert got[-1].num_batches_tracked.item() == 1


# ------------------------------------------------------------------ forward and backward, exact
@pytest.mark.parametrize("act_name", list(ACTS))
@pytest.mark.parametrize("M,N", BN_SHAPES)
def test_batch_norm_dropout_is_exact(M, N, act_name):
    case = _Case("bn", M, N, act_name)
    for p in PS:
        for with_resid in (False, True):
            _exact(case, p, with_resid)


@pytest.mark.parametrize("act_name", list(ACTS))
@pytest.mark.parametrize("M,N", LN_SHAPES)
def test_layer_norm_dropout_is_exact(M, N, act_name):
    case = _Case("ln", M, N, act_name)
    for p in PS:
        for with_resid in (False, True):
            _exact(case, p, with_resid)


@pytest.mark.parametrize("act_name", list(ACTS))
@pytest.mark.parametrize("F", GN_WIDTHS)
def test_graph_norm_dropout_is_exact(F, act_name):
    case = _Case("gn", sum(GN_SIZES), F, act_name)
    for p in PS:
        for with_resid in (False, True):
            _exact(case, p, with_resid)


def test_graph_norm_without_bias_and_mean_scale():
    case = _Case("gn", sum(GN_SIZES), 75, "leaky")
    mod = GraphNorm(75, bias=False, mean_scale=False).to(DEV).train()
    with torch.no_grad():
        mod.weight.copy_(case.mod.weight)
    case.mod = mod
    case.params = lambda m: [m.weight]
    _exact(case, 0.2, True)


# ------------------------------------------------------------------ identity cases
KINDS = [("bn", 129, 75), ("ln", 67, 256), ("gn", sum(GN_SIZES), 75)]
DROP_ENTRIES = ("batch_norm_act_drop_fwd", "batch_norm_act_drop_bwd", "layer_norm_act_drop_fwd",
                "layer_norm_act_drop_bwd", "graph_norm_act_drop_fwd", "graph_norm_act_drop_bwd")


def _count_drop_entries(monkeypatch):
    """Records ``<norm>_act_drop_fwd`` / ``_bwd`` for every call of a fused norm wrapper that is given a layer
    dropout (``drop`` not None, last positional argument or keyword): the calls that take the C ``*_drop_*`` entries."""
    calls = []
    for name in DROP_ENTRIES:
        wrapper = name.replace("_drop", "")
        orig = getattr(_native, wrapper)
        n_plain = orig.__code__.co_argcount - 1             # ``drop`` is the last parameter

        def spy(*a, _o=orig, _n=name, _k=n_plain, **k):
            drop = k["drop"] if "drop" in k else (a[_k] if len(a) > _k else None)
            if drop is not None:
                calls.append(_n)
            return _o(*a, **k)
        monkeypatch.setattr(_native, wrapper, spy)
    return calls


@pytest.mark.parametrize("kind,M,N", KINDS)
def test_p_zero_none_and_eval_take_the_existing_entries(kind, M, N, monkeypatch):
    case = _Case(kind, M, N, "leaky")
    calls = _count_drop_entries(monkeypatch)
    base = case.step(lambda mod, X, R: case.fa(mod, X, R), True)
    for dropout in (None, (SEED, 0.0), (SEED, 0)):
        got = case.step(lambda mod, X, R: case.fa(mod, X, R, dropout=dropout), True)
        for u, v in zip(got[:-1], base[:-1]):
            assert torch.equal(u, v)
    ev = copy.deepcopy(case.mod).eval()
    base_ev = case.step(lambda mod, X, R: case.fa(mod, X, R), True, mod=copy.deepcopy(ev))
    got_ev = case.step(lambda mod, X, R: case.fa(mod, X, R, dropout=(SEED, 0.5)), True, mod=copy.deepcopy(ev))
    for u, v in zip(got_ev[:-1], base_ev[:-1]):
        assert torch.equal(u, v)
    assert calls == [], f"eval mode / p == 0 must call the existing entries: {calls}"
    # ... and the new entries themselves, given p <= 0, run the kernels without dropout
    fn = {"bn": BatchNormActFunction, "ln": LayerNormActFunction, "gn": GraphNormActFunction}[kind]
    code = (_native.ACT_LEAKY, 0.2)

    def direct(mod, X, R):
        if kind == "bn":
            mod.num_batches_tracked.add_(1)
            return fn.apply(X, mod.weight, mod.bias, mod.running_mean, mod.running_var, True, mod.momentum, mod.eps,
                            code[0], code[1], R, (SEED, 0.0))
        if kind == "ln":
            return fn.apply(X, mod.weight, mod.bias, mod.eps, code[0], code[1], R, (SEED, -1.0))
        off = sirgcn.graph.node_offsets(case.graph, X.device)
        return fn.apply(X, mod.weight, mod.bias, mod.mean_scale, off, mod.eps, code[0], code[1], R, (SEED, 0.0))
    got = case.step(direct, True)
    assert len(calls) == 2
    for u, v in zip(got[:-1], base[:-1]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("kind,M,N", KINDS)
def test_p_one_drops_everything(kind, M, N):
    case = _Case(kind, M, N, "leaky")
    got = case.step(lambda mod, X, R: case.fa(mod, X, R, dropout=(SEED, 1.0)), True)
    assert torch.equal(got[0], case.R)
    assert torch.equal(got[1], torch.zeros_like(got[1])) and torch.equal(got[2], case.dY)
    got = case.step(lambda mod, X, R: case.fa(mod, X, None, dropout=(SEED, 1.0)), False)
    assert torch.equal(got[0], torch.zeros_like(got[0])) and not torch.signbit(got[0]).any()
    assert torch.equal(got[1], torch.zeros_like(got[1]))


def test_bad_probabilities_are_refused():
    case = _Case("ln", 5, 8, "relu")
    for p in (float("nan"), -0.1, 1.5):
        with pytest.raises(ValueError):
            case.fa(case.mod, case.X, None, dropout=(SEED, p))
    Y, mean = torch.empty_like(case.X), torch.empty(5, device=DEV)
    with pytest.raises(RuntimeError, match="sir_layer_norm_act_drop_fwd: dropout p is NaN"):
        _native.layer_norm_act_fwd(case.X, case.mod.weight.detach(), case.mod.bias.detach(), 1e-5, 1, 0.0, None,
                                   Y, mean, torch.empty_like(mean), drop=(SEED, float("nan")))


# ------------------------------------------------------------------ seeds
@pytest.mark.parametrize("kind,M,N", KINDS)
def test_device_seed_equals_seed_by_value_and_words_differ(kind, M, N):
    case = _Case(kind, M, N, "relu")
    st = torch.tensor([SEED], dtype=torch.int64, device=DEV)
    by_value = case.step(lambda mod, X, R: case.fa(mod, X, R, dropout=(SEED, 0.2)), True)
    by_ptr = case.step(lambda mod, X, R: case.fa(mod, X, R, dropout=(st, 0.2)), True)
    for u, v in zip(by_value[:-1], by_ptr[:-1]):
        assert torch.equal(u, v)
    other = case.step(lambda mod, X, R: case.fa(mod, X, R, dropout=(SEED + 1, 0.2)), True)
    assert not torch.equal(other[0], by_value[0])
    assert not torch.equal(_mask(M, N, SEED, 0.2), _mask(M, N, SEED + 1, 0.2))
    # the mask is a function of the global row: GraphNorm hashes the row of X, not the row within its graph
    if kind == "gn":
        a = case.fa(copy.deepcopy(case.mod), case.X)
        m = _mask(M, N, SEED, 0.2)
        assert torch.equal(by_value[0], torch.where(m != 0, a * m, torch.zeros_like(a)) + case.R)


def test_get_norm_passes_the_dropout_through():
    M, N = 130, 75
    case = _Case("bn", M, N, "leaky")
    wrap = GetNorm("bn", True, N).to(DEV).train()
    wrap.norm.load_state_dict(case.mod.state_dict())
    X = case.X.clone().requires_grad_(True)
    got = wrap.forward_act(None, X, case.act, case.R, dropout=(SEED, 0.2))
    want = case.fa(copy.deepcopy(case.mod), case.X, case.R, dropout=(SEED, 0.2))
    assert torch.equal(got, want)
    assert torch.equal(wrap.forward_act(None, X, case.act, case.R),
                       case.fa(copy.deepcopy(case.mod), case.X, case.R))


# ------------------------------------------------------------------ column slices, non-finite values
def _sliced(x, pad=3):
    """x as a column slice of a wider tensor whose padding columns hold NaN: ld > N, rows not 16-B aligned."""
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=x.device)
    wide[:, 1:1 + x.shape[1]] = x
    v = wide[:, 1:1 + x.shape[1]]
    assert v.stride(0) == x.shape[1] + pad
    return v


@pytest.mark.parametrize("kind,M,N", [("bn", 129, 128), ("ln", 67, 75)])
def test_column_slice_input_with_nan_padding(kind, M, N):
    """The padding columns of a view with ld > N are never read: the bits are those of the contiguous input.
    (LayerNorm at a scalar-column width: its float4 rows sum a row in another order than the scalar rows an
    unaligned view takes, so only equal vector widths are bit-comparable; BatchNorm's columns are independent.)"""
    case = _Case(kind, M, N, "leaky")
    base = case.step(lambda mod, X, R: case.fa(mod, X, R, dropout=(SEED, 0.2)), True)
    X = _sliced(case.X).detach().requires_grad_(True)
    R = _sliced(case.R)
    mod = copy.deepcopy(case.mod)
    Y = case.fa(mod, X, R, dropout=(SEED, 0.2))
    Y.backward(_sliced(case.dY))
    assert torch.equal(Y, base[0]) and torch.equal(X.grad, base[1])
    assert torch.equal(mod.weight.grad, base[3]) and torch.equal(mod.bias.grad, base[4])


def test_dropped_elements_are_zero_whatever_they_held():
    """Deviation (1) of the non-finite contract: a dropped element is +0 before the add (an Inf there does not
    reach the output), a kept one propagates, and a NaN of R comes through exactly where R holds it."""
    M, N, p = 9, 75, 0.5
    case = _Case("ln", M, N, "identity")
    with torch.no_grad():
        case.mod.weight[::2] = 3.0e38                  # y = xhat * 3e38 overflows wherever |xhat| > 1.13
    a = case.fa(copy.deepcopy(case.mod), case.X).detach()
    m = _mask(M, N, SEED, p)
    inf = torch.isinf(a)
    assert (inf & (m == 0)).any() and (inf & (m != 0)).any()
    R = case.R.clone()
    R[4, 7] = R[4, 70] = float("nan")
    out = case.fa(copy.deepcopy(case.mod), case.X, R, dropout=(SEED, p)).detach()
    assert torch.equal(torch.isnan(out), torch.isnan(R))
    dropped = (m == 0) & ~torch.isnan(R)
    assert torch.equal(out[dropped], R[dropped])
    kept_inf = inf & (m != 0) & ~torch.isnan(R)
    assert torch.equal(out[kept_inf], a[kept_inf])     # +-Inf * scale + R = +-Inf


# ------------------------------------------------------------------ the stack
def _batched_graph():
    g = torch.Generator().manual_seed(3)
    graphs = []
    for n in (23, 1, 40, 17, 31):
        e = 3 * n
        graphs.append(Graph(torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g), n))
    return sirgcn.batch(graphs)


def _composed(stack, graph, h, masks):
    """The reference's layer loop with the dropout as an explicit multiply by the layer's mask."""
    for i, conv in enumerate(stack.convs):
        resid = h
        h = conv(graph, h)
        if stack.order == "zinc":
            h = h + resid
        h = stack.activation(stack.norms[i](graph, h))
        h = h * masks[i]
        if stack.order == "arxiv":
            h = h + resid
    return h


def _make_stack(norm_cls, order, **kw):
    torch.manual_seed(5)
    stack = SIRStack(SIRConv, 64, 2, nn.LeakyReLU(0.2), order=order, norm_cls=norm_cls, dropout=0.2, **kw).to(DEV)
    with torch.no_grad():
        for norm in stack.norms:
            norm.weight.uniform_(0.5, 1.5)
            norm.bias.normal_()
    return stack.train()


def _stack_step(fn, stack, X, dY):
    stack.zero_grad(set_to_none=True)
    Xr = X.clone().requires_grad_(True)
    Y = fn(Xr)
    Y.backward(dY)
    return Y.detach(), Xr.grad, {n: q.grad.clone() for n, q in stack.named_parameters()}


@pytest.mark.parametrize("norm_cls,order,entry", [(GraphBatchNorm, "arxiv", "batch_norm"),
                                                  (GraphLayerNorm, "zinc", "layer_norm"),
                                                  (GraphNorm, "zinc", "graph_norm")])
def test_stack_takes_the_fused_dropout_pass(norm_cls, order, entry, monkeypatch):
    graph = _batched_graph()
    V = graph.num_nodes()
    stack = _make_stack(norm_cls, order)
    X, dY = torch.randn(V, 64, device=DEV), torch.randn(V, 64, device=DEV)
    calls = _count_drop_entries(monkeypatch)
    seeds = []

    def run(x):
        y = stack(graph, x)
        seeds.append(stack.layer_seeds.clone())       # the words of this step (one per layer)
        return y
    got = _stack_step(run, stack, X, dY)
    assert sorted(calls) == [entry + "_act_drop_bwd"] * 2 + [entry + "_act_drop_fwd"] * 2, calls
    words = seeds[0].tolist()
    assert len(words) == 2 and words[0] != words[1]
    masks = [_mask(V, 64, w, 0.2) for w in words]
    want = _stack_step(lambda x: _composed(stack, graph, x, masks), stack, X, dY)
    assert_close(got[0], want[0], 1e-5, "stack h*")
    assert_close(got[1], want[1], 1e-5, "stack dX")
    assert got[2].keys() == want[2].keys()
    for k in want[2]:
        assert_close(got[2][k], want[2][k], 1e-5, f"stack d{k}")
    # eval mode: no draw, the entries without dropout, the bits of a stack built without dropout
    del calls[:]
    stack.eval()
    y_eval = stack(graph, X)
    assert calls == [] and stack.layer_seeds is None
    plain = SIRStack(SIRConv, 64, 2, nn.LeakyReLU(0.2), order=order, norm_cls=norm_cls).to(DEV).eval()
    plain.load_state_dict(stack.state_dict())
    assert torch.equal(y_eval, plain(graph, X))


def test_layer_seed_words_are_never_a_convs(monkeypatch):
    """The layers' words come from the convs' single draw and differ from every conv's word (the conv's Q dropout
    hashes the same (row, col) domain)."""
    import sirgcn.conv as sc
    graph = _batched_graph()
    stack = _make_stack(GraphBatchNorm, "arxiv", feat_dropout=0.1)
    X = torch.randn(graph.num_nodes(), 64, device=DEV)
    draws = []
    orig = torch.randint
    monkeypatch.setattr(torch, "randint", lambda *a, **k: draws.append(orig(*a, **k)) or draws[-1])
    conv_seeds = []
    orig_drop = sc.SIRConv._drop
    monkeypatch.setattr(sc.SIRConv, "_drop", lambda self, dev: conv_seeds.append(orig_drop(self, dev)) or conv_seeds[-1])
    stack(graph, X)
    assert [d.numel() for d in draws] == [4], "one draw: two conv words, then two layer words"
    conv_words = [int(s[0].item()) for s in conv_seeds]
    layer_words = stack.layer_seeds.tolist()
    assert len(conv_words) == 2 and len(layer_words) == 2
    assert len(set(conv_words + layer_words)) == 4
    assert all(w < 2 ** 62 for w in conv_words) and all(w >= 2 ** 62 for w in layer_words)
    # without the layer dropout the draw is the convs' alone
    del draws[:]
    plain = SIRStack(SIRConv, 64, 2, nn.LeakyReLU(0.2), order="arxiv", norm_cls=GraphBatchNorm,
                     feat_dropout=0.1).to(DEV).train()
    plain(graph, X)
    assert [d.numel() for d in draws] == [2] and plain.layer_seeds is None


def test_stack_falls_back_to_its_own_dropout(monkeypatch):
    """A norm whose forward_act does not take ``dropout`` (or refuses), and a stack without a norm, get
    ``self.dropout`` at the reference's position."""
    graph = _batched_graph()
    V = graph.num_nodes()
    X = torch.randn(V, 64, device=DEV)
    stack = _make_stack(GraphBatchNorm, "arxiv")
    calls = _count_drop_entries(monkeypatch)
    seen = []
    stack.dropout.register_forward_hook(lambda mod, args, out: seen.append((args[0], out)))
    monkeypatch.setattr(GraphBatchNorm, "forward_act", lambda self, graphs, feats, activation, resid=None: None)
    stack(graph, X)
    assert calls == [] and len(seen) == 2
    nonorm = SIRStack(SIRConv, 64, 2, nn.LeakyReLU(0.2), order="zinc", dropout=0.2).to(DEV).train()
    hits = []
    nonorm.dropout.register_forward_hook(lambda mod, args, out: hits.append(1))
    import sirgcn.stacks as st
    monkeypatch.setattr(st, "_resid_act", lambda *a: pytest.fail("the norm-less fused pass has no dropout"))
    nonorm(graph, X)
    assert len(hits) == 2 and nonorm.layer_seeds is None


# ------------------------------------------------------------------ graph capture
def test_captured_training_step_draws_a_fresh_layer_mask_per_replay():
    """A training step of the stack captured in a HIP graph: the seed words are drawn on the device inside the
    capture, so two replays use two different masks, and within a replay the forward and the backward agree
    (they equal the composed step on that replay's own masks)."""
    graph = _batched_graph()
    V = graph.num_nodes()
    stack = _make_stack(GraphBatchNorm, "arxiv")
    gen = torch.Generator().manual_seed(8)
    X, dY = torch.randn(V, 64, generator=gen).to(DEV), torch.randn(V, 64, generator=gen).to(DEV)
    x = X.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up (plans, packs) outside the capture
        for _ in range(2):
            stack.zero_grad(set_to_none=False)
            x.grad = None
            stack(graph, x).backward(dY)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    x.grad = torch.zeros_like(x)
    stack.zero_grad(set_to_none=False)
    with torch.cuda.graph(cg):
        Y = stack(graph, x)
        Y.backward(dY)
    words = stack.layer_seeds
    outs = []
    for _ in range(2):
        x.grad.zero_()
        cg.replay()
        torch.cuda.synchronize()
        outs.append((words.clone(), Y.detach().clone(), x.grad.clone()))
    assert not torch.equal(outs[0][0], outs[1][0]), "the captured seed draw must run again on replay"
    assert not torch.equal(outs[0][1], outs[1][1]), "two replays must use two different masks"
    masks = [_mask(V, 64, w, 0.2) for w in outs[1][0].tolist()]
    x2 = X.clone().requires_grad_(True)
    Y2 = _composed(stack, graph, x2, masks)
    Y2.backward(dY)
    assert_close(outs[1][1], Y2.detach(), 1e-5, "replayed h*")
    assert_close(outs[1][2], x2.grad, 1e-5, "replayed dX")
