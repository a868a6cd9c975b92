"""sirgcn.param_norms / sirgcn.regularizer on the MI355X (sir_param_norms_fwd / _bwd), lists of
tests/paramnorm_cases.py:

1. exact forward: values whose sums are exact in every order -> torch.equal to the fp64 sum, every list and view;
2. N(0, 1) values: |ours - fp64| <= 64 * 2^-24 * fp64, the design's cap on the chain of roundings (the terms are
   non-negative, so the bound is relative);
3. gradients torch.equal to autograd through the torch composition on the same device and to the explicit
   expression fl(g1 sgn p) + fl(g2 fl(2 p)), with +-0 elements, a frozen tensor and an unused output;
4. with a model loss: .grad after (loss + penalty).backward() is g_model + g_penalty added once;
5. determinism, a non-default stream;  6. a captured step replays on changed parameters;
7. poison: NaN in the workspace, around every view and in the gaps of the gradient buffer; NaN / +-Inf
   parameters give the class the composition gives; guard words around the workspace stay;
8. routes: the native route for the above, the composition for bf16 / non-contiguous / CPU tensors."""
import ctypes
import types

import pytest
import torch
from torch import nn

import sirgcn
from sirgcn import _native, regularize

import paramnorm_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G1, G2 = 0.3, 0.7                       # not dyadic: every product rounds


def _list(name, kind):
    specs = pc.lists()[name]
    vals, ref = pc.values(name, kind)
    ps, bases = pc.materialise(specs, vals, DEV)
    return specs, ps, bases, ref


def _gs():
    return torch.tensor(G1, device=DEV), torch.tensor(G2, device=DEV)


def _native_norms(ps):
    out = sirgcn.param_norms(ps)
    assert sirgcn.param_norms.last_route == "native"
    return out


# ------------------------------------------------------------------ 1. exact forward
@pytest.mark.parametrize("name", pc.list_names())
def test_exact_forward_equals_fp64_sum(name):
    _, ps, _, (r1, r2) = _list(name, "exact")
    l1, l2 = _native_norms(ps)
    assert l1.dim() == 0 and l2.dim() == 0 and l1.dtype is torch.float32 and l1.device.type == "cuda"
    want1, want2 = torch.tensor(r1, dtype=torch.float64), torch.tensor(r2, dtype=torch.float64)
    assert float(want1.float()) == r1 and float(want2.float()) == r2          # the fp64 sums are fp32 numbers
    print(f"{name}: l1 {l1.item()!r} (fp64 {r1!r})  l2 {l2.item()!r} (fp64 {r2!r})")
    assert torch.equal(l1.cpu().double(), want1) and torch.equal(l2.cpu().double(), want2)


# ------------------------------------------------------------------ 2. the chain cap
@pytest.mark.parametrize("name", pc.list_names())
def test_normal_values_within_the_chain_cap(name):
    _, ps, _, (r1, r2) = _list(name, "normal")
    l1, l2 = _native_norms(ps)
    for what, got, t64 in (("l1", float(l1.double()), r1), ("l2", float(l2.double()), r2)):
        bound = 64 * 2.0 ** -24 * t64
        print(f"{name} {what}: |ours - fp64| = {abs(got - t64):.3e}, bound {bound:.3e}")
        assert abs(got - t64) <= bound, (name, what)


# ------------------------------------------------------------------ 3. gradients
def _explicit(p, g1, g2):
    s = torch.sign(p)
    if g1 is not None and g2 is not None:
        return g1 * s + g2 * (2 * p)
    return g1 * s if g2 is None else g2 * (2 * p)


@pytest.mark.parametrize("name", ["sizes", "views", "mixed", f"len{pc.list_lengths()[-1]}", "len1"])
def test_gradient_equals_autograd_of_the_composition(name):
    specs, ps, _, _ = _list(name, "normal")
    _, qs, _, _ = _list(name, "normal")
    with torch.no_grad():                                # +-0 elements: sgn = 0
        for t in ps + qs:
            if t.numel() >= 3:
                t[0], t[t.numel() // 2] = 0.0, -0.0
    live = [i for i, (_, _, frozen) in enumerate(specs) if not frozen]
    g1, g2 = _gs()
    for outs in ((g1, g2), (g1, None), (None, g2)):
        l = _native_norms(ps)
        r = pc.composition(qs)
        pick = [i for i in (0, 1) if outs[i] is not None]
        ga = torch.autograd.grad([l[i] for i in pick], [ps[i] for i in live], [outs[i] for i in pick])
        gb = torch.autograd.grad([r[i] for i in pick], [qs[i] for i in live], [outs[i] for i in pick])
        for i, a, b in zip(live, ga, gb):
            assert a.shape == ps[i].shape
            assert torch.equal(a, b), (name, i, outs)
            assert torch.equal(a, _explicit(ps[i].detach(), *outs)), (name, i)
    # one combined scalar gradient, through .backward(): the frozen tensor keeps no gradient
    l = _native_norms(ps)
    (G1 * l[0] + G2 * l[1]).backward()
    rl = pc.composition(qs)
    (G1 * rl[0] + G2 * rl[1]).backward()
    for i, (a, b) in enumerate(zip(ps, qs)):
        if i in live:
            assert torch.equal(a.grad, b.grad), (name, i)
        else:
            assert a.grad is None and b.grad is None


# ------------------------------------------------------------------ 4. with a model loss
@pytest.mark.parametrize("grad_present", [False, True])
def test_penalty_adds_once_to_the_model_gradient(grad_present):
    torch.manual_seed(7)
    m = nn.Sequential(nn.Linear(33, 17), nn.Tanh(), nn.Linear(17, 3)).to(DEV)
    x = torch.randn(19, 33, device=DEV)
    args = types.SimpleNamespace(l1=1e-3, l2=1e-2)
    ps = list(m.parameters())
    g_model = torch.autograd.grad(m(x).square().mean(), ps)
    g_pen = torch.autograd.grad(sirgcn.regularizer(m, args), ps)
    assert sirgcn.param_norms.last_route == "native"
    before = [torch.full_like(p, 0.5) for p in ps] if grad_present else None
    for i, p in enumerate(ps):
        p.grad = before[i].clone() if grad_present else None
    (m(x).square().mean() + sirgcn.regularizer(m, args)).backward()
    for i, p in enumerate(ps):
        want = g_model[i] + g_pen[i]
        if grad_present:
            want = before[i] + want
        assert torch.equal(p.grad, want), i


# ------------------------------------------------------------------ 5. determinism
def test_two_calls_and_a_side_stream_give_equal_bits():
    _, ps, _, _ = _list("mixed", "normal")
    live = [p for p in ps if p.requires_grad]

    def run():
        l = _native_norms(ps)
        return [l[0], l[1]] + list(torch.autograd.grad(l, live, _gs()))

    a, b = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


# ------------------------------------------------------------------ 6. captured step
def test_captured_step_replays_on_changed_parameters():
    specs, ps, _, _ = _list("mixed", "normal")
    live = [p for p in ps if p.requires_grad]
    g1, g2 = _gs()

    def step():
        l = _native_norms(ps)
        return [l[0], l[1]] + list(torch.autograd.grad(l, live, (g1, g2)))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    gen = torch.Generator().manual_seed(99)
    with torch.no_grad():
        for p in ps:                                   # changed in place: the addresses stay
            p.copy_(torch.randn(p.shape, generator=gen).to(DEV))
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    want = step()
    for a, b in zip(outs, want):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 7. poison
def _raw_fwd(ps, fill):
    """sir_param_norms_fwd on a caller-made workspace pre-filled with ``fill`` between guard words."""
    plan = regularize._plan(ps)
    guard = 4
    big = torch.full((guard + plan.work_floats + guard,), fill, device=DEV)
    big[:guard] = 12345.0
    big[-guard:] = 54321.0
    out2 = torch.full((2,), fill, device=DEV)
    _native.param_norms_fwd(plan.params_arr, plan.numel_arr, plan.T, big[guard:guard + plan.work_floats], out2)
    torch.cuda.synchronize()
    assert bool((big[:guard] == 12345.0).all()) and bool((big[-guard:] == 54321.0).all())
    return out2


@pytest.mark.parametrize("name", ["mixed", "views", "sizes"])
def test_poisoned_workspace_and_surroundings_change_nothing(name):
    specs = pc.lists()[name]
    vals, _ = pc.values(name, "normal")
    clean, _ = pc.materialise(specs, vals, DEV, poison=0.0)
    dirty, bases = pc.materialise(specs, vals, DEV, poison=float("nan"))
    want = _raw_fwd(clean, 0.0)
    got = _raw_fwd(dirty, float("nan"))
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    l = _native_norms(dirty)
    assert torch.equal(torch.stack(l), want)
    # backward into a caller-made buffer: the gaps between the slots and the frozen tensors keep their bits
    plan = regularize._plan(dirty)
    needs = tuple(not f for _, _, f in specs)
    offs, tot = plan.layout(needs)
    g1, g2 = _gs()
    bufs = []
    for ps, fill in ((clean, 0.0), (dirty, float("nan"))):
        p = regularize._plan(ps)
        buf = torch.full((tot + 8,), fill, device=DEV)
        base = buf.data_ptr()
        arr = (ctypes.c_void_p * p.T)(*[None if o is None else base + 4 * o for o in offs])
        _native.param_norms_bwd(p.params_arr, p.numel_arr, arr, p.T, g1, g2, torch.device(DEV))
        bufs.append(buf)
    torch.cuda.synchronize()
    written = torch.zeros(tot + 8, dtype=torch.bool, device=DEV)
    for o, (n, _, _) in zip(offs, specs):
        if o is not None:
            written[o:o + n] = True
    assert torch.equal(bufs[0][written], bufs[1][written])
    assert bool(torch.isnan(bufs[1][~written]).all()) and bool((bufs[0][~written] == 0).all())
    for i, (o, (n, _, _)) in enumerate(zip(offs, specs)):
        if o is not None:
            assert torch.equal(bufs[1][o:o + n], _explicit(dirty[i].detach(), g1, g2)), i
    for b, (n, off, _) in zip(bases, specs):              # nothing around a view was written
        assert bool(torch.isnan(b[:off]).all()) and bool(torch.isnan(b[off + n:]).all())


def _same_class(a, b):
    return (torch.equal(torch.isnan(a), torch.isnan(b))
            and torch.equal(torch.where(torch.isnan(a), 0, a), torch.where(torch.isnan(b), 0, b)))


POISONS = {"nan": (float("nan"),), "+inf": (float("inf"),), "-inf": (float("-inf"),),
           "both": (float("inf"), float("-inf"))}


@pytest.mark.parametrize("where", ["head", "first", "middle", "last"])
@pytest.mark.parametrize("what", list(POISONS))
def test_non_finite_parameters_give_the_compositions_class(what, where):
    CH = pc.consts()[0]
    specs = [(7, 0, False), (2 * CH + 3, 1, False), (5, 0, True), (CH, 0, False)]
    # tensor 1 sits 1 float past a 16-byte boundary: its elements 0..2 are the scalar head of chunk 0
    pos = {"head": 0, "first": CH, "middle": CH + CH // 2, "last": CH - 1}[where]
    gen = torch.Generator().manual_seed(5)
    vals = [torch.randn(n, generator=gen) for n, _, _ in specs]
    for k, v in enumerate(POISONS[what]):
        vals[1][pos + k * (7 if where != "last" else -7)] = v          # the second one a few elements away
    ps, _ = pc.materialise(specs, vals, DEV)
    qs, _ = pc.materialise(specs, vals, DEV)
    live = [0, 1, 3]
    zero = torch.zeros((), device=DEV)
    for grads in (_gs(), (_gs()[0], zero), (_gs()[0], None), (None, _gs()[1])):
        l = _native_norms(ps)
        r = pc.composition(qs)
        for a, b in zip(l, r):
            assert _same_class(a, b), (what, where, float(a), float(b))
        if what == "nan":
            assert bool(torch.isnan(l[0])) and bool(torch.isnan(l[1]))
        else:
            assert float(l[0]) == float("inf") and float(l[1]) == float("inf")
        pick = [i for i in (0, 1) if grads[i] is not None]
        ga = torch.autograd.grad([l[i] for i in pick], [ps[i] for i in live], [grads[i] for i in pick])
        gb = torch.autograd.grad([r[i] for i in pick], [qs[i] for i in live], [grads[i] for i in pick])
        for a, b in zip(ga, gb):
            assert _same_class(a, b), (what, where)
    if what != "nan":                                   # g2 = 0 times an infinite parameter is NaN, as in torch
        l = _native_norms(ps)
        ga = torch.autograd.grad(l, [ps[1]], (_gs()[0], zero))[0]
        assert bool(torch.isnan(ga[pos])) and int(torch.isnan(ga).sum()) == len(POISONS[what])


# ------------------------------------------------------------------ 8. routes
def test_other_tensors_take_the_torch_composition(monkeypatch):
    gen = torch.Generator().manual_seed(8)
    a = torch.randn(40, 6, generator=gen).to(DEV).requires_grad_(True)
    b = torch.randn(9, generator=gen).to(DEV).requires_grad_(True)
    others = {"bf16": torch.randn(12, generator=gen).to(DEV).to(torch.bfloat16).requires_grad_(True),
              "transposed": torch.randn(6, 5, generator=gen).to(DEV).t().requires_grad_(True),
              "cpu": torch.randn(11, generator=gen).requires_grad_(True)}
    assert not others["transposed"].is_contiguous()
    _native_norms([a, b])
    monkeypatch.setattr(_native, "param_norms_fwd", lambda *x, **k: pytest.fail("must not reach the kernels"))
    for what, o in others.items():
        ps = [a, o, b]
        l = sirgcn.param_norms(ps)
        assert sirgcn.param_norms.last_route == "torch", what
        r = pc.composition(ps)
        assert torch.equal(l[0], r[0]) and torch.equal(l[1], r[1]), what
        ga = torch.autograd.grad(l, ps, [torch.tensor(G1, device=DEV).to(l[0].dtype), torch.tensor(G2, device=DEV).to(l[1].dtype)])
        gb = torch.autograd.grad(r, ps, [torch.tensor(G1, device=DEV).to(r[0].dtype), torch.tensor(G2, device=DEV).to(r[1].dtype)])
        for x, y in zip(ga, gb):
            assert torch.equal(x, y), what


def test_no_graph_without_grad_mode_or_trainable_tensors():
    _, ps, _, _ = _list("sizes", "normal")
    with torch.no_grad():
        l1, l2 = _native_norms(ps)
    assert not l1.requires_grad and not l2.requires_grad
    frozen = [p.detach() for p in ps]
    f1, f2 = _native_norms(frozen)
    assert not f1.requires_grad and torch.equal(f1, l1) and torch.equal(f2, l2)
    with torch.autocast("cuda", dtype=torch.bfloat16):     # parameters stay fp32 under autocast
        a1, a2 = _native_norms(ps)
    assert a1.dtype is torch.float32 and torch.equal(a1, l1) and torch.equal(a2, l2)
    e1, e2 = _native_norms([torch.empty(0, device=DEV), torch.empty(0, 3, device=DEV)])
    assert float(e1) == 0.0 and float(e2) == 0.0


def test_exported():
    for name in ("param_norms", "regularizer"):
        assert hasattr(sirgcn, name) and name in sirgcn.__all__
