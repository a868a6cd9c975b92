"""DropEdge on the GPU: the plan sir_plan_drop_edges derives from a parent plan is, field for field and bit
for bit, the plan of the compacted COO built two independent ways — the native builder
(GraphPlan(src[keep], dst[keep], V, 'cuda', chunk)) and the host build_row_csr — and the layers that run
on the child compute what they compute on a fresh graph of the surviving edges."""
import pytest
import torch
from torch import nn

import sirgcn
from sirgcn import DropEdge, Graph, GraphPlan, SIRConv, SIREConv, _native, drop_edge_keep, get_plan
from sirgcn import dropedge
from sirgcn.graph import build_plans_native
from sirgcn.stacks import SIRStack

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CSR_FIELDS = ("rowptr", "col", "eid", "items")
COUNTS = ("n_rows", "n_items", "n_splits", "n_slots", "max_degree")


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")


def _same_csr(a, b, what):
    for f in COUNTS:
        assert getattr(a, f) == getattr(b, f), (what, f, getattr(a, f), getattr(b, f))
    for f in CSR_FIELDS:
        x, y = getattr(a, f).cpu(), getattr(b, f).cpu()
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, f)
    assert (a.splits is None) == (b.splits is None), (what, "splits")
    if a.splits is not None:
        assert torch.equal(a.splits.cpu(), b.splits.cpu()), (what, "splits")
    assert (a.perm is None) == (b.perm is None), (what, "perm")
    if a.perm is not None:
        assert a.perm.dtype == b.perm.dtype and torch.equal(a.perm.cpu(), b.perm.cpu()), (what, "perm")


def _same_plan(child, src, dst, V, keep, kept, chunk, what=""):
    """child (a derived GraphPlan) against the two builds of the compacted COO; kept against nonzero(keep)."""
    keep = keep.cpu().bool()
    want = torch.nonzero(keep).flatten()
    assert kept.dtype == torch.int64 and torch.equal(kept.cpu(), want), (what, "kept")
    s2, d2 = src[keep], dst[keep]
    assert child.num_edges == int(want.numel()) and child.num_nodes == V
    native = GraphPlan(s2, d2, V, DEV, chunk)
    host = GraphPlan(s2, d2, V, "cpu", chunk)
    for ref, name in ((native, "native"), (host, "host")):
        _same_csr(child.dst, ref.dst, f"{what} dst vs {name}")
        _same_csr(child.src, ref.src, f"{what} src vs {name}")
        assert torch.equal(child.in_deg.cpu(), ref.in_deg.cpu()) and torch.equal(child.out_deg.cpu(), ref.out_deg.cpu())
    for x, y in zip(child.norms("sym"), native.norms("sym")):
        assert torch.equal(x, y), (what, "norms")
    assert torch.equal(child.in_degree_f(), native.in_degree_f()), (what, "in_degree_f")


def _derive(src, dst, V, chunk, keep=None, drop=None):
    parent = GraphPlan(src, dst, V, DEV, chunk)
    k8 = None if keep is None else keep.to(DEV).to(torch.uint8).contiguous()
    child, kept = dropedge.derive_plan(parent, chunk, keep=k8, drop=drop)
    return parent, child, kept


def _multigraph(V=64, E=512, seed=0):
    """The goldens' multigraph family: isolated nodes at the end of the id range, self-loops, duplicate
    edges and one hub row."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, V - 6, (E,), generator=gen)
    dst = torch.randint(0, V - 6, (E,), generator=gen)
    dst[:16] = src[:16]                                  # self-loops
    src[48:80], dst[48:80] = src[16:48].clone(), dst[16:48].clone()     # duplicates
    dst[100:200] = 5                                     # the hub
    return src, dst


def _hub(V, deg, extra, seed=1):
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, V, (deg + extra,), generator=gen)
    dst = torch.cat([torch.full((deg,), 3), torch.randint(0, V, (extra,), generator=gen)])
    order = torch.randperm(deg + extra, generator=gen)   # the hub's edges spread over the id range
    return src[order], dst[order]


def _masks(src, dst, V, chunk):
    E = src.numel()
    host = GraphPlan(src, dst, V, "cpu", chunk)
    ones = torch.ones(E, dtype=torch.bool)
    out = {"all": ones, "none": ~ones, "hub row": dst != 5, "every second": torch.arange(E) % 2 == 0}
    for name, e in (("id 0", 0), ("id E-1", E - 1), ("last position", int(host.dst.eid[-1]))):
        out[name] = ones.clone()
        out[name][e] = False
    return out


@pytest.mark.parametrize("chunk", [4, 256])
def test_explicit_masks_on_the_multigraph(chunk):
    _gpu()
    V = 64
    src, dst = _multigraph(V)
    for name, keep in _masks(src, dst, V, chunk).items():
        parent, child, kept = _derive(src, dst, V, chunk, keep=keep)
        _same_plan(child, src, dst, V, keep, kept, chunk, f"chunk {chunk} mask {name}")
        if name == "all":                               # the parent's plan, bit for bit
            _same_csr(child.dst, parent.dst, "keep-all dst")
            _same_csr(child.src, parent.src, "keep-all src")
        if name == "none":
            assert child.num_edges == 0 and child.dst.n_items == V and child.dst.splits is None
            assert child.dst.max_degree == 0 and child.src.max_degree == 0 and child.src.n_items == V
            assert torch.equal(child.dst.items[:, 0].cpu(), torch.arange(V, dtype=torch.int32))


@pytest.mark.parametrize("chunk", [4, 256])
@pytest.mark.parametrize("p", [0.05, 0.5, 1.0])
def test_hash_masks_and_their_bits(chunk, p):
    """drop = (seed, p): the plan of the hash mask; the device's kept ids equal the host restatement's and
    the rows sir_dropout_apply keeps in column 0."""
    _gpu()
    V, seed = 64, 2 ** 40 + 7
    src, dst = _multigraph(V)
    E = src.numel()
    keep = drop_edge_keep(seed, E, p)
    _, child, kept = _derive(src, dst, V, chunk, drop=(seed, p))
    _same_plan(child, src, dst, V, keep, kept, chunk, f"hash p {p}")
    block = _native.dropout_apply(torch.ones(E, 4, device=DEV), (seed, p))
    assert torch.equal(kept, torch.nonzero(block[:, 0]).flatten())
    assert torch.equal(kept.cpu(), torch.nonzero(drop_edge_keep(seed, E, p, "cpu")).flatten())


def test_a_split_row_becomes_unsplit():
    _gpu()
    V, chunk = 40, 256
    src, dst = _hub(V, 300, 100)
    keep = torch.ones(400, dtype=torch.bool)
    keep[torch.nonzero(dst == 3).flatten()[::3]] = False          # the hub keeps 200 of 300
    parent, child, kept = _derive(src, dst, V, chunk, keep=keep)
    assert parent.dst.n_splits >= 1 and parent.dst.n_slots >= 2
    _same_plan(child, src, dst, V, keep, kept, chunk, "hub 300 -> 200")
    assert int((dst[keep] == 3).sum()) < 256


def test_a_split_row_stays_split_with_fewer_slots():
    _gpu()
    V, chunk = 40, 256
    src, dst = _hub(V, 700, 100)
    keep = torch.ones(800, dtype=torch.bool)
    keep[torch.nonzero(dst == 3).flatten()[::2]] = False          # 700 -> 350: three slots -> two
    parent, child, kept = _derive(src, dst, V, chunk, keep=keep)
    _same_plan(child, src, dst, V, keep, kept, chunk, "hub 700 -> 350")
    hub = [s for s in child.dst.splits.cpu().tolist() if s[0] == 3]
    assert hub and hub[0][2] == 2 and [s[2] for s in parent.dst.splits.cpu().tolist() if s[0] == 3] == [3]


@pytest.mark.parametrize("E", [0, 1, 255, 256, 257, 1025, 70001])
def test_scan_tile_and_block_boundaries(E):
    _gpu()
    V, chunk, seed = 37, 256, 99
    gen = torch.Generator().manual_seed(E)
    src, dst = torch.randint(0, V, (E,), generator=gen), torch.randint(0, V - 2, (E,), generator=gen)
    for keep, drop in ((torch.arange(E) % 3 != 1, None), (drop_edge_keep(seed, E, 0.5), (seed, 0.5))):
        _, child, kept = _derive(src, dst, V, chunk, keep=None if drop else keep, drop=drop)
        _same_plan(child, src, dst, V, keep, kept, chunk, f"E {E}")


def test_no_nodes():
    _gpu()
    g = Graph(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 0, [])
    child = sirgcn.drop_edges(g, torch.zeros(0, dtype=torch.bool), device=DEV)
    plan = get_plan(child, DEV)
    assert plan.num_nodes == 0 and plan.num_edges == 0 and plan.dst.n_items == 0 and plan.dst.rowptr.tolist() == [0]
    assert plan.src.rowptr.tolist() == [0] and child.num_edges() == 0


def test_rectangular_through_the_native_binding():
    _gpu()
    n_dst, n_src, E, chunk = 19, 53, 900, 16
    gen = torch.Generator().manual_seed(4)
    src = torch.randint(0, n_src, (E,), generator=gen).to(DEV)
    dst = torch.randint(0, n_dst - 3, (E,), generator=gen).to(DEV)
    d, s = build_plans_native(src, dst, n_dst, n_src, chunk)
    keep = (torch.arange(E) % 5 != 0).to(DEV)
    pd, ps, perm, kept, counts = _native.plan_drop_edges(d, s, chunk, keep=keep.to(torch.uint8))
    cnt = counts.cpu().tolist()
    E2 = cnt[8]
    assert E2 == int(keep.sum()) and torch.equal(kept[:E2], torch.nonzero(keep).flatten())
    rd, rs = build_plans_native(src[keep], dst[keep], n_dst, n_src, chunk)
    _same_csr(dropedge._csr(pd, n_dst, cnt[0:4], E2), rd, "rectangular dst")
    _same_csr(dropedge._csr(ps, n_src, cnt[4:8], E2, perm), rs, "rectangular src")


def _planned_cuda_graph(V=64, batch=None):
    src, dst = _multigraph(V)
    g = Graph(src, dst, V, batch).to(DEV)
    get_plan(g, DEV)
    return g


def _no_rebuild(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the plan was rebuilt")
    monkeypatch.setattr(_native, "csr_build", boom)
    monkeypatch.setattr(_native, "csr_perm", boom)


def test_no_rebuild(monkeypatch):
    _gpu()
    g = _planned_cuda_graph()
    _no_rebuild(monkeypatch)
    torch.manual_seed(3)
    de = DropEdge(0.3)
    child = de(g)
    assert isinstance(child, Graph) and child.device.type == "cuda" and 0 < child.num_edges() < g.num_edges()
    assert de.last_kept.device.type == "cuda" and de.last_kept.numel() == child.num_edges()
    src, dst = g.edges()
    assert torch.equal(child.edges()[0], src[de.last_kept]) and torch.equal(child.edges()[1], dst[de.last_kept])
    assert torch.equal(de.last_kept.cpu(), torch.nonzero(drop_edge_keep(de.last_seed, g.num_edges(), 0.3)).flatten())
    assert get_plan(child, DEV) is get_plan(child, DEV)
    m = SIRConv(16, 32, 16, nn.ReLU(), 0).to(DEV)
    X = torch.randn(64, 16, device=DEV, requires_grad=True)
    m(child, X).sum().backward()
    assert X.grad is not None and torch.isfinite(X.grad).all()
    # p = 0: the same object, the parent's cached plan keeps serving
    assert DropEdge(0)(g) is g


def _step(m, graph, X, *extra):
    m.zero_grad()
    Xd = X.clone().requires_grad_(True)
    Y = m(graph, Xd, *extra)
    Y.backward(torch.ones_like(Y) * 0.5)
    return [Y.detach(), Xd.grad] + [p.grad.clone() for p in m.parameters()]


def _equal_steps(a, b, what):
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, j)


@pytest.mark.parametrize("agg", ["sum", "sym", "max"])
def test_sirconv_on_the_child_equals_the_fresh_graph(agg, monkeypatch):
    _gpu()
    g = _planned_cuda_graph()
    torch.manual_seed(7)
    m = SIRConv(16, 32, 16, nn.ReLU(), 0, agg_type=agg).to(DEV)
    X = torch.randn(64, 16, device=DEV)
    de = DropEdge(0.3)
    child = de(g)
    src, dst = g.edges()
    fresh = Graph(src[de.last_kept].cpu(), dst[de.last_kept].cpu(), 64)
    ref = _step(m, fresh, X)
    _no_rebuild(monkeypatch)
    _equal_steps(_step(m, child, X), ref, agg)


@pytest.mark.parametrize("form", ["stream", "table"])
def test_sireconv_on_the_child_equals_the_fresh_graph(form):
    _gpu()
    g = _planned_cuda_graph()
    E, de_, H = g.num_edges(), 8, 32
    torch.manual_seed(8)
    m = SIREConv(16, de_, H, 16, nn.ReLU(), 0).to(DEV)
    if form == "table":
        m.linear_edge = nn.Embedding(5, H).to(DEV)
        ef = torch.randint(0, 5, (E,), device=DEV)
    else:
        ef = torch.randn(E, de_, device=DEV)
    X = torch.randn(64, 16, device=DEV)
    drop = DropEdge(0.3)
    child, ef_ = drop(g, ef)
    assert torch.equal(ef_, ef[drop.last_kept]) and ef_.shape[0] == child.num_edges()
    src, dst = g.edges()
    fresh = Graph(src[drop.last_kept].cpu(), dst[drop.last_kept].cpu(), 64)
    _equal_steps(_step(m, child, X, ef_), _step(m, fresh, X, ef[drop.last_kept]), form)


def test_label_spreading_on_the_child():
    _gpu()
    g = _planned_cuda_graph()
    drop = DropEdge(0.3)
    child = drop(g)
    src, dst = g.edges()
    fresh = Graph(src[drop.last_kept].cpu(), dst[drop.last_kept].cpu(), 64)
    y0 = torch.rand(64, 5, device=DEV)
    for use_sym in (True, False):
        assert torch.equal(sirgcn.label_spreading(child, y0, 3, 0.2, use_sym),
                           sirgcn.label_spreading(fresh, y0, 3, 0.2, use_sym))


def test_stack_equals_the_hand_loop():
    """SIRStack(edge_dropout): one DropEdge per layer in layer order — the conv on the dropped graph, the
    norm on the original — under the same torch.manual_seed as a hand loop."""
    _gpu()
    g = _planned_cuda_graph(batch=[20, 30, 14])
    torch.manual_seed(2)
    act = nn.ReLU()
    stack = SIRStack(SIRConv, 32, 3, act, "sum", "zinc", norm_cls=sirgcn.GraphNorm, edge_dropout=0.3).to(DEV)
    assert stack.edge_drop.p == 0.3
    X = torch.randn(64, 32, device=DEV)
    for train in (True, False):                         # DropEdge drops in eval mode too
        stack.train(train)
        torch.manual_seed(21)
        got = stack(g, X)
        kept_last = stack.edge_drop.last_kept
        torch.manual_seed(21)
        h, de = X, DropEdge(0.3)
        for conv, norm in zip(stack.convs, stack.norms):
            y = conv(de(g), h) + h
            out = norm.forward_act(g, y, act, None)
            h = out if out is not None else act(norm(g, y))
        assert torch.equal(got, h) and torch.equal(kept_last, de.last_kept)
        assert kept_last.numel() < g.num_edges()


def test_drop_all():
    _gpu()
    g = _planned_cuda_graph()
    child = DropEdge(1)(g)
    assert child.num_edges() == 0 and get_plan(child, DEV).dst.max_degree == 0
    X = torch.randn(64, 16, device=DEV)
    torch.manual_seed(1)
    m = SIRConv(16, 32, 16, nn.ReLU(), 0, agg_type="sum").to(DEV)
    assert torch.equal(m(child, X), m.linear_relation.bias.detach().expand(64, 16))
    mx = SIRConv(16, 32, 16, nn.ReLU(), 0, agg_type="max").to(DEV)
    assert torch.equal(mx(child, X), torch.zeros(64, 16, device=DEV))


def test_functional_form_on_a_host_graph():
    """drop_edges(graph, keep, efeats, device): a host graph planned on the GPU; the parent plan is built on
    first use and the child's is pre-filled under the key get_plan looks up."""
    _gpu()
    src, dst = _multigraph(64)
    g = Graph(src, dst, 64, [40, 24])
    keep = torch.arange(512) % 4 != 2
    ef = torch.randn(512, 3, device=DEV)
    child, ef_ = sirgcn.drop_edges(g, keep, ef, device="cuda", chunk=4)
    assert torch.equal(ef_, ef[keep.to(DEV)]) and torch.equal(child.batch_num_nodes(), g.batch_num_nodes())
    plan = child._plans[(DEV, 4)]
    assert get_plan(child, DEV, 4) is plan
    _same_plan(plan, src, dst, 64, keep, torch.nonzero(keep).flatten(), 4, "functional")
