"""CPU self-check of the poison tests (tests/poison_cases.py, tests/test_poison_gpu.py): the helpers do what
they say, the Part B cases keep their caps, and the checking path passes on a correct restatement and FAILS
on three deliberately leaky ones — a checker that cannot fail proves nothing."""
import pytest
import torch

import cpu_edge_backend
import exact_cases as xc
import oracle
import poison_cases as pc

from sirgcn.graph import GraphPlan

_PLANS = {}


def _plan(graph, chunk):
    if (graph, chunk) not in _PLANS:
        src, dst, V = xc.GRAPHS[graph]
        _PLANS[graph, chunk] = GraphPlan(src, dst, V, "cpu", chunk=chunk)
    return _PLANS[graph, chunk]


# ----------------------------------------------------------------------------- the helpers
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("misalign", [0, 1])
def test_embed_round_trips(dtype, misalign):
    """The logical view equals the original, everything else in the allocation is NaN, the leading
    dimension and the base offset are what was asked for."""
    t = xc.ints((5, 12), 4, 1).to(dtype)
    view, buf = pc.embed(t, pad_cols=4, pad_rows=2, misalign=misalign)
    assert torch.equal(view, t) and view.stride() == (16, 1)
    assert (view.data_ptr() - buf.data_ptr()) == (pc.GUARD + misalign) * t.element_size()
    assert buf.data_ptr() % 16 == 0 and (pc.GUARD * t.element_size()) % 16 == 0
    rest = torch.ones(buf.numel(), dtype=torch.bool)
    rest.as_strided((5, 12), (16, 1), pc.GUARD + misalign).fill_(False)
    assert int(rest.sum()) == buf.numel() - 60 and bool(torch.isnan(buf[rest]).all())
    assert not bool(torch.isnan(buf[~rest]).any())


@pytest.mark.parametrize("dtype", list(pc.SENTINEL))
def test_sentinel_comparison_detects_one_bit(dtype):
    """Every single changed bit of one element outside the logical output fails check_outside; the float
    sentinels are quiet NaNs."""
    out = pc.Out((3, 4), dtype, pad_cols=4, pad_rows=1)
    out.check_outside("untouched")
    if dtype.is_floating_point:
        assert bool(torch.isnan(out.buf).all())
    out.view.fill_(1)
    out.check_outside("logical part written")
    out.check_written("logical part written")
    nbits = 8 * out.buf.element_size()
    outside = torch.nonzero(~out.inside).flatten()
    for k, bit in enumerate(range(nbits)):
        o = pc.Out((3, 4), dtype, pad_cols=4, pad_rows=1)
        i = int(outside[k % outside.numel()])
        word = pc.bits(o.buf)
        flip = 1 << bit
        if bit == nbits - 1:
            flip = -(1 << bit)                  # the sign bit of a two's-complement word
        word[i] = int(word[i]) ^ flip
        with pytest.raises(AssertionError):
            o.check_outside(f"bit {bit}")
    o = pc.Out((3, 4), dtype)
    o.view[:2].fill_(1)
    with pytest.raises(AssertionError):
        o.check_written("a row left out")


def test_poisoned_empty_fills_floats_only():
    with pc.poisoned_empty():
        a, b = torch.empty(7), torch.empty((3,), dtype=torch.int32).fill_(5)
        c = torch.empty_like(torch.zeros(2, 2, dtype=torch.float16))
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(c).all()) and bool((b == 5).all())
    assert not bool(torch.isnan(torch.empty(4).fill_(0)).any())         # restored


def test_graphs_have_every_kind_of_unreferenced_node():
    """Isolated, receive-only and send-only nodes exist (graph B), so Q[v] / G[v] / K[u] of rows the result
    does not depend on are poisoned in fact."""
    no_in, no_out = pc.unreferenced("B")
    assert bool((no_in & no_out).any()) and bool((no_in & ~no_out).any()) and bool((~no_in & no_out).any())
    no_in, no_out = pc.unreferenced("A")
    assert bool((no_in & no_out).any())


# ----------------------------------------------------------------------------- Part B caps
@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("site", list(pc.SITES))
def test_edge_cases_keep_their_caps(site, agg, act):
    """Non-finite elements are at most a quarter of each output, every injected class shows in an output,
    the exempt rows of a non-finite z are at most a quarter of the rows — and the documented special values
    hold in the reference: ReLU(-inf) = 0, LeakyReLU(-inf) = -inf, inf - inf = NaN."""
    H = 12
    S, dQ, dK, ex_q, ex_k = pc.edge_case_expected(H, site, agg, act)
    seen = set()
    for name, ref in (("S", S), ("dQ", dQ), ("dK", dK)):
        assert pc.nonfinite_share(ref) <= 0.25, f"{site} {agg} {act} {name}: {pc.nonfinite_share(ref):.2f}"
        seen |= set(pc.classes(ref).unique().tolist())
    assert float(ex_q.float().mean()) <= 0.25 and float(ex_k.float().mean()) <= 0.25
    if site == "G":
        assert not bool(ex_q.any()) and bool(torch.isfinite(S).all()) and {1, 2, 3} <= seen
        # sigma' = 0 with t = inf is a select: 0 (ReLU) or slope * inf (LeakyReLU), never 0 * inf = NaN
        assert not bool(torch.isnan(dQ[:, :2]).any()) and not bool(torch.isnan(dK[:, :2]).any())
    else:
        assert bool(ex_q.any()) and ({1, 2, 3} if act == "leaky" else {1, 2}) <= set(pc.classes(S).unique().tolist())
    if site == "Q":
        for v in (0, 11):
            assert S[v, 1] == (0.0 if act == "relu" else -pc.INF) and S[v, 0] == pc.INF and torch.isnan(S[v, 2])
    if site == "K":         # node 5's +inf and node 6's -inf meet in the rows of the (6, 4) block they both feed
        assert bool(torch.isnan(S[5:11, 3]).any()) == (act == "leaky")
    if site == "Khub":
        assert bool(torch.isnan(S[11:16, 0]).all()) == (act == "leaky")


@pytest.mark.parametrize("kind", ["inf", "nan"])
@pytest.mark.parametrize("graph", ["A", "B"])
def test_max_cases(graph, kind):
    """max_nan_wins equals oracle.max_first_wins wherever no NaN is among the candidates (the all -inf rows
    included: -inf and the first edge), gives NaN and the FIRST NaN's edge otherwise; the cases hold rows
    of every kind and leave most of each output finite."""
    src, dst, V = xc.GRAPHS[graph]
    M = pc.max_messages_case(graph, 12, kind).double()
    Y, arg = pc.max_nan_wins(dst, V, M)
    has_edges = torch.bincount(dst, minlength=V) > 0
    assert bool((arg[has_edges] >= 0).all()) and bool((arg[~has_edges] == -1).all()) and bool((Y[~has_edges] == 0).all())
    assert bool((dst[arg[has_edges]] == torch.nonzero(has_edges)).all()), "arg is an edge of its row"
    if kind == "inf":
        Y0, arg0 = oracle.max_first_wins(dst, V, M)
        assert torch.equal(Y, Y0) and torch.equal(arg, arg0)
        assert bool((Y == -pc.INF).any()) and bool((Y == pc.INF).any())
    else:
        nan = torch.isnan(Y)
        assert bool(nan.any())
        r, f = torch.nonzero(nan, as_tuple=True)
        first = torch.full((V, 12), M.shape[0], dtype=torch.int64)
        e, ff = torch.nonzero(torch.isnan(M), as_tuple=True)
        for ei, fi in zip(e.tolist(), ff.tolist()):
            first[dst[ei], fi] = min(int(first[dst[ei], fi]), ei)
        assert torch.equal(arg[r, f], first[r, f])
        assert bool((torch.isnan(M).any(0)).any())
    assert pc.nonfinite_share(Y) <= 0.25 and bool(torch.isfinite(Y).any(1).all())


# ----------------------------------------------------------------------------- the checking path
class _Leaky:
    """cpu_edge_backend with one deliberate fault in the forward."""

    def __init__(self, fault):
        self.fault = fault

    def edge_agg_fwd(self, csr, Q, K, norm_row, norm_col, agg, act, slope, S, partial, mask_out=None):
        V, H = S.shape
        if self.fault == "skip row":
            keep = S[3].clone()
        cpu_edge_backend.edge_agg_fwd(csr, Q, K, norm_row, norm_col, agg, act, slope, S, partial, None)
        if self.fault == "pad times zero":         # a tail lane that multiplies what it loaded past H by 0
            wide = Q.as_strided((V, H + 1), Q.stride(), Q.storage_offset())
            S += (wide[:, H:] * 0.0)
        elif self.fault == "one past N":            # a store that spills into the row's padding
            S.as_strided((V, H + 1), S.stride(), S.storage_offset())[V - 1, H] = 0.0
        elif self.fault == "skip row":
            S[3] = keep
        elif self.fault == "unreferenced row":      # Q[v] of a row without edges used
            S += Q * 0.0
        elif self.fault == "workspace tail":
            partial.as_strided((partial.numel() + 1,), (1,), partial.storage_offset())[-1] = 0.0


@pytest.mark.parametrize("chunk", [4, 256])
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
def test_checking_path_passes_on_the_cpu_restatement(agg, chunk):
    """embed -> call -> the three assertions with tests/cpu_edge_backend.py in the kernel's place."""
    for graph in ("A", "B") if agg == "sum" else ("A",):
        for H, pad, mis in ((12, 4, 0), (3, 3, 1)):
            pc.check_edge_forward(cpu_edge_backend, _plan(graph, chunk), graph, H, agg, "leaky", pad_cols=pad,
                                  misalign=mis)


@pytest.mark.parametrize("fault", ["pad times zero", "one past N", "skip row", "unreferenced row", "workspace tail"])
def test_checking_path_fails_on_a_leaky_restatement(fault):
    with pytest.raises(AssertionError):
        pc.check_edge_forward(_Leaky(fault), _plan("B", 4), "B", 12, "sum", "relu")


@pytest.mark.parametrize("site", list(pc.SITES))
@pytest.mark.parametrize("H", [7, 256])
def test_edge_cases_keep_their_caps_at_the_other_widths(H, site):
    """The caps of the widths the GPU test also runs (the sites sit in columns 0 - 4)."""
    for agg in ("sum", "mean", "sym"):
        S, dQ, dK, ex_q, ex_k = pc.edge_case_expected(H, site, agg, "leaky")
        assert max(pc.nonfinite_share(t) for t in (S, dQ, dK)) <= 0.25
        assert float(ex_q.float().mean()) <= 0.25 and float(ex_k.float().mean()) <= 0.25


@pytest.mark.parametrize("graph", ["A", "B"])
@pytest.mark.parametrize("H,O", [(64, 64), (100, 200), (256, 40)])
def test_mlp_cases_keep_their_caps(H, O, graph):
    """The fused edge-MLP cases: at most a quarter of the rows see a NaN of Q / K, the bias columns hold each
    class in every row with edges, every row with edges has an arg edge of its own; the sum-family case marks
    whole rows only; the bias case's backward expectation is finite."""
    src, dst, V = xc.GRAPHS[graph]
    has = torch.bincount(dst, minlength=V) > 0
    for act in xc.ACT_NAMES:
        _, _, _, _, Y, arg = pc.mlp_max_case(graph, H, O, act)
        clean = has & torch.isfinite(Y[:, 3:]).all(1)
        assert pc.rows_share(Y[:, 3:]) <= 0.25 and bool(torch.isnan(Y[:, 3:]).all(1).any()) and bool(clean.any())
        assert bool((Y[clean][:, 0] == -pc.INF).all()) and bool((Y[clean][:, 1] == pc.INF).all())
        assert bool(torch.isnan(Y[has][:, 2]).all()) and bool((arg[has] >= 0).all()) and bool((arg[~has] == -1).all())
        assert bool((dst[arg[has]] == torch.nonzero(has)).all())
        *_, warg, want = pc.max_bias_case(graph, H, O, act)
        assert all(bool(torch.isfinite(t).all()) for t in want.values())
        first = torch.full((V,), src.numel()).scatter_reduce(0, dst, torch.arange(src.numel()), reduce="amin")
        assert torch.equal(warg[has][:, :3], first[has][:, None].expand(-1, 3))
    for agg in xc.AGGS_OF[graph]:
        for Hs, Fs in xc.SEQ_SHAPES[:2]:
            S = pc.seq_nan_case(graph, Hs, Fs, agg)[4]
            bad = ~torch.isfinite(S)
            assert 0 < pc.rows_share(S) <= 0.25 and torch.equal(bad, bad.any(1, keepdim=True).expand_as(bad))


@pytest.mark.parametrize("M,K,N", [(513, 256, 40), (33, 100, 260), (513, 128, 260)])
def test_gemm_case_keeps_its_caps(M, K, N):
    """NT marks three whole rows, TN three whole rows and two whole columns, nothing else; every class is there."""
    A, W, b, B = pc.gemm_nonfinite_case(M, K, N)
    ref = A.double() @ W.double().t() + b.double()
    bad = ~torch.isfinite(ref)
    assert int(bad.all(1).sum()) == 3 and torch.equal(bad, bad.all(1)[:, None].expand_as(bad)) and pc.rows_share(ref) <= 0.25
    refT = A.double().t() @ B.double()
    bad = ~torch.isfinite(refT)
    rows, cols = bad.all(1), bad.all(0)
    assert 0 < float(rows.float().mean()) <= 0.25 and 0 < float(cols.float().mean()) <= 0.25
    assert torch.equal(bad, rows[:, None] | cols[None, :]) and {1, 2, 3} <= set(pc.classes(A).unique().tolist())


def test_resid_and_col_sum_cases_keep_their_caps():
    """resid-act: every class shows in the forward reference of both orders and both activations and in the
    gradient, most of each output stays finite; col-sum: a NaN, a +inf and +inf meeting -inf, each in one column."""
    Y, R, D, D2 = pc.resid_case()
    for act in xc.ACT_NAMES:
        for order in (0, 1):
            z = Y.double() + R.double() if order == 0 else Y.double()
            out = oracle.act_fwd(z, act, xc.SLOPE) + (0 if order == 0 else R.double())
            need = {1, 2, 3} if (act == "leaky" or order == 1) else {1, 2}
            assert need <= set(pc.classes(out).unique().tolist()) and pc.nonfinite_share(out) <= 0.25
            assert float((~torch.isfinite(z)).any(1).float().mean()) <= 0.25
            if act == "relu" and order == 0:
                assert out[2, 2] == 0 and torch.isnan(out[3, 3])          # ReLU(-inf) = 0, ReLU(NaN) = NaN
    g = D.double() + D2.double()
    assert {1, 2, 3} <= set(pc.classes(g).unique().tolist()) and pc.nonfinite_share(g) <= 0.25
    for n, m in ((5, 16), (3001, 76)):
        ref = pc.col_sum_case(n, m).double().sum(0)
        assert pc.nonfinite_share(ref) <= 0.25 and torch.isnan(ref[1]) and ref[2] == pc.INF and torch.isnan(ref[3])
