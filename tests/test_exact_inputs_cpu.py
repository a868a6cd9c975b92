"""CPU self-check of the exact-arithmetic inputs (tests/exact_cases.py): the precondition under which
tests/test_exact_gpu.py may compare the kernels with ``torch.equal``.  For every (graph, agg, act) the GPU
tests use: the oracle in fp32 equals the oracle in fp64 bit for bit (so no summation order can matter), every
fp64 result is an fp32 number, the 16-bit inputs are 16-bit numbers, and the inputs do meet the edges they are
built for — z == 0 on >= 5 % of the (edge, column) pairs, an exact tie for the maximum on >= 25 % of the
(row, output) pairs.  The floors are conditions on the inputs, not measurements of the kernels."""
import pytest
import torch

import exact_cases as xc
import oracle

Z0_FLOOR = 0.05
TIE_FLOOR = 0.25
GRAPH_AGG = xc.GRAPH_AGG


def _edge_act(Q, K, graph, act):
    """sigma(Q[v] + K[u]) per edge: the per-edge Linear's input."""
    src, dst, _ = xc.GRAPHS[graph]
    return oracle.act_fwd(Q[dst] + K[src], act, xc.SLOPE)


def _same(a32, a64, what):
    assert a32.dtype == torch.float32 and a64.dtype == torch.float64
    assert torch.equal(a32.double(), a64), f"{what}: the fp32 oracle differs from the fp64 oracle"
    assert torch.equal(a64.float().double(), a64), f"{what}: not an fp32 number"
    assert a64.abs().max() < 2 ** 24, what


def test_graphs_are_what_the_cases_need():
    src, dst, V = xc.GRAPHS["A"]
    assert (V, src.numel()) == (27, 3117)
    ind, outd = torch.bincount(dst, minlength=V), torch.bincount(src, minlength=V)
    assert torch.equal(ind, outd)
    want = sum(([d] * n for n, d in xc.BLOCKS_A), []) + [0, 0, 0]
    assert ind.tolist() == want
    assert not torch.equal(dst, dst.sort().values)              # edge id order is not CSR order
    assert bool((src == dst).any())                             # self-loops
    for chunk in (4, 64, 256):                                  # degree == chunk (unsplit) and 4 chunk (split)
        assert chunk in want and 4 * chunk in want
    src, dst, V = xc.GRAPHS["B"]
    ind, outd = torch.bincount(dst, minlength=V), torch.bincount(src, minlength=V)
    assert ind[40:48].tolist() == list(xc.HUB_DEGREES_B) and outd[48:56].tolist() == list(xc.HUB_DEGREES_B)
    assert ind[56:].sum() == 0 and outd[56:].sum() == 0         # isolated nodes
    assert bool((src == dst).any())
    pairs = src * V + dst
    assert pairs.unique().numel() < pairs.numel()               # duplicate edges


def test_graph_c_is_a_degree_ladder():
    """Every row length 0..65 once on each side (tests/test_width_classes_cpu.py ties them to the kernels' chunk
    loops), self-loops, duplicate edges, isolated nodes, edge ids not in CSR order."""
    L = xc.LADDER_C
    src, dst, V = xc.GRAPHS["C"]
    assert (L, V, src.numel()) == (66, 134, 4290)
    ind, outd = torch.bincount(dst, minlength=V), torch.bincount(src, minlength=V)
    assert ind[:L].tolist() == list(range(L)) and outd[L:2 * L].tolist() == list(range(L))
    assert ind[2 * L:].sum() == 0 and outd[2 * L:].sum() == 0   # isolated nodes
    assert bool((src[dst < L] < L).all()) and bool((dst[src >= L] >= L).all())
    assert int((src == dst).sum()) == 65                        # self-loops
    pairs = src * V + dst
    assert pairs.numel() - pairs.unique().numel() == 946        # duplicate edges
    assert not torch.equal(dst, dst.sort().values)
    assert xc.AGGS_OF["C"] == ("sum",)                          # mean and sym are not dyadic on it


def test_graph_c_sums_survive_one_rounding_to_16_bits():
    """max |S| on graph C is 520 at the full width: finite, and an fp32 number, after the 16-bit kernels' one
    rounding of the output."""
    for act in xc.ACT_NAMES:
        S = xc.edge_expected("C", xc.WIDTH, "sum", act)[0]
        assert float(S.abs().max()) == 520.0
        for dt in (torch.bfloat16, torch.float16):
            assert bool(torch.isfinite(S.float().to(dt)).all())


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("graph,agg", GRAPH_AGG)
def test_edge_kernel_inputs(graph, agg, act):
    """At the full width (the narrower cases are column slices of it: the edge kernels never mix columns)."""
    H = xc.WIDTH
    r32, r64 = xc.edge_expected(graph, H, agg, act, torch.float32), xc.edge_expected(graph, H, agg, act)
    for name, a, b in zip(("S", "dQ", "dK"), r32, r64):
        _same(a, b, f"{graph} {agg} {act} {name}")
    Q, K, G, _ = xc.edge_inputs(graph, H)
    for dt in (torch.bfloat16, torch.float16):
        for t in (Q, K, G):
            assert torch.equal(t.to(dt).float(), t)
        if agg == "mean":           # g = G / deg is rounded to the storage type (include/sirconv.h): exact here
            deg = torch.bincount(xc.GRAPHS[graph][1], minlength=Q.shape[0]).clamp(min=1).float()[:, None]
            assert torch.equal((G / deg).to(dt).float(), G / deg)
    for h in xc.EDGE_H + xc.EDGE_H_SCALAR + xc.EDGE_H_UNALIGNED:
        share = float((xc.edge_z(graph, h) == 0).float().mean())
        assert share >= Z0_FLOOR, f"{graph} H={h}: z == 0 on {share:.3f} of the pairs"


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("graph,agg", GRAPH_AGG)
def test_sire_inputs(graph, agg, act):
    """The widest SIREConv case (the narrower ones are column slices of it, but for the table) and a narrow
    one, stream and table form."""
    for H in (1024, 32):
        for table in (None, xc.sire_table(graph, H)):
            r32 = xc.sire_expected(graph, H, agg, act, table, torch.float32)
            r64 = xc.sire_expected(graph, H, agg, act, table)
            for k in r64:
                _same(r32[k], r64[k], f"{graph} H={H} {agg} {act} table={table is not None} {k}")
            eh = None if table is None else table[0][table[1]]
            share = float((xc.edge_z(graph, H, True, eh) == 0).float().mean())
            assert share >= Z0_FLOOR, f"{graph} H={H}: z == 0 on {share:.3f} of the pairs"


@pytest.mark.parametrize("graph,agg", GRAPH_AGG)
@pytest.mark.parametrize("H,F", xc.SEQ_SHAPES)
def test_seq_sigma_inputs(H, F, graph, agg):
    r32, r64 = xc.seq_expected(graph, H, F, agg, torch.float32), xc.seq_expected(graph, H, F, agg)
    for k in r64:
        _same(r32[k], r64[k], f"seq {graph} {agg} H={H} F={F} {k}")


@pytest.mark.parametrize("act1,act2", xc.SEQ_ACT_PAIRS)
@pytest.mark.parametrize("graph,agg", GRAPH_AGG)
@pytest.mark.parametrize("H,F", xc.SEQ_SHAPES)
def test_seq_sigma_inputs_other_activations(H, F, graph, agg, act1, act2):
    """The (act1, act2) pairs of tests/test_activations_gpu.py::test_seq_sigma_kernels_exact_other_activations:
    Identity keeps integers, LeakyReLU(0.25) makes quarters — every result is still an fp32 number."""
    r32 = xc.seq_expected(graph, H, F, agg, torch.float32, act1, act2)
    r64 = xc.seq_expected(graph, H, F, agg, act1=act1, act2=act2)
    for k in r64:
        _same(r32[k], r64[k], f"seq {act1}/{act2} {graph} {agg} H={H} F={F} {k}")


def test_seq_expected_defaults_are_relu_relu():
    """The optional act1 / act2 of xc.seq_expected leave the (ReLU, ReLU) values as they were."""
    a = xc.seq_expected("A", 16, 16, "mean")
    b = xc.seq_expected("A", 16, 16, "mean", act1="relu", act2="relu")
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["S"], xc.seq_expected("A", 16, 16, "mean", act1="identity", act2="relu")["S"])


@pytest.mark.parametrize("graph,agg", GRAPH_AGG)
def test_identity_edge_kernel_inputs(graph, agg):
    """sigma = identity on the edge-kernel inputs, at the full width: sums of integers (mean / sym on graph A:
    divided by powers of two), the same in fp32 and fp64, |S| <= 4 * 2 * 1024.  "identity" is not one of
    xc.ACT_NAMES: that tuple also drives the sign-mask and sigma'(0) cases, which identity has none of."""
    assert "identity" not in xc.ACT_NAMES
    H = xc.WIDTH
    r32 = xc.edge_expected(graph, H, agg, "identity", torch.float32)
    r64 = xc.edge_expected(graph, H, agg, "identity")
    for name, a, b in zip(("S", "dQ", "dK"), r32, r64):
        _same(a, b, f"{graph} {agg} identity {name}")
        assert b.abs().max() <= 8192


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("graph", list(xc.GRAPHS))
@pytest.mark.parametrize("H,O", xc.MAX_SHAPES)
def test_max_inputs(H, O, graph, act):
    r32, r64 = xc.max_expected(graph, H, O, act, torch.float32), xc.max_expected(graph, H, O, act)
    assert torch.equal(r32["arg"], r64["arg"])
    for k in ("Y", "dQ", "dK", "dW", "db"):
        _same(r32[k], r64[k], f"max {graph} {act} H={H} O={O} {k}")
    Q, K = xc.mlp_inputs(graph, H, O)[:2]
    for dt in (torch.bfloat16, torch.float16):                  # the 16-bit forwards read Q, K and round a, W, b
        a = _edge_act(Q, K, graph, act)
        for t in (Q, K, a, *xc.mlp_inputs(graph, H, O)[2:4]):
            assert torch.equal(t.to(dt).float(), t)
    src, dst, _ = xc.GRAPHS[graph]
    assert float((Q[dst] + K[src] == 0).float().mean()) >= Z0_FLOOR
    share = xc.max_tie_share(graph, H, O, act)
    assert share >= TIE_FLOOR, f"max {graph} {act} H={H} O={O}: exact ties on {share:.3f} of the pairs"


@pytest.mark.parametrize("act", xc.ACT_NAMES)
@pytest.mark.parametrize("agg", xc.LAYER_AGGS)
@pytest.mark.parametrize("H,O", xc.LAYER_SHAPES)
def test_layer_inputs(H, O, agg, act):
    """Every output of the layer step is the same in fp32 and fp64, every GEMM operand of the native step is
    reproduced exactly by the split-fp16 pair under the kernels' scale rule, every value is below 2^24."""
    r32, r64 = xc.layer_expected(H, O, agg, act, torch.float32), xc.layer_expected(H, O, agg, act)
    for k in xc.LAYER_OUTPUTS:
        _same(r32[k], r64[k], f"layer {agg} {act} H={H} O={O} {k}")
    for name, t in r64["operands"].items():
        assert torch.equal(t.float().double(), t) and t.abs().max() < 2 ** 24, name
        if name == "G":             # a GEMM result that only the edge kernels read
            continue
        for dim in (0, 1):
            assert xc.split_exact(t, dim), f"layer {agg} {act} H={H} O={O}: operand {name} along dim {dim}"


def test_split_check_rejects_a_wide_operand():
    """split_exact is a real condition: a low part of 12 significant bits does not fit the fp16 lo term."""
    assert xc.split_exact(torch.tensor([[1.0, 4097.0, -3.0]]), 1)
    assert not xc.split_exact(torch.tensor([[1.0 + 2.0 ** -12 + 2.0 ** -23, 4.0]]), 1)


@pytest.mark.parametrize("M", xc.GEMM_M)
def test_small_gemm_inputs(M):
    for K in xc.GEMM_KN:
        for N in xc.GEMM_KN:
            A, W, b = xc.gemm_inputs(M, K, N)
            for t in (A, W):
                assert xc.split_exact(t, 0) and xc.split_exact(t, 1)
                assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.half().float(), t)
            assert (A.double() @ W.double().t() + b.double()).abs().max() < 2 ** 24
