"""GPU parity: the HIP kernels (through the C ABI) against the golden vectors produced by the
reference's own conv.py, against the CPU oracle on random shapes, and against a chunked torch
fp32 GPU reference at BASELINE size.  Run on the MI355X box:  pytest tests -m gpu
Tolerances: indexing bit-exact; fp32 ||d||/||ref|| <= 1e-5 and
allclose(rtol=1e-5, atol=1e-6*max|ref|); unsplit ReLU/LeakyReLU rows bit-exact."""
import numpy as np
import pytest
import torch
from torch import nn

import oracle
import width_cases as wc
from conftest import assert_close, assert_parity, golden_manifest, load_case, rel_err

import sirgcn
from sirgcn import _native
from sirgcn.conv import EdgeAggregate, SIRConv, activation_code
from sirgcn.graph import Graph, GraphPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [c for c in golden_manifest() if c["agg"] in ("sum", "mean", "sym") and c["act"] in ("relu", "leaky", "gelu")]
ACTS = {"relu": nn.ReLU(), "leaky": nn.LeakyReLU(0.2), "gelu": nn.GELU()}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _t(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def _kernel_run(z, case, chunk):
    V, H = case["V"], case["H"]
    plan = GraphPlan(torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), V, DEV, chunk=chunk)
    QK = torch.cat([_t(z["Q"]), _t(z["K"])], 1).requires_grad_(True)
    act, slope = activation_code(ACTS[case["act"]])
    S = EdgeAggregate.apply(QK, plan, H, case["agg"], act, slope)
    S.backward(_t(z["dS"]))
    torch.cuda.synchronize()
    return plan, S.cpu(), QK.grad[:, :H].cpu(), QK.grad[:, H:].cpu()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_edge_kernels_vs_reference_golden(case):
    z = load_case(case["name"])
    plan, S, dQ, dK = _kernel_run(z, case, chunk=256)
    exact = (case["dtype"] == "float32" and case["act"] in ("relu", "leaky")
             and plan.dst.n_splits == 0 and plan.src.n_splits == 0)
    f32 = lambda k: torch.from_numpy(z[k]).float()
    if exact:
        # unsplit rows accumulate in the reference's (DGL CSC / index_add) order -> identical bits
        assert torch.equal(S, f32("S")), f"S max diff {(S - f32('S')).abs().max()}"
        assert torch.equal(dQ, f32("dQ")), f"dQ max diff {(dQ - f32('dQ')).abs().max()}"
        assert torch.equal(dK, f32("dK")), f"dK max diff {(dK - f32('dK')).abs().max()}"
    else:
        _check_kernel_parity(z, case, S, dQ, dK)


def _truth_kernels(z, case):
    """The reference algorithm evaluated in fp64 by the (pinned) oracle from the fixture's Q, K, dS."""
    d = lambda k: torch.from_numpy(z[k]).double()
    S = oracle.edge_agg_fwd(z["src"], z["dst"], case["V"], d("Q"), d("K"), case["agg"], case["act"], case["slope"])
    dQ, dK = oracle.edge_agg_bwd(z["src"], z["dst"], case["V"], d("Q"), d("K"), d("dS"), case["agg"],
                                 case["act"], case["slope"])
    return S, dQ, dK


def _check_kernel_parity(z, case, S, dQ, dK):
    tS, tQ, tK = _truth_kernels(z, case)
    assert_parity(S, z["S"], tS, 1e-5, f"{case['name']} S")
    assert_parity(dQ, z["dQ"], tQ, 1e-5, f"{case['name']} dQ")
    assert_parity(dK, z["dK"], tK, 1e-5, f"{case['name']} dK")


@pytest.mark.parametrize("case", [c for c in CASES if c["name"].startswith("small") and c["dtype"] == "float32"],
                         ids=lambda c: c["name"])
def test_split_rows_match_reference(case):
    """chunk=4 forces most rows through the partial/combine path."""
    z = load_case(case["name"])
    plan, S, dQ, dK = _kernel_run(z, case, chunk=4)
    assert plan.dst.n_splits > 0 and plan.src.n_splits > 0
    _check_kernel_parity(z, case, S, dQ, dK)


def _load_reference_weights(m, z):
    with torch.no_grad():
        m.linear_query.weight.copy_(_t(z["W_Q"])); m.linear_query.bias.copy_(_t(z["b_Q"]))
        m.linear_key.weight.copy_(_t(z["W_K"]))
        m.linear_relation.weight.copy_(_t(z["W_R"])); m.linear_relation.bias.copy_(_t(z["b_R"]))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "modular"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_sirconv_layer_vs_reference_golden(case, fused):
    z = load_case(case["name"])
    m = SIRConv(case["d"], case["H"], case["O"], ACTS[case["act"]], 0, agg_type=case["agg"]).to(DEV)
    m.use_fused = fused
    _load_reference_weights(m, z)
    g = Graph(torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), case["V"])
    X = _t(z["X"]).requires_grad_(True)
    Y = m(g, X)
    Y.backward(_t(z["dY"]))
    torch.cuda.synchronize()
    got = {"Y": Y, "dX": X.grad, "dW_Q": m.linear_query.weight.grad, "db_Q": m.linear_query.bias.grad,
           "dW_K": m.linear_key.weight.grad, "dW_R": m.linear_relation.weight.grad,
           "db_R": m.linear_relation.bias.grad}
    d = lambda k: torch.from_numpy(z[k]).double()
    truth = oracle.layer_fwd_bwd(z["src"], z["dst"], case["V"], *[d(k) for k in ("X", "W_Q", "b_Q", "W_K", "W_R", "b_R", "dY")],
                                 case["agg"], case["act"], case["slope"])
    for k, v in got.items():      # Y (h*) on the strict 1e-5 bar of the north star
        assert_parity(v.detach().cpu(), z[k], truth[k], 1e-5, f"{case['name']} {k}", strict=(k == "Y"))


def test_state_dict_keys_match_reference_layout():
    m = SIRConv(16, 32, 8, nn.LeakyReLU(0.2), 0, agg_type="sym")
    assert sorted(m.state_dict().keys()) == sorted(
        ["linear_query.weight", "linear_query.bias", "linear_key.weight",
         "linear_relation.weight", "linear_relation.bias"])
    # current-code parameter count 3H^2+2H at d=H=O (SURVEY §6 known-answer note)
    m2 = SIRConv(256, 256, 256, nn.ReLU())
    assert sum(p.numel() for p in m2.parameters()) == 3 * 256 * 256 + 2 * 256


@pytest.mark.parametrize("H", wc.HIDDEN_SIZES)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
def test_hidden_sizes_vs_oracle(H, agg):
    gen = torch.Generator().manual_seed(H * 7 + len(agg))
    V, E = 300, 2500
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(0, V - 20, (E,), generator=gen)
    dst[:400] = 5                                            # a split row at chunk 256
    Q = torch.randn(V, H, generator=gen); K = torch.randn(V, H, generator=gen)
    dS = torch.randn(V, H, generator=gen)
    S_ref = oracle.edge_agg_fwd(src, dst, V, Q, K, agg, "leaky", 0.2)
    dQ_ref, dK_ref = oracle.edge_agg_bwd(src, dst, V, Q, K, dS, agg, "leaky", 0.2)
    S_64 = oracle.edge_agg_fwd(src, dst, V, Q.double(), K.double(), agg, "leaky", 0.2)
    dQ_64, dK_64 = oracle.edge_agg_bwd(src, dst, V, Q.double(), K.double(), dS.double(), agg, "leaky", 0.2)
    plan = GraphPlan(src, dst, V, DEV)
    QK = torch.cat([Q, K], 1).to(DEV).requires_grad_(True)
    S = EdgeAggregate.apply(QK, plan, H, agg, _native.ACT_LEAKY, 0.2)
    S.backward(dS.to(DEV))
    assert_parity(S.detach().cpu(), S_ref, S_64, 1e-5, "S")
    assert_parity(QK.grad[:, :H].cpu(), dQ_ref, dQ_64, 1e-5, "dQ")
    assert_parity(QK.grad[:, H:].cpu(), dK_ref, dK_64, 1e-5, "dK")


def test_unaligned_leading_dimension_takes_scalar_path():
    gen = torch.Generator().manual_seed(3)
    V, E, H = 200, 1500, 64
    src = torch.randint(0, V, (E,), generator=gen); dst = torch.randint(0, V, (E,), generator=gen)
    Q = torch.randn(V, H, generator=gen); K = torch.randn(V, H, generator=gen)
    buf = torch.zeros(V, 2 * H + 1, device=DEV)
    buf[:, :H] = Q.to(DEV); buf[:, H + 1:] = K.to(DEV)
    plan = GraphPlan(src, dst, V, DEV)
    S = torch.empty(V, H, device=DEV)
    _native.edge_agg_fwd(plan.dst, buf[:, :H], buf[:, H + 1:], None, None, "sum", _native.ACT_RELU, 0.0, S, None)
    assert_close(S.cpu(), oracle.edge_agg_fwd(src, dst, V, Q, K, "sum", "relu"), 1e-5, "S")


def test_errors_are_loud():
    g = Graph([0, 1], [1, 0], 2)
    m = SIRConv(8, 16, 4, nn.ReLU())
    with pytest.raises(RuntimeError):
        m(g, torch.randn(2, 8))              # CPU tensor: no CPU fallback
    plan = GraphPlan(torch.tensor([0, 1]), torch.tensor([1, 0]), 2, DEV)
    QK = torch.randn(2, 2 * 257, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported hidden size"):
        _native.edge_agg_fwd(plan.dst, QK[:, :257], QK[:, 257:], None, None, "sum", 1, 0.0,
                             torch.empty(2, 257, device=DEV), None)


def _chunked_torch_reference(src, dst, V, Q, K, dS, agg, slope):
    """torch GPU reference of the same math in Q's dtype, edge-chunked (never the product path)."""
    H = Q.shape[1]
    in_deg = torch.bincount(dst, minlength=V); out_deg = torch.bincount(src, minlength=V)
    in_norm = torch.pow(in_deg.float().clamp(min=1), -0.5); out_norm = torch.pow(out_deg.float().clamp(min=1), -0.5)
    degf = in_deg.clamp(min=1).to(Q.dtype).unsqueeze(1)
    G = dS / degf if agg == "mean" else dS
    S = torch.zeros(V, H, device=Q.device, dtype=Q.dtype); dQ = torch.zeros_like(S); dK = torch.zeros_like(S)
    step = 1 << 20
    for s in range(0, src.numel(), step):
        u, v = src[s:s + step], dst[s:s + step]
        z = Q[v] + K[u]
        m = torch.nn.functional.leaky_relu(z, slope)
        t = G[v]
        if agg == "sym":
            c = (out_norm[u] * in_norm[v]).unsqueeze(1)
            m = c * m; t = t * c
        dz = torch.where(z > 0, t, t * slope)
        S.index_add_(0, v, m); dQ.index_add_(0, v, dz); dK.index_add_(0, u, dz)
    if agg == "mean":
        S = S / degf
    return S, dQ, dK


@pytest.mark.parametrize("agg", ["sum", "sym", "mean"])
def test_full_size_S1_vs_torch_reference_and_deterministic(agg):
    from sirgcn.synth import powerlaw_graph
    g = powerlaw_graph(500_000, 10_000_000, 0.8, seed=0)
    V, H = g.num_nodes(), 256
    gen = torch.Generator(device=DEV).manual_seed(3)
    QK = torch.randn(V, 2 * H, device=DEV, generator=gen)
    dS = torch.randn(V, H, device=DEV, generator=gen)
    plan = GraphPlan(g._src, g._dst, V, DEV)
    assert plan.dst.n_splits > 0                            # hubs are split
    outs = []
    for use_mask in (True, True, False):
        EdgeAggregate.use_mask = use_mask
        try:
            x = QK.clone().requires_grad_(True)
            S = EdgeAggregate.apply(x, plan, H, agg, _native.ACT_LEAKY, 0.2)
            S.backward(dS)
            outs.append((S.detach(), x.grad))
        finally:
            EdgeAggregate.use_mask = True
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "not deterministic"
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1]), "mask != recompute"
    src, dst = g._src.to(DEV), g._dst.to(DEV)
    S, dQK = outs[0]
    ref32 = _chunked_torch_reference(src, dst, V, QK[:, :H], QK[:, H:], dS, agg, 0.2)
    ref64 = _chunked_torch_reference(src, dst, V, QK[:, :H].double(), QK[:, H:].double(), dS.double(), agg, 0.2)
    # per-tensor criterion of assert_parity (the fp32 torch reference's own error sets the floor)
    for got, r32, r64 in ((S, ref32[0], ref64[0]), (dQK[:, :H], ref32[1], ref64[1]), (dQK[:, H:], ref32[2], ref64[2])):
        e = rel_err(got, r64)
        assert e <= max(1e-5, 2 * rel_err(r32, r64)), (e, rel_err(r32, r64))


def test_degree_norms_bit_exact_vs_cpu_pow():
    """sir_degree_norms == CPU torch.pow(clamp(deg, 1).float(), -0.5) (conv.py:51-57) for EVERY
    degree 0..3,000,000 (int32 rowptr: degrees are fed in chunks whose sum fits)."""
    got, ref = [], []
    lo, top = 0, 3_000_001
    while lo < top:
        k = max(1, min(top - lo, (2 ** 31 - 1) // max(lo + 1, 1) - 1, 1 << 16))
        d = torch.arange(lo, lo + k, dtype=torch.int64)
        rp = torch.zeros(k + 1, dtype=torch.int64)
        torch.cumsum(d, 0, out=rp[1:])
        out = torch.empty(k, device=DEV)
        _native.degree_norms(rp.to(torch.int32).to(DEV), None, out, None)
        got.append(out)
        ref.append(torch.pow(d.float().clamp(min=1), -0.5))
        lo += k
    assert torch.equal(torch.cat(got).cpu(), torch.cat(ref))


@pytest.mark.parametrize("case", [c for c in CASES if c["H"] % 4 == 0 and c["act"] in ("relu", "leaky")],
                         ids=lambda c: c["name"])
def test_sign_mask_backward_bit_identical_to_recompute(case):
    z = load_case(case["name"])
    outs = []
    for use_mask in (True, False):
        EdgeAggregate.use_mask = use_mask
        try:
            outs.append(_kernel_run(z, case, chunk=256)[1:])
        finally:
            EdgeAggregate.use_mask = True
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("agg", ["sum", "sym", "mean"])
def test_edge_cut_path_single_rank_equals_single_gpu(agg):
    """sirgcn.dist with world=1 (no halo, exchanges degenerate) against the single-GPU layer
    (collectives: tests/test_dist_gloo.py and test_edge_cut_halo_exchange_on_device)."""
    from sirgcn.dist import DistGraph, DistSIRConv
    from sirgcn.synth import powerlaw_edges
    V, E, H = 3000, 60000, 256
    src, dst = powerlaw_edges(V, E, 0.8, seed=5)
    X = torch.randn(V, H, generator=torch.Generator().manual_seed(1)).to(DEV)
    dY = torch.randn(V, H, generator=torch.Generator().manual_seed(2)).to(DEV)
    torch.manual_seed(3)
    conv = SIRConv(H, H, H, nn.LeakyReLU(0.2), 0, agg_type=agg).to(DEV)
    x1 = X.clone().requires_grad_(True)
    Y1 = conv(Graph(src, dst, V), x1); Y1.backward(dY)
    g1 = {n: p.grad.clone() for n, p in conv.named_parameters()}
    conv.zero_grad(set_to_none=True)
    dg = DistGraph.from_global(src, dst, V, 0, 1, DEV)
    x2 = X.clone().requires_grad_(True)
    Y2 = DistSIRConv(conv)(dg, x2); Y2.backward(dY)
    torch.cuda.synchronize()
    # one packed GEMM vs separate GEMMs -> rounding-level differences: judge both against fp64
    w = [t.detach().cpu().double() for t in (conv.linear_query.weight, conv.linear_query.bias,
                                             conv.linear_key.weight, conv.linear_relation.weight,
                                             conv.linear_relation.bias)]
    truth = oracle.layer_fwd_bwd(src, dst, V, X.cpu().double(), *w, dY.cpu().double(), agg, "leaky", 0.2)
    assert_parity(Y2.detach().cpu(), Y1.detach().cpu(), truth["Y"], 1e-5, "Y")
    assert_parity(x2.grad.cpu(), x1.grad.cpu(), truth["dX"], 1e-5, "dX")
    names = {"linear_query.weight": "dW_Q", "linear_query.bias": "db_Q", "linear_key.weight": "dW_K",
             "linear_relation.weight": "dW_R", "linear_relation.bias": "db_R"}
    for n, p in conv.named_parameters():
        assert_parity(p.grad.cpu(), g1[n].cpu(), truth[names[n]], 1e-5, n)


@pytest.mark.parametrize("world,agg", [(2, "sum"), (3, "sym"), (2, "mean"), (4, "sum")])
def test_edge_cut_halo_exchange_on_device(world, agg):
    """Multi-rank edge-cut on the GPU in one process: one thread per rank, device tensors,
    in-process all-to-all (tests/thread_comm.py).  Exercises the halo plan, the packed sends,
    K_ext kernels, the reverse dK exchange and its deterministic add against the fp64 oracle."""
    from sirgcn.dist import DistGraph, DistSIRConvFunction
    from sirgcn.synth import powerlaw_edges
    from thread_comm import FakeCtx, ThreadComm, run_ranks
    V, E, H = 4000, 80000, 256
    src, dst = powerlaw_edges(V, E, 0.8, seed=6)
    X = torch.randn(V, H, generator=torch.Generator().manual_seed(1)).to(DEV)
    dY = torch.randn(V, H, generator=torch.Generator().manual_seed(2)).to(DEV)
    torch.manual_seed(3)
    conv = SIRConv(H, H, H, nn.LeakyReLU(0.2), 0, agg_type=agg).to(DEV)
    w = [conv.linear_query.weight.detach(), conv.linear_query.bias.detach(), conv.linear_key.weight.detach(),
         conv.linear_relation.weight.detach(), conv.linear_relation.bias.detach()]
    comms = ThreadComm.make(world)
    in_deg = torch.bincount(dst, minlength=V)
    from sirgcn.dist import partition_rows
    bounds = partition_rows(in_deg, world)

    def rank_fn(r):
        dg = DistGraph(src, dst, V, bounds, r, world, DEV, group=comms[r])
        ctx = FakeCtx((True,) * 6 + (False,) * 7)
        x = X[dg.row_begin:dg.row_end]
        with torch.no_grad():
            Y = DistSIRConvFunction.forward(ctx, x, w[0], w[1], w[2], w[3], w[4], dg, agg, _native.ACT_LEAKY, 0.2,
                                            _native, True)
            grads = DistSIRConvFunction.backward(ctx, dY[dg.row_begin:dg.row_end])
        torch.cuda.synchronize()
        return dg.n_halo, Y, grads

    outs = run_ranks(world, rank_fn)
    assert sum(o[0] for o in outs) > 0                     # real halos were exchanged
    Y = torch.cat([o[1] for o in outs]).cpu()
    dX = torch.cat([o[2][0] for o in outs]).cpu()
    gsum = [sum(o[2][i] for o in outs).cpu() for i in range(1, 6)]
    x1 = X.clone().requires_grad_(True)
    Y1 = conv(Graph(src, dst, V), x1)
    Y1.backward(dY)
    wd = [t.cpu().double() for t in w]
    truth = oracle.layer_fwd_bwd(src, dst, V, X.cpu().double(), *wd, dY.cpu().double(), agg, "leaky", 0.2)
    assert_parity(Y, Y1.detach().cpu(), truth["Y"], 1e-5, "Y")
    assert_parity(dX, x1.grad.cpu(), truth["dX"], 1e-5, "dX")
    for g, (name, p), key in zip(gsum, conv.named_parameters(), ("dW_Q", "db_Q", "dW_K", "dW_R", "db_R")):
        assert_parity(g, p.grad.cpu(), truth[key], 1e-5, name)


@pytest.mark.parametrize("n,m", [(0, 8), (1, 4), (1000, 256), (2_000_003, 256), (5000, 512), (777, 1028)])
def test_col_sum_bias_gradient(n, m):
    X = torch.randn(n, m, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n + m))
    got = _native.col_sum(X)
    ref32 = X.sum(0)
    truth = X.double().sum(0)
    assert_parity(got.cpu(), ref32.cpu(), truth.cpu(), 1e-5, "colsum")
    assert torch.equal(got, _native.col_sum(X))          # deterministic
    view = torch.randn(300, 2 * m, device=DEV)[:, :m]    # strided view (the dQ half of dQK)
    assert_parity(_native.col_sum(view).cpu(), view.sum(0).cpu(), view.double().sum(0).cpu(), 1e-5, "colsum view")


# ------------------------------------------------------------------ generic (edge-materialised) path
GENERIC = [c for c in golden_manifest() if c["agg"] == "max" or c["act"] in ("seq", "tanh")]


def _act_module(case, z):
    if case["act"] == "tanh":
        return nn.Tanh()
    if case["act"] == "seq":   # dictionary-lookup/model.py:17
        lin = nn.Linear(case["H"], case["H"])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(z["act_W"])); lin.bias.copy_(torch.from_numpy(z["act_b"]))
        return nn.Sequential(nn.ReLU(inplace=True), lin, nn.ReLU(inplace=True))
    return ACTS[case["act"]]


def _oracle_act(case, z):
    import copy
    if case["act"] in ("tanh", "seq"):
        return copy.deepcopy(_act_module(case, z)).double()
    return case["act"]


@pytest.mark.parametrize("case", GENERIC, ids=[c["name"] for c in GENERIC])
def test_generic_path_vs_reference_golden(case):
    z = load_case(case["name"])
    act = _act_module(case, z).to(DEV)
    m = SIRConv(case["d"], case["H"], case["O"], act, 0, agg_type=case["agg"]).to(DEV)
    _load_reference_weights(m, z)
    g = Graph(torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), case["V"])
    X = _t(z["X"]).requires_grad_(True)
    Y = m(g, X)
    Y.backward(_t(z["dY"]))
    torch.cuda.synchronize()
    d = lambda k: torch.from_numpy(z[k]).double()
    args = [d(k) for k in ("X", "W_Q", "b_Q", "W_K", "W_R", "b_R", "dY")]
    truth = oracle.reference_cpu_step(z["src"], z["dst"], case["V"], *args, case["agg"], _oracle_act(case, z), case["slope"])
    got = {"Y": Y, "dX": X.grad, "dW_Q": m.linear_query.weight.grad, "db_Q": m.linear_query.bias.grad,
           "dW_K": m.linear_key.weight.grad, "dW_R": m.linear_relation.weight.grad,
           "db_R": m.linear_relation.bias.grad}
    ties = case["agg"] == "max" and not case["name"].startswith("nodup")
    if ties:   # DGL semantics (first arg-max) differ from the fixture's tie-splitting: use the oracle
        f = lambda k: torch.from_numpy(z[k])
        ref32 = oracle.reference_cpu_step(z["src"], z["dst"], case["V"], *[f(k) for k in ("X", "W_Q", "b_Q", "W_K", "W_R", "b_R", "dY")],
                                          case["agg"], case["act"], case["slope"])
    for k, v in got.items():
        r = ref32[k] if ties else z[k]
        assert_parity(v.detach().cpu(), r, truth[k], 1e-5, f"{case['name']} {k}")
    if case["act"] == "seq":
        assert_close(act[1].weight.grad.cpu(), z["dact_W"], 1e-5, "dact_W")
        assert_close(act[1].bias.grad.cpu(), z["dact_b"], 1e-5, "dact_b")


SIRE = golden_manifest("sire")


@pytest.mark.parametrize("case", SIRE, ids=[c["name"] for c in SIRE])
def test_sireconv_vs_reference_golden(case):
    """SIREConv (models/conv.py:70-134) against the reference's own outputs and the fp64 oracle."""
    from sirgcn import SIREConv
    z = load_case(case["name"])
    dt = torch.float64 if case["dtype"] == "float64" else torch.float32
    act = _act_module(case, z)
    m = SIREConv(case["d"], case["de"], case["H"], case["O"], act, 0, agg_type=case["agg"]).to(DEV, dt)
    with torch.no_grad():
        for name, key in (("linear_query.weight", "W_Q"), ("linear_query.bias", "b_Q"), ("linear_key.weight", "W_K"),
                          ("linear_edge.weight", "W_E"), ("linear_relation.weight", "W_R"),
                          ("linear_relation.bias", "b_R")):
            m.get_parameter(name).copy_(_t(z[key], dt))
    g = Graph(torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), case["V"])
    X = _t(z["X"], dt).requires_grad_(True)
    Ef = _t(z["efeat"], dt).requires_grad_(True)
    Y = m(g, X, Ef)
    Y.backward(_t(z["dY"], dt))
    torch.cuda.synchronize()
    d = lambda k: torch.from_numpy(z[k]).double()
    truth = oracle.sire_reference_step(z["src"], z["dst"], case["V"],
                                       *[d(k) for k in ("X", "efeat", "W_Q", "b_Q", "W_K", "W_E", "W_R", "b_R", "dY")],
                                       case["agg"], _oracle_act(case, z), case["slope"])
    got = {"Y": Y, "dX": X.grad, "defeat": Ef.grad, "dW_Q": m.linear_query.weight.grad,
           "db_Q": m.linear_query.bias.grad, "dW_K": m.linear_key.weight.grad, "dW_E": m.linear_edge.weight.grad,
           "dW_R": m.linear_relation.weight.grad, "db_R": m.linear_relation.bias.grad}
    for k, v in got.items():
        assert v.dtype == dt, k
        assert_parity(v.detach().cpu(), z[k], truth[k], 1e-5, f"{case['name']} {k}")


def test_sireconv_embedding_edge_encoder():
    """zinc/model.py:12-15 swaps linear_edge for nn.Embedding (integer bond types)."""
    from sirgcn import SIREConv
    V, E, H = 50, 300, 32
    gen = torch.Generator().manual_seed(9)
    src, dst = torch.randint(0, V, (E,), generator=gen), torch.randint(0, V, (E,), generator=gen)
    m = SIREConv(H, 4, H, H, nn.LeakyReLU(0.2), 0, agg_type="sum").to(DEV)
    m.linear_edge = nn.Embedding(4, H).to(DEV)
    X = torch.randn(V, H, generator=gen).to(DEV)
    bond = torch.randint(0, 4, (E,), generator=gen).to(DEV)
    Y = m(Graph(src, dst, V), X, bond)
    Y.sum().backward()
    Ee = m.linear_edge.weight.detach().cpu()[bond.cpu()]
    w = [m.linear_query.weight, m.linear_query.bias, m.linear_key.weight, m.linear_relation.weight,
         m.linear_relation.bias]
    ref = oracle.sire_reference_step(src, dst, V, X.cpu(), Ee, *[t.detach().cpu() for t in w[:3]],
                                     torch.eye(H), *[t.detach().cpu() for t in w[3:]], torch.ones(V, H),
                                     "sum", "leaky", 0.2)
    assert_close(Y.detach().cpu(), ref["Y"], 1e-5, "Y")
    assert m.linear_edge.weight.grad is not None


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_generic_path_matches_fused_semantics(case):
    """The same layers through the edge-materialised path (sigma passed as an opaque callable):
    exercises sir_segment_sum (norms, mean, split rows, empty graph) + sir_edge_broadcast."""
    z = load_case(case["name"])
    base = ACTS[case["act"]]
    m = SIRConv(case["d"], case["H"], case["O"], lambda t: base(t), 0, agg_type=case["agg"]).to(DEV)
    _load_reference_weights(m, z)
    g = Graph(torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), case["V"])
    X = _t(z["X"]).requires_grad_(True)
    Y = m(g, X)
    Y.backward(_t(z["dY"]))
    d = lambda k: torch.from_numpy(z[k]).double()
    truth = oracle.layer_fwd_bwd(z["src"], z["dst"], case["V"], *[d(k) for k in ("X", "W_Q", "b_Q", "W_K", "W_R", "b_R", "dY")],
                                 case["agg"], case["act"], case["slope"])
    for k, v in {"Y": Y, "dX": X.grad, "dW_Q": m.linear_query.weight.grad, "dW_K": m.linear_key.weight.grad,
                 "dW_R": m.linear_relation.weight.grad}.items():
        assert_parity(v.detach().cpu(), z[k], truth[k], 1e-5, f"{case['name']} {k}")


@pytest.mark.parametrize("chunk", [4, 64, 256])
def test_max_split_rows_and_isolated_nodes(chunk):
    gen = torch.Generator().manual_seed(chunk)
    V, E, d, H, O = 300, 2500, 24, 64, 40
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(0, V - 30, (E,), generator=gen)        # 30 isolated destinations -> Y = 0
    dst[:600] = 5                                               # hub row split at every chunk
    X = torch.randn(V, d, generator=gen); dY = torch.randn(V, O, generator=gen)
    torch.manual_seed(chunk)
    m = SIRConv(d, H, O, nn.LeakyReLU(0.2), 0, agg_type="max").to(DEV)
    m.chunk = chunk
    x = X.to(DEV).requires_grad_(True)
    Y = m(Graph(src, dst, V), x); Y.backward(dY.to(DEV))
    w = [t.detach().cpu() for t in (m.linear_query.weight, m.linear_query.bias, m.linear_key.weight,
                                    m.linear_relation.weight, m.linear_relation.bias)]
    r32 = oracle.reference_cpu_step(src, dst, V, X, *w, dY, "max", "leaky", 0.2)
    r64 = oracle.reference_cpu_step(src, dst, V, X.double(), *[t.double() for t in w], dY.double(), "max", "leaky", 0.2)
    assert torch.all(Y[V - 30:] == 0)
    for k, v in {"Y": Y, "dX": x.grad, "dW_Q": m.linear_query.weight.grad, "dW_K": m.linear_key.weight.grad,
                 "dW_R": m.linear_relation.weight.grad, "db_R": m.linear_relation.bias.grad}.items():
        assert_parity(v.detach().cpu(), r32[k], r64[k], 1e-5, k)


def test_segment_max_first_wins_on_ties():
    plan = GraphPlan(torch.tensor([0, 1, 2, 2]), torch.tensor([0, 0, 0, 1]), 3, DEV)
    M = torch.tensor([[1.0, 5.0], [3.0, 5.0], [3.0, 0.0], [-7.0, -2.0]], device=DEV)
    Y = torch.empty(3, 2, device=DEV); arg = torch.empty(3, 2, device=DEV, dtype=torch.int32)
    _native.segment_max(plan.dst, M, Y, arg)
    assert Y.cpu().tolist() == [[3.0, 5.0], [-7.0, -2.0], [0.0, 0.0]]
    assert arg.cpu().tolist() == [[1, 0], [3, 3], [-1, -1]]
    dM = torch.empty_like(M)
    _native.segment_max_bwd(plan.dst, arg, torch.ones(3, 2, device=DEV), dM)
    assert dM.cpu().tolist() == [[0.0, 1.0], [1.0, 0.0], [0.0, 0.0], [1.0, 1.0]]


# ------------------------------------------------------------------ GraphNorm (models/norm.py:7-29)
GN = golden_manifest("graphnorm")


@pytest.mark.parametrize("case", GN, ids=[c["name"] for c in GN])
def test_graph_norm_vs_reference_golden(case):
    from sirgcn import GraphNorm, batch
    z = load_case(case["name"])
    sizes = z["batch_num_nodes"].tolist()
    g = batch([Graph(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), n) for n in sizes])
    gn = GraphNorm(case["F"], bias=case["bias"], mean_scale=case["mean_scale"]).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(_t(z["weight"]))
        if case["bias"]:
            gn.bias.copy_(_t(z["bias"]))
        if case["mean_scale"]:
            gn.mean_scale.copy_(_t(z["mean_scale"]))
    X = _t(z["X"]).requires_grad_(True)
    Y = gn(g, X)
    Y.backward(_t(z["dY"]))
    torch.cuda.synchronize()
    f32 = lambda k: torch.from_numpy(z[k]) if k in z else None
    f64 = lambda k: torch.from_numpy(z[k]).double() if k in z else None
    # reference op order with a correctly rounded sqrt: bit-exact (the reference's CPU
    # torch.sqrt is vectorised and not correctly rounded -> fixture Y is checked by accuracy)
    Y_ieee, _, _ = oracle.graph_norm_fwd(f32("X"), sizes, f32("weight"), f32("bias"), f32("mean_scale"),
                                         ieee_sqrt=True)
    assert torch.equal(Y.detach().cpu(), Y_ieee), "forward differs from the reference op order"
    Y64, mean, std = oracle.graph_norm_fwd(f64("X"), sizes, f64("weight"), f64("bias"), f64("mean_scale"))
    assert_parity(Y.detach().cpu(), z["Y"], Y64, 1e-5, "Y")
    dX, dw, db, dms = oracle.graph_norm_bwd(f64("X"), f64("dY"), sizes, f64("weight"), f64("mean_scale"), mean, std)
    assert_parity(X.grad.cpu(), z["dX"], dX, 1e-5, "dX")
    assert_parity(gn.weight.grad.cpu(), z["dweight"], dw, 1e-5, "dweight")
    if case["bias"]:
        assert_parity(gn.bias.grad.cpu(), z["dbias"], db, 1e-5, "dbias")
    if case["mean_scale"]:
        assert_parity(gn.mean_scale.grad.cpu(), z["dmean_scale"], dms, 1e-5, "dmean_scale")


@pytest.mark.parametrize("F", [300, 128, 6])
def test_graph_norm_column_widths_bit_identical(F, monkeypatch):
    """The one-column-per-lane GraphNorm kernels (default) and the 16-byte-column ones (SIR_GN_VW=4)
    take every per-graph sum in node order with the same per-element ops: bit-identical forward and
    backward, on molecule-sized graphs including an empty one."""
    from sirgcn import GraphNorm, batch
    g0 = torch.Generator().manual_seed(F)
    sizes = [int(v) for v in torch.randint(1, 60, (40,), generator=g0)] + [0, 3]
    g = batch([Graph(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), n) for n in sizes])
    V = sum(sizes)
    X = torch.randn(V, F, generator=g0).to(DEV)
    dY = torch.randn(V, F, generator=g0).to(DEV)
    outs = []
    for vw in ("1", "4"):
        monkeypatch.setenv("SIR_GN_VW", vw)
        torch.manual_seed(0)
        gn = GraphNorm(F, bias=True, mean_scale=True).to(DEV)
        with torch.no_grad():
            gn.weight.uniform_(0.5, 1.5)
            gn.mean_scale.uniform_(0.5, 1.5)
        Xd = X.clone().requires_grad_(True)
        Y = gn(g, Xd)
        Y.backward(dY)
        outs.append([Y.detach(), Xd.grad, gn.weight.grad, gn.bias.grad, gn.mean_scale.grad])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ device plan build (§8 f4)
def _plan_graphs():
    from sirgcn.synth import powerlaw_edges
    out = []
    for name in ("small_sum_leaky_f32", "long_sum_leaky_h256_f32", "empty_sum_leaky_f32"):
        z = load_case(name)
        out.append((name, torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), int(z["in_deg"].size)))
    s, d = powerlaw_edges(20000, 400000, 0.8, seed=3)
    out.append(("powerlaw_20k", s, d, 20000))
    out.append(("no_edges_V5", torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 5))
    return out


@pytest.mark.parametrize("chunk", [4, 256])
def test_native_plan_build_equals_reference_order(chunk):
    """sir_csr_build / sir_csr_perm == the torch restatement == the oracle's stable CSR, bit for bit."""
    from sirgcn.graph import build_plans_native, build_row_csr
    for name, src, dst, V in _plan_graphs():
        nd, ns = build_plans_native(src.to(DEV), dst.to(DEV), V, V, chunk)
        td = build_row_csr(dst, src, V, chunk)
        ts = build_row_csr(src, dst, V, chunk)
        for a, b in ((nd, td), (ns, ts)):
            assert (a.n_items, a.n_splits, a.n_slots, a.max_degree) == (b.n_items, b.n_splits, b.n_slots,
                                                                        b.max_degree), name
            for f in ("rowptr", "col", "eid", "items"):
                assert torch.equal(getattr(a, f).cpu(), getattr(b, f).cpu()), (name, f)
            assert (a.splits is None) == (b.splits is None), name
            if a.splits is not None:
                assert torch.equal(a.splits.cpu(), b.splits.cpu()), name
        pos = torch.empty(src.numel(), dtype=torch.int64)
        pos[td.eid] = torch.arange(src.numel())
        assert torch.equal(ns.perm.cpu().long(), pos[ts.eid]), name
        if src.numel():
            rowptr, col, eid = oracle.csr_by_dst(src.numpy(), dst.numpy(), V)
            assert np.array_equal(nd.rowptr.cpu().numpy(), rowptr) and np.array_equal(nd.eid.cpu().numpy(), eid)


def test_native_plan_build_rejects_bad_ids():
    from sirgcn.graph import build_plans_native
    src = torch.tensor([0, 1, 7], device=DEV)
    dst = torch.tensor([1, 2, 0], device=DEV)
    with pytest.raises(ValueError, match="out of range"):
        build_plans_native(src, dst, 3, 3)
    with pytest.raises(ValueError, match="out of range"):
        build_plans_native(torch.tensor([0], device=DEV), torch.tensor([-1], device=DEV), 3, 3)
    with pytest.raises(ValueError, match="out of range"):
        GraphPlan(torch.tensor([0, 5]), torch.tensor([1, 1]), 3, DEV)


def test_native_plan_build_batched_molecules_speed():
    """Batched small graphs (ZINC-shaped, SURVEY cfg2): the device builder must agree with the
    torch restatement and not be slower than it (printed for the record)."""
    import time
    from sirgcn.graph import batch, build_plans_native, build_row_csr
    gen = torch.Generator().manual_seed(0)
    gs = []
    for _ in range(128):
        n = int(torch.randint(10, 38, (1,), generator=gen))
        m = int(n * 2.15)
        gs.append(Graph(torch.randint(0, n, (m,), generator=gen), torch.randint(0, n, (m,), generator=gen), n))
    bg = batch(gs)
    src, dst = (t.to(DEV) for t in bg.edges())
    V = bg.num_nodes()

    def torch_plans():
        d = build_row_csr(dst, src, V)
        s_ = build_row_csr(src, dst, V)
        pos = torch.empty(src.numel(), dtype=torch.int64, device=DEV)
        pos[d.eid] = torch.arange(src.numel(), device=DEV)
        return d, s_, pos[s_.eid].to(torch.int32)

    ts = {}
    for name, f in (("torch", torch_plans), ("native", lambda: build_plans_native(src, dst, V, V))):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            f()
        torch.cuda.synchronize()
        ts[name] = (time.perf_counter() - t0) / 20 * 1e3
    print(f"plan build, {V} nodes / {src.numel()} edges: torch {ts['torch']:.3f} ms, native {ts['native']:.3f} ms")
    nd, ns = build_plans_native(src, dst, V, V)
    td, tsr, tperm = torch_plans()
    assert torch.equal(nd.items, td.items) and torch.equal(ns.perm, tperm)
    assert ts["native"] <= ts["torch"] * 1.5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("agg", ["sum", "sym", "mean"])
@pytest.mark.parametrize("chunk", [256, 4])
def test_one_launch_backward_bit_identical_to_two_passes(agg, dtype, chunk):
    _one_launch_vs_two_passes(agg, dtype, chunk, 256)


@pytest.mark.parametrize("H", [76, 128, 512])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("agg", ["sum", "sym", "mean"])
@pytest.mark.parametrize("chunk", [256, 4])
def test_one_launch_backward_bit_identical_to_two_passes_other_widths(agg, dtype, chunk, H):
    _one_launch_vs_two_passes(agg, dtype, chunk, H)


def _one_launch_vs_two_passes(agg, dtype, chunk, H):
    """sir_edge_agg_bwd (dQ pass || dK pass in one launch; MEAN on G / deg formed first) ==
    sir_edge_agg_bwd_dst + _src (MEAN: the dst pass divides and writes G / deg for the src pass),
    bit for bit — fp32 and both 16-bit storages, at a sub-wave width (76), 128, and one, two full-wave
    passes (256, 512; the widths beside 256 on a smaller graph)."""
    from sirgcn.conv import edge_backward
    gen = torch.Generator().manual_seed(21)
    V, E = (3000, 60000) if H == 256 else (1500, 24000)
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(0, V, (E,), generator=gen)
    dst[:3000] = 17                                       # hub rows: split items on both plans
    src[3000:5000] = 5
    plan = GraphPlan(src, dst, V, DEV, chunk=chunk)
    assert plan.dst.n_splits > 0 and plan.src.n_splits > 0
    QK = torch.randn(V, 2 * H, generator=gen).to(DEV, dtype)
    G = torch.randn(V, H, generator=gen).to(DEV, dtype)
    in_norm, out_norm = plan.norms(agg)
    S = torch.empty(V, H, device=DEV, dtype=dtype)
    mask = torch.empty(E * _native.mask_words(H, _native.ACT_LEAKY), device=DEV, dtype=torch.int64)
    part = torch.empty(max(plan.dst.n_slots, plan.src.n_slots) * H, device=DEV)
    _native.edge_agg_fwd(plan.dst, QK[:, :H], QK[:, H:], in_norm, out_norm, agg, _native.ACT_LEAKY, 0.2, S, part, mask)
    outs = []
    for dual in (True, False):
        EdgeAggregate.dual = dual
        try:
            dQK = torch.full((V, 2 * H), float("nan"), device=DEV, dtype=dtype)
            edge_backward(plan, H, agg, _native.ACT_LEAKY, 0.2, G, None, None, mask, dQK)
            outs.append(dQK)
        finally:
            EdgeAggregate.dual = True
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert torch.isfinite(outs[0]).all()


SIGN_MASK_WIDTHS = wc.SIGN_MASK_WIDTHS


@pytest.mark.parametrize("H", SIGN_MASK_WIDTHS)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("act", ["relu", "leaky"])
def test_sign_mask_backward_bit_identical_all_widths(H, agg, act):
    _sign_mask_vs_recompute(H, agg, act, torch.float32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("H", SIGN_MASK_WIDTHS)
@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("act", ["relu", "leaky"])
def test_sign_mask_backward_bit_identical_all_widths_16bit(H, agg, act, dtype):
    """The bf16 / fp16 compile units of the same passes (all widths are multiples of 4, as 16-bit storage
    requires): Q, K, G cast to the storage type before the call."""
    _sign_mask_vs_recompute(H, agg, act, dtype)


def _sign_mask_vs_recompute(H, agg, act, dtype):
    """Sign-mask backward == the recompute backward, bit for bit, at every mask layout: full-wave
    rows (wide-chunk dQ pass, every word count per edge, H = 136 .. 1024) and sub-wave rows (H <= 128:
    4 / 8 / 16 / 32 lanes per row, the reference's published widths 60, 76 = 75 padded, 80, 96 = 95
    padded, and config 2's 128), rows of 0 .. 300 edges, split hubs."""
    from sirgcn.conv import edge_backward
    gen = torch.Generator().manual_seed(H + len(agg) + len(act))
    V, E = 1500, 24000
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(0, V - 40, (E,), generator=gen)   # 40 isolated destinations
    dst[:300] = 11                                        # a hub row (split at chunk 64)
    plan = GraphPlan(src, dst, V, DEV, chunk=64)
    code = _native.ACT_RELU if act == "relu" else _native.ACT_LEAKY
    QK = torch.randn(V, 2 * H, generator=gen).to(DEV, dtype)
    G = torch.randn(V, H, generator=gen).to(DEV, dtype)
    in_norm, out_norm = plan.norms(agg)
    S = torch.empty(V, H, device=DEV, dtype=dtype)
    mask = torch.empty(E * _native.mask_words(H, code), device=DEV, dtype=torch.int64)
    part = torch.empty(max(plan.dst.n_slots, plan.src.n_slots, 1) * H, device=DEV)
    _native.edge_agg_fwd(plan.dst, QK[:, :H], QK[:, H:], in_norm, out_norm, agg, code, 0.2, S, part, mask)
    outs = []
    for m in (mask, None):
        dQK = torch.full((V, 2 * H), float("nan"), device=DEV, dtype=dtype)
        edge_backward(plan, H, agg, code, 0.2, G, QK[:, :H], QK[:, H:], m, dQK)
        outs.append(dQK)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert torch.isfinite(outs[0]).all()
