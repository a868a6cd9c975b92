"""TEST INFRASTRUCTURE: dyadic inputs for the exact-arithmetic tests (tests/test_exact_gpu.py and their
CPU self-check, tests/test_exact_inputs_cpu.py).

Every value here is a small integer (or, through LeakyReLU(0.25), the degree norms and the mean, a small
integer divided by a power of two), so every intermediate and every result of the kernels under test is
exactly representable in fp32 whatever the summation order, split-row plan or MFMA tiling: the fp64 oracle
is THE answer, the comparison is ``torch.equal``, and a tie (z == 0, two maximal edges) is an exact tie
with one specified resolution (sigma'(0) = 0 / slope, sign bit = z > 0, the first edge wins).

Nothing here touches the GPU; the encoder of the documented ``sir_mask_words`` layout lives here too."""
import numpy as np
import torch

import oracle

SLOPE = 0.25
ACT_NAMES = ("relu", "leaky")
BLOCKS_A = ((5, 1), (6, 4), (5, 16), (3, 64), (3, 256), (2, 1024))
HUB_DEGREES_B = (64, 65, 128, 129, 256, 257, 512, 513)      # chunk, chunk + 1, 2 chunk, 2 chunk + 1 at 64 / 256
WIDTH = 1024                # the edge-kernel inputs of width H are the first H columns of one [V, 1024] draw
ZERO_COLS = slice(1, None, 8)       # columns with K[:, c] = -Q[0, c]: z == 0 on every in-edge of node 0
ZERO_FULL = slice(0, None, 8)       # columns where, besides, Q[:, c] = Q[0, c]: z == 0 on every edge


def _graph_a():
    """Disjoint blocks (n, d): node v of a block receives d edges from (v + 1 + j) mod n, j < d (multi-edges
    and self-loops when d > n), so in- and out-degree are d for every node of the block — every sym norm and
    every mean division is a power of two.  3 isolated nodes; edge ids shuffled.  V = 27, E = 3117."""
    src, dst, base = [], [], 0
    for n, d in BLOCKS_A:
        v = torch.arange(n).repeat_interleave(d)
        j = torch.arange(d).repeat(n)
        dst.append(base + v)
        src.append(base + (v + 1 + j) % n)
        base += n
    src, dst = torch.cat(src), torch.cat(dst)
    p = torch.randperm(src.numel(), generator=torch.Generator().manual_seed(2024))
    return src[p].contiguous(), dst[p].contiguous(), base + 3


def _graph_b():
    """Arbitrary degrees (sum and max only): nodes 0..39 with random edges, duplicates and self-loops; nodes
    40..47 receive exactly HUB_DEGREES_B edges (from random nodes < 40), nodes 48..55 send exactly that many
    (to random nodes < 40); nodes 56..59 are isolated.  Edge ids shuffled.  V = 60."""
    gen = torch.Generator().manual_seed(4048)
    rs, rd = torch.randint(0, 40, (150,), generator=gen), torch.randint(0, 40, (150,), generator=gen)
    loops = torch.tensor([3, 3, 17, 39])
    src, dst = [rs, rs[:12], loops], [rd, rd[:12], loops]
    for i, deg in enumerate(HUB_DEGREES_B):
        src.append(torch.randint(0, 40, (deg,), generator=gen))
        dst.append(torch.full((deg,), 40 + i))
        src.append(torch.full((deg,), 48 + i))
        dst.append(torch.randint(0, 40, (deg,), generator=gen))
    src, dst = torch.cat(src), torch.cat(dst)
    p = torch.randperm(src.numel(), generator=gen)
    return src[p].contiguous(), dst[p].contiguous(), 60


LADDER_C = 66


def _graph_c():
    """A degree ladder (sum and max only): node v < 66 receives exactly v edges, from (5 v + 3 j + 1) mod 66,
    j < v; node 66 + u sends exactly u edges, to 66 + (7 u + 5 j + 2) mod 66, j < u; nodes 132, 133 are
    isolated.  In-degrees of nodes 0..65 and out-degrees of nodes 66..131 are exactly 0..65: every tail
    length after 0..4 full chunks of 16 / 8 / 5 / 4 edges, two periods of the longest loop structure,
    63 / 64 / 65 around chunk 64 and every split residue at chunk 4.  Edge ids shuffled.  V = 134, E = 4290."""
    L = LADDER_C
    v = torch.arange(L).repeat_interleave(torch.arange(L))
    j = torch.cat([torch.arange(d) for d in range(L)])
    src = torch.cat([(5 * v + 3 * j + 1) % L, L + v])
    dst = torch.cat([v, L + (7 * v + 5 * j + 2) % L])
    p = torch.randperm(src.numel(), generator=torch.Generator().manual_seed(606))
    return src[p].contiguous(), dst[p].contiguous(), 2 * L + 2


# the widths of a list take every kernel shape the dispatchers can pick at its lowest legal width, at its highest
# and in between (tests/width_cases.py holds the lists to that; tests/test_width_classes_cpu.py checks it)
EDGE_H = (4, 12, 32, 60, 76, 128, 136, 256, 512, 776, 1024,       # fp32, bf16, fp16
          16, 20, 36, 64, 68, 132, 260, 516, 640, 768, 772, 24, 300)
EDGE_H_SCALAR = (1, 3, 7, 30, 63, 65, 99, 127, 129, 191, 193, 255)    # fp32 only: scalar path, no sign mask
EDGE_H_UNALIGNED = (64, 128, 256)   # fp32, H % 4 == 0 rows behind an odd leading dimension: the scalar path, full
SIRE_H = (4, 32, 80, 128, 132, 256, 1024, 16, 20, 36, 64, 68, 260, 512, 516, 640, 768, 772,
          12, 24, 48, 200, 300, 776)
SEQ_SHAPES = ((16, 16), (32, 48), (100, 140), (256, 256), (32, 100), (200, 128))
MAX_SHAPES = ((64, 64), (100, 200), (256, 40), (256, 256), (512, 512), (32, 100), (64, 300), (200, 300))
HELPER_F = (3, 64, 300, 70, 127, 129, 190, 253, 516, 768, 1024, 1, 4, 63, 65, 255, 256, 260, 512)
GRAPHS = {"A": _graph_a(), "B": _graph_b(), "C": _graph_c()}
# mean / sym are exact on graph A only
AGGS_OF = {"A": ("sum", "mean", "sym"), "B": ("sum",), "C": ("sum",)}
GRAPH_AGG = [(g, a) for g in GRAPHS for a in AGGS_OF[g]]


def graphs_of(agg):
    return [g for g in GRAPHS if agg in AGGS_OF[g]]
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def ints(shape, bound, seed):
    """fp32 integers in [-bound, bound]."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=gen).float()


def _zero_columns(Q, K):
    K[:, ZERO_COLS] = -Q[0, ZERO_COLS]
    Q[:, ZERO_FULL] = Q[0, ZERO_FULL]
    K[:, ZERO_FULL] = -Q[0, ZERO_FULL]


def csr_order(graph):
    """Edge ids in destination-CSR order (stable by dst: the order of the plans and of DGL's CSC)."""
    src, dst, V = GRAPHS[graph]
    return cached(("eid", graph), lambda: torch.from_numpy(oracle.csr_by_dst(src.numpy(), dst.numpy(), V)[2]))


# ----------------------------------------------------------------------------- edge kernels (no GEMM)
def edge_inputs(graph, H):
    """Q, K, G [V, H] and Eh [E, H] (caller's edge order): integers in [-4, 4], fp32; z == 0 by construction in
    ZERO_COLS / ZERO_FULL (besides the one pair in nine that two such integers cancel on).  The first H columns
    of one draw per graph: the edge kernels are column-wise independent, so what holds at H = 1024 holds for
    every slice."""
    def make():
        src, _, V = GRAPHS[graph]
        seed = 11 if graph == "A" else 29
        Q, K, G = (ints((V, WIDTH), 4, seed + i) for i in range(3))
        Eh = ints((src.numel(), WIDTH), 4, seed + 3)
        _zero_columns(Q, K)
        return Q, K, G, Eh
    return tuple(t[:, :H].contiguous() for t in cached(("in", graph), make))


def edge_z(graph, H, with_e=False, eh=None):
    """z per edge (caller's edge order), fp64."""
    src, dst, _ = GRAPHS[graph]
    Q, K, _, Eh = edge_inputs(graph, H)
    z = Q.double()[dst] + K.double()[src]
    if with_e:
        z = z + (Eh if eh is None else eh).double()
    return z


def edge_expected(graph, H, agg, act, dtype=torch.float64):
    """(S, dQ, dK) of the oracle's edge kernels on edge_inputs in ``dtype``."""
    def make():
        src, dst, V = GRAPHS[graph]
        Q, K, G, _ = (t.to(dtype) for t in edge_inputs(graph, H))
        S = oracle.edge_agg_fwd(src, dst, V, Q, K, agg, act, SLOPE)
        dQ, dK = oracle.edge_agg_bwd(src, dst, V, Q, K, G, agg, act, SLOPE)
        return S, dQ, dK
    return cached(("edge", graph, H, agg, act, dtype), make)


def sire_expected(graph, H, agg, act, table=None, dtype=torch.float64):
    """oracle.sire_reference_step with identity projections (X = [Q | K], W_Q = [I 0], W_K = [0 I], W_R = I,
    zero biases) and W_E = I: Y = S, dX = [dQ | dK], defeat = dE per edge.  The edge term is Eh of
    edge_inputs, or T[ids] for ``table`` = (T [R, H], ids [E]).  With identity projections no column meets
    another, so wide cases are evaluated in column blocks of 128 (the identity GEMMs cost E H^2 otherwise)."""
    def block(Q, K, G, Eh):
        src, dst, V = GRAPHS[graph]
        h = Q.shape[1]
        eye, zero = torch.eye(h, dtype=dtype), torch.zeros(h, h, dtype=dtype)
        r = oracle.sire_reference_step(src, dst, V, torch.cat([Q, K], 1), Eh, torch.cat([eye, zero], 1),
                                       torch.zeros(h, dtype=dtype), torch.cat([zero, eye], 1), eye, eye,
                                       torch.zeros(h, dtype=dtype), G, agg, act, SLOPE)
        return {"S": r["Y"], "dQ": r["dX"][:, :h], "dK": r["dX"][:, h:], "dE": r["defeat"]}

    def make():
        Q, K, G, Eh = (t.to(dtype) for t in edge_inputs(graph, H))
        if table is not None:
            Eh = table[0].to(dtype)[table[1]]
        parts = [block(*(t[:, c:c + 128] for t in (Q, K, G, Eh))) for c in range(0, H, 128)]
        return {k: torch.cat([p[k] for p in parts], 1) for k in parts[0]}
    return cached(("sire", graph, H, agg, act, table is not None, dtype), make)


def sire_table(graph, H, rows=5):
    """A table of ``rows`` edge-term rows and one row id per edge."""
    E = GRAPHS[graph][0].numel()
    gen = torch.Generator().manual_seed(7 + H)
    return ints((rows, H), 4, 77 + H), torch.randint(0, rows, (E,), generator=gen)


def encode_mask(zpos, H):
    """The documented sir_mask_words layout of the boolean [E, H] array ``zpos`` (bits past H zero)."""
    E = zpos.shape[0]
    if H > 128:
        nw = 4 * ((H + 255) // 256)
        bit = lambda f: (4 * ((f // 4) // 64) + f % 4, (f // 4) % 64)
    else:
        hc = H // 4
        L = 4 if hc <= 4 else 8 if hc <= 8 else 16 if hc <= 16 else 32
        nw = max(L // 16, 1)
        bit = lambda f: divmod((f % 4) * L + f // 4, 64)[0:2]
    out = np.zeros((E, nw), dtype=np.uint64)
    for f in range(H):
        w, b = bit(f)
        out[:, w] |= zpos[:, f].astype(np.uint64) << np.uint64(b)
    return out


def expected_mask(graph, H, with_e=False, eh=None):
    """The sign mask of z > 0 in destination-CSR order, encoded (uint64 [E, words])."""
    z = edge_z(graph, H, with_e, eh)[csr_order(graph)]
    return encode_mask((z > 0).numpy(), H)


# ----------------------------------------------------------------------------- per-edge Linear forms
def _identity_layer(Q, K, H):
    """X, W_Q, b_Q, W_K of a layer whose projections reproduce Q and K: X = [Q | K]."""
    dt = Q.dtype
    eye, zero = torch.eye(H, dtype=dt), torch.zeros(H, H, dtype=dt)
    return torch.cat([Q, K], 1), torch.cat([eye, zero], 1), torch.zeros(H, dtype=dt), torch.cat([zero, eye], 1)


def mlp_inputs(graph, H, F):
    """Q, K [V, H] in [-4, 4]; the edge Linear W [F, H] in [-2, 2], b [F] in [-4, 4]; dOut [V, F] in [-4, 4]."""
    def make():
        V = GRAPHS[graph][2]
        s = 1000 + 3 * H + F + (0 if graph == "A" else 7)
        Q, K = ints((V, H), 4, s), ints((V, H), 4, s + 1)
        _zero_columns(Q, K)
        return Q, K, ints((F, H), 2, s + 2), ints((F,), 4, s + 3), ints((V, F), 4, s + 4)
    return cached(("mlpin", graph, H, F), make)


SEQ_ACT_MODULE = {"identity": torch.nn.Identity, "relu": torch.nn.ReLU, "leaky": lambda: torch.nn.LeakyReLU(SLOPE)}
# (act1, act2) of the Sequential sigma beside the (relu, relu) of every SEQ_SHAPES case: each stays dyadic
SEQ_ACT_PAIRS = (("identity", "relu"), ("identity", "identity"), ("leaky", "identity"), ("relu", "identity"))


def seq_expected(graph, H, F, agg, dtype=torch.float64, act1="relu", act2="relu"):
    """S = agg_e act2(W act1(Q[v] + K[u]) + b) (ReLU, ReLU by default; names of SEQ_ACT_MODULE) and its
    gradients, by oracle.reference_cpu_step with the callable sigma, identity projections and W_R = I."""
    def make():
        src, dst, V = GRAPHS[graph]
        Q, K, W, b, G = (t.to(dtype) for t in mlp_inputs(graph, H, F))
        lin = torch.nn.Linear(H, F).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(b)
        sigma = torch.nn.Sequential(SEQ_ACT_MODULE[act1](), lin, SEQ_ACT_MODULE[act2]())
        X, W_Q, b_Q, W_K = _identity_layer(Q, K, H)
        r = oracle.reference_cpu_step(src, dst, V, X, W_Q, b_Q, W_K, torch.eye(F, dtype=dtype),
                                      torch.zeros(F, dtype=dtype), G, agg, sigma)
        return {"S": r["Y"], "dQ": r["dX"][:, :H], "dK": r["dX"][:, H:], "dW": lin.weight.grad.clone(),
                "db": lin.bias.grad.clone()}
    return cached(("seq", graph, H, F, agg, dtype, act1, act2), make)


def max_messages(graph, H, O, act, dtype=torch.float64):
    """The max form's per-edge messages M = W_R sigma(Q[v] + K[u]) + b_R [E, O], caller's edge order."""
    src, dst, _ = GRAPHS[graph]
    Q, K, W, b, _ = (t.to(dtype) for t in mlp_inputs(graph, H, O))
    return oracle.act_fwd(Q[dst] + K[src], act, SLOPE) @ W.t() + b


def max_expected(graph, H, O, act, dtype=torch.float64):
    """Y, arg (edge ids, DGL's first arg-max, -1 for an empty row), dQ, dK, dW_R, db_R of the max form."""
    def make():
        src, dst, V = GRAPHS[graph]
        Q, K, W, b, dY = (t.to(dtype) for t in mlp_inputs(graph, H, O))
        Y, arg = oracle.max_first_wins(dst, V, max_messages(graph, H, O, act, dtype))
        X, W_Q, b_Q, W_K = _identity_layer(Q, K, H)
        r = oracle.reference_cpu_step(src, dst, V, X, W_Q, b_Q, W_K, W, b, dY, "max", act, SLOPE)
        assert torch.equal(r["Y"], Y)
        return {"Y": Y, "arg": arg, "dQ": r["dX"][:, :H], "dK": r["dX"][:, H:], "dW": r["dW_R"], "db": r["db_R"]}
    return cached(("max", graph, H, O, act, dtype), make)


def max_tie_share(graph, H, O, act):
    """Share of the (row, output) pairs, among rows of in-degree >= 2, whose maximum is attained by two or
    more edges."""
    _, dst, V = GRAPHS[graph]
    M = max_messages(graph, H, O, act)
    Y, _ = oracle.max_first_wins(dst, V, M)
    n_max = torch.zeros(V, O).index_add_(0, dst, (M == Y[dst]).float())
    rows = torch.bincount(dst, minlength=V) >= 2
    return float((n_max[rows] >= 2).float().mean())


# ----------------------------------------------------------------------------- one layer through the GEMMs
LAYER_D = 8
LAYER_SHAPES = ((64, 40), (256, 256))
LAYER_AGGS = ("sum", "mean", "sym", "max")
# magnitudes (X, weights, biases, dY) per (H, O): chosen so that every GEMM operand of the step passes
# split_exact and every result stays below 2^24 (test_exact_inputs_cpu.py)
LAYER_BOUNDS = {(64, 40): (2, 1, 2, 2), (256, 256): (1, 1, 1, 1)}


def layer_inputs(H, O):
    """X [V, 8], W_Q, b_Q, W_K, W_R, b_R, dY [V, O]: integers, graph A."""
    def make():
        V = GRAPHS["A"][2]
        bx, bw, bb, bg = LAYER_BOUNDS[(H, O)]
        s = 5000 + H + O
        return (ints((V, LAYER_D), bx, s), ints((H, LAYER_D), bw, s + 1), ints((H,), bb, s + 2),
                ints((H, LAYER_D), bw, s + 3), ints((O, H), bw, s + 4), ints((O,), bb, s + 5), ints((V, O), bg, s + 6))
    return cached(("layerin", H, O), make)


def layer_expected(H, O, agg, act, dtype=torch.float64):
    """oracle.reference_cpu_step of the layer in ``dtype`` plus the GEMM operands the native step forms on
    the way (QK, S, G = dY W_R, dQK), for the CPU-side split check."""
    def make():
        src, dst, V = GRAPHS["A"]
        X, W_Q, b_Q, W_K, W_R, b_R, dY = (t.to(dtype) for t in layer_inputs(H, O))
        r = dict(oracle.reference_cpu_step(src, dst, V, X, W_Q, b_Q, W_K, W_R, b_R, dY, agg, act, SLOPE))
        Q, K = X @ W_Q.t() + b_Q, X @ W_K.t()
        ops = {"X": X, "W_Q": W_Q, "W_K": W_K, "W_R": W_R, "dY": dY, "QK": torch.cat([Q, K], 1)}
        Xi, Wi, bi, Ki = _identity_layer(Q, K, H)
        if agg == "max":
            ri = oracle.reference_cpu_step(src, dst, V, Xi, Wi, bi, Ki, W_R, b_R, dY, "max", act, SLOPE)
            ops["dQK"] = ri["dX"]
        else:
            li = oracle.layer_fwd_bwd(src, dst, V, X, W_Q, b_Q, W_K, W_R, b_R, dY, agg, act, SLOPE)
            ops.update(S=li["S"], G=li["dS"], dQK=torch.cat([li["dQ"], li["dK"]], 1))
        r["operands"] = ops
        return r
    return cached(("layer", H, O, agg, act, dtype), make)


LAYER_OUTPUTS = ("Y", "dX", "dW_Q", "db_Q", "dW_K", "dW_R", "db_R")


def _binade(x):
    """Smallest e with |x| < 2^e (fp32 exponent field - 126), as the GEMM's bexp()."""
    return (x.float().abs().view(torch.int32) >> 23) - 126


def split_exact(x, dim):
    """True when every element of the GEMM operand ``x`` (contraction along ``dim``) is reproduced exactly
    by the split-fp16 pair, x s == fp16(x s) + fp16(x s - fp16(x s)), for EVERY power-of-two scale s the
    kernels' rule can be holding when the element is split (sirconv_gemm.hip: scale_exp / next_se): a
    packed weight row uses s = 2^(15 - e_max); a data row's running scale is reset to 2^(7 - e_c) at a
    chunk of binade e_c and kept while later chunks stay below 2^(e_c + 8) — so an element of binade e_x in
    a row of binade e_max meets 2^(7 - e_max) <= s <= 2^(15 - e_x)."""
    x = x.float()
    e_x = _binade(x)
    e_max = e_x.amax(dim, keepdim=True).expand_as(x)
    ok = torch.ones_like(x, dtype=torch.bool)
    nz = x != 0
    for se in range(int((7 - e_max).min()), int((15 - e_x[nz]).max()) + 1 if nz.any() else 0):
        live = nz & (se >= 7 - e_max) & (se <= 15 - e_x)
        y = x * 2.0 ** se
        hi = y.half().float()
        lo = (y - hi).half().float()
        ok &= ~live | ((hi + lo) == y)
    return bool(ok.all())


GEMM_M = (1, 33, 257)
GEMM_KN = (4, 36, 132, 256)


def gemm_inputs(M, K, N):
    """A [M, K] in [-4, 4], W [N, K] in [-2, 2], bias [N] in [-4, 4]: integers."""
    s = 9000 + 7 * M + 3 * K + N
    return ints((M, K), 4, s), ints((N, K), 2, s + 1), ints((N,), 4, s + 2)
