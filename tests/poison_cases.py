"""TEST INFRASTRUCTURE: the poison tests' inputs, embedding helpers and expected patterns
(tests/test_poison_gpu.py and their CPU self-check, tests/test_poison_inputs_cpu.py).

Part A, isolation.  A logical [M, N] operand lives inside a larger allocation (``embed``): a leading
dimension ld > N, rows past M, optionally a base that is not 16-byte aligned.  Everything a call must not
depend on holds NaN — one NaN that reaches an accumulator through any path, a multiply by zero included,
shows in the result, so the comparison needs no tolerance.  Outputs are views into buffers pre-filled with
one recognisable quiet-NaN bit pattern (``Out``), compared through an integer view: the logical output
equals the oracle, no sentinel is left inside it, every sentinel outside it is bit-unchanged.

Part B, propagation.  Single +inf / -inf / NaN values injected into the dyadic operands of
tests/exact_cases.py at traceable sites (``SITES``); ``check_propagation`` compares with the fp64 reference
evaluated on the same inputs: finite where it is finite and equal, non-finite where it is not, of the
same class where the kernel only selects, adds and scales.

Nothing here touches the GPU; integer operands (col, eidx, arg, offsets) are never poisoned."""
import contextlib

import torch

import exact_cases as xc
import oracle

NAN, INF = float("nan"), float("inf")
# one quiet NaN with a payload per float width, and one improbable integer per integer width
SENTINEL = {torch.float32: 0x7FD5A5A5, torch.bfloat16: 0x7FD5, torch.float16: 0x7F55,
            torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5B5A5A5A5B, torch.float64: 0x7FFD5A5A5A5A5A5A}
_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16,
             torch.int32: torch.int32, torch.int64: torch.int64, torch.float64: torch.int64}
GUARD = 16          # sentinel elements before (after the misalignment) and after every embedded allocation


def bits(t):
    """The integer view of a tensor's bit patterns."""
    return t.view(_INT_VIEW[t.dtype])


def _layout(M, N, pad_cols, pad_rows, misalign):
    ld = N + pad_cols
    base = GUARD + misalign
    total = base + (M + pad_rows) * ld + GUARD
    return ld, base, total


def embed(t, pad_cols=4, pad_rows=2, misalign=0):
    """The logical [M, N] operand ``t`` inside a NaN-filled allocation: returns (view, buffer).  ``view``
    has ``t``'s values, leading dimension N + pad_cols, pad_rows rows after it, and starts ``misalign``
    elements past a 16-byte boundary (GUARD is a multiple of 8 elements, torch allocations are aligned)."""
    assert t.dim() == 2 and t.dtype.is_floating_point
    M, N = t.shape
    ld, base, total = _layout(M, N, pad_cols, pad_rows, misalign)
    buf = torch.full((total,), NAN, dtype=t.dtype, device=t.device)
    view = buf.as_strided((M, N), (ld, 1), base)
    view.copy_(t)
    return view, buf


def poison_rows(t, rows):
    """A copy of ``t`` with NaN in the given rows (rows of a node matrix the call does not depend on)."""
    t = t.clone()
    t[rows] = NAN
    return t


class Out:
    """A logical [M, N] output inside a sentinel-filled allocation (``view``), or with ``flat`` a flat
    workspace of ``M * N`` elements with a sentinel tail."""

    def __init__(self, shape, dtype, device="cpu", pad_cols=4, pad_rows=2, misalign=0):
        M, N = shape
        self.shape, self.dtype = (M, N), dtype
        ld, base, total = _layout(M, N, pad_cols, pad_rows, misalign)
        self.buf = torch.zeros((total,), dtype=dtype, device=device)
        bits(self.buf).fill_(SENTINEL[dtype])
        self.view = self.buf.as_strided((M, N), (ld, 1), base)
        inside = torch.zeros((total,), dtype=torch.bool, device=device)
        inside.as_strided((M, N), (ld, 1), base).fill_(True)
        self.inside = inside

    def seed(self, t):
        """Give the logical part a defined previous content (SIR_AGG_ACCUMULATE, in-place kernels)."""
        self.view.copy_(t)
        return self

    def check_outside(self, what):
        b = bits(self.buf)
        changed = (b != SENTINEL[self.dtype]) & ~self.inside
        assert not bool(changed.any()), \
            f"{what}: {int(changed.sum())} elements outside the logical output were written " \
            f"(first at flat offset {int(torch.nonzero(changed)[0])})"

    def check_written(self, what, rows=None):
        """No sentinel left inside the logical output (``rows``: only these rows are the call's to write)."""
        left = bits(self.view.contiguous()) == SENTINEL[self.dtype]
        if rows is not None:
            left = left[rows]
        assert not bool(left.any()), f"{what}: {int(left.sum())} elements of the logical output were never written"

    def check(self, want, what):
        """The three assertions of Part A."""
        got = self.view
        assert got.shape == want.shape and got.dtype == want.dtype, what
        self.check_written(what)
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got)
            i = torch.nonzero(bad)[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the oracle, first "
                                 f"at {i}: got {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}")
        self.check_outside(what)


@contextlib.contextmanager
def poisoned_empty():
    """While active, every floating-point ``torch.empty`` / ``empty_like`` allocation is NaN-filled: the
    workspaces and outputs a Python layer allocates for a native call then hold what the contract allows
    them to hold.  Integer allocations are left alone (an integer workspace is never poisoned).  Only what
    goes through these two functions is reached (sirgcn allocates its workspaces and outputs with them;
    ``torch.zeros`` buffers are defined by design and ``new_empty`` is not used): the context yields the list
    of the shapes it filled, so a test can assert that the allocations it means were met."""
    real_empty, real_like = torch.empty, torch.empty_like
    filled = []

    def empty(*a, **k):
        t = real_empty(*a, **k)
        if t.dtype.is_floating_point:
            filled.append(tuple(t.shape))
            t.fill_(NAN)
        return t

    def empty_like(*a, **k):
        t = real_like(*a, **k)
        if t.dtype.is_floating_point:
            filled.append(tuple(t.shape))
            t.fill_(NAN)
        return t

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield filled
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


# ----------------------------------------------------------------------------- Part A: what a call ignores
def unreferenced(graph):
    """Boolean [V] masks (no_in, no_out): nodes without in-edges (Q[v], G[v] are don't-care, S[v] = dQ[v] = 0)
    and without out-edges (K[u], Gd[u] on the source side are don't-care, dK[u] = 0)."""
    src, dst, V = xc.GRAPHS[graph]
    return torch.bincount(dst, minlength=V) == 0, torch.bincount(src, minlength=V) == 0


def edge_operands(graph, H, dtype=torch.float32, device="cpu", pad_cols=4, misalign=0):
    """Poisoned Q, K, G of exact_cases.edge_inputs in ``dtype``: NaN pad columns and rows, NaN in Q[v], G[v]
    of the nodes without in-edges and in K[u] of the nodes without out-edges.  Returns the three views."""
    Q, K, G, _ = xc.edge_inputs(graph, H)
    no_in, no_out = unreferenced(graph)
    return tuple(embed(t.to(device, dtype), pad_cols, 2, misalign)[0]
                 for t in (poison_rows(Q, no_in), poison_rows(K, no_out), poison_rows(G, no_in)))


def check_edge_forward(backend, plan, graph, H, agg, act, dtype=torch.float32, device="cpu", pad_cols=4,
                       misalign=0, mask_words=0):
    """The whole checking path of Part A on the edge forward: embed -> ``backend.edge_agg_fwd`` (sirgcn._native,
    or tests/cpu_edge_backend.py in the CPU self-check) -> the three assertions; the partial workspace is
    NaN-filled to its size with a sentinel tail.  Returns (S, mask) for the backward checks."""
    code = {"relu": 1, "leaky": 2}[act]
    Q, K, _ = edge_operands(graph, H, dtype, device, pad_cols, misalign)
    V = Q.shape[0]
    in_norm, out_norm = plan.norms(agg)
    S = Out((V, H), dtype, device, pad_cols, 2, misalign)
    part = Out((1, max(plan.dst.n_slots, 1) * H), torch.float32, device, 0, 0)
    E = plan.dst.col.numel()
    mask = None
    if mask_words:
        mask = Out((E, mask_words), torch.int64, device, 0, 0)
    backend.edge_agg_fwd(plan.dst, Q, K, in_norm, out_norm, agg, code, xc.SLOPE if act == "leaky" else 0.0, S.view,
                         part.view[0], None if mask is None else mask.view.view(-1))
    what = f"{graph} {dtype} H={H} {agg} {act} ld=+{pad_cols} misalign={misalign}"
    want = xc.edge_expected(graph, H, agg, act)[0].float().to(dtype).to(device)
    S.check(want, what + " S")
    part.check_outside(what + " partial workspace")
    if mask is not None:
        mask.check_written(what + " mask")
        mask.check_outside(what + " mask")
    return S, mask


# ----------------------------------------------------------------------------- Part B: injection sites
# Graph A's blocks (exact_cases.BLOCKS_A): nodes 0-4 have one in-edge each (unsplit at every chunk), nodes
# 5-10 four, nodes 11-15 sixteen from all five of their block (split at chunk 4).  One class per column, so
# each can be traced; few nodes, so the rows a poisoned edge touches stay under a quarter of the graph.
SITES = {
    # name: (operand, [(node, column, value)])
    "Q": ("Q", [(0, 0, INF), (0, 1, -INF), (0, 2, NAN),                 # an unsplit row
                (11, 0, INF), (11, 1, -INF), (11, 2, NAN)]),            # a hub row, split at chunk 4
    "K": ("K", [(5, 3, INF), (6, 3, -INF),      # both reach rows of the (6, 4) block: +inf and -inf meet -> NaN
                (6, 1, -INF), (5, 2, NAN)]),
    "Khub": ("K", [(11, 0, INF), (12, 0, -INF),  # meet in every (split) row of the (5, 16) block
                   (11, 1, -INF), (11, 2, NAN), (12, 3, INF)]),
    # columns 0 and 1 hold z == 0 on every edge / on node 0's edges (exact_cases.ZERO_FULL, ZERO_COLS): there
    # sigma' = 0 (ReLU) or slope (LeakyReLU) meets t = inf; columns 3 and 4 have z > 0 on some of a hub's edges
    "G": ("G", [(0, 0, INF), (1, 1, -INF), (2, 2, NAN), (11, 0, INF), (12, 1, -INF), (13, 2, NAN),
                (11, 3, INF), (12, 4, -INF)]),
}


def inject(t, sites):
    t = t.clone()
    for node, colm, val in sites:
        if colm < t.shape[1]:
            t[node, colm] = val
    return t


def edge_case(H, site):
    """(Q, K, G) of graph A with the sites of ``site`` injected (fp32, exact otherwise)."""
    Q, K, G, _ = xc.edge_inputs("A", H)
    ops = {"Q": Q, "K": K, "G": G}
    name, where = SITES[site]
    ops[name] = inject(ops[name], where)
    return ops["Q"], ops["K"], ops["G"]


def edge_case_expected(H, site, agg, act):
    """fp64 oracle (S, dQ, dK) of edge_case, and for a non-finite z (sites in Q / K) the rows of dQ / dK the
    poisoned edges touch (the exempt rows of the backward: include/sirconv.h, deviation 2)."""
    def make():
        src, dst, V = xc.GRAPHS["A"]
        Q, K, G = (t.double() for t in edge_case(H, site))
        S = oracle.edge_agg_fwd(src, dst, V, Q, K, agg, act, xc.SLOPE)
        dQ, dK = oracle.edge_agg_bwd(src, dst, V, Q, K, G, agg, act, xc.SLOPE)
        bad = ~torch.isfinite(Q[dst] + K[src]).all(1)
        ex_q = torch.zeros(V, dtype=torch.bool).index_fill_(0, dst[bad], True)
        ex_k = torch.zeros(V, dtype=torch.bool).index_fill_(0, src[bad], True)
        return S, dQ, dK, ex_q, ex_k
    return xc.cached(("poison-edge", H, site, agg, act), make)


def classes(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    c = torch.zeros(t.shape, dtype=torch.int8, device=t.device)
    c[torch.isnan(t)] = 1
    c[t == INF] = 2
    c[t == -INF] = 3
    return c


def check_propagation(got, ref64, what, same_class=True, rows=None):
    """Part B's assertions for every element (of ``rows`` when given): where the reference is finite the
    value is finite and equal to it (rounded once to the output type); where it is not, the value is
    non-finite, and of the same class when ``same_class``."""
    want = ref64.to(got.dtype).to(got.device)
    if rows is not None:
        got, want = got[rows], want[rows]
    fin = torch.isfinite(want)
    silent = ~fin & torch.isfinite(got)
    assert not bool(silent.any()), \
        f"{what}: {int(silent.sum())} elements are finite where the reference is not (first at " \
        f"{torch.nonzero(silent)[0].tolist()}: got {got[tuple(torch.nonzero(silent)[0].tolist())].item()!r})"
    wrong = fin & ((got != want) | ~torch.isfinite(got))
    assert not bool(wrong.any()), \
        f"{what}: {int(wrong.sum())} elements differ where the reference is finite (first at " \
        f"{torch.nonzero(wrong)[0].tolist()})"
    if same_class:
        other = classes(got) != classes(want)
        assert not bool(other.any()), \
            f"{what}: {int(other.sum())} elements have another non-finite class than the reference (first at " \
            f"{torch.nonzero(other)[0].tolist()})"


def nonfinite_share(ref):
    """Share of the non-finite elements of a reference output; for a GEMM-like one use rows_share."""
    return float((~torch.isfinite(ref)).float().mean())


def rows_share(ref, dim=1):
    """Share of the rows (dim = 1) or columns (dim = 0) of ``ref`` that hold a non-finite element."""
    return float((~torch.isfinite(ref)).any(dim).float().mean())


# ----------------------------------------------------------------------------- the maximum with non-finite candidates
def max_nan_wins(dst, V, M):
    """The library's maximum (include/sirconv.h): torch.max's order — a NaN beats every number — with the
    first of equal candidates, and the first NaN, as arg (edge ids); a row without edges gives 0 / -1."""
    dst = torch.as_tensor(dst, dtype=torch.int64)
    E, F = M.shape
    idx = dst.unsqueeze(1).expand(E, F)
    Y = torch.zeros((V, F), dtype=M.dtype).scatter_reduce(0, idx, M, reduce="amax", include_self=False)
    eid = torch.arange(E).unsqueeze(1).expand(E, F)
    hit = (M == Y[dst]) | (torch.isnan(M) & torch.isnan(Y[dst]))
    arg = torch.full((V, F), E, dtype=torch.int64).scatter_reduce(0, idx, torch.where(hit, eid, E), reduce="amin")
    arg[arg == E] = -1
    return Y, arg


def max_messages_case(graph, F, kind):
    """Integer messages M [E, F] (caller's edge order) of graph ``graph`` with non-finite candidates:
    ``kind`` = 'inf': +inf / -inf among the candidates and every message of some rows -inf; 'nan': one NaN
    in the middle of some rows (hub rows included, so a chunk-4 plan cuts before and after it), two NaNs in
    others, and rows that are all NaN.  Column f of row v is touched when (v + f) % 4 == 0, so every row keeps
    finite columns."""
    def make():
        src, dst, V = xc.GRAPHS[graph]
        E = src.numel()
        M = xc.ints((E, F), 4, 4100 + F)
        order = xc.csr_order(graph)                      # edges by row, ascending id inside a row
        deg = torch.bincount(dst, minlength=V)
        start = torch.cumsum(deg, 0) - deg
        f = torch.arange(F)
        for v in range(V):
            d = int(deg[v])
            if d == 0:
                continue
            e = order[start[v]:start[v] + d]
            colm = f[(v + f) % 4 == 0]
            bad = NAN if kind == "nan" else -INF
            mode = v % 4
            if mode == 0:                                # every candidate
                M[e[:, None], colm[None, :]] = bad
            elif mode == 1:                              # one in the middle (not the first, when there is a choice)
                M[e[d // 2], colm] = bad if kind == "nan" else INF
            elif mode == 2 and d >= 2:                   # two: the first of them must win
                M[e[d // 3], colm] = bad if kind == "nan" else INF
                M[e[d - 1], colm] = bad if kind == "nan" else INF
            elif kind == "inf":                          # -inf among finite candidates: never the maximum
                M[e[0], colm] = -INF
        return M
    return xc.cached(("poison-max", graph, F, kind), make)


# ----------------------------------------------------------------------------- fused edge MLP with non-finite values
def _mlp_nan_sites(graph):
    """(hub row, short row, sender) whose Q / K get one NaN: few rows of the graph see it."""
    return (11, 0, 6) if graph == "A" else (44, 1, 2)


def mlp_max_case(graph, H, O, act):
    """Inputs of the fused max form with non-finite messages, and the fp64 expectation: bias columns 0 / 1 / 2
    are -inf / +inf / NaN (every message of those columns, in every row); one NaN in Q of a hub row and of a
    short row, one NaN in K of one source node (every message of the edges it sends)."""
    def make():
        src, dst, V = xc.GRAPHS[graph]
        Q, K, W, b, _ = (t.clone() for t in xc.mlp_inputs(graph, H, O))
        b[0], b[1], b[2] = -INF, INF, NAN
        hub, short, sender = _mlp_nan_sites(graph)
        Q[hub, 5], Q[short, 9], K[sender, 3] = NAN, NAN, NAN
        M = oracle.act_fwd(Q.double()[dst] + K.double()[src], act, xc.SLOPE) @ W.double().t() + b.double()
        Y, arg = max_nan_wins(dst, V, M)
        return Q, K, W, b, Y, arg
    return xc.cached(("poison-mlpmax", graph, H, O, act), make)


def max_bias_case(graph, H, O, act):
    """The max form with finite Q, K and bias columns 0 / 1 / 2 = -inf / +inf / NaN: (Q, K, W, b, dY, arg, want)
    with arg the oracle's arg edges (the first edge in those columns) and want = dQ, dK, dW, db of the backward
    evaluated in fp64 on those arg edges (the bias does not enter any of them)."""
    def make():
        src, dst, V = xc.GRAPHS[graph]
        Q, K, W, b, dY = (t.clone() for t in xc.mlp_inputs(graph, H, O))
        b[0], b[1], b[2] = -INF, INF, NAN
        z = Q.double()[dst] + K.double()[src]
        a = oracle.act_fwd(z, act, xc.SLOPE)
        _, arg = max_nan_wins(dst, V, a @ W.double().t() + b.double())
        dM = torch.zeros(src.numel(), O, dtype=torch.float64)
        r, f = torch.nonzero(arg >= 0, as_tuple=True)
        dM[arg[r, f], f] = dY.double()[r, f]
        dz = oracle.act_bwd(z, dM @ W.double(), act, xc.SLOPE)
        want = {"dQ": torch.zeros(V, H, dtype=torch.float64).index_add_(0, dst, dz),
                "dK": torch.zeros(V, H, dtype=torch.float64).index_add_(0, src, dz),
                "dW": dM.t() @ a, "db": dM.sum(0)}
        return Q, K, W, b, dY, arg, want
    return xc.cached(("poison-maxbias", graph, H, O, act), make)


def seq_nan_case(graph, H, F, agg):
    """The sum-family edge MLP (ReLU, Linear, ReLU) with the NaN sites of mlp_max_case in Q / K: (Q, K, W, b, S64)."""
    def make():
        src, dst, V = xc.GRAPHS[graph]
        Q, K, W, b, _ = (t.clone() for t in xc.mlp_inputs(graph, H, F))
        hub, short, sender = _mlp_nan_sites(graph)
        Q[hub, 5], Q[short, 9], K[sender, 3] = NAN, NAN, NAN
        ind = torch.bincount(dst, minlength=V)
        in_norm, out_norm = oracle.degree_norms(ind, torch.bincount(src, minlength=V), agg)
        m = torch.relu(torch.relu(Q.double()[dst] + K.double()[src]) @ W.double().t() + b.double())
        S = torch.zeros(V, F, dtype=torch.float64).index_add_(0, dst, (out_norm[src] * in_norm[dst]).double()[:, None] * m)
        if agg == "mean":
            S = S / ind.clamp(min=1).double()[:, None]
        return Q, K, W, b, S
    return xc.cached(("poison-seqnan", graph, H, F, agg), make)


def gemm_nonfinite_case(M, K, N):
    """A [M, K], W [N, K], b, B [M, N] on integers with a NaN, a +inf and a -inf in three rows of A and a +inf and
    a NaN in two columns' rows of B (the TN operands): NT marks three rows, TN three rows and two columns."""
    A, W, b = xc.gemm_inputs(M, K, N)
    A, B = A.clone(), xc.ints((M, N), 4, 17 + M + K + N)
    A[3, 5], A[M // 2, K - 1], A[M - 1, 0] = NAN, INF, -INF
    B[7, 2], B[M - 2, N - 1] = INF, NAN
    return A, W, b, B


def resid_case():
    """Y, R, D, D2 [37, 72] on integers with +inf / -inf / NaN in Y, R (one NaN in a row that also holds -inf)
    and in the gradient D."""
    Y, R, D, D2 = (xc.ints((37, 72), 4, 800 + i) for i in range(4))
    Y[1, 1], Y[2, 2], Y[3, 3] = INF, -INF, NAN
    R[4, 4], R[2, 5] = -INF, NAN
    D[5, 5], D[6, 6], D[7, 7] = INF, -INF, NAN
    return Y, R, D, D2


def col_sum_case(n, m):
    """X [n, m] on integers with a NaN in column 1, a +inf in column 2 and +inf meeting -inf in column 3."""
    X = xc.ints((n, m), 4, 950 + n)
    X[n // 2, 1], X[0, 2], X[n - 1, 3], X[1, 3] = NAN, INF, INF, -INF
    return X
