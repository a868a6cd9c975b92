"""Far-offset tests on the GPU (layout, graphs and checkers: tests/far_cases.py; their self-check:
tests/test_far_cases_cpu.py).

Every kernel addresses an operand as ``base + row * ld + col`` with ``row`` from an int32 id and ``ld`` an int64
argument.  Here the operands are column slices of one wide buffer (ld = 4096) of 2^19 + 300 rows, so the later
rows lie past 2^31 bytes, 2^32 bytes and 2^31 elements from the base, and the graphs give work to exactly the rows
around those marks (graph N: node matrices far; graph E: [E, *] operands far; batched offsets: graph boundaries
across the marks).  A missing 64-bit cast reads the sentinel NaN of the arena's front guard or another row's
values, or overwrites a sentinel: an assertion fails, the device does not fault.

Each entry runs twice through its ``_native`` binding, on the far views and on compact contiguous operands of the
same shape ("near").  The far result must
  * equal the fp64 oracle on the compact operands (``torch.equal``) wherever the inputs are dyadic — integers, SUM
    and the maximum, as in tests/test_exact_gpu.py and tests/test_poison_gpu.py; where an entry's own fp64 test
    uses a tolerance (MEAN and SYM on degrees that are no powers of two, the norms) that tolerance is reused
    unchanged and cited at the call;
  * equal the near result bit for bit (the same kernel, the same plan, the same summation order: only the
    addresses differ);
  * leave no sentinel inside a logical output, every input bit-unchanged and every sentinel outside the operands
    bit-unchanged (``Arena.close``).
The norms run on seeded random data; their gradient is zero where the activation's input is a near-tie (``_untie``).
A test skips if the device has less free memory than its arenas plus 4 GiB; on an MI355X none does."""
import pytest
import torch

import exact_cases as xc
import far_cases as fc
import oracle
import poison_cases as pc
import test_poison_gpu as pg            # GEMM_ROUTES, the TN call with its workspace, the max routes (pg.xg)
from conftest import assert_parity

from sirgcn import _native, edgemlp
from sirgcn.dropedge import _fmix, drop_threshold
from sirgcn.graph import GraphPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ACT = {"relu": (_native.ACT_RELU, 0.0), "leaky": (_native.ACT_LEAKY, xc.SLOPE)}
NAN = float("nan")
HEADROOM = 4 * 2 ** 30
CHUNK = 256
M = fc.M
ROWS = torch.tensor(fc.mark_rows(4))         # the 16-bit MARK_ROWS are a subset (tests/test_far_cases_cpu.py)
PARITY = 1e-5           # conftest.assert_parity's bound in tests/test_gpu_parity.py, test_econv_gpu.py,
#                         test_nodenorm_gpu.py, test_readout_gpu.py and test_labelprop_gpu.py


@pytest.fixture(scope="module")
def arenas():
    """The arenas of this module, one per element size, allocated on first use and freed with the module."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()
    held = {}
    yield held
    held.clear()
    _GRAPHS.clear()
    _DATA.clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _refill(arenas):
    """Re-fill after each test: a failed test leaves its operands behind.  The [M, N] host inputs go with it (the
    parameters of one test share them; 134 MB each at N = 64)."""
    yield
    _DATA.clear()
    for a in arenas.values():
        if a.sentinel is not None:
            a.store.fill_(a.sentinel)
            a.views = []


def _open(arenas, dtype):
    size = dtype.itemsize
    if size not in arenas:
        need = fc.FULL.total * size + HEADROOM
        free = torch.cuda.mem_get_info()[0]
        if free < need:
            pytest.skip(f"{free / 2 ** 30:.1f} GiB free, the {size}-byte arena and its headroom need {need / 2 ** 30:.1f}")
        arenas[size] = fc.Arena(fc.FULL, size, DEV)
    return arenas[size].open(dtype)


class Far:
    """Operands as views into the arenas: columns 0, 1024, 2048, 3072 (a call with more operands: multiples of 512
    or 256).  ``dt16``: the 16-bit type of the call, if it has one; 4-byte operands (fp32, int32) share the other."""

    def __init__(self, arenas, n_ops=4, dt16=None):
        self.a = {4: _open(arenas, torch.float32)}
        if dt16 is not None:
            self.a[2] = _open(arenas, dt16)
        self.step = 1024 if n_ops <= 4 else 512 if n_ops <= 8 else 256
        self.col = {4: 0, 2: 0}

    def _take(self, dtype):
        c = self.col[dtype.itemsize]
        self.col[dtype.itemsize] += self.step
        return self.a[dtype.itemsize], c

    def full(self, t):
        a, c = self._take(t.dtype)
        return a.put(t, c)

    def rows(self, idx, vals, n_rows):
        a, c = self._take(vals.dtype)
        return a.put_rows(idx, vals, n_rows, c)

    def out(self, n_rows, n, dtype=torch.float32, seed=None):
        a, c = self._take(dtype)
        return a.out(n_rows, n, c, dtype, seed)

    def check(self, view, want, what, rows=None):
        self.a[view.dtype.itemsize].check(view, want, what, rows)

    def written(self, view, what, rows=None):
        return self.a[view.dtype.itemsize].check_written(view, what, rows)

    def close(self, what):
        for a in self.a.values():
            a.close(what)


class Near:
    """The same operands as compact contiguous tensors (outputs pre-filled with NaN / -2)."""

    def full(self, t):
        return t.to(DEV).contiguous().clone()

    def rows(self, idx, vals, n_rows):
        t = torch.full((n_rows, vals.shape[1]), NAN, dtype=vals.dtype, device=DEV)
        t[idx.to(DEV)] = vals.to(DEV)
        return t

    def out(self, n_rows, n, dtype=torch.float32, seed=None):
        if seed is not None:
            return seed.to(DEV).contiguous().clone()
        return torch.full((n_rows, n), -2 if dtype == torch.int32 else NAN, dtype=dtype, device=DEV)


def _both(arenas, body, what, n_ops=4, dt16=None, dont_care=()):
    """Run ``body`` on the far views and on near operands: returns the far outputs {name: view} (the arenas still
    open) after asserting that they equal the near ones bit for bit.  ``dont_care``: {name: rows that count}."""
    near = body(Near())
    p = Far(arenas, n_ops, dt16)
    far = body(p)
    assert far.keys() == near.keys()
    for name, f in far.items():
        if f is None:
            continue
        g, n = f.contiguous(), near[name]
        if name in dont_care:
            g, n = g[dont_care[name]], n[dont_care[name]]
        if not torch.equal(pc.bits(g), pc.bits(n)):
            bad = torch.nonzero(pc.bits(g) != pc.bits(n))
            raise AssertionError(f"{what} {name}: {bad.shape[0]} elements differ between the far and the near call, "
                                 f"first at {bad[0].tolist()}: {g[tuple(bad[0].tolist())].item()!r} vs "
                                 f"{n[tuple(bad[0].tolist())].item()!r}")
    return p, far


def _want(t64, dtype=torch.float32):
    """The fp64 oracle result in the kernel's output type (exact for fp32, rounded once for 16-bit storage)."""
    return t64.float().to(dtype)


# ----------------------------------------------------------------------------- graphs
_GRAPHS = {}


class FarGraph:
    """Graph N or E with its plan (the project's normal plan build), and the same graph on compact node ids for
    the CPU oracle: graph N's nodes are the MARK_ROWS (every other row has no edge), graph E's are all 4096."""

    def __init__(self, name):
        self.name = name
        self.src, self.dst, self.V, _ = fc.graph_n() if name == "N" else fc.graph_e()
        self.E = self.src.numel()
        self.plan = GraphPlan(self.src, self.dst, self.V, DEV, chunk=CHUNK)
        if name == "N":
            self.rows = ROWS
            self.cs, self.cd = torch.searchsorted(ROWS, self.src), torch.searchsorted(ROWS, self.dst)
            assert torch.equal(ROWS[self.cs], self.src) and torch.equal(ROWS[self.cd], self.dst)
        else:
            self.rows, self.cs, self.cd = None, self.src, self.dst
        self.Vc = self.V if self.rows is None else self.rows.numel()
        self.eid = self.plan.dst.eid.cpu()              # dst-CSR position -> the caller's edge id
        self.has_in = torch.bincount(self.cd, minlength=self.Vc) > 0
        assert self.plan.dst.n_splits == 2 and self.plan.dst.max_degree == fc.HUB_DEGREE

    def node_in(self, p, t):
        """A node operand from its compact values: graph N — the MARK_ROWS hold them, every other row the
        sentinel; graph E — all rows."""
        return p.full(t) if self.rows is None else p.rows(self.rows, t, self.V)

    def expand(self, t):
        """A compact node result [Vc, F] as the [V, F] the kernel writes: zeros in every row without edges."""
        if self.rows is None:
            return t
        full = torch.zeros((self.V, t.shape[1]), dtype=t.dtype)
        full[self.rows] = t
        return full

    def live(self):
        """The rows whose content counts where rows without in-edges are don't-care (device index)."""
        idx = torch.nonzero(self.has_in).flatten()
        return (idx if self.rows is None else self.rows[idx]).to(DEV)


def _graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = FarGraph(name)
    return _GRAPHS[name]


def _check_node(p, g, view, ref64, what, exact, ref32=None):
    """A node output [V, F] against the compact oracle: ``exact`` — torch.equal with the fp64 result in the output
    type; else inside assert_parity's bound (PARITY) on the rows with edges and exactly zero everywhere else."""
    if exact:
        p.check(view, g.expand(_want(ref64, view.dtype)), what)
        return
    got = p.written(view, what).cpu()
    if g.rows is not None:
        rest = got.clone()
        rest[g.rows] = 0
        assert not bool(rest.any()), f"{what}: a row without edges is not zero"
        got = got[g.rows]
    assert_parity(got.float(), ref32.float(), ref64, PARITY, what)


# ----------------------------------------------------------------------------- edge passes (graph N)
EDGE_CASES = [("f32", 3), ("f32", 64), ("bf16", 64), ("f16", 64)]       # the scalar class at its lowest width, a vector class


@pytest.mark.parametrize("agg", ["sum", "mean", "sym"])
@pytest.mark.parametrize("dt,H", EDGE_CASES, ids=[f"{d}-{H}" for d, H in EDGE_CASES])
def test_edge_passes_far_nodes(arenas, dt, H, agg):
    """sir_edge_agg_fwd, _bwd_dst, _bwd_src (recompute and sign-mask) and the one-launch sir_edge_agg_bwd on graph N:
    Q, K, G, S, dQ, dK, Gm (and the one-launch form's g = G / deg) are far in their rows; the mask and the partial
    workspaces are near.  SUM equals the fp64 oracle; MEAN and SYM (degrees 3, 5, 17, 65, 700: no powers of two)
    stay inside the parity bound of tests/test_gpu_parity.py in fp32 and equal the near call bit for bit in every
    type."""
    dtype = DTYPES[dt]
    g = _graph("N")
    plan, V, R = g.plan, g.V, g.Vc
    code, slope = ACT["leaky"]
    Qc, Kc, Gc = (fc.ints((R, H), 4, 40 + H + i, dtype) for i in range(3))
    nw = _native.mask_words(H, code)
    in_norm, out_norm = plan.norms(agg)
    n_part = max(plan.dst.n_slots, plan.src.n_slots, 1) * H
    what = f"edge N {dt} H={H} {agg}"
    deg = plan.in_degree_f()[ROWS.to(DEV)]

    def body(p):
        Q, K, G = (g.node_in(p, t) for t in (Qc, Kc, Gc))
        S = p.out(V, H, dtype)
        mask = pc.Out((g.E, nw), torch.int64, DEV, 0, 0) if nw else None
        part, part_s = (pc.Out((1, n_part), torch.float32, DEV, 0, 0) for _ in range(2))
        m = None if mask is None else mask.view.view(-1)
        _native.edge_agg_fwd(plan.dst, Q, K, in_norm, out_norm, agg, code, slope, S, part.view[0], m)
        out = {"S": S}
        forms = [("recompute", None, False)] + ([("mask", m, False), ("dual", m, True)] if m is not None else [])
        for name, mk, dual in forms:
            dQ, dK = p.out(V, H, dtype), p.out(V, H, dtype)
            if dual:
                ga, bagg = G, agg
                if agg == "mean":       # as conv.edge_backward: the one-launch form runs SUM on g = G / deg
                    gd = torch.div(Gc.to(DEV), deg, out=torch.zeros((R, H), dtype=dtype, device=DEV))
                    ga, bagg = g.node_in(p, gd), "sum"
                b_in, b_out = plan.norms(bagg)
                _native.edge_agg_bwd(plan.dst, plan.src, ga, mk, b_in, b_out, bagg, code, slope, dQ, dK, part.view[0],
                                     part_s.view[0])
            else:
                Gm = p.out(V, H, dtype) if agg == "mean" else None
                qk = (None, None) if mk is not None else (Q, K)
                _native.edge_agg_bwd_dst(plan.dst, qk[0], qk[1], G, in_norm, out_norm, agg, code, slope, dQ, Gm,
                                         part.view[0], mk)
                _native.edge_agg_bwd_src(plan.src, qk[1], qk[0], G if Gm is None else Gm, out_norm, in_norm, agg, code,
                                         slope, dK, part.view[0], mk)
                out[f"Gm {name}"] = Gm
            out[f"dQ {name}"], out[f"dK {name}"] = dQ, dK
        if mask is not None:
            mask.check_written(what + " mask")
            mask.check_outside(what + " mask")
            out["mask"] = mask.view
        part.check_outside(what + " partial")
        part_s.check_outside(what + " partial_s")
        return out

    live = g.live()
    p, far = _both(arenas, body, what, 16, None if dt == "f32" else dtype,
                   {k: live for k in ("Gm recompute", "Gm mask")})
    exact = agg == "sum"
    refs = {}
    for prec in (torch.float64, torch.float32):
        a = [t.to(prec) for t in (Qc, Kc, Gc)]
        refs[prec] = (oracle.edge_agg_fwd(g.cs, g.cd, R, a[0], a[1], agg, "leaky", xc.SLOPE),) + \
            tuple(oracle.edge_agg_bwd(g.cs, g.cd, R, a[0], a[1], a[2], agg, "leaky", xc.SLOPE))
    if exact or dt == "f32":            # 16-bit MEAN / SYM: the near call is the reference
        for name, view in far.items():
            if view is None or name == "mask" or name.startswith("Gm"):
                continue
            k = ("S", "dQ", "dK").index(name.split()[0])
            _check_node(p, g, view, refs[torch.float64][k], f"{what} {name}", exact, refs[torch.float32][k])
    for name in ("Gm recompute", "Gm mask"):        # G / deg, rounded once; rows without in-edges are don't-care
        if far.get(name) is not None:
            wGm = torch.div(Gc.to(DEV), deg, out=torch.zeros((R, H), dtype=dtype, device=DEV))
            p.check(far[name], wGm[g.has_in.to(DEV)], f"{what} {name}", rows=live)
    p.close(what)


def test_edge_forward_accumulate_far_nodes(arenas):
    """SIR_AGG_ACCUMULATE once (fp32, H = 64, SUM): S[v] += the sum, on an S that holds integers in every row —
    the rows without edges keep theirs."""
    g, H = _graph("N"), 64
    plan, V, R = g.plan, g.V, g.Vc
    code, slope = ACT["leaky"]
    Qc, Kc = (fc.ints((R, H), 4, 70 + i) for i in range(2))
    seed = fc.ints((V, H), 4, 72)
    what = "edge N accumulate"

    def body(p):
        Q, K = g.node_in(p, Qc), g.node_in(p, Kc)
        S = p.out(V, H, seed=seed)
        part = pc.Out((1, max(plan.dst.n_slots, 1) * H), torch.float32, DEV, 0, 0)
        _native.edge_agg_fwd(plan.dst, Q, K, None, None, "sum", code, slope, S, part.view[0], None, accumulate=True)
        part.check_outside(what + " partial")
        return {"S": S}

    p, far = _both(arenas, body, what)
    S64 = oracle.edge_agg_fwd(g.cs, g.cd, R, Qc.double(), Kc.double(), "sum", "leaky", xc.SLOPE)
    p.check(far["S"], _want(seed.double() + g.expand(S64)), what)
    p.close(what)


# ----------------------------------------------------------------------------- SIREConv (graphs N and E)
@pytest.mark.parametrize("agg", ["sum", "sym"])
@pytest.mark.parametrize("H", [4, 64])
@pytest.mark.parametrize("graph", ["N", "E"])
def test_sire_kernels_far(arenas, graph, H, agg):
    """sir_edge_e_agg_fwd / sir_edge_e_bwd with and without ``eidx``: on graph N Q, K, S, G are far (Eh, dE have
    E rows of the same wide buffer), on graph E Eh and dE are far in the edge position and, through ``eidx`` (a
    permutation of all E rows), in the gathered row.  SUM equals the fp64 oracle; SYM stays inside the parity
    bound of tests/test_econv_gpu.py and equals the near call bit for bit."""
    g = _graph(graph)
    plan, V, R, E = g.plan, g.V, g.Vc, g.E
    code, slope = ACT["leaky"]
    Qc, Kc, Gc = (fc.ints((R, H), 4, 80 + H + i) for i in range(3))
    Eh = fc.ints((E, H), 4, 83 + H)                     # the caller's edge order
    nw = _native.mask_words(H, code)
    in_norm, out_norm = plan.norms(agg)
    eid32 = plan.dst.eid.to(torch.int32)
    what = f"sire {graph} H={H} {agg}"

    def body(p):
        Q, K, G = (g.node_in(p, t) for t in (Qc, Kc, Gc))
        out = {}
        for form, rows, eidx in (("eidx", Eh, eid32), ("none", Eh[g.eid], None)):
            Ev = p.full(rows)
            S, dE = p.out(V, H), p.out(E, H)
            mask = pc.Out((E, nw), torch.int64, DEV, 0, 0)
            part = pc.Out((1, max(plan.dst.n_slots, 1) * H), torch.float32, DEV, 0, 0)
            _native.edge_e_agg_fwd(plan.dst, Q, K, Ev, eidx, in_norm, out_norm, agg, code, slope, S, part.view[0],
                                   mask.view.view(-1))
            _native.edge_e_bwd(plan.dst, mask.view.view(-1), G, in_norm, out_norm, agg, code, slope, eidx, dE)
            mask.check_written(f"{what} {form} mask")
            mask.check_outside(f"{what} {form} mask")
            part.check_outside(f"{what} {form} partial")
            out.update({f"S {form}": S, f"dE {form}": dE, f"mask {form}": mask.view})
        return out

    p, far = _both(arenas, body, what, 16)
    refs = {}
    for prec in (torch.float64, torch.float32):
        Q, K, G, Ee = (t.to(prec) for t in (Qc, Kc, Gc, Eh))
        n_in, n_out = oracle.degree_norms(torch.bincount(g.cd, minlength=R), torch.bincount(g.cs, minlength=R), agg)
        c = (n_out[g.cs] * n_in[g.cd]).to(prec)[:, None]
        z = Q[g.cd] + K[g.cs] + Ee
        S = torch.zeros(R, H, dtype=prec).index_add_(0, g.cd, c * oracle.act_fwd(z, "leaky", xc.SLOPE))
        refs[prec] = (S, oracle.act_bwd(z, c * G[g.cd], "leaky", xc.SLOPE))
    r64, r32 = refs[torch.float64], refs[torch.float32]
    for form, order in (("eidx", None), ("none", g.eid)):
        _check_node(p, g, far[f"S {form}"], r64[0], f"{what} {form} S", agg == "sum", r32[0])
        w64, w32 = (r[1] if order is None else r[1][order] for r in (r64, r32))
        if agg == "sum":
            p.check(far[f"dE {form}"], _want(w64), f"{what} {form} dE")
        else:
            assert_parity(p.written(far[f"dE {form}"], f"{what} {form} dE").cpu(), w32, w64, PARITY, f"{what} {form} dE")
    p.close(what)


# ----------------------------------------------------------------------------- edge-materialised helpers
@pytest.mark.parametrize("F", [3, 64])
@pytest.mark.parametrize("graph", ["N", "E"])
def test_edge_materialised_helpers_far(arenas, graph, F):
    """sir_edge_gather_add, _gather_act, sir_segment_sum (plain with ``perm``, and with the SYM norms),
    sir_edge_broadcast, sir_segment_max and sir_segment_max_bwd: graph N makes Q, K, dS, S, Y, arg far, graph E the
    [E, F] operands Z, A, M, dZ, dM.  Integers: everything but the SYM forms equals the fp64 oracle; those stay
    inside the parity bound of tests/test_gpu_parity.py and equal the near call."""
    g = _graph(graph)
    plan, V, R, E = g.plan, g.V, g.Vc, g.E
    code, slope = ACT["leaky"]
    Qc, Kc, dSc = (fc.ints((R, F), 4, 90 + F + i) for i in range(3))
    Mc, dZc = fc.ints((E, F), 4, 93 + F)[g.eid], fc.ints((E, F), 4, 94 + F)[g.eid]      # dst-CSR order, as the kernels take them
    s_in, s_out = plan.norms("sym")
    n_slots = max(plan.dst.n_slots, plan.src.n_slots, 1) * F
    what = f"helpers {graph} F={F}"

    def body(p):
        Q, K, dS = (g.node_in(p, t) for t in (Qc, Kc, dSc))
        Mv, dZ = p.full(Mc), p.full(dZc)
        out = {n: p.out(E, F) for n in ("Z", "A", "dM", "dM sym", "dMax")}
        out.update({n: p.out(V, F) for n in ("dQ", "dK", "S sym", "Y")})
        out["arg"] = p.out(V, F, torch.int32)
        ws = [pc.Out((1, n_slots), dt, DEV, 0, 0) for dt in (torch.float32, torch.float32, torch.int32)]
        _native.edge_gather_add(plan.dst, Q, K, out["Z"])
        _native.edge_gather_act(plan.dst, Q, K, code, slope, out["A"])
        _native.segment_sum(plan.dst, dZ, out["dQ"], partial=ws[0].view[0])
        _native.segment_sum(plan.src, dZ, out["dK"], perm=plan.src.perm, partial=ws[0].view[0])
        _native.segment_sum(plan.dst, Mv, out["S sym"], s_in, s_out, False, partial=ws[0].view[0])
        _native.edge_broadcast(plan.dst, dS, out["dM"])
        _native.edge_broadcast(plan.dst, dS, out["dM sym"], s_in, s_out, False)
        _native.segment_max(plan.dst, Mv, out["Y"], out["arg"], ws[1].view[0], ws[2].view[0])
        _native.segment_max_bwd(plan.dst, out["arg"], dS, out["dMax"])
        for w in ws:
            w.check_outside(what + " workspace")
        return out

    p, far = _both(arenas, body, what, 16)
    cs, cd = g.cs[g.eid], g.cd[g.eid]                   # the compact graph in dst-CSR edge order
    Q, K, dS, Md, dZ = (t.double() for t in (Qc, Kc, dSc, Mc, dZc))
    wZ = Q[cd] + K[cs]
    p.check(far["Z"], _want(wZ), what + " gather_add")
    p.check(far["A"], _want(oracle.act_fwd(wZ, "leaky", xc.SLOPE)), what + " gather_act")
    zeros = torch.zeros(R, F, dtype=torch.float64)
    _check_node(p, g, far["dQ"], zeros.clone().index_add_(0, cd, dZ), what + " segment_sum", True)
    _check_node(p, g, far["dK"], zeros.clone().index_add_(0, cs, dZ), what + " segment_sum perm", True)
    p.check(far["dM"], _want(dS[cd]), what + " edge_broadcast")
    sym = {}
    for prec in (torch.float64, torch.float32):
        n_in, n_out = oracle.degree_norms(torch.bincount(cd, minlength=R), torch.bincount(cs, minlength=R), "sym")
        c = (n_out[cs] * n_in[cd]).to(prec)[:, None]
        sym[prec] = (torch.zeros(R, F, dtype=prec).index_add_(0, cd, c * Mc.to(prec)), c * dSc.to(prec)[cd])
    _check_node(p, g, far["S sym"], sym[torch.float64][0], what + " segment_sum sym", False, sym[torch.float32][0])
    assert_parity(p.written(far["dM sym"], what + " edge_broadcast sym").cpu(), sym[torch.float32][1],
                  sym[torch.float64][1], PARITY, what + " edge_broadcast sym")
    wY, warg = oracle.max_first_wins(cd, R, Md)         # arg: positions in dst-CSR order (ascending edge id per row)
    _check_node(p, g, far["Y"], wY, what + " segment_max", True)
    full_arg = torch.full((V, F), -1, dtype=torch.int32)
    full_arg[torch.arange(V) if g.rows is None else g.rows] = warg.to(torch.int32)
    p.check(far["arg"], full_arg, what + " segment_max arg")
    wdMax = torch.zeros(E, F, dtype=torch.float64)
    r, f = torch.nonzero(warg >= 0, as_tuple=True)
    wdMax[warg[r, f], f] = dS[r, f]
    p.check(far["dMax"], _want(wdMax), what + " segment_max_bwd")
    p.close(what)


# ----------------------------------------------------------------------------- row-wise passes
_DATA = {}


def _ints(n, seed, dtype=torch.float32, rows=M):
    """Seeded integers in [-4, 4], [rows, n] (cached: the tests of one width share them)."""
    key = (rows, n, seed, dtype)
    if key not in _DATA:
        _DATA[key] = fc.ints((rows, n), 4, seed, dtype)
    return _DATA[key]


DROP = (0x5EEDFACE12345, 0.5)       # p = 0.5: the scale 1 / (1 - p) = 2 keeps integers exact
_M32 = 0xFFFFFFFF


def _keep(n, rows=M, drop=DROP):
    """bool [rows, n]: the keep bits of an [rows, n] block at col0 = 0 — sirgcn.dropedge's host restatement of the
    counter hash (csrc/sirconv_dropout.h: drop_row_hash, drop_keep) extended to columns.  The bit of row r is the
    hash of r itself, whatever r * ld is."""
    key = ("keep", rows, n, drop)
    if key not in _DATA:
        seed, p = drop
        thr = drop_threshold(p)
        s0, s1 = seed & _M32, ((seed >> 32) ^ 0x6A09E667) & _M32
        r = torch.arange(rows, dtype=torch.int64)
        rh = _fmix(((r * 0x9E3779B1) & _M32) ^ s0)              # the row's high word is 0: rows < 2^32
        c = (torch.arange(n, dtype=torch.int64) * 0xCC9E2D51 + s1) & _M32
        _DATA[key] = _fmix(rh[:, None] ^ c[None, :]) >= thr
    return _DATA[key]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt,N", [("f32", 4), ("f32", 64), ("bf16", 64), ("f16", 4)])
def test_resid_act_far(arenas, dt, N, order):
    """sir_resid_act_fwd / _bwd: Y, R, D, D2, out, dY, dR far in all M rows, integers: equal to the fp64 oracle."""
    dtype = DTYPES[dt]
    code, slope = ACT["leaky"]
    Y, R, D, D2 = (_ints(N, 100 + i) for i in range(4))
    Y = Y.to(dtype)
    what = f"resid_act {dt} N={N} order={order}"

    def body(p):
        Yv, Rv, Dv, D2v = (p.full(t) for t in (Y, R, D, D2))
        out, dY, dR = p.out(M, N), p.out(M, N, dtype), p.out(M, N)
        _native.resid_act_fwd(Yv, Rv, code, slope, order, out)
        _native.resid_act_bwd(Dv, Yv, Rv if order == 0 else None, code, slope, order, dY, dR, D2=D2v)
        return {"out": out, "dY": dY, "dR": dR}

    p, far = _both(arenas, body, what, 8, None if dt == "f32" else dtype)
    y, r, g = Y.double(), R.double(), D.double() + D2.double()
    z = y + r if order == 0 else y
    p.check(far["out"], _want(oracle.act_fwd(z, "leaky", xc.SLOPE) + (0 if order == 0 else r)), what + " out")
    wdY = oracle.act_bwd(z, g, "leaky", xc.SLOPE)
    p.check(far["dY"], _want(wdY, dtype), what + " dY")
    p.check(far["dR"], _want(wdY if order == 0 else g), what + " dR")
    p.close(what)


@pytest.mark.parametrize("dt,N", [("f32", 4), ("f32", 64), ("bf16", 64), ("f16", 4)])
def test_drop_act_and_dropout_far(arenas, dt, N):
    """sir_drop_act_fwd / _bwd (out = act(dropout(Y)) + R, R and out in Y's type) and sir_dropout_apply in place,
    far in all M rows: the mask of row r is the host restatement's hash of r; integers and p = 0.5, so the fp64
    composition on that mask is exact."""
    dtype = DTYPES[dt]
    code, slope = ACT["leaky"]
    Y, R, D, X = (_ints(N, 110 + i, dtype) for i in range(4))
    keep = _keep(N)
    what = f"drop_act {dt} N={N}"

    def body(p):
        Yv, Rv, Dv = (p.full(t) for t in (Y, R, D))
        out, dY = p.out(M, N, dtype), p.out(M, N, dtype)
        Xv = p.out(M, N, dtype, seed=X)
        _native.drop_act_fwd(Yv, Rv, code, slope, out, DROP)
        _native.drop_act_bwd(Dv, Yv, code, slope, dY, DROP)
        _native.dropout_apply(Xv, DROP)
        return {"out": out, "dY": dY, "X": Xv}

    p, far = _both(arenas, body, what, 8, None if dt == "f32" else dtype)
    scale = keep.double() * 2
    z = Y.double() * scale
    p.check(far["out"], _want(oracle.act_fwd(z, "leaky", xc.SLOPE) + R.double(), dtype), what + " out")
    p.check(far["dY"], _want(oracle.act_bwd(z, D.double(), "leaky", xc.SLOPE) * scale, dtype), what + " dY")
    p.check(far["X"], _want(X.double() * scale, dtype), what + " dropout_apply")
    p.close(what)


@pytest.mark.parametrize("N", [4, 64])
def test_col_sum_far(arenas, N):
    """sir_col_sum of a far [M, N] view (it takes N % 4 == 0 only; integers: |sum| < 2^24, exact in any order)."""
    X = _ints(N, 120)
    a = _open(arenas, torch.float32)
    got = _native.col_sum(a.put(X, fc.COLS[1]))
    want = _want(X.double().sum(0)).to(DEV)
    assert torch.equal(got, want), f"col_sum N={N}: {int((got != want).sum())} columns differ"
    assert torch.equal(got, _native.col_sum(X.to(DEV)))
    a.close(f"col_sum N={N}")


# ----------------------------------------------------------------------------- norms
def _randn(n, seed, rows=M):
    key = ("randn", rows, n, seed)
    if key not in _DATA:
        _DATA[key] = torch.randn(rows, n, generator=torch.Generator().manual_seed(seed))
    return _DATA[key]


TIE = 1e-4


def _params(n, seed, shifts):
    """Seeded [n] parameters, uniform in [shift, shift + 1)."""
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand(n, generator=gen) + sh for sh in shifts]


def _untie(dY, pre64):
    """dY with a zero wherever the fp64 norm output (the activation's input) lies within TIE of 0.  LeakyReLU' jumps
    there: a kernel whose fp32 y (error ~1e-6 over a 1000-row graph) falls on the other side than the reference's
    moves that element's gradient by 0.75 |dY w / std| and, through the per-graph sums, a whole graph's dX — one
    such element among the 2 M of a far operand is 1e-3 of dX's norm, a hundred times the bound.  sigma' at exact
    and near ties is the business of tests/test_exact_gpu.py; here those ~130 gradients are zero, so either side
    gives the same result."""
    dY = dY.clone()
    dY[pre64.abs() < TIE] = 0
    return dY


def _norm_refs(fn, X, dY, R, params, keep):
    """(Y, dX, dparams...) of ``Y = dropout(leaky(fn(X, *params))) + R`` by autograd, in fp32 and fp64."""
    out = {}
    for prec in (torch.float32, torch.float64):
        x = X.to(prec).requires_grad_(True)
        ps = [t.to(prec).requires_grad_(True) for t in params]
        y = torch.nn.functional.leaky_relu(fn(x, *ps), xc.SLOPE)
        if keep is not None:
            y = y * (keep.to(prec) * 2)
        y = y + R.to(prec)
        grads = torch.autograd.grad(y, [x] + ps, dY.to(prec))
        out[prec] = (y.detach(),) + tuple(grads)
    return out


def _parity(p, far, refs, names, what):
    for k, name in enumerate(names):
        got = far[name]
        got = p.written(got, f"{what} {name}") if got.dim() == 2 and got.shape[0] == M else got
        assert_parity(got.cpu().float().reshape(refs[torch.float32][k].shape), refs[torch.float32][k],
                      refs[torch.float64][k], PARITY, f"{what} {name}")


@pytest.mark.parametrize("drop", [None, DROP], ids=["plain", "drop"])
@pytest.mark.parametrize("N", [3, 4])
def test_batch_norm_far(arenas, N, drop):
    """sir_batch_norm_stats, sir_batch_norm_act_fwd / _bwd and their _drop_ forms: X, R, Y, dY, dX far in all M
    rows.  Bit-equal to the near call, inside the bound of tests/test_nodenorm_gpu.py (assert_parity, 1e-5) of
    torch's composition, the dropout mask the host restatement's."""
    code, slope = ACT["leaky"]
    X, dY, R = (_randn(N, 130 + i) for i in range(3))
    w, b = _params(N, 133, (0.5, -0.5))
    eps = 1e-5
    what = f"batch_norm N={N} {'drop' if drop else 'plain'}"
    fn = lambda x, ww, bb: torch.nn.functional.batch_norm(x, None, None, ww, bb, True, 0.0, eps)
    dY = _untie(dY, fn(X.double(), w.double(), b.double()))

    def body(p):
        Xv, dYv, Rv = (p.full(t) for t in (X, dY, R))
        Y, dX = p.out(M, N), p.out(M, N)
        mean, invstd = (torch.full((N,), NAN, device=DEV, dtype=torch.float64) for _ in range(2))
        dw, db = (torch.full((N,), NAN, device=DEV) for _ in range(2))
        wd, bd = w.to(DEV), b.to(DEV)
        _native.batch_norm_stats(Xv, eps, 0.1, None, None, mean, invstd, _native.batch_norm_work(M, N, DEV))
        _native.batch_norm_act_fwd(Xv, mean, invstd, wd, bd, code, slope, Rv, Y, drop)
        _native.batch_norm_act_bwd(Xv, dYv, mean, invstd, wd, bd, code, slope, True, dX, dw, db,
                                   _native.batch_norm_work(M, N, DEV), drop)
        return {"Y": Y, "dX": dX, "mean": mean, "invstd": invstd, "dw": dw, "db": db}

    p, far = _both(arenas, body, what, 8)
    refs = _norm_refs(fn, X, dY, R, (w, b), _keep(N) if drop else None)
    _parity(p, far, refs, ("Y", "dX", "dw", "db"), what)
    p.close(what)


@pytest.mark.parametrize("drop", [None, DROP], ids=["plain", "drop"])
@pytest.mark.parametrize("N", [3, 4])
def test_layer_norm_far(arenas, N, drop):
    """sir_layer_norm_act_fwd / _bwd and their _drop_ forms, far in all M rows (mean, rstd [M] and the slab
    partials are near): as the BatchNorm test."""
    code, slope = ACT["leaky"]
    X, dY, R = (_randn(N, 140 + i) for i in range(3))
    w, b = _params(N, 143, (0.5, -0.5))
    eps = 1e-5
    what = f"layer_norm N={N} {'drop' if drop else 'plain'}"
    fn = lambda x, ww, bb: torch.nn.functional.layer_norm(x, (N,), ww, bb, eps)
    dY = _untie(dY, fn(X.double(), w.double(), b.double()))

    def body(p):
        Xv, dYv, Rv = (p.full(t) for t in (X, dY, R))
        Y, dX = p.out(M, N), p.out(M, N)
        mean, rstd = (torch.full((M,), NAN, device=DEV) for _ in range(2))
        wd, bd = w.to(DEV), b.to(DEV)
        _native.layer_norm_act_fwd(Xv, wd, bd, eps, code, slope, Rv, Y, mean, rstd, drop)
        dw, db = _native.layer_norm_act_bwd(Xv, dYv, wd, bd, mean, rstd, code, slope, dX, drop)
        return {"Y": Y, "dX": dX, "mean": mean, "rstd": rstd, "dw": dw.contiguous(), "db": db.contiguous()}

    p, far = _both(arenas, body, what, 8)
    refs = _norm_refs(fn, X, dY, R, (w, b), _keep(N) if drop else None)
    _parity(p, far, refs, ("Y", "dX", "dw", "db"), what)
    p.close(what)


@pytest.mark.parametrize("form", ["plain", "act", "drop"])
@pytest.mark.parametrize("F", [3, 4])
def test_graph_norm_far(arenas, F, form):
    """sir_graph_norm_fwd / _bwd, the _act_ and the _act_drop_ forms over the batched offsets of far_cases (graph
    sizes 0, 1, 7, 64, 300, 1000 cycling: boundaries straddle every mark): X, R, Y, dY, dX far in the node rows; the
    [B, F] statistics and partials stay near (stated, not tested).  Bit-equal to the near call, inside the golden
    test's bound (1e-5, tests/test_gpu_parity.py) of the fp64 oracle."""
    code, slope = ACT["leaky"]
    off, sizes = fc.batch_offsets()
    B = len(sizes)
    X, dY, R = (_randn(F, 150 + i) for i in range(3))
    w, b, ms = _params(F, 153, (0.5, -0.5, 0.5))
    eps = 1e-5
    drop = DROP if form == "drop" else None
    what = f"graph_norm F={F} {form}"
    offd = off.to(DEV)
    nz = [n for n in sizes if n > 0]
    if form != "plain":
        dY = _untie(dY, oracle.graph_norm_fwd(X.double(), nz, w.double(), b.double(), ms.double(), eps)[0])

    def body(p):
        Xv, dYv = p.full(X), p.full(dY)
        Rv = p.full(R) if form != "plain" else None
        Y, dX = p.out(M, F), p.out(M, F)
        mean, std, pw, pb, pms = (torch.full((B, F), NAN, device=DEV) for _ in range(5))
        wd, bd, msd = w.to(DEV), b.to(DEV), ms.to(DEV)
        if form == "plain":
            _native.graph_norm_fwd(offd, Xv, wd, bd, msd, eps, Y, mean, std)
            _native.graph_norm_bwd(offd, Xv, dYv, wd, msd, mean, std, dX, pw, pms, pb)
        else:
            _native.graph_norm_act_fwd(offd, Xv, wd, bd, msd, eps, code, slope, Rv, Y, mean, std, drop)
            _native.graph_norm_act_bwd(offd, Xv, dYv, wd, bd, msd, mean, std, code, slope, dX, pw, pms, pb, drop)
        live = (torch.tensor(sizes) > 0).to(DEV)
        return {"Y": Y, "dX": dX, "mean": mean[live], "std": std[live], "dw": pw[live].sum(0), "db": pb[live].sum(0),
                "dms": pms[live].sum(0)}

    p, far = _both(arenas, body, what, 8)
    refs = {}
    for prec in (torch.float32, torch.float64):
        x = X.to(prec).requires_grad_(True)
        ps = [t.to(prec).requires_grad_(True) for t in (w, b, ms)]
        y = oracle.graph_norm_fwd(x, nz, ps[0], ps[1], ps[2], eps)[0]
        if form != "plain":
            y = torch.nn.functional.leaky_relu(y, xc.SLOPE)
            if drop is not None:
                y = y * (_keep(F).to(prec) * 2)
            y = y + R.to(prec)
        refs[prec] = (y.detach(),) + tuple(torch.autograd.grad(y, [x] + ps, dY.to(prec)))
    _parity(p, far, refs, ("Y", "dX", "dw", "db", "dms"), what)
    p.close(what)


# ----------------------------------------------------------------------------- graph readout
@pytest.mark.parametrize("dt,F", [("f32", 3), ("f32", 64), ("bf16", 64), ("f16", 4)])
def test_readout_far(arenas, dt, F):
    """sir_graph_pool_fwd / _bwd (sum, mean, max) over the batched offsets: X and dX far in the node rows, P, dP and
    arg [B, F] near.  Integers / 4 as tests/readout_cases.py: sum and max equal the fp64 restatement; the mean (one
    division) equals the near call bit for bit."""
    dtype = DTYPES[dt]
    off, sizes = fc.batch_offsets()
    B = len(sizes)
    n = torch.tensor(sizes)
    gid = torch.repeat_interleave(torch.arange(B), n)
    X = (_ints(F, 160) * 2 / 4).to(dtype)               # integers in [-8, 8] / 4
    dP = (fc.ints((B, F), 8, 161) / 4).to(dtype)
    offd = off.to(DEV)
    what = f"readout {dt} F={F}"
    live = (n > 0).to(DEV)

    def body(p):
        Xv = p.full(X)
        out = {}
        for op, code in (("sum", _native.POOL_SUM), ("mean", _native.POOL_MEAN), ("max", _native.POOL_MAX)):
            P = torch.full((B, F), NAN, device=DEV, dtype=dtype)
            arg = torch.full((B, F), -2, device=DEV, dtype=torch.int32) if op == "max" else None
            dX = p.out(M, F, dtype)
            _native.graph_pool_fwd(offd, Xv, code, P, arg)
            _native.graph_pool_bwd(offd, dP.to(DEV), code, dX, arg)
            out.update({f"P {op}": P, f"dX {op}": dX})
            if arg is not None:
                out["arg"] = arg[live]
        return out

    p, far = _both(arenas, body, what, 4, None if dt == "f32" else dtype)
    x64 = X.double()
    wsum = torch.zeros(B, F, dtype=torch.float64).index_add_(0, gid, x64)
    assert torch.equal(far["P sum"], _want(wsum, dtype).to(DEV)), what + " P sum"
    p.check(far["dX sum"], dP[gid], what + " dX sum")
    idx = gid[:, None].expand(M, F)
    wmax = torch.zeros(B, F, dtype=torch.float64).scatter_reduce(0, idx, x64, reduce="amax", include_self=False)
    assert torch.equal(far["P max"], _want(wmax, dtype).to(DEV)), what + " P max"
    rel = (torch.arange(M) - off[:-1][gid])[:, None].expand(M, F)       # the first maximal row within its graph wins
    warg = torch.full((B, F), M, dtype=torch.int64).scatter_reduce(0, idx, torch.where(x64 == wmax[gid], rel, M),
                                                                   reduce="amin")
    assert torch.equal(far["arg"].long().cpu(), warg[n > 0]), what + " arg"
    p.check(far["dX max"], torch.where(rel == warg[gid], dP[gid], torch.zeros((), dtype=dtype)), what + " dX max")
    p.written(far["dX mean"], what + " dX mean")
    p.close(what)


# ----------------------------------------------------------------------------- label propagation (graph N)
@pytest.mark.parametrize("post", ["clamp", "fix"])
@pytest.mark.parametrize("F", [3, 64])
def test_label_prop_step_far(arenas, F, post):
    """sir_label_prop_step on graph N (SUM, alpha = beta = 1/2 on integers: exact), one Clamp run and one FixRows
    run: Y, Y0, Yfix and out far in all M rows — a row without edges still gets post(beta * Y0)."""
    g = _graph("N")
    plan, R = g.plan, g.Vc
    Y, Y0, Yfix = (_ints(F, 170 + i) for i in range(3))
    fixed = (torch.arange(M) % 3 == 0)
    lo, hi = -1.5, 2.0
    what = f"label_prop F={F} {post}"

    def body(p):
        Yv, Y0v = p.full(Y), p.full(Y0)
        out = p.out(M, F)
        part = pc.Out((1, max(plan.dst.n_slots, 1) * F), torch.float32, DEV, 0, 0)
        if post == "clamp":
            _native.label_prop_step(plan.dst, Yv, Y0v, None, "sum", 0.5, 0.5, out, _native.LP_POST_CLAMP, lo, hi,
                                    partial=part.view[0])
        else:
            _native.label_prop_step(plan.dst, Yv, Y0v, None, "sum", 0.5, 0.5, out, _native.LP_POST_FIX,
                                    fixed=fixed.to(DEV, torch.uint8), Yfix=p.full(Yfix), partial=part.view[0])
        part.check_outside(what + " partial")
        return {"out": out}

    p, far = _both(arenas, body, what)
    S = torch.zeros(R, F, dtype=torch.float64).index_add_(0, g.cd, Y.double()[g.src])
    want = 0.5 * Y0.double()
    want[ROWS] += 0.5 * S
    want = want.clamp(lo, hi) if post == "clamp" else torch.where(fixed[:, None], Yfix.double(), want)
    p.check(far["out"], _want(want), what)
    p.close(what)


# ----------------------------------------------------------------------------- GEMMs
# the smallest K, N each forced route accepts, and K = 128, N = 132: the persistent kernel with its fused dact
# epilogue (N > 128, K a multiple of the 32-wide chunk with 4, 8 or 16 chunks) on the block route
GEMM_KN = [(4, 4), (128, 132)]
SAMPLE = 4096


def _gemm_rows(K, N):
    """None (all rows) when K * N <= 64 * 64, else MARK_ROWS plus 4096 seeded random rows."""
    if K * N <= 64 * 64:
        return None
    extra = torch.randperm(M, generator=torch.Generator().manual_seed(K + N))[:SAMPLE]
    return torch.unique(torch.cat([ROWS, extra]))


def _check_gemm(p, view, A, Wt, add, rows, what, post=None):
    """C = A Wt (+ add) against fp64 on ``rows`` (None: all); with a sample, every row is written and finite."""
    if rows is not None:
        got = p.written(view, what)
        assert bool(torch.isfinite(got).all()), what + ": a row is not finite"
    a = A.double() if rows is None else A.double()[rows]
    want = a @ Wt.double() + (0 if add is None else add.double())
    if post is not None:
        want = post(want, rows)
    p.check(view, _want(want, view.dtype), what, rows=None if rows is None else rows.to(DEV))


@pytest.mark.parametrize("route", list(pg.GEMM_ROUTES))
@pytest.mark.parametrize("K,N", GEMM_KN)
def test_gemm_nt_far(arenas, K, N, route, monkeypatch):
    """sir_gemm_nt, _nt_dact, _nt_direct, _nt_direct2 on every route of the poison module's GEMM_ROUTES: A, the gate
    and C far in their M rows (the weights are near), integers: equal to fp64."""
    monkeypatch.setenv("SIR_GEMM_SMALL_ROWS", pg.GEMM_ROUTES[route])
    code, slope = ACT["leaky"]
    A, gate = _ints(K, 180), fc.ints((M, N), 2, 181 + N)
    W, W2, b = fc.ints((N, K), 4, 182 + K), fc.ints((N, K), 4, 183 + K), fc.ints((N,), 4, 184)
    rows = _gemm_rows(K, N)
    what = f"gemm {route} K={K} N={N}"

    def body(p):
        Av, gv = p.full(A), p.full(gate)
        Wd, W2d, bd = W.to(DEV), W2.to(DEV), b.to(DEV)
        packed = _native.gemm_pack(Wd)
        out = {"nt": p.out(M, N), "dact": p.out(M, N), "direct": p.out(M, N), "direct2": p.out(M, 2 * N)}
        _native.gemm_nt(Av, packed, bd, out=out["nt"])
        _native.gemm_nt_dact(Av, packed, gv, code, slope, out=out["dact"])
        _native.gemm_nt_direct(Av, Wd, False, bd, out=out["direct"])
        _native.gemm_nt_direct2(Av, Wd, W2d, False, bd, out=out["direct2"])
        return out

    p, far = _both(arenas, body, what, 8)
    _check_gemm(p, far["nt"], A, W.t(), b, rows, what + " gemm_nt")
    gated = lambda c, r: torch.where((gate if r is None else gate[r]).double() > 0, c, c * xc.SLOPE)
    _check_gemm(p, far["dact"], A, W.t(), None, rows, what + " gemm_nt_dact", gated)
    _check_gemm(p, far["direct"], A, W.t(), b, rows, what + " gemm_nt_direct")
    _check_gemm(p, far["direct2"], A, torch.cat([W, W2]).t(), torch.cat([b, torch.zeros(N)]), rows,
                what + " gemm_nt_direct2")
    p.close(what)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gemm_nt16_far(arenas, dt):
    """sir_gemm_nt16 at its smallest shape (K = 128, N = 8): an fp32 A, its 16-bit copy Acopy and C far in their M
    rows; integers, all rows against fp64."""
    dtype = DTYPES[dt]
    K, N = 128, 8
    A, W, b = _ints(K, 180), fc.ints((N, K), 4, 190), fc.ints((N,), 4, 191)
    what = f"gemm_nt16 {dt}"

    def body(p):
        Av = p.full(A)
        C, Ac = p.out(M, N), p.out(M, K, dtype)
        _native.gemm_nt16(Av, _native.gemm_pack16(W.to(DEV), dtype), b.to(DEV), torch.float32, acopy=Ac, out=C)
        return {"C": C, "Acopy": Ac}

    p, far = _both(arenas, body, what, 4, dtype)
    _check_gemm(p, far["C"], A, W.t(), b, None, what)
    p.check(far["Acopy"], A.to(dtype), what + " Acopy")
    p.close(what)


@pytest.mark.parametrize("route", list(pg.GEMM_ROUTES))
def test_gemm_tn_far(arenas, route, monkeypatch):
    """sir_gemm_tn and sir_gemm_tn16 with R = M: A and B far along the contracted rows (C, the column sums and the
    workspace are near).  Integers: every sum stays below 2^24, so C = A^T B and colsum equal fp64."""
    monkeypatch.setenv("SIR_GEMM_SMALL_ROWS", pg.GEMM_ROUTES[route])
    Mc, Nc = 4, 4
    A, B = _ints(Mc, 180), _ints(Nc, 195)
    wC, wcs = _want(A.double().t() @ B.double()).to(DEV), _want(A.double().sum(0)).to(DEV)
    for dt in ("f32", "bf16", "f16"):
        dtype = DTYPES[dt]
        what = f"gemm_tn {route} {dt}"
        p = Far(arenas, 4, None if dt == "f32" else dtype)
        Av, Bv = p.full(A.to(dtype)), p.full(B.to(dtype))
        C, cs = pc.Out((Mc, Nc), torch.float32, DEV), pc.Out((1, Mc), torch.float32, DEV, 0, 0)
        pg._tn_call("sir_gemm_tn" if dt == "f32" else "sir_gemm_tn16", Av, Bv, C.view, cs.view[0],
                    None if dt == "f32" else dtype)
        C.check(wC, what)
        cs.check(wcs[None], what + " colsum")
        p.close(what)


# ----------------------------------------------------------------------------- max path and per-edge MLP (graph N)
MLP_SHAPES = [(4, 4), (64, 8)]


def _mlp_case(g, H, O):
    R = g.Vc
    Q, K, dY = fc.ints((R, H), 4, 200 + H), fc.ints((R, H), 4, 201 + H), fc.ints((R, O), 4, 202 + O)
    W, b = fc.ints((O, H), 2, 203 + H + O), fc.ints((O,), 4, 204 + O)
    return Q, K, W, b, dY


def _full_dy(g, dY):
    """dY [V, O] near (the Python layer makes it contiguous anyway): NaN in the rows without in-edges."""
    full = torch.full((g.V, dY.shape[1]), NAN)
    idx = torch.nonzero(g.has_in).flatten()
    full[g.rows[idx]] = dY[idx]
    return full.to(DEV)


@pytest.mark.parametrize("H,O", MLP_SHAPES)
def test_max_path_far_nodes(arenas, H, O, monkeypatch):
    """The max forward (sir_edge_mlp_fwd; sir_edge_mlp_fwd_st on bf16 / fp16 rows) and every backward route within
    its limits (sir_edge_max_bwd_sparse — V * O < 2^31 holds, O is small —, sir_edge_max_bwd_dst / _src,
    sir_max_dw_qk, sir_max_dw_rows, the edge-materialised helpers) on graph N: Q, K, Y, arg, dQ, dK far in their rows
    (dY is made contiguous by the Python layer, dW_R / db_R are near).  Equal to the first-wins fp64 oracle."""
    g = _graph("N")
    plan, V, R = g.plan, g.V, g.Vc
    code, slope = ACT["leaky"]
    Qc, Kc, W, b, dYc = _mlp_case(g, H, O)
    dYd = _full_dy(g, dYc)
    monkeypatch.setattr(edgemlp, "STREAM", False)
    what = f"max N H={H} O={O}"
    routes = [(r, sw) for r, (sw, applies) in pg.xg.MAX_ROUTES.items() if applies(H, O, V)]
    assert len(routes) >= 4

    def body(p):
        Q, K = g.node_in(p, Qc), g.node_in(p, Kc)
        Wd, bd = W.to(DEV), b.to(DEV)
        Y, arg = p.out(V, O), p.out(V, O, torch.int32)
        edgemlp._fwd(plan, Q, K, Wd, bd, "max", code, slope, _native.ACT_IDENTITY, Y, arg)
        out = {"Y": Y, "arg": arg}
        for route, switches in routes:
            for k, v in switches.items():
                monkeypatch.setattr(edgemlp.EdgeMaxLinear, k, v)
            dQ, dK = p.out(V, H), p.out(V, H)
            dW, db = edgemlp.max_linear_backward(plan, Q, K, Wd, arg, dYd, code, slope, dQ, dK)
            out.update({f"dQ {route}": dQ, f"dK {route}": dK, f"dW {route}": dW.contiguous(), f"db {route}": db.contiguous()})
        return out

    p, far = _both(arenas, body, what, 16)
    Q, K, Wd, bb, dY = (t.double() for t in (Qc, Kc, W, b, dYc))
    z = Q[g.cd] + K[g.cs]
    a = oracle.act_fwd(z, "leaky", xc.SLOPE)
    wY, warg = oracle.max_first_wins(g.cd, R, a @ Wd.t() + bb)          # arg: the caller's edge ids
    dM = torch.zeros(g.E, O, dtype=torch.float64)
    r, f = torch.nonzero(warg >= 0, as_tuple=True)
    dM[warg[r, f], f] = dY[r, f]
    dz = oracle.act_bwd(z, dM @ Wd, "leaky", xc.SLOPE)
    zeros = torch.zeros(R, H, dtype=torch.float64)
    _check_node(p, g, far["Y"], wY, what + " Y", True)
    pos = p.written(far["arg"], what + " arg").long()
    ids = torch.where(pos >= 0, plan.dst.eid[pos.clamp_min(0)], pos).cpu()
    want_ids = torch.full((V, O), -1, dtype=torch.int64)
    want_ids[g.rows] = warg
    assert torch.equal(ids, want_ids), what + " arg"
    for route, _ in routes:
        _check_node(p, g, far[f"dQ {route}"], zeros.clone().index_add_(0, g.cd, dz), f"{what} {route} dQ", True)
        _check_node(p, g, far[f"dK {route}"], zeros.clone().index_add_(0, g.cs, dz), f"{what} {route} dK", True)
        assert torch.equal(far[f"dW {route}"].cpu(), _want(dM.t() @ a)), f"{what} {route} dW_R"
        assert torch.equal(far[f"db {route}"].cpu(), _want(dM.sum(0))), f"{what} {route} db_R"
    p.close(what)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_max_forward_16bit_far_nodes(arenas, dt):
    """sir_edge_mlp_fwd_st: 16-bit Q, K far in the 2-byte arena, fp32 Y and int32 arg far in the 4-byte arena."""
    dtype = DTYPES[dt]
    g, (H, O) = _graph("N"), MLP_SHAPES[1]
    plan, V, R = g.plan, g.V, g.Vc
    code, slope = ACT["leaky"]
    Qc, Kc, W, b, _ = _mlp_case(g, H, O)
    what = f"max N {dt} H={H} O={O}"

    def body(p):
        Q, K = g.node_in(p, Qc.to(dtype)), g.node_in(p, Kc.to(dtype))
        Y, arg = p.out(V, O), p.out(V, O, torch.int32)
        edgemlp._fwd_st(plan, Q, K, W.to(DEV), b.to(DEV), code, slope, Y, arg)
        return {"Y": Y, "arg": arg}

    p, far = _both(arenas, body, what, 4, dtype)
    a = oracle.act_fwd(Qc.double()[g.cd] + Kc.double()[g.cs], "leaky", xc.SLOPE)
    wY, warg = oracle.max_first_wins(g.cd, R, a @ W.double().t() + b.double())
    _check_node(p, g, far["Y"], wY, what + " Y", True)
    pos = p.written(far["arg"], what + " arg").long()
    ids = torch.where(pos >= 0, plan.dst.eid[pos.clamp_min(0)], pos).cpu()
    want_ids = torch.full((V, O), -1, dtype=torch.int64)
    want_ids[g.rows] = warg
    assert torch.equal(ids, want_ids), what + " arg"
    p.close(what)


@pytest.mark.parametrize("H,F", MLP_SHAPES)
def test_seq_sigma_forward_far_nodes(arenas, H, F):
    """sir_edge_mlp_fwd in its sum family (ReLU, Linear, ReLU; SUM) on graph N: Q, K, S far in their rows."""
    g = _graph("N")
    plan, V, R = g.plan, g.V, g.Vc
    Qc, Kc, W, b, _ = _mlp_case(g, H, F)
    what = f"seq N H={H} F={F}"

    def body(p):
        Q, K = g.node_in(p, Qc), g.node_in(p, Kc)
        S = p.out(V, F)
        edgemlp._fwd(plan, Q, K, W.to(DEV), b.to(DEV), "sum", _native.ACT_RELU, 0.0, _native.ACT_RELU, S)
        return {"S": S}

    p, far = _both(arenas, body, what)
    m = torch.relu(torch.relu(Qc.double()[g.cd] + Kc.double()[g.cs]) @ W.double().t() + b.double())
    _check_node(p, g, far["S"], torch.zeros(R, F, dtype=torch.float64).index_add_(0, g.cd, m), what, True)
    p.close(what)


@pytest.mark.parametrize("H,F", MLP_SHAPES)
def test_seq_sigma_backward_far_nodes(arenas, H, F):
    """sir_edge_mlp_bwd_dst / _bwd_src (ReLU, Linear, ReLU; SUM) on graph N, called as EdgeMLPSum.backward calls
    them (which itself copies QK to a contiguous tensor): Q, K, G and dQK = [dQ | dK] far in their rows, the
    per-wave dW / db partials near.  Equal to the fp64 oracle."""
    g = _graph("N")
    plan, V, R = g.plan, g.V, g.Vc
    Qc, Kc, W, b, Gc = _mlp_case(g, H, F)
    act = _native.ACT_RELU
    what = f"seq bwd N H={H} F={F}"
    lib, P = _native.load(), _native._ptr
    d, s = plan.dst, plan.src
    FP, HP = (F + 31) // 32 * 32, (H + 7) // 8 * 8

    def body(p):
        Q, K, G = (g.node_in(p, t) for t in (Qc, Kc, Gc))
        Wd, bd = W.to(DEV), b.to(DEV)
        packed = edgemlp._pack(Wd)
        dQK = p.out(V, 2 * H)
        waves = lib.sir_edge_mlp_bwd_parts(d.n_items, H, F)
        wpart = torch.full((waves, FP * HP + FP), NAN, device=DEV)
        part = pc.Out((1, max(d.n_slots, s.n_slots, 1) * H), torch.float32, DEV, 0, 0)
        st = _native._stream(torch.device(DEV))
        code = _native.AGG["sum"]
        rc = lib.sir_edge_mlp_bwd_dst(P(d.rowptr), P(d.col), P(d.items), d.n_items, P(d.splits), d.n_splits, H, F, P(Q),
                                      Q.stride(0), P(K), K.stride(0), P(G), G.stride(0), None, None, code, act, 0.0, act,
                                      P(packed), P(Wd), P(bd), P(dQK), dQK.stride(0), None, P(part.view), P(wpart), st)
        _native._check(rc, lib)
        rc = lib.sir_edge_mlp_bwd_src(P(s.rowptr), P(s.col), P(s.items), s.n_items, P(s.splits), s.n_splits, H, F, P(K),
                                      K.stride(0), P(Q), Q.stride(0), P(G), G.stride(0), None, None, code, act, 0.0, act,
                                      P(packed), P(Wd), P(bd), P(dQK[:, H:]), dQK.stride(0), P(part.view), st)
        _native._check(rc, lib)
        part.check_outside(what + " partial")
        tot = _native.col_sum(wpart)
        return {"dQK": dQK, "dW": tot[:FP * HP].view(FP, HP)[:F, :H].contiguous(), "db": tot[FP * HP:FP * HP + F].contiguous()}

    p, far = _both(arenas, body, what)
    Q, K, Wd, bb, G = (t.double() for t in (Qc, Kc, W, b, Gc))
    z = Q[g.cd] + K[g.cs]
    a = torch.relu(z)
    pre = a @ Wd.t() + bb
    dm = torch.where(pre > 0, G[g.cd], torch.zeros((), dtype=torch.float64))
    dz = torch.where(z > 0, dm @ Wd, torch.zeros((), dtype=torch.float64))
    zeros = torch.zeros(R, H, dtype=torch.float64)
    want = torch.cat([zeros.clone().index_add_(0, g.cd, dz), zeros.clone().index_add_(0, g.cs, dz)], 1)
    _check_node(p, g, far["dQK"], want, what + " dQK", True)
    assert torch.equal(far["dW"].cpu(), _want(dm.t() @ a)), what + " dW"
    assert torch.equal(far["db"].cpu(), _want(dm.sum(0))), what + " db"
    p.close(what)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_stream_forward_far_nodes(arenas, dt, monkeypatch):
    """sir_edge_mlp_fwd_stream (max, and the sum family) and sir_edge_mlp_fwd_stream_st at the one width they take
    (H = 256) on graph N: Q, K, Y / S and arg far in their rows."""
    dtype = DTYPES[dt]
    g, (H, O) = _graph("N"), (256, 8)
    plan, V, R = g.plan, g.V, g.Vc
    code, slope = ACT["leaky"]
    Qc, Kc, W, b, _ = _mlp_case(g, H, O)
    monkeypatch.setattr(edgemlp, "STREAM", True)
    what = f"stream N {dt}"

    def body(p):
        Q, K = g.node_in(p, Qc.to(dtype)), g.node_in(p, Kc.to(dtype))
        Wd, bd = W.to(DEV), b.to(DEV)
        Y, arg = p.out(V, O), p.out(V, O, torch.int32)
        out = {"Y": Y, "arg": arg}
        if dt == "f32":
            edgemlp._fwd(plan, Q, K, Wd, bd, "max", code, slope, _native.ACT_IDENTITY, Y, arg)
            out["S"] = p.out(V, O)
            edgemlp._fwd(plan, Q, K, Wd, bd, "sum", _native.ACT_RELU, 0.0, _native.ACT_RELU, out["S"])
        else:
            edgemlp._fwd_st(plan, Q, K, Wd, bd, code, slope, Y, arg)
        return out

    p, far = _both(arenas, body, what, 8, None if dt == "f32" else dtype)
    z = Qc.double()[g.cd] + Kc.double()[g.cs]
    lin = lambda a: a @ W.double().t() + b.double()
    wY, warg = oracle.max_first_wins(g.cd, R, lin(oracle.act_fwd(z, "leaky", xc.SLOPE)))
    _check_node(p, g, far["Y"], wY, what + " Y", True)
    pos = p.written(far["arg"], what + " arg").long()
    ids = torch.where(pos >= 0, plan.dst.eid[pos.clamp_min(0)], pos).cpu()
    want_ids = torch.full((V, O), -1, dtype=torch.int64)
    want_ids[g.rows] = warg
    assert torch.equal(ids, want_ids), what + " arg"
    if "S" in far:
        wS = torch.zeros(R, O, dtype=torch.float64).index_add_(0, g.cd, torch.relu(lin(torch.relu(z))))
        _check_node(p, g, far["S"], wS, what + " S", True)
    p.close(what)
