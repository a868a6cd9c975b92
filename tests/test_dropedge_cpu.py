"""CPU-only checks of DropEdge (sir_plan_drop_edges / sir_plan_drop_workspace, added under ABI 17, and
sirgcn.DropEdge / drop_edges / drop_edge_keep): the symbols are exported and bound; every argument check is
synchronous, returns EINVAL and leaves a sir_last_error text that begins with the function name — no GPU work is
issued (the pointers below are host memory or NULL); the host restatement of the keep hash equals the C header's;
the kept counts lie in the binomial band; the host route and the SIRStack keyword behave as documented."""
import ctypes
import hashlib
import json
import math
import os
import shutil
import subprocess

import pytest
import torch
from torch import nn

import sirgcn
from sirgcn import DropEdge, Graph, _native, drop_edge_keep
from sirgcn.stacks import SIRStack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sir-gcn_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dropedge_keep.json")
EINVAL = 1
NAME = b"sir_plan_drop_edges: "
HASH_E = 1000
HASH_P = (0.05, 0.5, 1.0, 1e-12)
HASH_SEEDS = (0, 1234, 2 ** 40 + 7)


def _null():
    return ctypes.c_void_p(None)


_KEEP = [ctypes.create_string_buffer(256) for _ in range(3)]
_P1, _P2, _P3 = (ctypes.c_void_p((ctypes.addressof(b) + 15) & ~15) for b in _KEEP)
_DROP = _native.Dropout(1234, 0.3, None)
_NAN_DROP = _native.Dropout(1234, float("nan"), None)

PARENT = ("dst_rowptr", "dst_col", "dst_eid", "src_rowptr", "src_col", "src_eid", "src_perm")
OUT_EDGE = ("out_dst_col", "out_dst_eid", "out_src_col", "out_src_eid", "out_src_perm", "kept")
OUT_PLAN = ("out_dst_items", "out_dst_splits", "out_src_items", "out_src_splits")
OUT_ALWAYS = ("out_dst_rowptr", "out_src_rowptr", "counts")
ORDER = PARENT + ("E", "n_dst_rows", "n_src_rows", "chunk", "keep", "drop", "out_dst_rowptr", "out_dst_col",
                  "out_dst_eid", "out_dst_items", "out_dst_splits", "out_src_rowptr", "out_src_col", "out_src_eid",
                  "out_src_items", "out_src_splits", "out_src_perm", "kept", "counts", "workspace", "workspace_bytes",
                  "stream")
_DEFAULT = dict({k: _P1 for k in PARENT}, E=8, n_dst_rows=4, n_src_rows=4, chunk=256, keep=_P2, drop=None,
                workspace=_P3, workspace_bytes=1 << 40, stream=_null(),
                **{k: _P3 for k in OUT_EDGE + OUT_PLAN + OUT_ALWAYS})


def _call(lib, **kw):
    """The call with valid arguments (E = 8, 4 x 4 rows, a keep mask) and the given overrides.  Never made
    without an override that must be rejected: the defaults point at host memory."""
    a = dict(_DEFAULT)
    a.update(kw)
    return lib.sir_plan_drop_edges(*(a[k] for k in ORDER))


def _rejected(lib, text, **kw):
    assert kw, "the valid default call would launch"
    assert _call(lib, **kw) == EINVAL, kw
    err = lib.sir_last_error()
    assert err.startswith(NAME + text), (kw, err)


def test_symbols_and_version():
    lib = _native.load()
    assert _native.ABI_VERSION == 17 and lib.sir_abi_version() == 17
    for name, n_args in (("sir_plan_drop_edges", 29), ("sir_plan_drop_workspace", 3)):
        assert name in _native.SIGNATURES and hasattr(lib, name)
        assert len(_native.SIGNATURES[name][1]) == n_args
    assert len(ORDER) == 29
    assert hasattr(_native, "plan_drop_edges")
    for name in ("DropEdge", "drop_edges", "drop_edge_keep"):
        assert hasattr(sirgcn, name) and name in sirgcn.__all__
    assert hasattr(sirgcn.GraphPlan, "from_parts")


def test_workspace_is_positive_and_monotone_in_E():
    lib = _native.load()
    prev = 0
    for E in (0, 1, 255, 256, 257, 1025, 70001, 10 ** 6, 2 ** 31 - 2):
        w = lib.sir_plan_drop_workspace(64, 64, E)
        assert w > 0 and w >= prev, (E, w, prev)
        prev = w
    assert lib.sir_plan_drop_workspace(0, 0, 0) > 0
    assert lib.sir_plan_drop_workspace(10 ** 6, 64, 100) > lib.sir_plan_drop_workspace(64, 64, 100)
    for bad in ((-1, 4, 8), (4, -1, 8), (4, 4, -1), (4, 4, 2 ** 31 - 1), (2 ** 31 - 1, 4, 8)):
        assert lib.sir_plan_drop_workspace(*bad) == -1, bad


def test_argument_checks_are_synchronous_and_reported():
    lib = _native.load()
    n = _null()
    # exactly one keep source
    _rejected(lib, b"exactly one keep source", keep=_P2, drop=ctypes.byref(_DROP))
    _rejected(lib, b"exactly one keep source", keep=n, drop=None)
    _rejected(lib, b"dropout p is NaN", keep=n, drop=ctypes.byref(_NAN_DROP))
    for chunk in (0, -1):
        _rejected(lib, b"chunk must be", chunk=chunk)
    for k in ("E", "n_dst_rows", "n_src_rows"):
        _rejected(lib, b"negative size", **{k: -1})
    _rejected(lib, b"int32 plan", E=2 ** 31 - 1)
    _rejected(lib, b"int32 plan", E=2 ** 31)
    _rejected(lib, b"int32 plan", n_dst_rows=2 ** 31 - 1)
    _rejected(lib, b"edges need rows", n_dst_rows=0)
    _rejected(lib, b"edges need rows", n_src_rows=0)
    for k in PARENT:
        _rejected(lib, b"NULL parent CSR buffer", **{k: n})
    for k in OUT_EDGE:
        _rejected(lib, b"NULL output edge buffer", **{k: n})
    for k in OUT_PLAN:
        _rejected(lib, b"NULL items/splits", **{k: n})
    for k in OUT_ALWAYS:
        _rejected(lib, b"NULL output rowptr/counts", **{k: n})
        _rejected(lib, b"NULL output rowptr/counts", E=0, **{k: n})
    need = lib.sir_plan_drop_workspace(4, 4, 8)
    _rejected(lib, b"workspace too small", workspace_bytes=need - 1)
    _rejected(lib, b"workspace too small", workspace=n)
    _rejected(lib, b"workspace too small", workspace_bytes=0, keep=n, drop=ctypes.byref(_DROP))


# ------------------------------------------------------------------------------------ the hash
_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "sirconv_dropout.h"
// argv: E, then (seed, p) pairs; one line of '0' / '1' per pair: the keep bit of every edge id
int main(int argc, char** argv) {
    const long E = atol(argv[1]);
    for (int k = 2; k + 1 < argc; k += 2) {
        const sir::Drop d = sir::make_drop(atof(argv[k + 1]), strtoull(argv[k], nullptr, 10));
        for (long e = 0; e < E; ++e)
            putchar(!d.on() || sir::drop_keep(d, sir::drop_row_hash(d, e), 0) ? '1' : '0');
        putchar('\n');
    }
    return 0;
}
"""


def _combos():
    return [(seed, p) for seed in HASH_SEEDS for p in HASH_P]


def _bits(mask):
    return "".join("1" if b else "0" for b in mask.tolist())


def _c_hash_bits(tmp_path):
    """The header's bits from a stand-alone host program, or None without a HIP compiler."""
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        return None
    src = tmp_path / "keep_bits.cpp"
    src.write_text(_PROGRAM)
    exe = tmp_path / "keep_bits"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    args = [str(HASH_E)]
    for seed, p in _combos():
        args += [str(seed), repr(p)]
    out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    return out[:len(_combos())]


def test_drop_edge_keep_is_the_c_hash(tmp_path):
    """drop_edge_keep against make_drop / drop_row_hash / drop_keep of sirconv_dropout.h compiled for the host,
    and against the committed digests of that program's output (the only check without a compiler)."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    c_bits = _c_hash_bits(tmp_path)
    for j, (seed, p) in enumerate(_combos()):
        mine = _bits(drop_edge_keep(seed, HASH_E, p))
        rec = golden[f"{seed}:{p!r}"]
        assert mine.count("1") == rec["kept"], (seed, p, mine.count("1"), rec["kept"])
        assert hashlib.sha256(mine.encode()).hexdigest() == rec["sha256"], (seed, p)
        if c_bits is not None:
            assert mine == c_bits[j], (seed, p)
        if p == 1.0:
            assert mine.count("1") == 0
        if p == 1e-12:                      # thr = 1: only a hash of exactly 0 drops
            assert mine.count("1") >= HASH_E - 1
    assert drop_edge_keep(5, 0, 0.5).shape == (0,) and drop_edge_keep(5, 7, 0.0).all()
    with pytest.raises(ValueError):
        drop_edge_keep(5, 7, float("nan"))


def test_kept_count_band():
    """Binomial band: |kept - E(1 - p)| <= 4 sqrt(E p (1 - p)).  Measured: 70127 (p = 0.3, 0.9 sigma) and 95045
    (p = 0.05, 0.7 sigma) of 100000; seeds 1234 / 1235 at p = 0.5 agree on 49.80 % of the edges."""
    E = 100000
    for p in (0.3, 0.05):
        kept = int(drop_edge_keep(1234, E, p).sum())
        sigma = math.sqrt(E * p * (1 - p))
        print(f"p={p}: kept {kept} of {E}, {(kept - E * (1 - p)) / sigma:+.2f} sigma")
        assert abs(kept - E * (1 - p)) <= 4 * sigma, (p, kept)
    a, b = drop_edge_keep(1234, E, 0.5), drop_edge_keep(1235, E, 0.5)
    agree = float((a == b).float().mean())
    print(f"seeds 1234 / 1235 agree on {100 * agree:.2f} %")
    assert 0.48 <= agree <= 0.52, agree


# ------------------------------------------------------------------------------------ the host route
def _graph():
    gen = torch.Generator().manual_seed(3)
    src = torch.randint(0, 12, (200,), generator=gen)
    dst = torch.randint(0, 10, (200,), generator=gen)
    return Graph(src, dst, 12, [5, 4, 3]), torch.randn(200, 3, generator=gen)


def test_host_route():
    g, ef = _graph()
    src, dst = g.edges()
    de = DropEdge(0.4)
    torch.manual_seed(11)
    child, ef_ = de(g, ef)
    kept = de.last_kept
    keep = drop_edge_keep(de.last_seed, 200, 0.4)
    assert kept.dtype == torch.int64 and torch.equal(kept, torch.nonzero(keep).flatten())
    assert 0 < kept.numel() < 200
    cs, cd = child.edges()
    assert torch.equal(cs, src[keep]) and torch.equal(cd, dst[keep]) and torch.equal(ef_, ef[keep])
    assert child.num_nodes() == 12 and torch.equal(child.batch_num_nodes(), g.batch_num_nodes())
    assert isinstance(child, Graph) and child is not g
    # the same torch.manual_seed gives the same draw; consecutive calls differ
    torch.manual_seed(11)
    again = de(g)
    assert isinstance(again, Graph) and torch.equal(de.last_kept, kept)
    de(g)
    assert not torch.equal(de.last_kept, kept)
    # the functional form with an explicit mask
    c2, e2 = sirgcn.drop_edges(g, keep, ef)
    assert torch.equal(c2.edges()[0], src[keep]) and torch.equal(e2, ef[keep])
    assert torch.equal(sirgcn.drop_edges(g, keep.to(torch.uint8)).edges()[1], dst[keep])
    with pytest.raises(ValueError):
        sirgcn.drop_edges(g, keep[:-1])
    # the plan of the child is the plan of the compacted COO
    plan = sirgcn.get_plan(child, "cpu")
    ref = sirgcn.build_row_csr(dst[keep], src[keep], 12)
    assert torch.equal(plan.dst.rowptr, ref.rowptr) and torch.equal(plan.dst.eid, ref.eid)


def test_an_edges_object_is_accepted():
    """Anything get_plan takes: here an object with edges() and num_nodes() only."""
    class Edges:
        def edges(self):
            return torch.tensor([0, 1, 2, 2]), torch.tensor([1, 2, 0, 1])

        def num_nodes(self):
            return 3

    g = Edges()
    child = sirgcn.drop_edges(g, torch.tensor([1, 0, 1, 1], dtype=torch.uint8))
    assert isinstance(child, Graph) and child.num_nodes() == 3
    assert child.edges()[0].tolist() == [0, 2, 2] and child.edges()[1].tolist() == [1, 0, 1]
    torch.manual_seed(0)
    de = DropEdge(0.5)
    dropped = de(g)
    assert dropped.num_edges() == de.last_kept.numel() and dropped.batch_num_nodes().tolist() == [3]


def test_p_edge_values():
    g, ef = _graph()
    keep0 = DropEdge(0)
    assert keep0(g) is g
    out = keep0(g, ef)
    assert out[0] is g and out[1] is ef and keep0.last_kept is None
    child, ef_ = DropEdge(1)(g, ef)
    assert child.num_edges() == 0 and ef_.shape == (0, 3) and child.num_nodes() == 12
    assert torch.equal(child.batch_num_nodes(), g.batch_num_nodes())
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            DropEdge(bad)
    assert DropEdge().p == 0.5


# ------------------------------------------------------------------------------------ SIRStack
def test_stack_keyword():
    from cpu_stack_modules import GraphNorm, SIRConv
    g, _ = _graph()
    torch.manual_seed(5)
    a = SIRStack(SIRConv, 8, 2, nn.ReLU(), "sum", "zinc", norm_cls=GraphNorm)
    torch.manual_seed(5)
    b = SIRStack(SIRConv, 8, 2, nn.ReLU(), "sum", "zinc", norm_cls=GraphNorm, edge_dropout=0)
    assert list(a.state_dict()) == list(b.state_dict())
    assert isinstance(b.edge_drop, DropEdge) and b.edge_drop.p == 0 and not isinstance(b.edge_drop, nn.Module)
    X = torch.randn(12, 8)
    assert torch.equal(a(g, X), b(g, X))
    torch.manual_seed(5)
    c = SIRStack(SIRConv, 8, 2, nn.ReLU(), "sum", "zinc", norm_cls=GraphNorm, edge_dropout=0.25)
    assert c.edge_drop.p == 0.25 and list(c.state_dict()) == list(a.state_dict())
    # the dropped stack: every layer's conv on its own dropped graph, the norm on the original; eval mode too
    c.eval()
    torch.manual_seed(9)
    got = c(g, X)
    torch.manual_seed(9)
    h, de = X, DropEdge(0.25)
    for conv, norm in zip(c.convs, c.norms):
        h = torch.relu(norm(g, conv(de(g), h) + h))
    assert torch.equal(got, h) and not torch.equal(got, a(g, X))
