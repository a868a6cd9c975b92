"""CPU-only checks of the graph readout entry points (added under ABI 17): the symbols are exported and
bound, the sizing calls are functions of their arguments, every argument check is synchronous, returns
EINVAL and leaves a sir_last_error text that begins with the function name — no GPU work is issued (the
pointers below are host memory or NULL) — and the Python surface refuses what it must on the CPU."""
import ctypes

import pytest
import torch

import sirgcn
from sirgcn import Graph, _native

NEW = ("sir_graph_pool_fwd", "sir_graph_pool_bwd", "sir_graph_pool_work_floats", "sir_graph_pool_slab_rows")
EINVAL = 1
SUM, MEAN, MAX = 0, 1, 2
F32, BF16, F16 = 0, 1, 2


def _null():
    return ctypes.c_void_p(None)


def _buf():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def _fwd(lib, off, B, V, F, op, dtype, X, ldx, P, ldp, arg, work):
    return lib.sir_graph_pool_fwd(off, B, V, F, op, dtype, X, ldx, P, ldp, arg, work, _null())


def _bwd(lib, off, B, V, F, op, dtype, dP, ldg, arg, dX, lddx):
    return lib.sir_graph_pool_bwd(off, B, V, F, op, dtype, dP, ldg, arg, dX, lddx, _null())


def test_symbols_and_version():
    lib = _native.load()
    assert _native.ABI_VERSION == 17 and lib.sir_abi_version() == 17
    for name in NEW:
        assert name in _native.SIGNATURES and hasattr(lib, name)
    for name in ("graph_pool_fwd", "graph_pool_bwd", "graph_pool_work"):
        assert hasattr(_native, name)
    assert (_native.POOL_SUM, _native.POOL_MEAN, _native.POOL_MAX) == (SUM, MEAN, MAX)
    for name in ("SumPooling", "AvgPooling", "MaxPooling", "readout_nodes", "broadcast_nodes"):
        assert hasattr(sirgcn, name) and name in sirgcn.__all__
    for cls in (sirgcn.SumPooling, sirgcn.AvgPooling, sirgcn.MaxPooling):
        assert isinstance(cls(), torch.nn.Module) and not list(cls().parameters())


def test_sizing_calls():
    lib = _native.load()
    R = lib.sir_graph_pool_slab_rows()
    assert R == _native.POOL_SLAB_ROWS == 1024
    wf = lib.sir_graph_pool_work_floats
    # no graph can be longer than one slab while V <= R: no partials
    for op in (SUM, MEAN, MAX):
        assert wf(0, 3, 75, op) == 0
        assert wf(R, 1, 256, op) == 0
        assert wf(1600, 0, 300, op) == 0
    # B + V / R slab slots of F values (and F args for max); a function of its arguments alone
    assert wf(R + 1, 1, 256, SUM) == 2 * 256
    assert wf(R + 1, 1, 256, MAX) == 2 * 2 * 256
    assert wf(1600, 64, 300, MEAN) == 65 * 300
    assert wf(3 * R + 7, 1, 1, SUM) == 4
    assert wf(400000, 4, 256, MAX) == 2 * (4 + 390) * 256
    assert wf(400000, 4, 256, MAX) == wf(400000, 4, 256, MAX)
    for V, B, F, op in ((-1, 4, 4, SUM), (4, -1, 4, SUM), (4, 4, 0, SUM), (4, 4, 65537, SUM), (4, 4, 4, -1),
                        (4, 4, 4, 3)):
        assert wf(V, B, F, op) == -1


def test_no_graphs_is_a_no_op():
    lib = _native.load()
    n = _null()
    for op in (SUM, MEAN, MAX):
        for dt in (F32, BF16, F16):
            assert _fwd(lib, n, 0, 0, 75, op, dt, n, 75, n, 75, n, n) == 0
            assert _bwd(lib, n, 0, 0, 75, op, dt, n, 75, n, n, 75) == 0


def test_forward_argument_checks_are_synchronous_and_reported():
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    name = b"sir_graph_pool_fwd: "
    for F in (0, -4, 65537):
        assert _fwd(lib, p, 2, 8, F, SUM, F32, p, 1 << 17, p, 1 << 17, n, n) == EINVAL
        assert lib.sir_last_error().startswith(name + b"F must be in [1, 65536]")
    for B, V in ((-1, 8), (2, -1)):
        assert _fwd(lib, p, B, V, 8, SUM, F32, p, 8, p, 8, n, n) == EINVAL
        assert lib.sir_last_error().startswith(name + b"B and V")
    for ldx, ldp in ((7, 8), (8, 7)):
        assert _fwd(lib, p, 2, 8, 8, SUM, F32, p, ldx, p, ldp, n, n) == EINVAL
        assert lib.sir_last_error().startswith(name + b"leading")
    for op in (-1, 3, 9):
        assert _fwd(lib, p, 2, 8, 8, op, F32, p, 8, p, 8, p, n) == EINVAL
        assert lib.sir_last_error().startswith(name + b"op must be")
    for dt in (-1, 3):
        assert _fwd(lib, p, 2, 8, 8, SUM, dt, p, 8, p, 8, n, n) == EINVAL
        assert lib.sir_last_error().startswith(name + b"dtype must be")
    # NULL required buffers when there is work: off, X, P
    for a in range(3):
        args = [p, p, p]
        args[a] = n
        assert _fwd(lib, args[0], 2, 8, 8, MEAN, F32, args[1], 8, args[2], 8, n, n) == EINVAL
        assert lib.sir_last_error().startswith(name + b"NULL")
    assert _fwd(lib, p, 2, 8, 8, MAX, BF16, p, 8, p, 8, n, n) == EINVAL
    assert lib.sir_last_error().startswith(name + b"MAX needs arg")
    R = _native.POOL_SLAB_ROWS
    for op, arg in ((SUM, n), (MAX, p)):
        assert lib.sir_graph_pool_work_floats(R + 1, 2, 8, op) > 0
        assert _fwd(lib, p, 2, R + 1, 8, op, F16, p, 8, p, 8, arg, n) == EINVAL
        assert lib.sir_last_error().startswith(name + b"work needed")
    del keep


def test_backward_argument_checks_are_synchronous_and_reported():
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    name = b"sir_graph_pool_bwd: "
    for F in (0, -4, 65537):
        assert _bwd(lib, p, 2, 8, F, SUM, F32, p, 1 << 17, n, p, 1 << 17) == EINVAL
        assert lib.sir_last_error().startswith(name + b"F must be in [1, 65536]")
    for B, V in ((-1, 8), (2, -1)):
        assert _bwd(lib, p, B, V, 8, SUM, F32, p, 8, n, p, 8) == EINVAL
        assert lib.sir_last_error().startswith(name + b"B and V")
    for ldg, lddx in ((7, 8), (8, 7)):
        assert _bwd(lib, p, 2, 8, 8, SUM, F32, p, ldg, n, p, lddx) == EINVAL
        assert lib.sir_last_error().startswith(name + b"leading")
    for op in (-1, 3, 9):
        assert _bwd(lib, p, 2, 8, 8, op, F32, p, 8, p, p, 8) == EINVAL
        assert lib.sir_last_error().startswith(name + b"op must be")
    for dt in (-1, 3):
        assert _bwd(lib, p, 2, 8, 8, SUM, dt, p, 8, n, p, 8) == EINVAL
        assert lib.sir_last_error().startswith(name + b"dtype must be")
    for a in range(3):
        args = [p, p, p]
        args[a] = n
        assert _bwd(lib, args[0], 2, 8, 8, MEAN, F32, args[1], 8, n, args[2], 8) == EINVAL
        assert lib.sir_last_error().startswith(name + b"NULL")
    assert _bwd(lib, p, 2, 8, 8, MAX, F32, p, 8, n, p, 8) == EINVAL
    assert lib.sir_last_error().startswith(name + b"MAX needs arg")
    del keep


def _batched():
    e = torch.zeros(0, dtype=torch.int64)
    return sirgcn.batch([Graph(e, e, 3), Graph(e, e, 0), Graph(e, e, 5)])


def test_python_surface_on_the_cpu():
    g = _batched()
    assert g.num_nodes() == 8 and g.batch_size == 3
    pools = (sirgcn.SumPooling(), sirgcn.AvgPooling(), sirgcn.MaxPooling())
    # the row count is checked first, before the device
    for pool in pools:
        with pytest.raises(ValueError, match="8 leading rows"):
            pool(g, torch.zeros(7, 4))
        with pytest.raises(RuntimeError, match=r"needs a ROCm GPU tensor \(no CPU fallback\)"):
            pool(g, torch.zeros(8, 4))
    with pytest.raises(ValueError, match="op must be"):
        sirgcn.readout_nodes(g, torch.zeros(8, 4), "min")
    with pytest.raises(ValueError, match="3 leading rows"):
        sirgcn.broadcast_nodes(g, torch.zeros(8, 4))
    with pytest.raises(RuntimeError, match=r"needs a ROCm GPU tensor \(no CPU fallback\)"):
        sirgcn.broadcast_nodes(g, torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sirgcn.readout_nodes(g, torch.zeros(8), "mean")
