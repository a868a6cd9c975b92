"""CPU-only checks of sir_param_norms_* (the L1 / L2 parameter penalty): the symbols are exported and bound,
every argument check is synchronous with its code and text, empty work is a no-op, the workspace size is
monotone.  The validation reads HOST arrays; fake device addresses are never dereferenced."""
import ctypes

import sirgcn
from sirgcn import _native

NAMES = ("sir_param_norms_chunk", "sir_param_norms_max_tensors", "sir_param_norms_combine_threads",
         "sir_param_norms_work_floats", "sir_param_norms_fwd", "sir_param_norms_bwd")
EINVAL = 1


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _ptrs(vals):
    return _arr(ctypes.c_void_p, vals)


def _counts(vals):
    return _arr(ctypes.c_int64, vals)


def test_symbols_exported_and_bound():
    lib = _native.load()
    assert lib.sir_abi_version() == 17 and _native.ABI_VERSION == 17
    for name in NAMES:
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    CH, TM, CT = lib.sir_param_norms_chunk(), lib.sir_param_norms_max_tensors(), lib.sir_param_norms_combine_threads()
    assert CH > 0 and CH % 4 == 0 and TM >= 2 and CT >= 64
    assert _native.param_norms_chunk() == CH


def test_work_floats_monotone_and_positive():
    lib = _native.load()
    prev = 0
    for c in (0, 1, 2, 3, 7, 255, 256, 257, 4096, 1 << 20, 1 << 30):
        w = lib.sir_param_norms_work_floats(c)
        assert w > 0 and w >= prev and w >= 2 * c, c
        prev = w
    assert lib.sir_param_norms_work_floats(-1) == -1


def test_forward_argument_checks():
    lib = _native.load()
    n = ctypes.c_void_p(None)
    A = 0x10000                                   # a 16-byte aligned fake device address
    P, N = _ptrs([A, A + 64]), _counts([4, 8])
    w, o = ctypes.c_void_p(A + 4096), ctypes.c_void_p(A + 8192)

    def err(rc, needle):
        assert rc == EINVAL and needle in lib.sir_last_error() and b"sir_param_norms_fwd" in lib.sir_last_error(), \
            (rc, lib.sir_last_error())

    err(lib.sir_param_norms_fwd(P, N, -1, w, 64, o, n), b"T must be")
    err(lib.sir_param_norms_fwd(P, _counts([4, -8]), 2, w, 64, o, n), b"negative element count")
    err(lib.sir_param_norms_fwd(n, N, 2, w, 64, o, n), b"NULL host array")
    err(lib.sir_param_norms_fwd(P, n, 2, w, 64, o, n), b"NULL host array")
    err(lib.sir_param_norms_fwd(_ptrs([A, None]), N, 2, w, 64, o, n), b"NULL parameter")
    err(lib.sir_param_norms_fwd(_ptrs([A, A + 66]), N, 2, w, 64, o, n), b"4-B aligned")
    err(lib.sir_param_norms_fwd(P, N, 2, w, 3, o, n), b"work smaller")
    err(lib.sir_param_norms_fwd(P, N, 2, n, 64, o, n), b"work smaller")
    err(lib.sir_param_norms_fwd(P, N, 2, w, 64, n, n), b"out2")
    CH = lib.sir_param_norms_chunk()
    need = lib.sir_param_norms_work_floats(3)     # CH + 1 elements are 2 chunks, 4 more are a third
    err(lib.sir_param_norms_fwd(P, _counts([CH + 1, 4]), 2, w, need - 1, o, n), b"work smaller")


def test_backward_argument_checks():
    lib = _native.load()
    n = ctypes.c_void_p(None)
    A = 0x10000
    P, N, G = _ptrs([A, A + 68]), _counts([4, 8]), _ptrs([A + 256, A + 512])
    g = ctypes.c_void_p(A + 1024)

    def err(rc, needle):
        assert rc == EINVAL and needle in lib.sir_last_error() and b"sir_param_norms_bwd" in lib.sir_last_error(), \
            (rc, lib.sir_last_error())

    err(lib.sir_param_norms_bwd(P, N, G, -1, g, g, n), b"T must be")
    err(lib.sir_param_norms_bwd(P, _counts([-1, 8]), G, 2, g, g, n), b"negative element count")
    err(lib.sir_param_norms_bwd(P, N, n, 2, g, g, n), b"NULL host array")
    err(lib.sir_param_norms_bwd(n, N, G, 2, g, g, n), b"NULL host array")
    err(lib.sir_param_norms_bwd(_ptrs([None, A]), N, G, 2, g, g, n), b"NULL parameter")
    err(lib.sir_param_norms_bwd(_ptrs([A, A + 2]), N, G, 2, g, g, n), b"4-B aligned")
    err(lib.sir_param_norms_bwd(P, N, _ptrs([A + 256, A + 516]), 2, g, g, n), b"16-B aligned")
    err(lib.sir_param_norms_bwd(P, N, G, 2, n, n, n), b"both NULL")


def test_empty_work_is_a_no_op():
    lib = _native.load()
    n = ctypes.c_void_p(None)
    assert lib.sir_param_norms_fwd(n, n, 0, n, 0, n, n) == 0
    assert lib.sir_param_norms_bwd(n, n, n, 0, n, n, n) == 0
    # every count zero: nothing is looked at but the counts (NULL and misaligned addresses included)
    P, N, G = _ptrs([None, 0x10002]), _counts([0, 0]), _ptrs([None, 0x10004])
    assert lib.sir_param_norms_fwd(P, N, 2, n, 0, n, n) == 0
    assert lib.sir_param_norms_bwd(P, N, G, 2, n, n, n) == 0


def test_exported():
    for name in ("param_norms", "regularizer"):
        assert hasattr(sirgcn, name) and name in sirgcn.__all__
