"""CPU-only checks of the SIREConv edge-term entry points (ABI 17): sir_edge_e_agg_fwd and
sir_edge_e_bwd are exported, and every argument check is synchronous, returns its code and leaves a
sir_last_error text — no GPU work is issued (the pointers below are host memory or NULL)."""
import ctypes

from sirgcn import _native


def _null():
    return ctypes.c_void_p(None)


def _buf():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def _fwd(lib, rowptr, col, items, n_items, H, dtype, Q, ldq, K, ldk, Eh, lde, n_erows, eidx, nr, nc, agg, act, S, lds,
         mask=None, splits=None, n_splits=0, partial=None):
    n = _null()
    return lib.sir_edge_e_agg_fwd(rowptr, col, items, n_items, splits if splits is not None else n, n_splits, H, dtype,
                                  Q, ldq, K, ldk, Eh, lde, n_erows, eidx, nr, nc, agg, act, 0.2, S, lds,
                                  mask if mask is not None else n, partial if partial is not None else n, n)


def _bwd(lib, rowptr, col, items, n_items, H, dtype, mask, G, ldg, nr, nc, agg, act, eidx, n_erows, dE, ldde):
    return lib.sir_edge_e_bwd(rowptr, col, items, n_items, H, dtype, mask, G, ldg, nr, nc, agg, act, 0.2, eidx,
                              n_erows, dE, ldde, _null())


def test_symbols_and_version():
    lib = _native.load()
    assert _native.ABI_VERSION == 17 and lib.sir_abi_version() == 17
    for name in ("sir_edge_e_agg_fwd", "sir_edge_e_bwd"):
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert hasattr(_native, "edge_e_agg_fwd") and hasattr(_native, "edge_e_bwd")


def test_empty_work_is_a_no_op():
    lib = _native.load()
    n = _null()
    for agg in (0, 1, 2):
        assert _fwd(lib, n, n, n, 0, 256, 0, n, 256, n, 256, n, 256, 0, n, n, n, agg, 2, n, 256) == 0
    for agg in (0, 2):
        assert _bwd(lib, n, n, n, 0, 256, 0, n, n, 256, n, n, agg, 1, n, 0, n, 256) == 0


def test_forward_argument_checks_are_synchronous_and_reported():
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    # storage dtype: fp32 only (unknown dtypes are invalid, the 16-bit ones unsupported)
    assert _fwd(lib, n, n, n, 0, 256, 7, n, 256, n, 256, n, 256, 0, n, n, n, 0, 2, n, 256) == 1
    assert b"F32" in lib.sir_last_error()
    for dt in (1, 2):
        assert _fwd(lib, p, p, p, 1, 16, dt, p, 16, p, 16, p, 16, 1, n, n, n, 0, 2, p, 16) == 2
        assert b"F32" in lib.sir_last_error()
    # bad agg
    assert _fwd(lib, n, n, n, 0, 256, 0, n, 256, n, 256, n, 256, 0, n, n, n, 9, 2, n, 256) == 1
    assert b"agg" in lib.sir_last_error()
    # activations outside the ReLU family: identity, GELU (erf / tanh)
    for act in (0, 3, 4):
        assert _fwd(lib, p, p, p, 1, 16, 0, p, 16, p, 16, p, 16, 1, n, n, n, 0, act, p, 16) == 2
        assert b"RELU" in lib.sir_last_error()
    # H: out of range, not a multiple of 4
    assert _fwd(lib, p, p, p, 1, 2048, 0, p, 2048, p, 2048, p, 2048, 1, n, n, n, 0, 2, p, 2048) == 1
    assert b"H must be" in lib.sir_last_error()
    assert _fwd(lib, p, p, p, 1, 30, 0, p, 32, p, 32, p, 32, 1, n, n, n, 0, 2, p, 32) == 2
    assert b"H % 4" in lib.sir_last_error()
    # NULL buffers when there is work: rowptr / items / S, then Q / K / Eh
    assert _fwd(lib, n, p, n, 1, 16, 0, p, 16, p, 16, p, 16, 1, n, n, n, 0, 2, n, 16) == 1
    assert b"non-NULL" in lib.sir_last_error()
    for q, k, e in ((n, p, p), (p, n, p), (p, p, n)):
        assert _fwd(lib, p, p, p, 1, 16, 0, q, 16, k, 16, e, 16, 1, n, n, n, 0, 2, p, 16) == 1
        assert b"Q/K/Eh" in lib.sir_last_error()
    # leading dimensions below H (Q, K, Eh, S)
    for lds in ((8, 16, 16, 16), (16, 8, 16, 16), (16, 16, 8, 16), (16, 16, 16, 8)):
        assert _fwd(lib, p, p, p, 1, 16, 0, p, lds[0], p, lds[1], p, lds[2], 1, n, n, n, 0, 2, p, lds[3]) == 1
        assert b"leading" in lib.sir_last_error()
    # SYM requires both norms
    assert _fwd(lib, p, p, p, 1, 16, 0, p, 16, p, 16, p, 16, 1, n, n, n, 2, 2, p, 16) == 1
    assert b"SYM" in lib.sir_last_error()
    assert _fwd(lib, p, p, p, 1, 16, 0, p, 16, p, 16, p, 16, 1, n, p, n, 2, 2, p, 16) == 1
    # no edge rows with work
    for n_erows in (0, -3):
        assert _fwd(lib, p, p, p, 1, 16, 0, p, 16, p, 16, p, 16, n_erows, n, n, n, 0, 2, p, 16) == 1
        assert b"n_erows" in lib.sir_last_error()
    # split rows need the splits and the partial workspace
    assert _fwd(lib, p, p, p, 1, 16, 0, p, 16, p, 16, p, 16, 1, n, n, n, 0, 2, p, 16, n_splits=1) == 1
    assert b"split" in lib.sir_last_error()
    # rows that are not 16-B aligned are unsupported (checked before any launch)
    off = ctypes.c_void_p(p.value + 4)
    assert _fwd(lib, p, p, p, 1, 16, 0, p, 16, p, 16, off, 16, 1, n, n, n, 0, 2, p, 16) == 2
    assert b"aligned" in lib.sir_last_error()
    assert _fwd(lib, p, p, p, 1, 16, 0, p, 16, p, 16, p, 18, 1, n, n, n, 0, 2, p, 16) == 2
    assert b"aligned" in lib.sir_last_error()
    del keep


def test_backward_argument_checks_are_synchronous_and_reported():
    lib = _native.load()
    n = _null()
    keep, p = _buf()
    # MEAN is the caller's division: pass G / deg with SUM
    assert _bwd(lib, p, p, p, 1, 16, 0, p, p, 16, n, n, 1, 2, n, 1, p, 16) == 2
    assert b"MEAN" in lib.sir_last_error()
    # dtype, activation, H
    assert _bwd(lib, n, n, n, 0, 16, 7, n, n, 16, n, n, 0, 2, n, 0, n, 16) == 1
    assert b"F32" in lib.sir_last_error()
    assert _bwd(lib, p, p, p, 1, 16, 1, p, p, 16, n, n, 0, 2, n, 1, p, 16) == 2
    assert b"F32" in lib.sir_last_error()
    assert _bwd(lib, p, p, p, 1, 16, 0, p, p, 16, n, n, 0, 3, n, 1, p, 16) == 2
    assert b"RELU" in lib.sir_last_error()
    assert _bwd(lib, p, p, p, 1, 18, 0, p, p, 20, n, n, 0, 2, n, 1, p, 20) == 2
    assert b"H % 4" in lib.sir_last_error()
    # NULL buffers when there is work: dE, then mask / G
    assert _bwd(lib, p, p, p, 1, 16, 0, p, p, 16, n, n, 0, 2, n, 1, n, 16) == 1
    assert b"non-NULL" in lib.sir_last_error()
    for m, g in ((n, p), (p, n)):
        assert _bwd(lib, p, p, p, 1, 16, 0, m, g, 16, n, n, 0, 2, n, 1, p, 16) == 1
        assert b"mask/G" in lib.sir_last_error()
    # leading dimensions below H
    assert _bwd(lib, p, p, p, 1, 16, 0, p, p, 8, n, n, 0, 2, n, 1, p, 16) == 1
    assert b"leading" in lib.sir_last_error()
    assert _bwd(lib, p, p, p, 1, 16, 0, p, p, 16, n, n, 0, 2, n, 1, p, 8) == 1
    assert b"leading" in lib.sir_last_error()
    # SYM requires the norms; no edge rows with work
    assert _bwd(lib, p, p, p, 1, 16, 0, p, p, 16, n, n, 2, 2, n, 1, p, 16) == 1
    assert b"SYM" in lib.sir_last_error()
    assert _bwd(lib, p, p, p, 1, 16, 0, p, p, 16, n, n, 0, 2, n, 0, p, 16) == 1
    assert b"n_erows" in lib.sir_last_error()
    # unaligned gradient rows
    assert _bwd(lib, p, p, p, 1, 16, 0, p, p, 18, n, n, 0, 2, n, 1, p, 16) == 2
    assert b"aligned" in lib.sir_last_error()
    del keep
