"""The two-block persistent NT GEMM (k_gemm_nt_p2: two independent 4-wave blocks per CU, 128 x 256
tiles, weight fragments loaded straight into registers; env SIR_NT_2B=1) against the one-block kernel (k_gemm_nt_p, SIR_NT_2B=0):
per output element both run the same operations in the same order, so the outputs are equal bit for
bit — on partial and odd tile counts, a partial feature tile, with bias, dropout and a strided A, and
on rows that force scale resets and accumulator rescales.  Independently of the old kernel, the
error against fp64 stays within the bar of tests/test_gemm_gpu.py (2x torch fp32's own), and NaN
behind the operands' edges does not reach C.  SIR_GEMM_SMALL_ROWS=0 sends every M to the block
routes.  Runs: pytest tests -m gpu."""
import pytest
import torch

from sirgcn import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"

MS = [1, 127, 128, 129, 257, 1000]          # one row, partial / single / odd tile counts split over blocks
KNS = [(256, 512), (256, 256), (512, 256), (128, 256), (256, 300)]   # (256, 300): a partial feature tile


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    _native.load()


def _both(monkeypatch, fn):
    """fn() on route 0 (k_gemm_nt_p) and route 1 (k_gemm_nt_p2)."""
    monkeypatch.setenv("SIR_GEMM_SMALL_ROWS", "0")
    outs = []
    for route in ("0", "1"):
        monkeypatch.setenv("SIR_NT_2B", route)
        outs.append(fn())
    torch.cuda.synchronize()
    return outs


def _same(c0, c1, what):
    assert c0.shape == c1.shape
    bad = (c0.view(torch.int32) != c1.view(torch.int32))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at " \
                          f"{bad.nonzero()[0].tolist()}"


def _operands(M, K, N, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + M * 7 + K * 3 + N)
    A = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    return A, W, b


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("K,N", KNS)
@pytest.mark.parametrize("M", MS)
def test_two_block_route_bit_identical(M, K, N, with_bias, monkeypatch):
    A, W, b = _operands(M, K, N)
    pk = _native.gemm_pack(W)
    c0, c1 = _both(monkeypatch, lambda: _native.gemm_nt(A, pk, b if with_bias else None))
    _same(c0, c1, f"M={M} K={K} N={N} bias={with_bias}")


@pytest.mark.parametrize("K,N", KNS)
def test_two_block_route_bit_identical_dropout(K, N, monkeypatch):
    """The dropout epilogue at a fixed seed: the same mask and the same kept values."""
    for M in MS:
        A, W, b = _operands(M, K, N, seed=1)
        pk = _native.gemm_pack(W)
        c0, c1 = _both(monkeypatch, lambda: _native.gemm_nt(A, pk, b, drop=(1234, 0.25)))
        _same(c0, c1, f"dropout M={M} K={K} N={N}")
        if M == 1000:
            frac = (c1 == 0).float().mean().item()
            assert 0.2 < frac < 0.3, f"dropped fraction {frac}"


@pytest.mark.parametrize("K,N", KNS)
def test_two_block_route_bit_identical_strided_a_and_c(K, N, monkeypatch):
    """A as a column slice of a wider tensor (lda > K: the dQK-style view) and C likewise (ldc > N):
    the neighbours of C keep their values."""
    for M in MS:
        A, W, b = _operands(M, K, N, seed=2)
        wideA = torch.randn(M, K + 72, device=DEV)
        wideA[:, 8:8 + K] = A
        Av = wideA[:, 8:8 + K]
        pk = _native.gemm_pack(W)

        def run():
            wide = torch.full((M, N + 44), 7.0, device=DEV)
            _native.gemm_nt(Av, pk, b, out=wide[:, 8:8 + N])
            return wide
        w0, w1 = _both(monkeypatch, run)
        _same(w0, w1, f"strided M={M} K={K} N={N}")
        assert torch.all(w1[:, :8] == 7.0) and torch.all(w1[:, 8 + N:] == 7.0)
        _same(w1[:, 8:8 + N].contiguous(), _both(monkeypatch, lambda: _native.gemm_nt(A, pk, b))[1], "strided vs dense")


def test_two_block_route_scale_resets_and_rescales(monkeypatch):
    """M = 257, K = 512: rows spanning 2^-40 .. 2^40, and rows whose maximum grows along K by 2^12 per
    32-k chunk (more than the reset headroom: every chunk resets the scale and rescales the
    accumulators), rising and falling, with zero and late-starting rows."""
    g = torch.Generator(device=DEV).manual_seed(5)
    M, K, N = 257, 512, 256
    A = torch.randn(M, K, device=DEV, generator=g)
    A *= torch.exp2(torch.randint(-40, 41, (M, 1), device=DEV, generator=g).float())
    step = torch.exp2(12.0 * (torch.arange(K, device=DEV) // 32).float() - 96.0)      # 2^12 per chunk
    A[32:96] = torch.randn(64, K, device=DEV, generator=g) * step
    A[96:128] = torch.randn(32, K, device=DEV, generator=g) * step.flip(0)
    A[7] = 0
    A[128:140, :96] = 0                      # leading zero chunks: the first scale is set late
    A[250:257, 64:] *= 2.0 ** 20             # the last, partial tile too
    W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    pk = _native.gemm_pack(W)
    c0, c1 = _both(monkeypatch, lambda: _native.gemm_nt(A, pk))
    _same(c0, c1, "scale resets")
    assert torch.all(c1[7] == 0) and torch.isfinite(c1).all()


@pytest.mark.parametrize("M,K,N", [(257, 256, 512), (1000, 512, 256), (129, 256, 300)])
def test_two_block_route_vs_fp64(M, K, N, monkeypatch):
    """Independent of k_gemm_nt_p: the bar of tests/test_gemm_gpu.py — per element
    |C - C64| <= max(8e-7, 2x torch fp32's worst) * sum_k |a||b|, relative L2 <= max(2x torch's, 1e-6)."""
    A, W, b = _operands(M, K, N, seed=3)
    monkeypatch.setenv("SIR_GEMM_SMALL_ROWS", "0")
    monkeypatch.setenv("SIR_NT_2B", "1")
    C = _native.gemm_nt(A, _native.gemm_pack(W), b)
    ref32 = torch.addmm(b, A, W.t())
    C64 = A.double() @ W.double().t() + b.double()
    den = A.double().abs() @ W.double().abs().t() + b.double().abs() + 1e-300
    worst = ((C.double() - C64).abs() / den).max().item()
    worst_torch = ((ref32.double() - C64).abs() / den).max().item()
    e_ours = ((C.double() - C64).norm() / C64.norm()).item()
    e_torch = ((ref32.double() - C64).norm() / C64.norm()).item()
    print(f"M={M} K={K} N={N}: worst {worst:.3e} (torch {worst_torch:.3e}), relL2 {e_ours:.3e} (torch {e_torch:.3e})")
    assert worst <= max(8e-7, 2 * worst_torch), f"max |err| / sum|a||b| = {worst:.2e} (torch fp32: {worst_torch:.2e})"
    assert e_ours <= max(2 * e_torch, 1e-6), f"relL2 {e_ours:.2e} vs torch fp32 {e_torch:.2e}"


def test_two_block_route_ignores_poison(monkeypatch):
    """NaN in the rows of A's buffer past M, in its columns outside the K of the view, and in the padding
    rows (features N .. Npad) of the packed weight image reaches no element of C."""
    M, K, N = 1000, 256, 300
    A, W, b = _operands(M, K, N, seed=4)
    buf = torch.full((M + 300, K + 40), float("nan"), device=DEV)
    buf[:M, 4:4 + K] = A
    Av = buf[:M, 4:4 + K]
    pk, n_, k_ = _native.gemm_pack(W)
    clean = pk.clone()
    npad, kc = (N + 255) // 256 * 256, K // 32
    img = pk[:kc * 4 * npad * 32].view(torch.int16).view(kc * 4, npad // 32, 2, 32, 8)   # [plane][row / 32][h][row % 32]
    for n in range(N, npad):
        img[:, n // 32, :, n % 32, :] = 0x7e00                                              # fp16 NaN
    assert not torch.equal(pk, clean)
    wide = torch.full((M + 8, N + 44), 7.0, device=DEV)
    monkeypatch.setenv("SIR_GEMM_SMALL_ROWS", "0")
    monkeypatch.setenv("SIR_NT_2B", "1")
    _native.gemm_nt(Av, (pk, n_, k_), b, out=wide[:M, 8:8 + N])
    want = _native.gemm_nt(A, (clean, n_, k_), b)
    assert torch.isfinite(wide).all()
    _same(wide[:M, 8:8 + N].contiguous(), want, "poison")
    assert torch.all(wide[:, :8] == 7.0) and torch.all(wide[:, 8 + N:] == 7.0) and torch.all(wide[M:] == 7.0)
