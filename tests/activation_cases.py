"""TEST INFRASTRUCTURE: the activation codes the kernels are instantiated for, paired with the oracle's names,
and the random inputs of the kernel-level activation sweep (tests/test_activations_gpu.py), shared with its
CPU self-check (tests/test_activations_cpu.py).  Nothing here touches the GPU."""
import torch

from sirgcn import _native

# every code between the first and the last one, so a code added to the library arrives here without a name
# (ORACLE_NAME[code] raises) instead of arriving untested
CODES = tuple(range(_native.ACT_IDENTITY, _native.ACT_GELU_TANH + 1))
ORACLE_NAME = {_native.ACT_IDENTITY: "identity", _native.ACT_RELU: "relu", _native.ACT_LEAKY: "leaky",
               _native.ACT_GELU: "gelu", _native.ACT_GELU_TANH: "gelu_tanh"}
SLOPE = {_native.ACT_LEAKY: 0.2}        # every other code ignores its slope
# the codes without a sign-mask backward: sigma' needs z itself, so the backward recomputes it
RECOMPUTE_CODES = tuple(c for c in CODES if c not in (_native.ACT_RELU, _native.ACT_LEAKY))

# 3, 30, 70, 130: the scalar path (fp32 only) at 1, 2, 4 values per lane; every other width class once or more
# (tests/width_cases.py)
EDGE_H = (3, 30, 4, 16, 60, 76, 128, 136, 256, 300, 512, 1024, 24, 70, 130, 640)
EDGE_H_16BIT = (16, 128, 256, 300, 1024, 24, 60, 640)
EDGE_CHUNKS = (4, 256)
AGGS = ("sum", "mean", "sym")


def slope_of(code):
    return SLOPE.get(code, 0.0)


def edge_inputs(H, agg):
    """src, dst, V, Q, K, dS of the width sweep (tests/test_gpu_parity.py::test_hidden_sizes_vs_oracle's
    graph): V = 300, E = 2500, 400 edges into node 5, 20 isolated destinations; fp32 randn rows."""
    gen = torch.Generator().manual_seed(H * 7 + len(agg))
    V, E = 300, 2500
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(0, V - 20, (E,), generator=gen)
    dst[:400] = 5
    Q, K, dS = (torch.randn(V, H, generator=gen) for _ in range(3))
    return src, dst, V, Q, K, dS
