"""Host side of the activation matrix: which kernel code every activation callable of the drop-in layer maps
to (sirgcn.conv.activation_code, sirgcn.edgemlp._elementwise_code / seq_sigma), what is refused, and the
condition on the inputs of tests/test_activations_gpu.py under which its fp32 cases tell erf-GELU from
tanh-GELU.  No GPU."""
import pytest
import torch
from torch import nn
import torch.nn.functional as F

import activation_cases as ac
import oracle
from conftest import rel_err

from sirgcn import _native
from sirgcn.conv import activation_code
from sirgcn.edgemlp import _elementwise_code, seq_sigma

N = _native
MODULES = [(nn.Identity(), (N.ACT_IDENTITY, 0.0)), (nn.ReLU(), (N.ACT_RELU, 0.0)),
           (nn.LeakyReLU(0.3), (N.ACT_LEAKY, 0.3)), (nn.GELU(), (N.ACT_GELU, 0.0)),
           (nn.GELU(approximate="tanh"), (N.ACT_GELU_TANH, 0.0))]
FUNCTIONS = [(torch.relu, (N.ACT_RELU, 0.0)), (F.relu, (N.ACT_RELU, 0.0)), (F.leaky_relu, (N.ACT_LEAKY, 0.01)),
             (F.gelu, (N.ACT_GELU, 0.0))]


def _check(got, want):
    assert got is not None and tuple(got) == want, (got, want)


def test_code_table_names_every_code_once():
    assert ac.CODES == (0, 1, 2, 3, 4)
    assert sorted(ac.ORACLE_NAME) == list(ac.CODES)
    assert sorted(ac.ORACLE_NAME.values()) == sorted(oracle.ACTS)
    assert set(ac.RECOMPUTE_CODES) == {N.ACT_IDENTITY, N.ACT_GELU, N.ACT_GELU_TANH}


@pytest.mark.parametrize("act,want", MODULES + FUNCTIONS, ids=lambda v: getattr(v, "__name__", None) or repr(v))
def test_activation_code(act, want):
    _check(activation_code(act), want)


@pytest.mark.parametrize("act,want", MODULES, ids=lambda v: repr(v))
def test_elementwise_code_and_seq_sigma_act1(act, want):
    _check(_elementwise_code(act), want)
    for a2, c2 in ((nn.ReLU(), N.ACT_RELU), (nn.Identity(), N.ACT_IDENTITY)):
        lin = nn.Linear(16, 24)
        sq = seq_sigma(nn.Sequential(act, lin, a2), 16)
        assert sq is not None
        _check(sq[:2], want)
        assert sq[2] is lin and sq[3] == c2


def test_unknown_activation_is_refused():
    with pytest.raises(NotImplementedError):
        activation_code(nn.Tanh())
    assert _elementwise_code(nn.Tanh()) is None
    assert _elementwise_code(torch.relu) is None                # a module form only
    assert seq_sigma(nn.Sequential(nn.Tanh(), nn.Linear(16, 16), nn.ReLU()), 16) is None
    assert seq_sigma(nn.ReLU(), 16) is None


@pytest.mark.parametrize("a2", [nn.LeakyReLU(0.2), nn.GELU(), nn.GELU(approximate="tanh"), nn.Tanh()], ids=repr)
def test_seq_sigma_refuses_other_act2(a2):
    assert seq_sigma(nn.Sequential(nn.ReLU(), nn.Linear(16, 16), a2), 16) is None


def test_seq_sigma_refuses_shapes_past_the_kernels():
    mk = lambda h, f: nn.Sequential(nn.ReLU(), nn.Linear(h, f), nn.ReLU())
    assert seq_sigma(mk(256, 256), 256) is not None
    assert seq_sigma(mk(260, 64), 260) is None                  # H > 256
    assert seq_sigma(mk(512, 64), 512) is None
    assert seq_sigma(mk(64, 260), 64) is None                   # F > 256
    assert seq_sigma(mk(30, 16), 30) is None                    # H % 4
    assert seq_sigma(mk(64, 64), 32) is None                    # the Linear does not take the layer's H


@pytest.mark.parametrize("agg", ac.AGGS)
def test_fp32_sweep_inputs_tell_erf_gelu_from_tanh_gelu(agg):
    """A condition on the inputs, not a tolerance: on the very Q, K, dS of the GPU sweep the fp64 oracle with
    "gelu" and with "gelu_tanh" lies further apart (relL2 >= 5e-5, in S, dQ and dK) than the 1e-5 bar the fp32
    GPU cases apply, so a dispatch arm that picked the other GELU fails them.  (The two formulas differ by
    <= 5e-4 absolute per message, below one bf16 / fp16 ulp of most elements: the 16-bit cases are not what
    separates them.)"""
    H = 64
    src, dst, V, Q, K, dS = ac.edge_inputs(H, agg)
    Q, K, dS = Q.double(), K.double(), dS.double()
    out = {}
    for act in ("gelu", "gelu_tanh"):
        out[act] = (oracle.edge_agg_fwd(src, dst, V, Q, K, agg, act),) + oracle.edge_agg_bwd(src, dst, V, Q, K, dS,
                                                                                            agg, act)
    for name, a, b in zip(("S", "dQ", "dK"), out["gelu"], out["gelu_tanh"]):
        gap = rel_err(b, a)
        assert gap >= 5e-5, f"{agg} {name}: erf and tanh GELU only {gap:.2e} apart"


def test_sweep_graph_has_the_rows_the_cases_name():
    src, dst, V, Q, K, dS = ac.edge_inputs(16, "sum")
    ind, outd = torch.bincount(dst, minlength=V), torch.bincount(src, minlength=V)
    assert (V, src.numel()) == (300, 2500) and Q.shape == K.shape == dS.shape == (300, 16)
    assert ind[5] >= 400 and int((ind[-20:] == 0).all()) == 1
    assert ind.max() > 256 and outd.max() > 4 and outd.max() <= 256     # chunk 256 splits dst rows only
