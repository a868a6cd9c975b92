"""CPU-only checks of the pre-norm block (``sirgcn.drop_act``, ``sirgcn.PreNormSIRModel``, ``sir_drop_act_fwd`` /
``_bwd``): the model's attributes and state_dict keys are the reference's (the fixture manifest's), the fixtures
load and are small, the library exports the two entries at ABI 17 and they refuse bad arguments synchronously,
and a CPU tensor raises (no CPU fallback)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN, load_case

import sirgcn
from sirgcn import _native

with open(os.path.join(GOLDEN, "prenorm_manifest.json")) as _f:
    CASES = json.load(_f)["cases"]
EINVAL = 1
F32, BF16, F16 = 0, 1, 2


def build_model(c, **kw):
    return sirgcn.PreNormSIRModel(c["input_dim"], c["hidden_dim"], c["output_dim"], num_layers=c["num_layers"],
                                  norm=c["norm"], residual=c["residual"], agg_type=c["agg"], **kw)


def test_the_cases_the_fixtures_cover():
    got = {(c["norm"], c["agg"], c["num_layers"], c["residual"]) for c in CASES}
    for norm in ("ln", "bn", "none"):
        for agg in ("sym", "mean"):
            assert (norm, agg, 2, True) in got
    assert any(not c["residual"] for c in CASES)
    assert any(c["agg"] == "max" and c["num_layers"] == 1 and c["graph"] == "graph_small_nodup" and c["min_gap"] > 0
               for c in CASES)
    assert {c["output_dim"] for c in CASES} == {1, 3}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_attributes_and_state_dict_keys_are_the_references(c):
    model = build_model(c)
    for name in ("input_linear", "input_drop", "drop", "activation", "norms", "convs", "linears", "output_norm",
                 "output_linear", "num_layers", "residual"):
        assert hasattr(model, name), name
    assert list(model.state_dict().keys()) == c["state_keys"]
    assert [k for k, _ in model.named_parameters()] == c["param_keys"]
    assert [k for k, _ in model.named_buffers()] == c["buffer_keys"]
    assert model.num_layers == c["num_layers"] and model.residual == c["residual"]
    assert isinstance(model.activation, nn.GELU) and model.activation.approximate == "none"
    assert isinstance(model.input_drop, nn.Dropout) and isinstance(model.drop, nn.Dropout)
    assert all(isinstance(n, sirgcn.GetNorm) for n in list(model.norms) + [model.output_norm])
    assert all(isinstance(m, sirgcn.SIRConv) and m.activation is model.activation for m in model.convs)
    assert type(model).fused_tail is True and model.site_seeds is None


def test_constructor_defaults_and_dropout_arguments():
    model = sirgcn.PreNormSIRModel(12, 32, 3, 2, 0.3, 0.2, "ln", True, 0.1, "sym", unused_keyword=1)
    assert model.input_drop.p == 0.3 and model.drop.p == 0.2
    assert all(m.dropout.p == 0.1 and m._agg_type == "sym" for m in model.convs)
    plain = sirgcn.PreNormSIRModel(12, 32, 3)
    assert plain.num_layers == 1 and plain.residual is False and plain.convs[0]._agg_type == "mean"
    assert isinstance(plain.norms[0].norm, nn.Identity)
    with pytest.raises(NotImplementedError):
        sirgcn.PreNormSIRModel(12, 32, 3, norm="cn")


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_fixture_loads_into_the_model_and_is_small(c):
    path = os.path.join(GOLDEN, c["name"] + ".npz")
    assert os.path.getsize(path) < 256 * 1024          # the largest of the other fixtures are of this order
    z = load_case(c["name"])
    assert sorted(z) == c["keys"]
    V, O = c["V"], c["output_dim"]
    assert z["X"].shape == (V, c["input_dim"]) and z["X"].dtype == np.float32
    assert z["dY"].shape == ((V, O) if O > 1 else (V,))           # squeeze(1)
    assert z["Y32"].shape == z["Y64"].shape == z["dY"].shape
    assert z["Y32"].dtype == np.float32 and z["Y64"].dtype == np.float64 and z["dX64"].dtype == np.float64
    assert z["src"].max() < V and z["dst"].max() < V
    model = build_model(c)
    model.load_state_dict({k: torch.from_numpy(z["s." + k]) for k in c["state_keys"]})
    for k in c["param_keys"]:
        assert z["g32." + k].shape == z["g64." + k].shape == z["s." + k].shape
        assert np.isfinite(z["g64." + k]).all()
    for k in c["buffer_keys"]:
        assert z["b32." + k].shape == z["s." + k].shape
    if c["norm"] == "bn":
        assert int(z["b32.output_norm.norm.num_batches_tracked"]) == 1


def test_new_symbols_are_in_the_library_at_abi_17():
    lib = _native.load()
    assert lib.sir_abi_version() == 17 == _native.ABI_VERSION
    for name in ("sir_drop_act_fwd", "sir_drop_act_bwd"):
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert sirgcn.drop_act is sirgcn.prenorm.drop_act and "PreNormSIRModel" in sirgcn.__all__


def _aligned(buf, align=16, off=0):
    return ctypes.c_void_p(((ctypes.addressof(buf) + 63) & ~63) + off)


def test_entries_refuse_bad_arguments():
    """Every refusal is synchronous (SIR_EINVAL with a message, nothing launched): no GPU is needed."""
    lib = _native.load()
    n = ctypes.c_void_p(None)
    buf = ctypes.create_string_buffer(512)
    p = _aligned(buf)

    def fwd(Y=p, ldy=8, dt=F32, R=p, ldr=8, out=p, ldo=8, odt=F32, M=1, N=8, act=3, drop=None):
        return lib.sir_drop_act_fwd(Y, ldy, dt, R, ldr, out, ldo, odt, M, N, act, 0.0, drop, n)

    def bwd(D=p, ldd=8, odt=F32, Y=p, ldy=8, dt=F32, dY=p, lddy=8, M=1, N=8, act=3, drop=None):
        return lib.sir_drop_act_bwd(D, ldd, odt, Y, ldy, dt, dY, lddy, M, N, act, 0.0, drop, n)

    for call in (fwd, bwd):
        assert call(act=5) == EINVAL and b"activation" in lib.sir_last_error()
        assert call(act=-1) == EINVAL
        assert call(dt=3) == EINVAL and b"dtype" in lib.sir_last_error()
        assert call(N=6) == EINVAL and b"N % 4" in lib.sir_last_error()
        assert call(N=0) == EINVAL and call(M=-1) == EINVAL
        assert call(Y=n) == EINVAL and b"NULL" in lib.sir_last_error()
        # R / out / D are fp32 or Y's own 16-bit type: nothing mixed
        assert call(dt=F32, odt=BF16) == EINVAL and b"fp32 or the 16-bit type" in lib.sir_last_error()
        assert call(dt=BF16, odt=F16) == EINVAL and call(dt=F16, odt=BF16) == EINVAL and call(odt=7) == EINVAL
        assert call(ldy=4) == EINVAL and b"ld >= N" in lib.sir_last_error()          # ld < N
        assert call(ldy=10) == EINVAL                                                 # ld % 4
        assert call(Y=_aligned(buf, off=8)) == EINVAL                                 # fp32 rows: 16 B
        assert call(Y=_aligned(buf, off=4), dt=BF16, odt=F32) == EINVAL               # 16-bit rows: 8 B
        nan = _native.Dropout(1, float("nan"), None)
        assert call(drop=ctypes.byref(nan)) == EINVAL and b"NaN" in lib.sir_last_error()
        assert call(M=0, Y=n) == 0                                                    # empty: success, no launch
    assert fwd(out=n) == EINVAL and bwd(D=n) == EINVAL and bwd(dY=n) == EINVAL
    assert fwd(ldr=4) == EINVAL and fwd(ldo=4) == EINVAL and bwd(ldd=4) == EINVAL and bwd(lddy=4) == EINVAL
    assert fwd(R=_aligned(buf, off=8)) == EINVAL and fwd(out=_aligned(buf, off=8)) == EINVAL
    assert fwd(M=0, R=n, Y=n, out=n) == 0                                             # R is optional


def test_cpu_tensors_raise():
    y = torch.randn(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sirgcn.drop_act(y, nn.GELU())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sirgcn.drop_act(y, None, y, (1, 0.5))
    model = build_model(CASES[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(sirgcn.Graph(torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 4), torch.randn(4, 12))


def test_bad_probability_raises_before_any_device_work():
    for p in (float("nan"), -0.1, 1.5):
        with pytest.raises(ValueError, match="between 0 and 1"):
            sirgcn.prenorm._dropout((1, p))
    assert sirgcn.prenorm._dropout((1, 0.0)) is None and sirgcn.prenorm._dropout(None) is None
    assert sirgcn.prenorm._dropout((1, 0.5), training=False) is None
    assert sirgcn.prenorm._dropout((7, 0.5)) == (7, 0.5)
