"""CPU tests of the MLP block entries: bad arguments are refused before any device work, the Python module
refuses bad inputs the way torch does (ValueError) and runs on the GPU only, the layer/sample seed mirror follows the
header's formula, and the module layout and state_dict keys are the reference's."""
import ctypes

import pytest

from grand_plus_amd import _native

NULL = None
P, S0 = ctypes.c_void_p(16), ctypes.c_void_p(0)
SEED = ctypes.c_uint64(1)
M64 = 2**64 - 1


def _fwd(S=2, B=8, F=4, N=3, flags=0, x=P, w=P, dropout=0.0, eps=1e-5, mom=0.1, out=P, saved=P, ws=P, rm=P, rv=P):
    return _native.lib().gp_mlp_block_forward(0, x, S, B, F, N, w, NULL, flags, NULL, NULL, rm, rv, NULL, eps, mom, dropout,
                                              SEED, 0, NULL, out, saved, NULL, ws, S0)


def _bwd(S=2, B=8, F=4, N=3, flags=0, x=P, w=P, dropout=0.0, gy=P, ws=P, saved=P, gw=NULL, a=NULL):
    return _native.lib().gp_mlp_block_backward(0, x, S, B, F, N, w, flags, NULL, dropout, SEED, 0, NULL, saved, a, gy,
                                               NULL, gw, NULL, NULL, NULL, ws, S0)


@pytest.mark.parametrize("S", [0, 17, -1])
def test_entries_refuse_a_sample_count_outside_1_16(S):
    L = _native.lib()
    assert _fwd(S=S) == _native.GP_ERR_INVALID_ARG
    assert "gp_mlp_block_forward" in L.gp_last_error().decode()
    assert _bwd(S=S) == _native.GP_ERR_INVALID_ARG
    assert "gp_mlp_block_backward" in L.gp_last_error().decode()


def test_entries_check_sizes_flags_and_pointers_before_the_device():
    E, N = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL
    BN, TR = _native.GP_MLP_BN, _native.GP_MLP_TRAINING
    assert _fwd(B=0) == E
    assert _fwd(F=0) == E
    assert _fwd(N=0) == E
    assert _fwd(flags=16) == E                                       # unknown flag
    assert _fwd(dropout=-0.1) == E and _fwd(dropout=1.5) == E
    assert _fwd(flags=BN | TR, B=1) == E                             # BatchNorm needs 2 rows per sample in training
    assert _fwd(flags=BN | TR, eps=0.0) == E
    assert _fwd(flags=BN | TR, mom=1.5) == E
    assert _fwd(x=NULL) == N and _fwd(w=NULL) == N and _fwd(out=NULL) == N and _fwd(ws=NULL) == N
    assert _fwd(flags=_native.GP_MLP_NORM, saved=NULL) == N          # row scales need the saved buffer
    assert _fwd(flags=BN, rm=NULL, rv=NULL) == N                      # eval BatchNorm needs running statistics
    assert _bwd(B=0) == E and _bwd(dropout=2.0) == E
    assert _bwd(gy=NULL) == N and _bwd(ws=NULL) == N
    assert _bwd(gw=P, a=NULL) == N                                    # the weight gradient needs the saved input


def _mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def test_layer_seed_follows_the_header_formula():
    from grand_plus_amd.mlp import layer_seed
    for seed in (0, 1, 0x1234_5678_9ABC, M64):
        for s in (0, 1, 5, 15):
            for layer in (0, 1, 2):
                ss = seed if s == 0 else _mix(seed ^ ((s * 0xD6E8FEB86659FD93) & M64))
                assert layer_seed(seed, layer, s) == _mix(ss ^ (((layer + 1) * 0xA0761D6478BD642F) & M64))
    # known values
    assert layer_seed(1, 0) == 0x63A183183ED6D2E0
    assert layer_seed(1, 1, 2) == 0xD40B1008E1366164
    assert layer_seed(1, 0, 0) != layer_seed(1, 1, 0) != layer_seed(1, 0, 1)


def _ref_layout(nlayers, F=30, H=16, C=4):
    """Module names and shapes of model.py's MLP constructor (model.py:18-35) and model_mag.py's (model_mag.py:18-37)."""
    if nlayers == 1:
        model = {"fcs.0.weight": (C, F), "fcs.0.bias": (C,), "bns.0.weight": (F,)}
        mag = {"embeds.weight": (F, C)}
    else:
        model = {"fcs.0.weight": (H, F), "bns.0.weight": (F,)}
        mag = {"embeds.weight": (F, H)}
        for i in range(1, nlayers - 1):
            model[f"fcs.{i}.weight"] = (H, H)
            mag[f"fcs.{i - 1}.weight"] = (H, H)
        model[f"fcs.{nlayers - 1}.weight"] = (C, H)
        model[f"bns.{nlayers - 1}.weight"] = (H,)
        mag[f"fcs.{nlayers - 2}.weight"] = (C, H)
        mag[f"bns.{nlayers - 2}.weight"] = (H,)
    return model, mag


@pytest.mark.parametrize("nlayers", [1, 2, 3])
def test_module_layout_and_state_dict_keys_are_the_references(nlayers):
    from grand_plus_amd.mlp import GrandPlusMLP, MagMLP
    a = GrandPlusMLP(30, 4, 16, nlayers, True, 0.5, 0.2, True)
    m = MagMLP(30, 4, 16, nlayers, True, 0.0, 0.2, True)
    model, mag = _ref_layout(nlayers)
    for mod, want in ((a, model), (m, mag)):
        sd = mod.state_dict()
        for k, shape in want.items():
            assert tuple(sd[k].shape) == shape, k
        n_fc = sum(1 for k in sd if k.startswith("fcs.") and k.endswith(".weight"))
        n_bn = sum(1 for k in sd if k.startswith("bns.") and k.endswith(".running_mean"))
        assert n_fc == n_bn
        for k in sd:
            assert k.split(".")[0] in ("fcs", "bns", "embeds")
            assert k.split(".")[-1] in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    assert (a.input_droprate, a.hidden_droprate, a.use_bn, a.node_norm) == (0.5, 0.2, True, True)
    assert len(a.fcs) == nlayers and len(m.fcs) == nlayers - 1


def test_forward_refuses_bad_inputs_before_any_launch():
    import torch
    from grand_plus_amd.mlp import GrandPlusMLP
    m = GrandPlusMLP(6, 3, 8, 2, True, 0.1, 0.1, False).train()
    with pytest.raises(ValueError):
        m(torch.zeros((17, 4, 6)))                                   # S > 16
    with pytest.raises(ValueError):
        m(torch.zeros((2, 4, 6), dtype=torch.float64))               # dtype
    with pytest.raises(ValueError):
        m(torch.zeros((2, 6, 4)).transpose(1, 2))                    # not contiguous
    with pytest.raises(ValueError):
        m(torch.zeros((2, 3, 4, 6)))                                 # rank
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros((2, 1, 6)))                                    # BatchNorm in training over one row, as torch
    with pytest.raises(ValueError, match="GPU only"):
        m(torch.zeros((2, 4, 6)))                                    # no CPU fallback
    m.bns[0].momentum = None
    with pytest.raises(ValueError, match="momentum=None"):
        m(torch.zeros((2, 4, 6)))
    m.eval()
    m.bns[0].momentum = 0.1
    with pytest.raises(ValueError, match="GPU only"):
        m(torch.zeros((1, 6)))                                       # one row is fine in eval, but still GPU only
