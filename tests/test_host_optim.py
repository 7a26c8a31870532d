"""CPU tests of the optimiser: ClipAdam refuses what it cannot run (TypeError: there is no CPU fallback) and
what torch.optim.Adam refuses (ValueError, its messages), a fresh ClipAdam has
torch Adam's state_dict layout, and gp_clip_adam_step returns its error codes before any GPU work."""
import ctypes
import re

import pytest
import torch

from grand_plus_amd import _native

P = ctypes.c_void_p(16)


def _param(t):
    p = torch.nn.Parameter(t)
    p.grad = torch.zeros_like(t)
    return p


# every tensor here is on the CPU: dtype and layout are refused before the device is looked at, each with its own message
@pytest.mark.parametrize("make,msg", [
    (lambda: torch.zeros(5), "must be a CUDA tensor"),
    (lambda: torch.zeros(5, dtype=torch.float64), "must be float32, got torch.float64"),
    (lambda: torch.zeros(5, dtype=torch.float16), "must be float32, got torch.float16"),
    (lambda: torch.zeros(6, 4).t(), "must be contiguous, got strides (1, 4)"),
], ids=["cpu", "float64", "half", "non-contiguous"])
def test_step_refuses_parameters_it_cannot_run(make, msg):
    from grand_plus_amd import ClipAdam, clip_grad_norm
    p = _param(make())
    before = p.detach().clone()
    opt = ClipAdam([p], lr=1e-2)
    for run in (opt.step, lambda: clip_grad_norm([p], 1.0)):
        with pytest.raises(TypeError, match=re.escape(msg)) as err:
            run()
        assert "no CPU fallback" in str(err.value)
    assert torch.equal(p.detach(), before) and len(opt.state) == 0     # nothing ran in torch instead


def test_sparse_gradients_are_refused():
    from grand_plus_amd import ClipAdam
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.zeros(4, 3).to_sparse()
    with pytest.raises(TypeError, match="sparse"):
        ClipAdam([p]).step()


def test_parameters_without_a_gradient_are_skipped_without_state():
    from grand_plus_amd import ClipAdam
    p = torch.nn.Parameter(torch.zeros(5))                            # a CPU parameter, but nothing to do for it
    opt = ClipAdam([p])
    norm = opt.step()
    assert float(norm) == 0.0 and norm.dtype == torch.float32 and norm.dim() == 0 and norm.device == p.device
    assert len(opt.state) == 0


def test_the_lazy_names_stay_out_of_star_imports():
    import grand_plus_amd
    assert not {"ClipAdam", "clip_grad_norm"} & set(grand_plus_amd.__all__)
    assert grand_plus_amd.ClipAdam.__module__ == "grand_plus_amd.optim"


@pytest.mark.parametrize("kw,msg", [
    (dict(lr=-1e-3), "Invalid learning rate: -0.001"),
    (dict(eps=-1e-8), "Invalid epsilon value: -1e-08"),
    (dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0: 1.0"),
    (dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1: -0.1"),
    (dict(weight_decay=-1.0), "Invalid weight_decay value: -1.0"),
])
def test_hyper_parameter_ranges_and_messages_are_torch_adams(kw, msg):
    from grand_plus_amd import ClipAdam
    with pytest.raises(ValueError, match=re.escape(msg)):
        ClipAdam([torch.nn.Parameter(torch.zeros(3))], **kw)
    with pytest.raises(ValueError, match=re.escape(msg)):
        torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], **kw)


def test_amsgrad_and_maximize_are_refused():
    from grand_plus_amd import ClipAdam
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="amsgrad or maximize"):
            ClipAdam([torch.nn.Parameter(torch.zeros(3))], **kw)
    for name in ("capturable", "fused", "foreach"):
        with pytest.raises(TypeError):
            ClipAdam([torch.nn.Parameter(torch.zeros(3))], **{name: True})
    # a loaded torch checkpoint that asks for amsgrad is refused at the step
    p = _param(torch.zeros(3))
    opt = ClipAdam([p])
    opt.load_state_dict(torch.optim.Adam([p], amsgrad=True).state_dict())
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()


def test_a_fresh_clipadam_has_torch_adams_state_dict_layout():
    from grand_plus_amd import ClipAdam
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    kw = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-4)
    ours = ClipAdam([{"params": ps[:1]}, {"params": ps[1:], "lr": 1e-4}], clip_norm=0.5, **kw).state_dict()
    ref = torch.optim.Adam([{"params": ps[:1]}, {"params": ps[1:], "lr": 1e-4}], **kw).state_dict()
    assert ours == ref and ours["state"] == {}
    assert isinstance(ClipAdam(ps), torch.optim.Optimizer)


def _call(tab, n, flags=0, max_norm=0.1, beta1=0.9, ws=P, norm=P):
    return _native.lib().gp_clip_adam_step(0, tab, n, flags, max_norm, 1e-2, beta1, 0.999, 1e-8, 0.0, 1e-2, 1.0, ws, norm, None)


def test_entry_returns_its_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL
    tab = (_native.GpOptimTensor * 2)()
    assert _call(tab, -1) == E
    assert "gp_clip_adam_step" in _native.lib().gp_last_error().decode()
    assert _call(None, 1) == N                                        # null table with n_tensors > 0
    assert _call(tab, 1, flags=8) == E                                # unknown flag
    assert _call(tab, 1, flags=_native.GP_OPTIM_NORM_ONLY | _native.GP_OPTIM_NORM_READY) == E
    assert _call(tab, 1, beta1=float("nan")) == E and _call(tab, 1, max_norm=float("inf")) == E
    assert _call(tab, 0, ws=None) == N and _call(tab, 0, norm=None) == N
    tab[1].numel = -1
    assert _call(tab, 2) == E                                         # negative size
    tab[1].numel = 4
    assert _call(tab, 2) == N                                         # elements but no pointers
    tab[1].grad = 16
    assert _call(tab, 2) == N                                         # the state pointers are needed ...
    with pytest.raises(ValueError):
        _native.raise_for_status(N)
