"""Seeds and tensor plumbing shared by augment.py, embedding.py, mlp.py and objective.py.

The seed formulas mirror include/grandplus.h (and csrc/gp_common.hpp on the device) bit for bit; this is their only
Python definition.  Seeds drawn for calls without an explicit one come from one counter for the whole process.
"""
from __future__ import annotations

import ctypes
import itertools

import torch

_M64 = 2**64 - 1
_GOLDEN = 0x9E3779B97F4A7C15
_LAYER_MUL = 0xA0761D6478BD642F
_SLOT_MUL = 0xE7037ED1A0B428DB
_STEP_MUL = 0x8CB92BA72F3D8DD7
_FIT_ROUND_MUL, _FIT_EPOCH_MUL, _FIT_UNLABEL_MUL = 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x27D4EB2F165667C5   # csrc/fit_perm.hpp

_seed_counter = itertools.count(0x5EED)


def _new_seed():
    return next(_seed_counter) * _GOLDEN & _M64


def _mix(x: int) -> int:
    x = (x + _GOLDEN) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sample_seed(seed: int, s: int) -> int:
    """Seed of sample s of an S-sample call (the formula of grandplus.h): seed itself for s = 0."""
    seed &= _M64
    return seed if s == 0 else _mix(seed ^ ((s * 0xD6E8FEB86659FD93) & _M64))


def layer_seed(seed: int, layer: int, s: int = 0) -> int:
    """Dropout seed of (layer, sample s) of a call with `seed`: GP_MLP_LAYER_SEED(gp_sample_seed(seed, s), layer)."""
    return _mix(sample_seed(seed, s) ^ (((layer + 1) * _LAYER_MUL) & _M64))


def mag_slot_seed(seed: int, s: int, e: int) -> int:
    """Input-dropout seed of (sample s, slot e = r * K + k) of a mag_prop_rows call: GP_MAG_SLOT_SEED of grandplus_mag.h."""
    return _mix(sample_seed(seed, s) ^ (((e + 1) * _SLOT_MUL) & _M64))


def step_seed(base: int, t: int) -> int:
    """Seed of step t >= 1 of a training run with `base` (gp_step_state.seed of grandplus_step.h): mix(base ^ t * GP_STEP_MUL)."""
    return _mix((base & _M64) ^ ((t * _STEP_MUL) & _M64))


def perm_index(key: int, n: int, i: int) -> int:
    """The image of i < n under the keyed permutation of [0, n) of csrc/fit_perm.hpp, 1 <= n < 2**31: a 4-round
    Feistel network over an even number of bits, walked along its cycle until it lands below n."""
    if not 1 <= n < 2**31 or not 0 <= i < n:
        raise ValueError(f"perm_index needs 1 <= n < 2**31 and 0 <= i < n, got n={n}, i={i}")
    h = (max((n - 1).bit_length(), 2) + 1) // 2
    mask = (1 << h) - 1
    key &= _M64
    x = i
    while True:
        L, R = x >> h, x & mask
        for r in range(4):
            L, R = R, L ^ (_mix(key ^ (((r + 1) * _FIT_ROUND_MUL) & _M64) ^ R) & mask)
        x = (L << h) | R
        if x < n:
            return x


def _check(t, dtype, name):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda:
        raise TypeError(f"{name} must be a contiguous CUDA tensor of dtype {dtype}")


def _deterministic(flag):
    """The `deterministic` keyword of random_prop_rows and the embedding bag: None follows
    torch.are_deterministic_algorithms_enabled(); anything but None or a bool is refused."""
    if flag is None:
        return torch.are_deterministic_algorithms_enabled()
    if not isinstance(flag, bool):
        raise TypeError(f"deterministic must be None, True or False, got {flag!r}")
    return flag


def _dev_index(t):
    if not t.is_cuda:
        raise TypeError("random_prop runs on the GPU only: tensors must be CUDA tensors (no CPU fallback)")
    return t.device.index


def _cuda_device(device, owner):
    """`device` as a torch.device with its index filled in; `owner` names the class whose memory it is, for the message."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{owner} lives in GPU memory: device must be a CUDA device (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _stream(t, stream=None):
    """The stream argument of a native call: the caller's raw stream handle, or the current stream of t's device."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream if stream is None else stream)


def _ptr(t):
    return t.data_ptr() if t is not None else None
