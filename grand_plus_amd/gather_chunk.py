"""Chunked deterministic segment sums: what the three deterministic backwards share to use the entry points
of csrc/gather_chunk_abi.hpp.

The deterministic backwards of `random_prop_rows`, the embedding bag and `mag_prop_rows` sum every destination row's
contributions left to right on one wave: a hub destination (a word that sits in a third of the bags, a node in every row's
top-K) is one serial chain of as many adds as it has entries.  `segment_chunk=C` on those calls cuts every segment into
chunks of C sorted positions, counted from the segment's own first position: the chunks are summed by separate waves into
scratch rows, and a second launch sums a destination's scratch rows in chunk order.  The chain is C + ceil(n / C) adds
whatever n is, the result is still bitwise the same run to run, and for a destination of at most C entries it is bit for bit
the unchunked result.  Nothing is read back, so the path runs under `torch.cuda.set_sync_debug_mode("error")` and inside a
captured graph.  The order contract is stated in csrc/gather_chunk_abi.hpp.

The entry points are extern "C" symbols of libgrandplus.so declared in csrc/gather_chunk_abi.hpp; they are not part of
C ABI 4, so `_native.PRIVATE_ABI` binds them, not `_native.ABI`.
"""
from __future__ import annotations

import torch

from . import _native

__all__ = ["MIN_CHUNK", "MAX_CHUNK", "check_chunk", "resolve", "scratch_bytes", "scratch"]

MIN_CHUNK, MAX_CHUNK = 64, 4096


def lib():
    """`_native.lib()`, looked up at each call: this module binds nothing, and a patch of `_native.lib` reaches it."""
    return _native.lib()


def check_chunk(segment_chunk):
    """`segment_chunk` as None or an int that is a power of two in [64, 4096] (ValueError otherwise)."""
    if segment_chunk is None:
        return None
    c = segment_chunk
    if isinstance(c, bool) or not isinstance(c, int) or not MIN_CHUNK <= c <= MAX_CHUNK or c & (c - 1):
        raise ValueError(f"segment_chunk must be None or a power of two in [{MIN_CHUNK}, {MAX_CHUNK}], got {segment_chunk!r}")
    return c


def resolve(segment_chunk, deterministic, what):
    """`segment_chunk` checked for a call of `what` whose backward mode resolved to `deterministic`.  The keyword cuts the
    deterministic backward's segments; with the atomic backward it would do nothing, and that is refused (ValueError)
    rather than ignored: a silent no-op would hide a misconfiguration."""
    c = check_chunk(segment_chunk)
    if c is not None and not deterministic:
        raise ValueError(f"segment_chunk= of {what} chunks the deterministic backward's segment sums: it needs deterministic=True "
                         "(or torch's deterministic mode); the atomic backward has no segments to cut")
    return c


def scratch_bytes(n_sorted, chunk, width):
    """GP_GATHER_CHUNK_SCRATCH_BYTES of gather_chunk_abi.hpp: two float rows of `width` per span of `chunk` positions."""
    return 2 * ((n_sorted + chunk - 1) // chunk) * width * 4


def scratch(n_sorted, chunk, width, device):
    """The scratch of one chunked backward, from torch's caching allocator (uninitialised: the kernels write what they
    read), and its size in bytes."""
    nbytes = scratch_bytes(n_sorted, chunk, width)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), nbytes
