"""lab5 operator: ascending in-place sort of the reference's binary lab5
fixtures' element types (lab5/data/{int10,float10,uchar10}; SURVEY §4 — the
reference ships the inputs but no program, so the order contract is ours),
and the stable key-value forms built on the same radix passes: sort_pairs_,
argsort and the out-of-place sort, ascending or descending."""

from __future__ import annotations

import numpy as np
import torch

from .. import _native

DTYPES = {torch.int32: 0, torch.float32: 1, torch.uint8: 2}
FIXTURE_DTYPES = {"int": np.int32, "float": np.float32, "uchar": np.uint8}


def sort_(x: torch.Tensor) -> torch.Tensor:
    """Sort a contiguous int32 / float32 / uint8 tensor ascending, in place
    (flattened). Floats follow the IEEE total order of their bit patterns
    (-NaN < -inf < -0.0 < +0.0 < +inf < +NaN). GPU tensors run the gfx950
    radix (int32/float32, bitonic for n <= 4096) / counting-sort (uint8)
    kernels with scratch from torch's caching allocator on the tensor's stream;
    CPU tensors run the C reference."""
    if x.dtype not in DTYPES:
        raise ValueError("sort_ supports int32, float32 and uint8")
    if not x.is_contiguous():
        raise ValueError("input must be contiguous")
    L = _native.lib()
    if x.is_cuda:
        dt = DTYPES[x.dtype]
        nbytes = int(L.mpx_sort_workspace_bytes(x.numel(), dt))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device) if nbytes else None
        _native.check(L.mpx_sort_ws(x.data_ptr(), x.numel(), dt, ws.data_ptr() if ws is not None else None, nbytes,
                                    _native.stream_of(x)))
    else:
        L.mpx_cpu_sort(x.data_ptr(), x.numel(), DTYPES[x.dtype])
    return x


PAIR_KEY_DTYPES = {torch.int32: 0, torch.float32: 1}
SORT_IOTA, SORT_DESCENDING = 1, 2  # MPX_SORT_IOTA, MPX_SORT_DESCENDING (capi.h)
MAX_PAIRS = 1 << 30  # 30-bit radix counts, 32-bit payload index


def _pairs(keys: torch.Tensor, values: torch.Tensor, flags: int) -> None:
    """mpx_sort_pairs_ws / mpx_cpu_sort_pairs on checked arguments."""
    L = _native.lib()
    n, dt = keys.numel(), PAIR_KEY_DTYPES[keys.dtype]
    if keys.is_cuda:
        nbytes = int(L.mpx_sort_pairs_workspace_bytes(n, dt))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=keys.device) if nbytes else None
        with torch.cuda.device(keys.device):
            _native.check(L.mpx_sort_pairs_ws(keys.data_ptr(), values.data_ptr(), n, dt, flags,
                                              ws.data_ptr() if ws is not None else None, nbytes,
                                              _native.stream_of(keys)))
    else:
        L.mpx_cpu_sort_pairs(keys.data_ptr(), values.data_ptr(), n, dt, flags)


def _check_keys(x: torch.Tensor, allowed, what: str) -> None:
    if x.dtype not in allowed:
        raise ValueError(f"{what} supports {', '.join(str(d).split('.')[-1] for d in allowed)} keys, not {x.dtype}")
    if not x.is_contiguous():
        raise ValueError("input must be contiguous")
    if x.numel() >= MAX_PAIRS:
        raise ValueError("key-value sorts take fewer than 2^30 elements")


def sort_pairs_(keys: torch.Tensor, values: torch.Tensor, descending: bool = False):
    """Stable key-value sort in place (both flattened): ``keys`` is a contiguous
    int32 / float32 tensor (floats in the IEEE total order of ``sort_``),
    ``values`` a contiguous tensor of the same numel and device with a 4-byte
    dtype (int32, float32, ...) whose bits move with their key and are never
    interpreted. Equal keys keep their input order, ascending and descending
    (``torch.sort(stable=True, descending=True)``'s rule). Fewer than 2^30
    elements. GPU tensors run the gfx950 pairs radix sort with scratch from
    torch's caching allocator on the tensor's stream; CPU tensors run the C
    reference. Returns ``(keys, values)``."""
    _check_keys(keys, PAIR_KEY_DTYPES, "sort_pairs_")
    if values.element_size() != 4 or values.is_complex():
        raise ValueError("values must have a 4-byte dtype (int32, float32)")
    if not values.is_contiguous():
        raise ValueError("values must be contiguous")
    if values.numel() != keys.numel():
        raise ValueError(f"keys have {keys.numel()} elements, values {values.numel()}")
    if values.device != keys.device:
        raise ValueError(f"keys are on {keys.device}, values on {values.device}")
    _pairs(keys, values, SORT_DESCENDING if descending else 0)
    return keys, values


def _sorted_with_indices(x: torch.Tensor, descending: bool, what: str):
    _check_keys(x, DTYPES, what)
    # uint8 keys are widened to int32: correct, untuned (four radix passes where one would do)
    keys = x.to(torch.int32) if x.dtype == torch.uint8 else x.clone()
    idx = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    _pairs(keys, idx, SORT_IOTA | (SORT_DESCENDING if descending else 0))
    return keys, idx


def argsort(x: torch.Tensor, descending: bool = False) -> torch.Tensor:
    """The stable sorting permutation of a contiguous int32 / float32 / uint8
    tensor (flattened): ``x.flatten()[argsort(x)]`` is sorted, equal keys in
    input order in both directions. ``x`` is left untouched (the keys are
    sorted in a scratch copy). The indices are **int32** — a sort takes fewer
    than 2^30 elements — so a caller who needs int64 converts. The index is
    generated inside the first radix pass, not filled and loaded. uint8 keys
    take the int32 path after widening: correct but untuned."""
    return _sorted_with_indices(x, descending, "argsort")[1]


def sort(x: torch.Tensor, descending: bool = False):
    """Out-of-place stable sort: ``(values, indices)`` as ``torch.sort(x,
    stable=True, descending=descending)`` on the flattened tensor, except that
    floats follow the IEEE total order of ``sort_`` and the indices are
    **int32** (fewer than 2^30 elements; convert for int64). uint8 keys are
    widened to int32 for the sort: correct but untuned."""
    keys, idx = _sorted_with_indices(x, descending, "sort")
    return (keys.to(torch.uint8) if x.dtype == torch.uint8 else keys), idx


def read_fixture(path: str, kind: str) -> np.ndarray:
    """A lab5 binary array: little-endian int32 n, then n elements of ``kind``
    (int / float / uchar)."""
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw[:4], dtype="<i4")[0])
    dt = np.dtype(FIXTURE_DTYPES[kind]).newbyteorder("<")
    if len(raw) != 4 + n * dt.itemsize:
        raise ValueError(f"{path}: size {len(raw)} does not match n = {n} of {kind}")
    return np.frombuffer(raw[4:], dtype=dt).astype(FIXTURE_DTYPES[kind])
