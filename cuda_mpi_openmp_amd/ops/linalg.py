"""lab4 operators: dense LU with partial pivoting in fp64 and what follows from
its factors (solve, log-determinant, unpacking). The matrix lab has no reference
program, so the contract is this package's (capi.h, ``mpx_lu_factor_f64``):
LAPACK ``getrf`` storage, 0-based int32 pivots, the lowest row among equal
magnitudes, ``info = k + 1`` for the first exactly zero pivot.

GPU tensors run the gfx950 kernels (the trailing update on
``v_mfma_f64_16x16x4_f64``) on the tensor's current stream with scratch from
torch's allocator; CPU tensors run the unblocked OpenMP reference. The MFMA's
accumulation order is unspecified, so the two agree to the componentwise
backward-error bounds of LU, not bit for bit (tests/test_lu.py)."""

from __future__ import annotations

import torch

from .. import _native


def _check_matrix(a: torch.Tensor, what: str) -> int:
    if not isinstance(a, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if a.dtype != torch.float64:
        raise ValueError(f"{what} must be float64 (fp64 only), not {a.dtype}")
    if a.dim() != 2:
        raise ValueError(f"{what} must be 2-D, not {a.dim()}-D")
    n = a.shape[0]
    if a.shape[1] != n:
        raise ValueError(f"{what} must be square, not {tuple(a.shape)}")
    if n >= 2 ** 31:
        raise ValueError(f"{what} is too large")
    if n and a.stride(1) != 1:
        raise ValueError(f"{what} must have contiguous rows (stride(1) == 1)")
    if n > 1 and a.stride(0) < n:
        raise ValueError(f"{what} must have a row stride of at least n")
    return n


def _pitch(a: torch.Tensor, width: int) -> int:
    return max(a.stride(0), width) if a.shape[0] > 1 else width


def lu_factor_(a: torch.Tensor):
    """LU with partial pivoting of a square float64 matrix, in place. Rows must
    be contiguous; any row stride >= n is honoured as the pitch (a column slice
    of a wider tensor works, its padding is never touched). Returns
    ``(a, piv, info)``: L (unit lower, below the diagonal) and U in ``a``,
    ``piv[k]`` the 0-based row interchanged with row k (int32), ``info`` a
    one-element int32 tensor on ``a``'s device: 0, or k + 1 for the first
    exactly zero pivot (that column is left as it is and elimination goes on).
    No host synchronisation."""
    n = _check_matrix(a, "A")
    piv = torch.empty(n, dtype=torch.int32, device=a.device)
    if n == 0:
        return a, piv, torch.zeros(1, dtype=torch.int32, device=a.device)
    info = torch.empty(1, dtype=torch.int32, device=a.device)
    L = _native.lib()
    if a.is_cuda:
        nbytes = int(L.mpx_lu_workspace_bytes(n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        with torch.cuda.device(a.device):
            _native.check(L.mpx_lu_factor_f64(a.data_ptr(), n, _pitch(a, n), piv.data_ptr(), info.data_ptr(),
                                              ws.data_ptr(), nbytes, _native.stream_of(a)))
    else:
        L.mpx_cpu_lu_factor_f64(a.data_ptr(), n, _pitch(a, n), piv.data_ptr(), info.data_ptr())
    return a, piv, info


def lu_factor(a: torch.Tensor):
    """``lu_factor_`` on a contiguous copy; ``a`` is left untouched."""
    _check_matrix(a, "A")
    return lu_factor_(a.clone(memory_format=torch.contiguous_format))


def _check_solve(lu: torch.Tensor, piv: torch.Tensor, b: torch.Tensor) -> int:
    n = _check_matrix(lu, "LU")
    if not isinstance(piv, torch.Tensor) or piv.dtype != torch.int32 or piv.dim() != 1 or piv.shape[0] != n:
        raise ValueError(f"piv must be an int32 vector of {n} elements")
    if not piv.is_contiguous():
        raise ValueError("piv must be contiguous")
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float64:
        raise ValueError("B must be float64 (fp64 only)")
    if b.dim() not in (1, 2):
        raise ValueError(f"B must be (n,) or (n, k), not {b.dim()}-D")
    if b.shape[0] != n:
        raise ValueError(f"B has {b.shape[0]} rows, LU {n}")
    if piv.device != lu.device or b.device != lu.device:
        raise ValueError(f"LU is on {lu.device}, piv on {piv.device}, B on {b.device}")
    return n


def lu_solve_(lu: torch.Tensor, piv: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Solve A X = B in place in ``b`` ((n,) or (n, k), float64) with the
    factors of ``lu_factor``: rows interchanged by ``piv``, forward substitution
    with unit L, back substitution with U. A 2-D ``b`` needs contiguous rows
    (any row stride >= k is the pitch); a 1-D ``b`` may have any stride."""
    n = _check_solve(lu, piv, b)
    if b.dim() == 1:
        nrhs, pitch_b = 1, (max(b.stride(0), 1) if n > 1 else 1)
        if n > 1 and b.stride(0) < 1:
            raise ValueError("B must have a positive stride")
    else:
        nrhs = b.shape[1]
        if nrhs and b.stride(1) != 1:
            raise ValueError("B must have contiguous rows (stride(1) == 1)")
        if n > 1 and b.stride(0) < nrhs:
            raise ValueError("B must have a row stride of at least its width")
        pitch_b = _pitch(b, nrhs)
    if n == 0 or nrhs == 0:
        return b
    L = _native.lib()
    if lu.is_cuda:
        with torch.cuda.device(lu.device):
            _native.check(L.mpx_lu_solve_f64(lu.data_ptr(), n, _pitch(lu, n), piv.data_ptr(), b.data_ptr(), nrhs,
                                             pitch_b, None, 0, _native.stream_of(lu)))
    else:
        L.mpx_cpu_lu_solve_f64(lu.data_ptr(), n, _pitch(lu, n), piv.data_ptr(), b.data_ptr(), nrhs, pitch_b)
    return b


def lu_solve(lu: torch.Tensor, piv: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``lu_solve_`` on a contiguous copy of ``b``."""
    _check_solve(lu, piv, b)
    return lu_solve_(lu, piv, b.clone(memory_format=torch.contiguous_format))


def solve(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """X with A X = B: factor a copy of ``a``, read ``info`` (the one host
    read), solve on a copy of ``b``. A singular matrix (an exactly zero pivot)
    raises ``RuntimeError`` naming the pivot's column."""
    n = _check_matrix(a, "A")
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float64:
        raise ValueError("B must be float64 (fp64 only)")
    if b.dim() not in (1, 2) or b.shape[0] != n:
        raise ValueError(f"B must be ({n},) or ({n}, k), not {tuple(b.shape)}")
    if b.device != a.device:
        raise ValueError(f"A is on {a.device}, B on {b.device}")
    lu, piv, info = lu_factor(a)
    k = int(info.item())
    if k:
        raise RuntimeError(f"solve: the matrix is singular (zero pivot in column {k - 1})")
    return lu_solve(lu, piv, b)


def slogdet(lu: torch.Tensor, piv: torch.Tensor):
    """``(sign, logabsdet)`` of the factored matrix: the diagonal of U and the
    parity of the interchanges (0-dim float64 tensors, no host read)."""
    n = _check_matrix(lu, "LU")
    if piv.dtype != torch.int32 or piv.dim() != 1 or piv.shape[0] != n or piv.device != lu.device:
        raise ValueError(f"piv must be an int32 vector of {n} elements on {lu.device}")
    d = torch.diagonal(lu)
    swaps = (piv != torch.arange(n, dtype=torch.int32, device=lu.device)).sum()
    sign = torch.sign(d).prod() * (1 - 2 * (swaps % 2)).to(torch.float64)
    return sign, torch.log(torch.abs(d)).sum()


def lu_unpack(lu: torch.Tensor, piv: torch.Tensor):
    """``(perm, L, U)`` with ``A[perm] = L @ U``: ``perm`` (int64) is the row
    order the interchanges produce (reads ``piv`` on the host)."""
    n = _check_matrix(lu, "LU")
    if piv.dtype != torch.int32 or piv.dim() != 1 or piv.shape[0] != n or piv.device != lu.device:
        raise ValueError(f"piv must be an int32 vector of {n} elements on {lu.device}")
    perm = list(range(n))
    for k, p in enumerate(piv.tolist()):
        perm[k], perm[p] = perm[p], perm[k]
    low = torch.tril(lu, -1) + torch.eye(n, dtype=lu.dtype, device=lu.device)
    return torch.tensor(perm, dtype=torch.int64, device=lu.device), low, torch.triu(lu)
