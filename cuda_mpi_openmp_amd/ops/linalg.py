"""lab4 operators: dense LU with partial pivoting in fp64 and what follows from
its factors (solve, log-determinant, unpacking), and further down the
Cholesky factorisation of symmetric positive definite matrices (``cholesky_*``,
``solve_spd``, ``logdet_spd``; the contract is capi.h's ``mpx_chol_factor_f64``). The matrix lab has no reference
program, so the contract is this package's (capi.h, ``mpx_lu_factor_f64``):
LAPACK ``getrf`` storage, 0-based int32 pivots, the lowest row among equal
magnitudes, ``info = k + 1`` for the first exactly zero pivot.

GPU tensors run the gfx950 kernels (the trailing update on
``v_mfma_f64_16x16x4_f64``) on the tensor's current stream with scratch from
torch's allocator; CPU tensors run the unblocked OpenMP reference. The MFMA's
accumulation order is unspecified, so the two agree to the componentwise
backward-error bounds of LU, not bit for bit (tests/test_lu.py).

The last section is Householder QR of a tall or square matrix (``qr_factor*``,
``qr_mul_q*``, ``qr_solve_r_``, ``qr_unpack``, ``lstsq``; the contract is
capi.h's ``mpx_qr_factor_f64``): LAPACK ``geqrf`` storage, ``dlarfg``'s sign rule
without its rescaling. There too the GPU (block reflectors on the MFMA, its own
fixed reduction orders over the rows) and the CPU reference (rows summed in
ascending order) agree to Householder QR's backward-error bounds, not bit for
bit, and exactly where every intermediate is exactly representable
(tests/test_qr.py).

The ``*_batched`` functions take ``(B, n, n)``. For n <= 64 the whole batch is
one launch of plain VALU kernels in the CPU reference's operation order
(lu_batched.hip), and there GPU and CPU do agree bit for bit, matrix by matrix
(tests/test_lu_batched.py); larger n loops over the single-matrix kernels. The
same holds for ``cholesky_*_batched``, ``solve_spd_batched`` and
``logdet_spd_batched`` (chol_batched.hip, tests/test_cholesky_batched.py)."""

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


def _b_layout(b: torch.Tensor, rows: int):
    """``(nrhs, pitch_b)`` of a right-hand side solved in place: ``lu_solve_``'s stride rules."""
    if b.dim() == 1:
        if rows > 1 and b.stride(0) < 1:
            raise ValueError("B must have a positive stride")
        return 1, (max(b.stride(0), 1) if rows > 1 else 1)
    nrhs = b.shape[1]
    if nrhs and b.stride(1) != 1:
        raise ValueError("B must have contiguous rows (stride(1) == 1)")
    if rows > 1 and b.stride(0) < nrhs:
        raise ValueError("B must have a row stride of at least its width")
    return nrhs, _pitch(b, nrhs)


def _check_rhs(b: torch.Tensor, rows: int, factors: torch.Tensor, what: str, *, in_place: bool = False,
               letter: str = "n", owner: str | None = None, sized: bool = False, piv: torch.Tensor | None = None):
    """The checks of a right-hand side ``b`` ((rows,) or (rows, k), float64, on
    ``factors``' device; ``what`` is ``factors``' name in the messages).
    ``in_place``: ``b`` is solved where it lies, so ``_b_layout``'s stride rules
    hold too and ``(nrhs, pitch_b)`` is returned; the functions that work on a
    contiguous copy take any strides. The rest only picks a wording: ``letter``
    names the row count, ``owner`` the matrix of the row-count message where it
    is not ``what``, ``sized`` is the wording of the functions that factor a
    copy (one message with the sizes for dimension and row count), ``piv`` are
    LU's pivots, which its device message names."""
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float64:
        raise ValueError("B must be float64 (fp64 only)")
    if sized:
        if b.dim() not in (1, 2) or b.shape[0] != rows:
            raise ValueError(f"B must be ({rows},) or ({rows}, k), not {tuple(b.shape)}")
    else:
        if b.dim() not in (1, 2):
            raise ValueError(f"B must be ({letter},) or ({letter}, k), not {b.dim()}-D")
        if b.shape[0] != rows:
            raise ValueError(f"B has {b.shape[0]} rows, {owner or what} {rows}")
    if piv is not None:
        if piv.device != factors.device or b.device != factors.device:
            raise ValueError(f"{what} is on {factors.device}, piv on {piv.device}, B on {b.device}")
    elif b.device != factors.device:
        raise ValueError(f"{what} is on {factors.device}, B on {b.device}")
    return _b_layout(b, rows) if in_place else None


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


def _check_solve(lu: torch.Tensor, piv: torch.Tensor, b: torch.Tensor, in_place: bool = False):
    n = _check_matrix(lu, "LU")
    if not isinstance(piv, torch.Tensor) or piv.dtype != torch.int32 or piv.dim() != 1 or piv.shape[0] != n:
        raise ValueError(f"piv must be an int32 vector of {n} elements")
    if not piv.is_contiguous():
        raise ValueError("piv must be contiguous")
    return n, _check_rhs(b, n, lu, "LU", in_place=in_place, piv=piv)


def lu_solve_(lu: torch.Tensor, piv: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Solve A X = B in place in ``b`` ((n,) or (n, k), float64) with the
    factors of ``lu_factor``: rows interchanged by ``piv``, forward substitution
    with unit L, back substitution with U. A 2-D ``b`` needs contiguous rows
    (any row stride >= k is the pitch); a 1-D ``b`` may have any stride."""
    n, (nrhs, pitch_b) = _check_solve(lu, piv, b, in_place=True)
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
    _check_rhs(b, _check_matrix(a, "A"), a, "A", sized=True)
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


# ---------------------------------------------------------------- batched: (B, n, n)
def _check_batch(a: torch.Tensor, what: str):
    if not isinstance(a, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if a.dtype != torch.float64:
        raise ValueError(f"{what} must be float64 (fp64 only), not {a.dtype}")
    if a.dim() != 3:
        raise ValueError(f"{what} must be 3-D (batch, n, n), not {a.dim()}-D")
    batch, n = a.shape[0], a.shape[1]
    if a.shape[2] != n:
        raise ValueError(f"{what} must be a batch of square matrices, not {tuple(a.shape)}")
    if n >= 2 ** 31 or batch >= 2 ** 31:
        raise ValueError(f"{what} is too large")
    if n > 1 and a.stride(2) != 1:
        raise ValueError(f"{what} must have contiguous rows (stride(2) == 1)")
    if n > 1 and a.stride(1) < n:
        raise ValueError(f"{what} must have a row stride of at least n")
    pitch = a.stride(1) if n > 1 else max(n, 1)
    span = (n - 1) * pitch + n
    if batch > 1 and n and a.stride(0) < span:
        raise ValueError(f"{what} must have a batch stride of at least (n - 1) * stride(1) + n")
    return batch, n, pitch, (a.stride(0) if batch > 1 else span)


def _check_batch_piv(piv: torch.Tensor, lu: torch.Tensor, batch: int, n: int) -> None:
    if (not isinstance(piv, torch.Tensor) or piv.dtype != torch.int32 or piv.dim() != 2
            or tuple(piv.shape) != (batch, n)):
        raise ValueError(f"piv must be an int32 tensor of shape ({batch}, {n})")
    if not piv.is_contiguous():
        raise ValueError("piv must be contiguous")
    if piv.device != lu.device:
        raise ValueError(f"LU is on {lu.device}, piv on {piv.device}")


def lu_factor_batched_(a: torch.Tensor):
    """LU with partial pivoting of every matrix of a float64 batch ``(B, n, n)``,
    in place: per matrix exactly ``lu_factor_`` of the CPU reference (bit for
    bit for n <= 64, where the whole batch is one launch; larger n loops over
    ``lu_factor_``'s kernels). Rows must be contiguous; any row stride >= n and
    any batch stride >= (n - 1) * stride(1) + n are honoured (a slice of a
    larger buffer works, its padding is never touched). Returns
    ``(a, piv (B, n) int32, info (B,) int32)``; ``info[m]`` is 0, or k + 1 for
    matrix m's first exactly zero pivot. No host synchronisation."""
    batch, n, pitch, stride = _check_batch(a, "A")
    piv = torch.empty((batch, n), dtype=torch.int32, device=a.device)
    if batch == 0 or n == 0:
        return a, piv, torch.zeros(batch, dtype=torch.int32, device=a.device)
    info = torch.empty(batch, dtype=torch.int32, device=a.device)
    L = _native.lib()
    if a.is_cuda:
        nbytes = int(L.mpx_lu_batched_workspace_bytes(batch, n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device) if nbytes else None
        with torch.cuda.device(a.device):
            _native.check(L.mpx_lu_factor_batched_f64(a.data_ptr(), batch, n, pitch, stride, piv.data_ptr(),
                                                      info.data_ptr(), ws.data_ptr() if nbytes else None, nbytes,
                                                      _native.stream_of(a)))
    else:
        L.mpx_cpu_lu_factor_batched_f64(a.data_ptr(), batch, n, pitch, stride, piv.data_ptr(), info.data_ptr())
    return a, piv, info


def lu_factor_batched(a: torch.Tensor):
    """``lu_factor_batched_`` on a contiguous copy; ``a`` is left untouched."""
    _check_batch(a, "A")
    return lu_factor_batched_(a.clone(memory_format=torch.contiguous_format))


def _check_batch_b(b: torch.Tensor, factors: torch.Tensor, what: str, batch: int, n: int) -> None:
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float64:
        raise ValueError("B must be float64 (fp64 only)")
    if b.dim() not in (2, 3):
        raise ValueError(f"B must be (batch, n) or (batch, n, k), not {b.dim()}-D")
    if b.shape[0] != batch or b.shape[1] != n:
        raise ValueError(f"B must be ({batch}, {n}) or ({batch}, {n}, k), not {tuple(b.shape)}")
    if b.device != factors.device:
        raise ValueError(f"{what} is on {factors.device}, B on {b.device}")


def _check_solve_batched(lu: torch.Tensor, piv: torch.Tensor, b: torch.Tensor):
    batch, n, pitch, stride = _check_batch(lu, "LU")
    _check_batch_piv(piv, lu, batch, n)
    _check_batch_b(b, lu, "LU", batch, n)
    return batch, n, pitch, stride


def _batch_b_layout(b: torch.Tensor, batch: int, n: int):
    """``(nrhs, pitch_b, stride_b)`` of a checked batched right-hand side that is
    solved in place: a 3-D ``b`` needs contiguous rows, a 2-D one any positive
    element stride, and the members must not overlap."""
    if b.dim() == 2:
        nrhs = 1
        if n > 1 and b.stride(1) < 1:
            raise ValueError("B must have a positive stride")
        pitch_b = b.stride(1) if n > 1 else 1
    else:
        nrhs = b.shape[2]
        if nrhs > 1 and b.stride(2) != 1:
            raise ValueError("B must have contiguous rows (stride(2) == 1)")
        if n > 1 and b.stride(1) < nrhs:
            raise ValueError("B must have a row stride of at least its width")
        pitch_b = b.stride(1) if n > 1 else max(nrhs, 1)
    span_b = (n - 1) * pitch_b + nrhs
    if batch > 1 and n and nrhs and b.stride(0) < span_b:
        raise ValueError("B must have a batch stride of at least (n - 1) * stride(1) + k")
    return nrhs, pitch_b, (b.stride(0) if batch > 1 else span_b)


def lu_solve_batched_(lu: torch.Tensor, piv: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Solve A_m X_m = B_m in place in ``b`` ((B, n, k) or (B, n), float64) with
    the factors of ``lu_factor_batched``: per matrix exactly ``lu_solve_`` of the
    CPU reference (bit for bit for n <= 64, one launch). A 3-D ``b`` needs
    contiguous rows; any row stride >= k and batch stride >= (n - 1) * stride(1)
    + k are honoured. A 2-D ``b`` may have any positive element stride."""
    batch, n, pitch, stride = _check_solve_batched(lu, piv, b)
    nrhs, pitch_b, stride_b = _batch_b_layout(b, batch, n)
    if batch == 0 or n == 0 or nrhs == 0:
        return b
    L = _native.lib()
    if lu.is_cuda:
        with torch.cuda.device(lu.device):
            _native.check(L.mpx_lu_solve_batched_f64(lu.data_ptr(), batch, n, pitch, stride, piv.data_ptr(),
                                                     b.data_ptr(), nrhs, pitch_b, stride_b, _native.stream_of(lu)))
    else:
        L.mpx_cpu_lu_solve_batched_f64(lu.data_ptr(), batch, n, pitch, stride, piv.data_ptr(), b.data_ptr(), nrhs,
                                       pitch_b, stride_b)
    return b


def lu_solve_batched(lu: torch.Tensor, piv: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``lu_solve_batched_`` on a contiguous copy of ``b``."""
    _check_solve_batched(lu, piv, b)
    return lu_solve_batched_(lu, piv, b.clone(memory_format=torch.contiguous_format))


def _raise_if_singular(info: torch.Tensor, who: str) -> None:
    """The one host read: the first singular member of the batch and its column."""
    host = info.tolist()
    for m, k in enumerate(host):
        if k:
            raise RuntimeError(f"{who}: matrix {m} of the batch is singular (zero pivot in column {k - 1})")


def solve_batched(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """X with A_m X_m = B_m for every member: factor a copy of ``a``, read
    ``info`` (the one host read), solve on a copy of ``b``. A singular member
    raises ``RuntimeError`` naming the first such batch index and its column."""
    batch, n, _, _ = _check_batch(a, "A")
    _check_batch_b(b, a, "A", batch, n)
    lu, piv, info = lu_factor_batched(a)
    _raise_if_singular(info, "solve_batched")
    return lu_solve_batched(lu, piv, b)


def slogdet_batched(lu: torch.Tensor, piv: torch.Tensor):
    """``(sign (B,), logabsdet (B,))`` of the factored matrices: the diagonals
    of U and the parity of the interchanges (float64, no host read)."""
    batch, n, _, _ = _check_batch(lu, "LU")
    _check_batch_piv(piv, lu, batch, n)
    d = torch.diagonal(lu, dim1=1, dim2=2)
    swaps = (piv != torch.arange(n, dtype=torch.int32, device=lu.device)).sum(dim=1)
    sign = torch.sign(d).prod(dim=1) * (1 - 2 * (swaps % 2)).to(torch.float64)
    return sign, torch.log(torch.abs(d)).sum(dim=1)


def lu_unpack_batched(lu: torch.Tensor, piv: torch.Tensor):
    """``(perm (B, n) int64, L, U)`` with ``A[m][perm[m]] = L[m] @ U[m]`` (reads
    ``piv`` on the host)."""
    batch, n, _, _ = _check_batch(lu, "LU")
    _check_batch_piv(piv, lu, batch, n)
    host = piv.cpu()
    perm = torch.arange(n, dtype=torch.int64).repeat(batch, 1)
    rows = torch.arange(batch)
    for k in range(n):
        p = host[:, k].long()
        at_k, at_p = perm[rows, k].clone(), perm[rows, p].clone()
        perm[rows, k] = at_p
        perm[rows, p] = at_k
    low = torch.tril(lu, -1) + torch.eye(n, dtype=lu.dtype, device=lu.device)
    return perm.to(lu.device), low, torch.triu(lu)


# ---------------------------------------------------------------- Cholesky: SPD, lower storage
def cholesky_factor_(a: torch.Tensor):
    """Cholesky factorisation A = L Lᵀ of a symmetric positive definite float64
    matrix, in place, lower storage: only the lower triangle of ``a`` (diagonal
    included) is read, and it holds L on return; the strict upper triangle and
    any pitch padding are never read or written. Rows must be contiguous; any
    row stride >= n is the pitch. Returns ``(a, info)``; ``info`` is a
    one-element int32 tensor on ``a``'s device: 0, or j + 1 for the first column
    whose reduced diagonal is not > 0 (zero, negative or NaN: not positive
    definite). Columns before it are valid factor columns, the rest is
    unspecified. GPU tensors run chol.hip on the current stream (two launches
    per 64 columns, the update on ``v_mfma_f64_16x16x4_f64``), CPU tensors the
    unblocked reference; columns 0..63 agree bit for bit, the rest to Cholesky's
    backward-error bounds (tests/test_cholesky.py). No host synchronisation."""
    n = _check_matrix(a, "A")
    if n == 0:
        return a, torch.zeros(1, dtype=torch.int32, device=a.device)
    info = torch.empty(1, dtype=torch.int32, device=a.device)
    L = _native.lib()
    if a.is_cuda:
        with torch.cuda.device(a.device):
            _native.check(L.mpx_chol_factor_f64(a.data_ptr(), n, _pitch(a, n), info.data_ptr(), _native.stream_of(a)))
    else:
        L.mpx_cpu_chol_factor_f64(a.data_ptr(), n, _pitch(a, n), info.data_ptr())
    return a, info


def cholesky_factor(a: torch.Tensor):
    """``cholesky_factor_`` on a contiguous copy; ``a`` is left untouched (the
    copy's upper triangle is ``a``'s)."""
    _check_matrix(a, "A")
    return cholesky_factor_(a.clone(memory_format=torch.contiguous_format))


def _check_cholesky_solve(l: torch.Tensor, b: torch.Tensor, in_place: bool = False):
    n = _check_matrix(l, "L")
    return n, _check_rhs(b, n, l, "L", in_place=in_place)


def cholesky_solve_(l: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Solve A X = B in place in ``b`` ((n,) or (n, k), float64) with the factor
    of ``cholesky_factor``: forward substitution with L, back substitution with
    Lᵀ, both dividing by the diagonal; only L's lower triangle is read. ``b``
    has ``lu_solve_``'s stride rules: a 2-D ``b`` needs contiguous rows (any row
    stride >= k is the pitch), a 1-D ``b`` may have any positive stride."""
    n, (nrhs, pitch_b) = _check_cholesky_solve(l, b, in_place=True)
    if n == 0 or nrhs == 0:
        return b
    L = _native.lib()
    if l.is_cuda:
        with torch.cuda.device(l.device):
            _native.check(L.mpx_chol_solve_f64(l.data_ptr(), n, _pitch(l, n), b.data_ptr(), nrhs, pitch_b,
                                               _native.stream_of(l)))
    else:
        L.mpx_cpu_chol_solve_f64(l.data_ptr(), n, _pitch(l, n), b.data_ptr(), nrhs, pitch_b)
    return b


def cholesky_solve(l: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``cholesky_solve_`` on a contiguous copy of ``b``."""
    _check_cholesky_solve(l, b)
    return cholesky_solve_(l, b.clone(memory_format=torch.contiguous_format))


def solve_spd(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """X with A X = B for a symmetric positive definite A (its lower triangle is
    what counts): factor a copy of ``a``, read ``info`` (the one host read),
    solve on a copy of ``b``. A matrix that is not positive definite raises
    ``RuntimeError`` naming the column where the factorisation broke down."""
    _check_rhs(b, _check_matrix(a, "A"), a, "A", sized=True)
    l, info = cholesky_factor(a)
    k = int(info.item())
    if k:
        raise RuntimeError(f"solve_spd: the matrix is not positive definite (column {k - 1})")
    return cholesky_solve(l, b)


def logdet_spd(l: torch.Tensor) -> torch.Tensor:
    """log det A = 2 Σ log l_ii from the factor of ``cholesky_factor`` (a 0-dim
    float64 tensor, no host read)."""
    _check_matrix(l, "L")
    return 2.0 * torch.log(torch.diagonal(l)).sum()


# ---------------------------------------------------------------- batched Cholesky: (B, n, n), lower storage
def cholesky_factor_batched_(a: torch.Tensor):
    """Cholesky factorisation of every member of a float64 batch ``(B, n, n)``
    of symmetric positive definite matrices, in place, lower storage: per
    member exactly ``cholesky_factor_`` of the CPU reference (bit for bit for
    n <= 64, where the whole batch is one launch of chol_batched.hip; larger n
    loops over ``cholesky_factor_``'s kernels). Only the lower triangles
    (diagonals included) are read or written. Rows must be contiguous; any row
    stride >= n and any batch stride >= (n - 1) * stride(1) + n are honoured (a
    slice of a larger buffer works, its padding is never touched). Returns
    ``(a, info (B,) int32)``; ``info[m]`` is 0, or j + 1 for member m's first
    column whose reduced diagonal is not > 0 (zero, negative or NaN); such a
    member changes nothing in any other. No host synchronisation."""
    batch, n, pitch, stride = _check_batch(a, "A")
    if batch == 0 or n == 0:
        return a, torch.zeros(batch, dtype=torch.int32, device=a.device)
    info = torch.empty(batch, dtype=torch.int32, device=a.device)
    L = _native.lib()
    if a.is_cuda:
        with torch.cuda.device(a.device):
            _native.check(L.mpx_chol_factor_batched_f64(a.data_ptr(), batch, n, pitch, stride, info.data_ptr(),
                                                        _native.stream_of(a)))
    else:
        L.mpx_cpu_chol_factor_batched_f64(a.data_ptr(), batch, n, pitch, stride, info.data_ptr())
    return a, info


def cholesky_factor_batched(a: torch.Tensor):
    """``cholesky_factor_batched_`` on a contiguous copy; ``a`` is left
    untouched (the copy's upper triangles are ``a``'s)."""
    _check_batch(a, "A")
    return cholesky_factor_batched_(a.clone(memory_format=torch.contiguous_format))


def _check_cholesky_solve_batched(l: torch.Tensor, b: torch.Tensor):
    batch, n, pitch, stride = _check_batch(l, "L")
    _check_batch_b(b, l, "L", batch, n)
    return batch, n, pitch, stride


def cholesky_solve_batched_(l: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Solve A_m X_m = B_m in place in ``b`` ((B, n, k) or (B, n), float64) with
    the factors of ``cholesky_factor_batched``: per member exactly
    ``cholesky_solve_`` of the CPU reference (bit for bit for n <= 64, one
    launch); only L's lower triangles are read. ``b`` has
    ``lu_solve_batched_``'s stride rules."""
    batch, n, pitch, stride = _check_cholesky_solve_batched(l, b)
    nrhs, pitch_b, stride_b = _batch_b_layout(b, batch, n)
    if batch == 0 or n == 0 or nrhs == 0:
        return b
    L = _native.lib()
    if l.is_cuda:
        with torch.cuda.device(l.device):
            _native.check(L.mpx_chol_solve_batched_f64(l.data_ptr(), batch, n, pitch, stride, b.data_ptr(), nrhs,
                                                       pitch_b, stride_b, _native.stream_of(l)))
    else:
        L.mpx_cpu_chol_solve_batched_f64(l.data_ptr(), batch, n, pitch, stride, b.data_ptr(), nrhs, pitch_b, stride_b)
    return b


def cholesky_solve_batched(l: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``cholesky_solve_batched_`` on a contiguous copy of ``b``."""
    _check_cholesky_solve_batched(l, b)
    return cholesky_solve_batched_(l, b.clone(memory_format=torch.contiguous_format))


def _raise_if_not_spd(info: torch.Tensor, who: str) -> None:
    """The one host read: the first member that is not positive definite and its column."""
    for m, k in enumerate(info.tolist()):
        if k:
            raise RuntimeError(f"{who}: matrix {m} of the batch is not positive definite (column {k - 1})")


def solve_spd_batched(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """X with A_m X_m = B_m for symmetric positive definite members (their
    lower triangles are what counts): factor a copy of ``a``, read ``info`` (the
    one host read), solve on a copy of ``b``. A member that is not positive
    definite raises ``RuntimeError`` naming the first such batch index and the
    column where its factorisation broke down."""
    batch, n, _, _ = _check_batch(a, "A")
    _check_batch_b(b, a, "A", batch, n)
    l, info = cholesky_factor_batched(a)
    _raise_if_not_spd(info, "solve_spd_batched")
    return cholesky_solve_batched(l, b)


def logdet_spd_batched(l: torch.Tensor) -> torch.Tensor:
    """log det A_m = 2 Σ log l_ii from the factors of ``cholesky_factor_batched``
    (a ``(B,)`` float64 tensor, no host read)."""
    _check_batch(l, "L")
    return 2.0 * torch.log(torch.diagonal(l, dim1=1, dim2=2)).sum(dim=1)


# ---------------------------------------------------------------- Householder QR: m >= n, geqrf storage
def _check_tall(a: torch.Tensor, what: str):
    """``_check_matrix`` for a rectangular matrix with at least as many rows as columns."""
    if not isinstance(a, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if a.dtype != torch.float64:
        raise ValueError(f"{what} must be float64 (fp64 only), not {a.dtype}")
    if a.dim() != 2:
        raise ValueError(f"{what} must be 2-D, not {a.dim()}-D")
    m, n = a.shape
    if m < n:
        raise ValueError(f"{what} must have at least as many rows as columns (m >= n), not {tuple(a.shape)}")
    if m >= 2 ** 31:
        raise ValueError(f"{what} is too large")
    if m and n and a.stride(1) != 1:
        raise ValueError(f"{what} must have contiguous rows (stride(1) == 1)")
    if m > 1 and a.stride(0) < n:
        raise ValueError(f"{what} must have a row stride of at least n")
    return m, n


def _check_tau(tau: torch.Tensor, qr: torch.Tensor, n: int) -> None:
    if not isinstance(tau, torch.Tensor) or tau.dtype != torch.float64 or tau.dim() != 1 or tau.shape[0] != n:
        raise ValueError(f"tau must be a float64 vector of {n} elements")
    if not tau.is_contiguous():
        raise ValueError("tau must be contiguous")
    if tau.device != qr.device:
        raise ValueError(f"QR is on {qr.device}, tau on {tau.device}")


def qr_factor_(a: torch.Tensor):
    """Householder QR A = Q R of a float64 matrix with m >= n, in place, in
    LAPACK ``geqrf`` storage. Rows must be contiguous; any row stride >= n is
    the pitch, and the padding is never read or written. Returns
    ``(a, tau, info)``: R in the upper triangle of ``a[:n]``, column j below the
    diagonal holds ``v_j[j+1:]`` (``v_j[j] = 1`` implied), ``tau`` n float64,
    ``H_j = I - tau_j v_j v_jᵀ``, ``Q = H_0 H_1 … H_{n-1}``. The reflectors
    follow LAPACK's ``dlarfg`` without its rescaling (capi.h,
    ``mpx_qr_factor_f64``): ``beta = -copysign(sqrt(alpha² + sigma), alpha)``,
    so the diagonal of R may be negative, and a column that is already zero
    below its diagonal keeps ``tau = 0``. The sums of squares are plain fp64:
    the squares of the entries must neither overflow nor underflow to zero.
    ``info`` is a one-element int32 tensor on ``a``'s device: 0, or j + 1 for
    the first column with ``R_jj == 0`` exactly; the factorisation runs on
    regardless. Two runs give the same bits, and the factorisation of
    ``a[:, :k]`` is the first k columns of that of ``a`` bit for bit. GPU
    tensors run qr.hip on the current stream (one launch per column for the
    panels, the block reflectors on ``v_mfma_f64_16x16x4_f64``), CPU tensors the
    unblocked reference; the two agree to Householder QR's backward-error
    bounds, not bit for bit (tests/test_qr.py). No host synchronisation."""
    m, n = _check_tall(a, "A")
    tau = torch.empty(n, dtype=torch.float64, device=a.device)
    if m == 0 or n == 0:
        return a, tau, torch.zeros(1, dtype=torch.int32, device=a.device)
    info = torch.empty(1, dtype=torch.int32, device=a.device)
    L = _native.lib()
    if a.is_cuda:
        nbytes = int(L.mpx_qr_workspace_bytes(m, n, 0))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        with torch.cuda.device(a.device):
            _native.check(L.mpx_qr_factor_f64(a.data_ptr(), m, n, _pitch(a, n), tau.data_ptr(), info.data_ptr(),
                                              ws.data_ptr(), nbytes, _native.stream_of(a)))
    else:
        L.mpx_cpu_qr_factor_f64(a.data_ptr(), m, n, _pitch(a, n), tau.data_ptr(), info.data_ptr())
    return a, tau, info


def qr_factor(a: torch.Tensor):
    """``qr_factor_`` on a contiguous copy; ``a`` is left untouched."""
    _check_tall(a, "A")
    return qr_factor_(a.clone(memory_format=torch.contiguous_format))


def _check_mul_q(qr: torch.Tensor, tau: torch.Tensor, b: torch.Tensor, in_place: bool = False):
    m, n = _check_tall(qr, "QR")
    _check_tau(tau, qr, n)
    return m, n, _check_rhs(b, m, qr, "QR", in_place=in_place, letter="m")


def qr_mul_q_(qr: torch.Tensor, tau: torch.Tensor, b: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """``b <- Q b`` (or ``Qᵀ b`` with ``transpose=True``) in place, Q the full
    m x m orthogonal factor of ``qr_factor``, applied from the stored reflectors
    (four launches per 64 of them on the GPU; T is rebuilt, never stored). ``b``
    is (m,) or (m, k) float64 with ``lu_solve_``'s stride rules; its columns are
    independent."""
    m, n, (nrhs, pitch_b) = _check_mul_q(qr, tau, b, in_place=True)
    if m == 0 or n == 0 or nrhs == 0:
        return b
    L = _native.lib()
    if qr.is_cuda:
        nbytes = int(L.mpx_qr_workspace_bytes(m, n, nrhs))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=qr.device)
        with torch.cuda.device(qr.device):
            _native.check(L.mpx_qr_apply_f64(qr.data_ptr(), m, n, _pitch(qr, n), tau.data_ptr(), b.data_ptr(), nrhs,
                                             pitch_b, 1 if transpose else 0, ws.data_ptr(), nbytes,
                                             _native.stream_of(qr)))
    else:
        L.mpx_cpu_qr_apply_f64(qr.data_ptr(), m, n, _pitch(qr, n), tau.data_ptr(), b.data_ptr(), nrhs, pitch_b,
                               1 if transpose else 0)
    return b


def qr_mul_q(qr: torch.Tensor, tau: torch.Tensor, b: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """``qr_mul_q_`` on a contiguous copy of ``b``."""
    _check_mul_q(qr, tau, b)
    return qr_mul_q_(qr, tau, b.clone(memory_format=torch.contiguous_format), transpose)


def qr_solve_r_(qr: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``b <- R⁻¹ b`` in place by blocked back substitution with the upper
    triangle of ``qr[:n]``; ``b`` is (n,) or (n, k) with ``lu_solve_``'s stride
    rules. A zero on R's diagonal (``info`` of ``qr_factor``) divides by zero."""
    _, n = _check_tall(qr, "QR")
    nrhs, pitch_b = _check_rhs(b, n, qr, "QR", in_place=True, owner="R")
    if n == 0 or nrhs == 0:
        return b
    L = _native.lib()
    if qr.is_cuda:
        with torch.cuda.device(qr.device):
            _native.check(L.mpx_qr_rsolve_f64(qr.data_ptr(), n, _pitch(qr, n), b.data_ptr(), nrhs, pitch_b,
                                              _native.stream_of(qr)))
    else:
        L.mpx_cpu_qr_rsolve_f64(qr.data_ptr(), n, _pitch(qr, n), b.data_ptr(), nrhs, pitch_b)
    return b


def qr_unpack(qr: torch.Tensor, tau: torch.Tensor):
    """``(Q, R)`` with ``A = Q @ R``: the thin Q (m x n: Q applied to the
    leading columns of the identity) and the n x n upper-triangular R."""
    m, n = _check_tall(qr, "QR")
    _check_tau(tau, qr, n)
    q = torch.eye(m, n, dtype=torch.float64, device=qr.device)
    return qr_mul_q_(qr, tau, q), torch.triu(qr[:n])


def lstsq(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The minimiser of ``‖A x − b‖₂`` for a float64 ``a`` with m >= n of full
    column rank, by Householder QR: factor a copy of ``a``, read ``info`` (the
    one host read), apply ``Qᵀ`` to a copy of ``b`` ((m,) or (m, k)), solve
    with R. Returns (n,) or (n, k). A rank-deficient matrix (an exactly zero
    ``R_jj``) raises ``RuntimeError`` naming the column. For m = n this is a
    linear solve."""
    m, n = _check_tall(a, "A")
    _check_rhs(b, m, a, "A", sized=True)
    qr, tau, info = qr_factor(a)
    k = int(info.item())
    if k:
        raise RuntimeError(f"lstsq: the matrix is rank-deficient (zero on R's diagonal in column {k - 1})")
    y = qr_mul_q(qr, tau, b, transpose=True)
    return qr_solve_r_(qr, y[:n]).clone(memory_format=torch.contiguous_format)
