"""lab4 workload: a dense fp64 linear system by LU with partial pivoting.

``DenseLU`` factors its matrix once (a copy; on the matrix's device) and
answers from the factors: ``solve(B)``, ``slogdet()`` and ``inverse()``, which
solves against the identity. A singular matrix (an exactly zero pivot) raises
``RuntimeError`` at construction, the one host read.

``BatchedDenseLU`` is the same for a batch ``(B, n, n)`` of small matrices: one
launch factors them all, one launch solves (``ops.lu_factor_batched``); any
singular member raises at construction, naming its batch index and column.

``DenseCholesky`` is ``DenseLU`` for a symmetric positive definite matrix (its
lower triangle is what counts): half the work and no pivot search
(``ops.cholesky_factor``). A matrix that is not positive definite raises at
construction, naming the column where the factorisation broke down.

``BatchedDenseCholesky`` is ``BatchedDenseLU`` for a batch of small symmetric
positive definite matrices (``ops.cholesky_factor_batched``): one launch each
way; a member that is not positive definite raises at construction, naming its
batch index and column.

``DenseQR`` factors a tall or square matrix (m >= n) by Householder QR
(``ops.qr_factor``) and answers least-squares problems from the factors:
``solve(b)`` minimises ``‖A x − b‖₂``, ``q()`` and ``r()`` unpack the thin Q and
R, ``mul_q(b, transpose=)`` applies the full Q or Qᵀ, ``logabsdet()`` is
``log |det A|`` of a square matrix. A rank-deficient matrix (an exactly zero
``R_jj``) raises at construction, naming the column.
"""

from __future__ import annotations

import torch

from .. import ops


class DenseLU:
    def __init__(self, a: torch.Tensor):
        self.lu, self.piv, info = ops.lu_factor(a)
        k = int(info.item())
        if k:
            raise RuntimeError(f"DenseLU: the matrix is singular (zero pivot in column {k - 1})")
        self.n = self.lu.shape[0]

    def solve(self, b: torch.Tensor) -> torch.Tensor:
        return ops.lu_solve(self.lu, self.piv, b)

    def slogdet(self):
        return ops.slogdet(self.lu, self.piv)

    def inverse(self) -> torch.Tensor:
        return ops.lu_solve_(self.lu, self.piv, torch.eye(self.n, dtype=torch.float64, device=self.lu.device))


class BatchedDenseLU:
    def __init__(self, a: torch.Tensor):
        self.lu, self.piv, info = ops.lu_factor_batched(a)
        for m, k in enumerate(info.tolist()):
            if k:
                raise RuntimeError(f"BatchedDenseLU: matrix {m} of the batch is singular "
                                   f"(zero pivot in column {k - 1})")
        self.batch, self.n = self.lu.shape[0], self.lu.shape[1]

    def solve(self, b: torch.Tensor) -> torch.Tensor:
        return ops.lu_solve_batched(self.lu, self.piv, b)

    def slogdet(self):
        return ops.slogdet_batched(self.lu, self.piv)

    def inverse(self) -> torch.Tensor:
        eye = torch.eye(self.n, dtype=torch.float64, device=self.lu.device)
        return ops.lu_solve_batched_(self.lu, self.piv, eye.repeat(self.batch, 1, 1))


class DenseCholesky:
    def __init__(self, a: torch.Tensor):
        self.l, info = ops.cholesky_factor(a)
        k = int(info.item())
        if k:
            raise RuntimeError(f"DenseCholesky: the matrix is not positive definite (column {k - 1})")
        self.n = self.l.shape[0]

    def solve(self, b: torch.Tensor) -> torch.Tensor:
        return ops.cholesky_solve(self.l, b)

    def logdet(self) -> torch.Tensor:
        return ops.logdet_spd(self.l)

    def inverse(self) -> torch.Tensor:
        return ops.cholesky_solve_(self.l, torch.eye(self.n, dtype=torch.float64, device=self.l.device))


class BatchedDenseCholesky:
    def __init__(self, a: torch.Tensor):
        self.l, info = ops.cholesky_factor_batched(a)
        for m, k in enumerate(info.tolist()):
            if k:
                raise RuntimeError(f"BatchedDenseCholesky: matrix {m} of the batch is not positive definite "
                                   f"(column {k - 1})")
        self.batch, self.n = self.l.shape[0], self.l.shape[1]

    def solve(self, b: torch.Tensor) -> torch.Tensor:
        return ops.cholesky_solve_batched(self.l, b)

    def logdet(self) -> torch.Tensor:
        return ops.logdet_spd_batched(self.l)

    def inverse(self) -> torch.Tensor:
        eye = torch.eye(self.n, dtype=torch.float64, device=self.l.device)
        return ops.cholesky_solve_batched_(self.l, eye.repeat(self.batch, 1, 1))


class DenseQR:
    def __init__(self, a: torch.Tensor):
        self.qr, self.tau, info = ops.qr_factor(a)
        k = int(info.item())
        if k:
            raise RuntimeError(f"DenseQR: the matrix is rank-deficient (zero on R's diagonal in column {k - 1})")
        self.m, self.n = self.qr.shape

    def solve(self, b: torch.Tensor) -> torch.Tensor:
        y = ops.qr_mul_q(self.qr, self.tau, b, transpose=True)
        return ops.qr_solve_r_(self.qr, y[:self.n]).clone(memory_format=torch.contiguous_format)

    def q(self) -> torch.Tensor:
        return ops.qr_unpack(self.qr, self.tau)[0]

    def r(self) -> torch.Tensor:
        return torch.triu(self.qr[:self.n])

    def mul_q(self, b: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        return ops.qr_mul_q(self.qr, self.tau, b, transpose)

    def logabsdet(self) -> torch.Tensor:
        if self.m != self.n:
            raise ValueError(f"logabsdet needs a square matrix, not {(self.m, self.n)}")
        return torch.log(torch.abs(torch.diagonal(self.qr))).sum()
