"""lab4 workload: a dense fp64 linear system by LU with partial pivoting.

``DenseLU`` factors its matrix once (a copy; on the matrix's device) and
answers from the factors: ``solve(B)``, ``slogdet()`` and ``inverse()``, which
solves against the identity. A singular matrix (an exactly zero pivot) raises
``RuntimeError`` at construction, the one host read.
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
