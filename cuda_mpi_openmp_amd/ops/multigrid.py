"""Operators of the geometric multigrid V-cycle for the 2-D Poisson solver.

Layout: a grid is an (H, W) tensor; rows 0 and H-1 and columns 0 and W-1 hold
Dirichlet values, the interior is rows 1..H-2, columns 1..W-2 (``SlabJacobi``'s
buffer at world size 1, H = rows + 2). The coarse grid of (H, W) is (Hc, Wc)
with H = 2 Hc - 1 and W = 2 Wc - 1; coarse point (I, J) sits on fine (2I, 2J).

Every operator takes pitched 2-D tensors: ``stride(1) == 1`` and
``stride(0) >= W`` (contiguous included). Padding elements are never read for
a result and never written. GPU tensors: the kernel is enqueued on the current
stream, nothing is allocated or synchronised. CPU tensors (float64): the
OpenMP reference runs. Every + - * is one rounded operation in the working
dtype, identical on GPU fp32/fp64, the CPU library and the torch expressions
of ``ops.reference``.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from .. import _native

_GPU_DTYPES = (torch.float64, torch.float32)


def _pitched(name: str, t: torch.Tensor) -> int:
    """The row pitch (elements) of a pitched 2-D tensor."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D tensor")
    h, w = t.shape
    if w < 1 or h < 1:
        raise ValueError(f"{name} is empty")
    if t.stride(1) != 1 and w > 1:
        raise ValueError(f"{name} must have unit column stride")
    pitch = t.stride(0) if h > 1 else w
    if pitch < w:
        raise ValueError(f"{name}: row stride smaller than the width")
    if pitch >= 2 ** 31:
        raise ValueError(f"{name}: row stride too large")
    return pitch


def _same_kind(a_name: str, a: torch.Tensor, b_name: str, b: torch.Tensor) -> None:
    if a.dtype != b.dtype or a.device != b.device:
        raise ValueError(f"{b_name} must match {a_name}'s dtype and device")


def _check_dtype(u: torch.Tensor, what: str) -> None:
    if u.is_cuda:
        if u.dtype not in _GPU_DTYPES:
            raise ValueError(f"{what} supports float64/float32")
    elif u.dtype != torch.float64:
        raise ValueError(f"CPU {what} reference is float64")


def _resid_ptr(resid: Optional[torch.Tensor], u: torch.Tensor):
    if resid is None:
        return None
    if not isinstance(resid, torch.Tensor) or resid.numel() != 1 or resid.dtype != u.dtype or resid.device != u.device:
        raise ValueError("resid must be a 1-element tensor of u's dtype and device")
    return resid.data_ptr()


def jacobi_relax(u: torch.Tensor, un: torch.Tensor, r0: int, r1: int, omega: float,
                 resid: Optional[torch.Tensor] = None, rhs: Optional[torch.Tensor] = None) -> Optional[float]:
    """Damped Jacobi sweep over rows [r0, r1): with s the plain or Poisson value
    of ``jacobi_sweep`` and c the centre value of ``u``, interior points of
    ``un`` get c + omega * (s - c) (three rounded operations, omega rounded once
    to the dtype; finite and positive). Boundary columns copy through; ``un`` is
    output only; ``resid`` folds max|s - c| as the sweeps do. ``u``, ``un`` and
    ``rhs`` share one shape and one row pitch."""
    omega = float(omega)
    if not (math.isfinite(omega) and omega > 0.0):
        raise ValueError("omega must be finite and positive")
    pitch = _pitched("u", u)
    if _pitched("un", un) != pitch or u.shape != un.shape:
        raise ValueError("u/un must have the same shape and row pitch")
    _same_kind("u", u, "un", un)
    if rhs is not None:
        if _pitched("rhs", rhs) != pitch or rhs.shape != u.shape:
            raise ValueError("rhs must have u's shape and row pitch")
        _same_kind("u", u, "rhs", rhs)
    _check_dtype(u, "jacobi_relax")
    rows2, cols = u.shape
    if not (1 <= r0 <= r1 <= rows2 - 1):
        raise ValueError("rows out of range")
    rp = _resid_ptr(resid, u)
    bp = None if rhs is None else rhs.data_ptr()
    L = _native.lib()
    if u.is_cuda:
        fn = L.mpx_jacobi_relax_f64 if u.dtype == torch.float64 else L.mpx_jacobi_relax_f32
        _native.check(fn(u.data_ptr(), bp, un.data_ptr(), cols, pitch, r0, r1, omega, rp, _native.stream_of(u)))
        return None
    r = L.mpx_cpu_jacobi_relax_f64(u.data_ptr(), bp, un.data_ptr(), cols, pitch, r0, r1, omega)
    if resid is not None:
        resid.fill_(max(float(resid.item()), r))
    return r


def mg_residual(u: torch.Tensor, r: torch.Tensor, rhs: Optional[torch.Tensor] = None,
                resid: Optional[torch.Tensor] = None) -> Optional[float]:
    """r = ((((up + dn) + (l + rt)) + b) - 4 c) at the interior points (without
    ``rhs`` the "+ b" step is left out); r's boundary is not written. ``resid``
    (1 element, zeroed by the caller) receives max|r|. CPU: returns the maximum."""
    pu, pr = _pitched("u", u), _pitched("r", r)
    if u.shape != r.shape:
        raise ValueError("r must have u's shape")
    _same_kind("u", u, "r", r)
    pb = 0
    if rhs is not None:
        pb = _pitched("rhs", rhs)
        if rhs.shape != u.shape:
            raise ValueError("rhs must have u's shape")
        _same_kind("u", u, "rhs", rhs)
    _check_dtype(u, "mg_residual")
    rows, cols = u.shape
    if rows < 3 or cols < 3:
        raise ValueError("need at least 3 rows and 3 columns")
    rp = _resid_ptr(resid, u)
    bp = None if rhs is None else rhs.data_ptr()
    L = _native.lib()
    if u.is_cuda:
        fn = L.mpx_mg_residual_f64 if u.dtype == torch.float64 else L.mpx_mg_residual_f32
        _native.check(fn(u.data_ptr(), bp, r.data_ptr(), rows, cols, pu, pb, pr, rp, _native.stream_of(u)))
        return None
    m = L.mpx_cpu_mg_residual_f64(u.data_ptr(), bp, r.data_ptr(), rows, cols, pu, pb, pr)
    if resid is not None:
        resid.fill_(max(float(resid.item()), m))
    return m


def _coarse_of(fine: torch.Tensor, coarse: torch.Tensor, fine_name: str, coarse_name: str):
    pf, pc = _pitched(fine_name, fine), _pitched(coarse_name, coarse)
    (h, w), (hc, wc) = fine.shape, coarse.shape
    if hc < 2 or wc < 2 or h != 2 * hc - 1 or w != 2 * wc - 1:
        raise ValueError(f"{coarse_name} {tuple(coarse.shape)} is not the coarse grid of {fine_name} "
                         f"{tuple(fine.shape)}: need H = 2 Hc - 1 and W = 2 Wc - 1")
    _same_kind(fine_name, fine, coarse_name, coarse)
    return pf, pc, hc, wc


def mg_restrict(r: torch.Tensor, bc: torch.Tensor) -> None:
    """Full weighting of the fine ``r`` into the coarse interior of ``bc``,
    scaled for the h^2-scaled coarse right-hand side: with i = 2I, j = 2J,
    e = (r[i-1,j] + r[i+1,j]) + (r[i,j-1] + r[i,j+1]),
    d = (r[i-1,j-1] + r[i-1,j+1]) + (r[i+1,j-1] + r[i+1,j+1]),
    bc[I,J] = (r[i,j] + e*0.5) + d*0.25. bc's boundary is not written and r's
    boundary is not read for a result."""
    pr, pc, hc, wc = _coarse_of(r, bc, "r", "bc")
    _check_dtype(r, "mg_restrict")
    L = _native.lib()
    if r.is_cuda:
        fn = L.mpx_mg_restrict_f64 if r.dtype == torch.float64 else L.mpx_mg_restrict_f32
        _native.check(fn(r.data_ptr(), bc.data_ptr(), hc, wc, pr, pc, _native.stream_of(r)))
        return
    if L.mpx_cpu_mg_restrict_f64(r.data_ptr(), bc.data_ptr(), hc, wc, pr, pc) != 0:
        raise ValueError("mg_restrict: bad arguments")


def mg_prolong_add_(e: torch.Tensor, u: torch.Tensor) -> None:
    """Bilinear interpolation of the coarse ``e`` added in place to the fine
    interior of ``u``: (2I,2J) += e[I,J]; (2I+1,2J) += (e[I,J] + e[I+1,J])*0.5;
    (2I,2J+1) += (e[I,J] + e[I,J+1])*0.5; (2I+1,2J+1) +=
    ((e[I,J] + e[I+1,J]) + (e[I,J+1] + e[I+1,J+1]))*0.25. e's boundary is read;
    u's boundary is not written."""
    pu, pe, hc, wc = _coarse_of(u, e, "u", "e")
    _check_dtype(u, "mg_prolong_add_")
    L = _native.lib()
    if u.is_cuda:
        fn = L.mpx_mg_prolong_add_f64 if u.dtype == torch.float64 else L.mpx_mg_prolong_add_f32
        _native.check(fn(e.data_ptr(), u.data_ptr(), hc, wc, pe, pu, _native.stream_of(u)))
        return
    if L.mpx_cpu_mg_prolong_add_f64(e.data_ptr(), u.data_ptr(), hc, wc, pe, pu) != 0:
        raise ValueError("mg_prolong_add_: bad arguments")
