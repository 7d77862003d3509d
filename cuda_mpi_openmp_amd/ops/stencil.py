"""2-D Jacobi sweep on a row slab with one halo row above and below.

Layout: ``u`` has shape (rows + 2, cols); row 0 and row rows+1 are halo rows
(neighbour data, or the fixed Dirichlet boundary at the global edges), columns
0 and cols-1 are Dirichlet boundary. A sweep writes owned rows [r0, r1)
(1-based) of ``un`` and optionally folds max|un - u| into ``resid``.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from .. import _native


def jacobi_sweep(u: torch.Tensor, un: torch.Tensor, r0: int, r1: int,
                 resid: Optional[torch.Tensor] = None, rhs: Optional[torch.Tensor] = None,
                 omega: Optional[float] = None) -> Optional[float]:
    """GPU: enqueue the sweep (resid, a 1-element tensor zeroed by the caller,
    accumulates the max on device). CPU: run it and return the residual.

    ``rhs`` (u's shape, dtype and device, contiguous): the Poisson sweep
    un = (((up + down) + (left + right)) + rhs) * 0.25 for -Laplace(u) = f with
    rhs = h^2 f; read at the interior points of rows [r0, r1) only.

    ``omega`` (a finite, positive float): the Chebyshev step. ``un`` is in-out:
    on entry rows [r0, r1) hold the iterate before ``u``, p, and the sweep writes
    p + omega * (s - p) with s the plain or Poisson value (three rounded
    operations, omega rounded once to u's dtype). The residual stays
    max|s - u|. Without omega the call launches the plain sweeps."""
    if omega is not None:
        omega = float(omega)
        if not (math.isfinite(omega) and omega > 0.0):
            raise ValueError("omega must be finite and positive")
    if u.shape != un.shape or u.dim() != 2 or u.dtype != un.dtype:
        raise ValueError("u/un must be matching 2-D tensors")
    if not (u.is_contiguous() and un.is_contiguous()):
        raise ValueError("u/un must be contiguous")
    if rhs is not None:
        if not isinstance(rhs, torch.Tensor) or rhs.shape != u.shape or rhs.dtype != u.dtype or rhs.device != u.device:
            raise ValueError("rhs must match u's shape, dtype and device")
        if not rhs.is_contiguous():
            raise ValueError("rhs must be contiguous")
    rows2, cols = u.shape
    if not (1 <= r0 <= r1 <= rows2 - 1):
        raise ValueError("rows out of range")
    L = _native.lib()
    if u.is_cuda:
        rp = 0 if resid is None else resid.data_ptr()
        if resid is not None and (resid.dtype != u.dtype or resid.device != u.device):
            raise ValueError("resid must match u's dtype and device")
        if u.dtype not in (torch.float64, torch.float32):
            raise ValueError("jacobi supports float64/float32")
        if omega is not None:
            fn = L.mpx_jacobi_accel_f64 if u.dtype == torch.float64 else L.mpx_jacobi_accel_f32
            _native.check(fn(u.data_ptr(), None if rhs is None else rhs.data_ptr(), un.data_ptr(), cols, cols, r0, r1,
                             omega, rp, _native.stream_of(u)))
        elif rhs is not None:
            fn = L.mpx_jacobi_rhs_f64 if u.dtype == torch.float64 else L.mpx_jacobi_rhs_f32
            _native.check(fn(u.data_ptr(), rhs.data_ptr(), un.data_ptr(), cols, cols, r0, r1, rp, _native.stream_of(u)))
        elif u.dtype == torch.float64:
            _native.check(L.mpx_jacobi_f64(u.data_ptr(), un.data_ptr(), cols, cols, r0, r1, rp, _native.stream_of(u)))
        elif u.dtype == torch.float32:
            _native.check(L.mpx_jacobi_f32(u.data_ptr(), un.data_ptr(), cols, cols, r0, r1, rp, _native.stream_of(u)))
        else:
            raise ValueError("jacobi supports float64/float32")
        return None
    if u.dtype != torch.float64:
        raise ValueError("CPU jacobi reference is float64")
    if omega is not None:
        r = L.mpx_cpu_jacobi_accel_f64(u.data_ptr(), None if rhs is None else rhs.data_ptr(), un.data_ptr(), cols, cols,
                                       r0, r1, omega)
    elif rhs is not None:
        r = L.mpx_cpu_jacobi_rhs_f64(u.data_ptr(), rhs.data_ptr(), un.data_ptr(), cols, cols, r0, r1)
    else:
        r = L.mpx_cpu_jacobi_f64(u.data_ptr(), un.data_ptr(), cols, cols, r0, r1)
    if resid is not None:
        resid.fill_(max(float(resid.item()), r))
    return r


def jacobi3d_tile(dtype: torch.dtype, rhs: bool = False, accel: bool = False) -> dict:
    """Wave form and tile of the production 3-D launches for ``dtype`` and the
    sweep kind (``rhs``: with a right-hand side, ``accel``: with omega):
    {"form": 0 rows-in-plane walk | 1 z-march (+ 2: workgroups remapped per XCD),
    "ty": rows per wave, "kz": planes marched per wave, "min_waves": the wave
    count below which a launch halves its tile (rows: ty, march: kz)}."""
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("jacobi3d supports float64/float32")
    out = _native.i32_array([0, 0, 0, 0])
    _native.check(_native.lib().mpx_jacobi3d_tile(int(dtype == torch.float64), int(bool(rhs)), int(bool(accel)), out))
    return {"form": out[0], "ty": out[1], "kz": out[2], "min_waves": out[3]}


def jacobi3d_sweep(u: torch.Tensor, un: torch.Tensor, k0: int, k1: int,
                   resid: Optional[torch.Tensor] = None, rhs: Optional[torch.Tensor] = None,
                   omega: Optional[float] = None) -> Optional[float]:
    """3-D sweep (7-point stencil) over planes [k0, k1) of a plane slab.

    ``u`` / ``un`` (and ``rhs``): contiguous (planes + 2, ny, nx) tensors, x
    fastest; planes 0 and planes + 1 are halo planes, rows 0 / ny - 1 and columns
    0 / nx - 1 Dirichlet. Interior points of the swept planes get
    s = ((((zm + zp) + (ym + yp)) + (xm + xp)) [+ rhs]) * c with c = 1/6 rounded
    once to the dtype and every operation rounded; boundary elements of a swept
    plane receive u's value; other planes are not written. ``omega``: the
    Chebyshev step, ``un`` in-out, p + omega * (s - p) with p found in ``un``.
    The residual is max|s - u| over the swept interior points.

    GPU: enqueue on the tensor's stream (resid, a 1-element tensor zeroed by the
    caller, accumulates the max on device). CPU (float64): run it and return
    the residual."""
    if omega is not None:
        omega = float(omega)
        if not (math.isfinite(omega) and omega > 0.0):
            raise ValueError("omega must be finite and positive")
    if u.dim() != 3 or u.shape != un.shape or u.dtype != un.dtype or u.device != un.device:
        raise ValueError("u/un must be matching 3-D tensors")
    if not (u.is_contiguous() and un.is_contiguous()):
        raise ValueError("u/un must be contiguous")
    if rhs is not None:
        if not isinstance(rhs, torch.Tensor) or rhs.shape != u.shape or rhs.dtype != u.dtype or rhs.device != u.device:
            raise ValueError("rhs must match u's shape, dtype and device")
        if not rhs.is_contiguous():
            raise ValueError("rhs must be contiguous")
    planes2, ny, nx = u.shape
    if nx < 3 or ny < 3 or ny * nx >= 2 ** 31:
        raise ValueError("need nx >= 3, ny >= 3 and ny * nx < 2^31")
    if not (1 <= k0 <= k1 <= planes2 - 1):
        raise ValueError("planes out of range")
    L = _native.lib()
    bp = None if rhs is None else rhs.data_ptr()
    if u.is_cuda:
        if u.dtype not in (torch.float64, torch.float32):
            raise ValueError("jacobi3d supports float64/float32")
        if resid is not None and (resid.dtype != u.dtype or resid.device != u.device):
            raise ValueError("resid must match u's dtype and device")
        rp = None if resid is None else resid.data_ptr()
        f64 = u.dtype == torch.float64
        if omega is not None:
            fn = L.mpx_jacobi3d_accel_f64 if f64 else L.mpx_jacobi3d_accel_f32
            _native.check(fn(u.data_ptr(), bp, un.data_ptr(), nx, ny, k0, k1, omega, rp, _native.stream_of(u)))
        else:
            fn = L.mpx_jacobi3d_f64 if f64 else L.mpx_jacobi3d_f32
            _native.check(fn(u.data_ptr(), bp, un.data_ptr(), nx, ny, k0, k1, rp, _native.stream_of(u)))
        return None
    if u.dtype != torch.float64:
        raise ValueError("CPU jacobi3d reference is float64")
    if omega is not None:
        r = L.mpx_cpu_jacobi3d_accel_f64(u.data_ptr(), bp, un.data_ptr(), nx, ny, k0, k1, omega)
    else:
        r = L.mpx_cpu_jacobi3d_f64(u.data_ptr(), bp, un.data_ptr(), nx, ny, k0, k1)
    if resid is not None:
        resid.fill_(max(float(resid.item()), r))
    return r
