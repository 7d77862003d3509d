"""Operators of the geometric multigrid V-cycle for the 3-D Poisson solver.

Layout: a grid is a (D, H, W) tensor, x fastest, with Dirichlet values on all
six faces (``SlabJacobi3D``'s buffer at world size 1, D = planes + 2). The
coarse grid of (D, H, W) is (Dc, Hc, Wc) with D = 2 Dc - 1, H = 2 Hc - 1 and
W = 2 Wc - 1; coarse point (K, J, I) sits on fine (2K, 2J, 2I). The discrete
equation is 6 u - (sum of the six neighbours) = b with b = h^2 f.

Every operator takes pitched 3-D tensors: ``stride(2) == 1``,
``stride(1) >= W`` (the row pitch) and ``stride(0) >= H * stride(1)`` (the
plane stride), contiguous included. Padding elements are never read for a
result and never written. GPU tensors: the kernel is enqueued on the current
stream, nothing is allocated or synchronised. CPU tensors (float64): the
OpenMP reference runs. Every + - * is one rounded operation in the working
dtype, identical on GPU fp32/fp64, the CPU library and the torch expressions
of ``ops.reference``.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .. import _native
from .multigrid import _check_dtype, _resid_ptr, _same_kind, _tail_levels, _tail_on_cpu, _tail_params


def _pitched3(name: str, t: torch.Tensor) -> Tuple[int, int]:
    """(row pitch, plane stride), in elements, of a pitched 3-D tensor."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        raise ValueError(f"{name} must be a 3-D tensor")
    d, h, w = t.shape
    if d < 1 or h < 1 or w < 1:
        raise ValueError(f"{name} is empty")
    if t.stride(2) != 1 and w > 1:
        raise ValueError(f"{name} must have unit stride in x")
    pitch = t.stride(1) if h > 1 else w
    if pitch < w:
        raise ValueError(f"{name}: row stride smaller than the width")
    if pitch >= 2 ** 31:
        raise ValueError(f"{name}: row stride too large")
    plane = t.stride(0) if d > 1 else h * pitch
    if plane < h * pitch:
        raise ValueError(f"{name}: plane stride smaller than H * row stride")
    return pitch, plane


def mg3_walk() -> dict:
    """The walks of the 3-D multigrid launches: {"rows": rows of a plane walked
    per lane by relax / residual, "restrict_planes" / "prolong_planes": coarse
    planes walked per lane by the two transfers, "min_waves": the wave count
    below which a launch halves its walk, "waves": waves (row blocks, coarse
    rows) per workgroup}."""
    out = _native.i32_array([0, 0, 0, 0, 0])
    _native.check(_native.lib().mpx_mg3_walk(out))
    return {"rows": out[0], "restrict_planes": out[1], "prolong_planes": out[2], "min_waves": out[3], "waves": out[4]}


def mg3_cubic_walk() -> dict:
    """The walk of ``mg3_prolong_cubic``'s launches: {"planes": coarse planes
    walked per lane, "min_waves": the wave count below which a launch halves
    that walk (``mg3_walk``'s), "waves": waves (coarse rows) per workgroup}."""
    out = _native.i32_array([0, 0, 0])
    _native.check(_native.lib().mpx_mg3_cubic_walk(out))
    return {"planes": out[0], "min_waves": out[1], "waves": out[2]}


def jacobi3d_relax(u: torch.Tensor, un: torch.Tensor, k0: int, k1: int, omega: float,
                   resid: Optional[torch.Tensor] = None, rhs: Optional[torch.Tensor] = None) -> Optional[float]:
    """Damped 3-D Jacobi sweep over planes [k0, k1): with s the plain or Poisson
    value of ``jacobi3d_sweep`` and c the centre value of ``u``, interior points
    of ``un`` get c + omega * (s - c) (three rounded operations, omega rounded
    once to the dtype; finite and positive). Boundary rows and columns of a
    swept plane copy through; ``un`` is output only; ``resid`` folds max|s - c|
    as the sweeps do. ``u``, ``un`` and ``rhs`` share one shape, one row pitch
    and one plane stride."""
    omega = float(omega)
    if not (math.isfinite(omega) and omega > 0.0):
        raise ValueError("omega must be finite and positive")
    strides = _pitched3("u", u)
    if _pitched3("un", un) != strides or u.shape != un.shape:
        raise ValueError("u/un must have the same shape, row pitch and plane stride")
    _same_kind("u", u, "un", un)
    if rhs is not None:
        if _pitched3("rhs", rhs) != strides or rhs.shape != u.shape:
            raise ValueError("rhs must have u's shape, row pitch and plane stride")
        _same_kind("u", u, "rhs", rhs)
    _check_dtype(u, "jacobi3d_relax")
    d, ny, nx = u.shape
    if d < 3 or ny < 3 or nx < 3:
        raise ValueError("need at least 3 planes, 3 rows and 3 columns")
    if not (1 <= k0 <= k1 <= d - 1):
        raise ValueError("planes out of range")
    rp = _resid_ptr(resid, u)
    bp = None if rhs is None else rhs.data_ptr()
    pitch, plane = strides
    L = _native.lib()
    if u.is_cuda:
        fn = L.mpx_jacobi3d_relax_f64 if u.dtype == torch.float64 else L.mpx_jacobi3d_relax_f32
        _native.check(fn(u.data_ptr(), bp, un.data_ptr(), d, ny, nx, pitch, plane, k0, k1, omega, rp,
                         _native.stream_of(u)))
        return None
    r = L.mpx_cpu_jacobi3d_relax_f64(u.data_ptr(), bp, un.data_ptr(), d, ny, nx, pitch, plane, k0, k1, omega)
    if resid is not None:
        resid.fill_(max(float(resid.item()), r))
    return r


def mg3_residual(u: torch.Tensor, r: torch.Tensor, rhs: Optional[torch.Tensor] = None,
                 resid: Optional[torch.Tensor] = None) -> Optional[float]:
    """r = ((((zm + zp) + (ym + yp)) + (xm + xp)) + b) - 6 c at the interior
    points (without ``rhs`` the "+ b" step is left out); r's boundary is not
    written. ``resid`` (1 element, zeroed by the caller) receives max|r|. CPU:
    returns the maximum."""
    (pu, su), (pr, sr) = _pitched3("u", u), _pitched3("r", r)
    if u.shape != r.shape:
        raise ValueError("r must have u's shape")
    _same_kind("u", u, "r", r)
    pb = sb = 0
    if rhs is not None:
        pb, sb = _pitched3("rhs", rhs)
        if rhs.shape != u.shape:
            raise ValueError("rhs must have u's shape")
        _same_kind("u", u, "rhs", rhs)
    _check_dtype(u, "mg3_residual")
    d, ny, nx = u.shape
    if d < 3 or ny < 3 or nx < 3:
        raise ValueError("need at least 3 planes, 3 rows and 3 columns")
    rp = _resid_ptr(resid, u)
    bp = None if rhs is None else rhs.data_ptr()
    L = _native.lib()
    if u.is_cuda:
        fn = L.mpx_mg3_residual_f64 if u.dtype == torch.float64 else L.mpx_mg3_residual_f32
        _native.check(fn(u.data_ptr(), bp, r.data_ptr(), d, ny, nx, pu, su, pb, sb, pr, sr, rp, _native.stream_of(u)))
        return None
    m = L.mpx_cpu_mg3_residual_f64(u.data_ptr(), bp, r.data_ptr(), d, ny, nx, pu, su, pb, sb, pr, sr)
    if resid is not None:
        resid.fill_(max(float(resid.item()), m))
    return m


def _coarse3_of(fine: torch.Tensor, coarse: torch.Tensor, fine_name: str, coarse_name: str):
    sf, sc = _pitched3(fine_name, fine), _pitched3(coarse_name, coarse)
    (d, h, w), (dc, hc, wc) = fine.shape, coarse.shape
    if min(dc, hc, wc) < 2 or d != 2 * dc - 1 or h != 2 * hc - 1 or w != 2 * wc - 1:
        raise ValueError(f"{coarse_name} {tuple(coarse.shape)} is not the coarse grid of {fine_name} "
                         f"{tuple(fine.shape)}: need D = 2 Dc - 1, H = 2 Hc - 1 and W = 2 Wc - 1")
    _same_kind(fine_name, fine, coarse_name, coarse)
    return sf, sc, dc, hc, wc


def mg3_restrict(r: torch.Tensor, bc: torch.Tensor) -> None:
    """27-point full weighting of the fine ``r`` into the coarse interior of
    ``bc``, scaled for the h^2-scaled coarse right-hand side, defined separably:
    P_k[J,I] is ``mg_restrict``'s 2-D rule in fine plane k, then
    bc[K,J,I] = (P_2K + (P_2K-1 + P_2K+1) * 0.5) * 0.5 (weights: centre 0.5,
    face 0.25, edge 0.125, corner 0.0625). bc's boundary is not written and r's
    boundary is not read for a result; without a coarse interior the call is a
    no-op."""
    (pr, sr), (pc, sc), dc, hc, wc = _coarse3_of(r, bc, "r", "bc")
    _check_dtype(r, "mg3_restrict")
    L = _native.lib()
    if r.is_cuda:
        fn = L.mpx_mg3_restrict_f64 if r.dtype == torch.float64 else L.mpx_mg3_restrict_f32
        _native.check(fn(r.data_ptr(), bc.data_ptr(), dc, hc, wc, pr, sr, pc, sc, _native.stream_of(r)))
        return
    if L.mpx_cpu_mg3_restrict_f64(r.data_ptr(), bc.data_ptr(), dc, hc, wc, pr, sr, pc, sc) != 0:
        raise ValueError("mg3_restrict: bad arguments")


def mg3_prolong_add_(e: torch.Tensor, u: torch.Tensor) -> None:
    """Trilinear interpolation of the coarse ``e`` added in place to the fine
    interior of ``u``: unscaled pair sums in z (e[K] + e[K+1] at odd planes),
    then y, then x, and one exact scale 0.5^(number of odd coordinates), with no
    multiply when that factor is 1. e's boundary is read; u's boundary is not
    written."""
    (pu, su), (pe, se), dc, hc, wc = _coarse3_of(u, e, "u", "e")
    _check_dtype(u, "mg3_prolong_add_")
    L = _native.lib()
    if u.is_cuda:
        fn = L.mpx_mg3_prolong_add_f64 if u.dtype == torch.float64 else L.mpx_mg3_prolong_add_f32
        _native.check(fn(e.data_ptr(), u.data_ptr(), dc, hc, wc, pe, se, pu, su, _native.stream_of(u)))
        return
    if L.mpx_cpu_mg3_prolong_add_f64(e.data_ptr(), u.data_ptr(), dc, hc, wc, pe, se, pu, su) != 0:
        raise ValueError("mg3_prolong_add_: bad arguments")


def mg3_prolong_cubic(c: torch.Tensor, u: torch.Tensor) -> None:
    """Tricubic interpolation of the coarse ``c`` written over the fine
    interior of ``u`` (the interpolant of full multigrid; ``u``'s interior on
    entry is ignored). Separable, from ``mg_prolong_cubic``'s 1-D rule
    unchanged (even points copy c, the midpoint between K and K + 1 is
    ``(a + (a - o) * 0.125) * 0.5`` with a = c[K] + c[K+1] and
    o = c[K-1] + c[K+2], cubic ghosts for n >= 4, parabola ghosts for n = 3):
    along x in every coarse row, then along y down the columns of those rows
    (ghost rows element by element from the interpolated rows), then along z
    through the interpolated planes (ghost planes element by element from
    them). The interior of fine plane 2K, 1 <= K <= Dc - 2, therefore equals
    ``mg_prolong_cubic`` of coarse plane K bit for bit. c's boundary is read
    (the coarse Dirichlet values); u's boundary is not written. Needs a coarse
    grid of at least 3 x 3 x 3."""
    (pu, su), (pc, sc), dc, hc, wc = _coarse3_of(u, c, "u", "c")
    if min(dc, hc, wc) < 3:
        raise ValueError("mg3_prolong_cubic needs a coarse grid of at least 3 x 3 x 3")
    _check_dtype(u, "mg3_prolong_cubic")
    L = _native.lib()
    if u.is_cuda:
        fn = L.mpx_mg3_prolong_cubic_f64 if u.dtype == torch.float64 else L.mpx_mg3_prolong_cubic_f32
        _native.check(fn(c.data_ptr(), u.data_ptr(), dc, hc, wc, pc, sc, pu, su, _native.stream_of(u)))
        return
    if L.mpx_cpu_mg3_prolong_cubic_f64(c.data_ptr(), u.data_ptr(), dc, hc, wc, pc, sc, pu, su) != 0:
        raise ValueError("mg3_prolong_cubic: bad arguments")


# ---------------------------------------------------------------------------
# the coarse levels of a V-cycle in one kernel
# ---------------------------------------------------------------------------
def _tail3_desc(levels):
    """The validated mpx_mg3_level array of ``levels``: u, un, b and r of a
    level share one shape, row pitch and plane stride, and every level is the
    coarse grid of the one before it."""
    levels = _tail_levels(levels, "mg3_tail")
    desc = (_native.Mg3Level * len(levels))()
    for k, (u, un, b, r) in enumerate(levels):
        strides = _pitched3(f"levels[{k}].u", u)
        for name, t in (("un", un), ("b", b), ("r", r)):
            if t is None:
                continue
            if _pitched3(f"levels[{k}].{name}", t) != strides or t.shape != u.shape:
                raise ValueError(f"levels[{k}]: {name} must have u's shape, row pitch and plane stride")
            _same_kind("u", u, name, t)
        if k:
            _same_kind("levels[0].u", levels[0][0], f"levels[{k}].u", u)
            _coarse3_of(levels[k - 1][0], u, f"levels[{k - 1}].u", f"levels[{k}].u")
        d, h, w = u.shape
        if min(d, h, w) < 3:
            raise ValueError(f"levels[{k}]: need at least 3 planes, 3 rows and 3 columns")
        desc[k] = _native.Mg3Level(u.data_ptr(), un.data_ptr(), b.data_ptr(), None if r is None else r.data_ptr(), d, h,
                                   w, strides[0], strides[1])
    _check_dtype(levels[0][0], "mg3_tail")
    return desc


def _tail3_launch(desc, dtype, nu1, nu2, coarse_sweeps, omega, stream) -> None:
    L = _native.lib()
    fn = L.mpx_mg3_tail_f64 if dtype == torch.float64 else L.mpx_mg3_tail_f32
    _native.check(fn(desc, len(desc), nu1, nu2, coarse_sweeps, omega, stream))


def mg3_tail(levels, nu1: int, nu2: int, coarse_sweeps: int, omega: float) -> None:
    """``mg_tail`` for the 3-D solver: the V-cycle from ``levels[0]`` down and
    back up as ``PoissonMultigrid3D._vcycle`` runs it for a level k >= 1, with
    ``jacobi3d_relax``, ``mg3_residual``, ``mg3_restrict`` and
    ``mg3_prolong_add_``; the last level runs one undamped sweep when it is
    3 x 3 x 3. ``levels``: ``(u, un, b, r_or_None)`` per level, finest first,
    the four tensors of a level sharing one shape, row pitch and plane stride.

    Where the results lie: as ``mg_tail`` — in ``un`` for a level that ran an
    odd number of sweeps (``tail_sweeps``), in ``u`` otherwise, counted from
    the zeroed ``u`` below ``levels[0]``; planes 0 and D - 1 and rows 0 and
    H - 1 of ``un`` are never written: they are input, the boundary values.

    GPU tensors: one launch of one workgroup on the current stream, nothing
    allocated, no synchronisation; bit-identical to the launched operators.
    CPU float64 tensors: the same sequence with the CPU operators."""
    nu1, nu2, coarse_sweeps, omega = _tail_params(nu1, nu2, coarse_sweeps, omega)
    desc = _tail3_desc(levels)
    levels = [tuple(lv) for lv in levels]
    u0 = levels[0][0]
    if u0.is_cuda:
        _tail3_launch(desc, u0.dtype, nu1, nu2, coarse_sweeps, omega, _native.stream_of(u0))
        return
    _tail_on_cpu(levels, nu1, nu2, coarse_sweeps, omega, lambda t: tuple(t.shape) == (3, 3, 3),
                 lambda u, un, om, b: jacobi3d_relax(u, un, 1, u.shape[0] - 1, om, rhs=b), mg3_residual, mg3_restrict,
                 mg3_prolong_add_)
