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


def mg_prolong_cubic(c: torch.Tensor, u: torch.Tensor) -> None:
    """Cubic interpolation of the coarse ``c`` (Hc, Wc) written over the fine
    interior of ``u`` (2 Hc - 1, 2 Wc - 1): the interpolant of full multigrid,
    which carries a solution (with its Dirichlet values in c's boundary) where
    ``mg_prolong_add_`` carries a correction. u's boundary is not written; c's
    boundary is read; Hc, Wc >= 3.

    The 1-D rule takes c[0..n-1] to 2n - 1 values: the even ones copy c, the
    midpoint between K and K + 1 is m = (a + (a - o) * 0.125) * 0.5 with
    a = c[K] + c[K+1], o = c[K-1] + c[K+2] (the weights (-1, 9, 9, -1) / 16).
    c[-1] and c[n] are ghosts extrapolated from the same values: for n >= 4
    c[-1] = ((c[0] + c[2]) * 4 - c[3]) - c[1] * 6 (which makes the end midpoint
    the one-sided cubic (5, 15, -5, 1) / 16), for n = 3
    c[-1] = (c[0] - c[1]) * 3 + c[2] (the parabola (3, 6, -1) / 8), and c[n]
    is the mirror image. The 2-D rule applies the 1-D rule along every coarse
    row and then down the columns of the Hc interpolated rows, whose ghost
    rows are formed element by element."""
    pu, pc, hc, wc = _coarse_of(u, c, "u", "c")
    if hc < 3 or wc < 3:
        raise ValueError("mg_prolong_cubic needs a coarse grid of at least 3 x 3")
    _check_dtype(u, "mg_prolong_cubic")
    L = _native.lib()
    if u.is_cuda:
        fn = L.mpx_mg_prolong_cubic_f64 if u.dtype == torch.float64 else L.mpx_mg_prolong_cubic_f32
        _native.check(fn(c.data_ptr(), u.data_ptr(), hc, wc, pc, pu, _native.stream_of(u)))
        return
    if L.mpx_cpu_mg_prolong_cubic_f64(c.data_ptr(), u.data_ptr(), hc, wc, pc, pu) != 0:
        raise ValueError("mg_prolong_cubic: bad arguments")


# ---------------------------------------------------------------------------
# the coarse levels of a V-cycle in one kernel
# ---------------------------------------------------------------------------
def tail_sweeps(n: int, nu1: int, nu2: int, coarse_sweeps: int, single_point_last: bool) -> list:
    """Sweeps run by each of the ``n`` levels of a fused tail: nu1 + nu2, and
    on the last level ``coarse_sweeps`` or 1 (a single interior point). A
    level's iterate ends in ``un`` when its count is odd, in ``u`` otherwise."""
    last = 1 if single_point_last else coarse_sweeps
    return [nu1 + nu2] * (n - 1) + [last]


def _tail_params(nu1, nu2, coarse_sweeps, omega):
    nu1, nu2, coarse_sweeps, omega = int(nu1), int(nu2), int(coarse_sweeps), float(omega)
    if nu1 < 0 or nu2 < 1:
        raise ValueError("need nu1 >= 0 and nu2 >= 1")
    if coarse_sweeps < 1:
        raise ValueError("need coarse_sweeps >= 1")
    if not (math.isfinite(omega) and omega > 0.0):
        raise ValueError("omega must be finite and positive")
    return nu1, nu2, coarse_sweeps, omega


def _tail_levels(levels, what: str):
    levels = [tuple(lv) for lv in levels]
    if not 1 <= len(levels) <= _native.MG_TAIL_MAX_LEVELS:
        raise ValueError(f"{what} takes 1 to {_native.MG_TAIL_MAX_LEVELS} levels")
    if any(len(lv) != 4 for lv in levels):
        raise ValueError(f"{what}: a level is (u, un, b, r_or_None)")
    if any(lv[3] is None for lv in levels[:-1]):
        raise ValueError(f"{what}: every level but the last needs r")
    return levels


def _tail_desc(levels):
    """The validated mpx_mg_level array of ``levels``: u, un, b and r of a
    level share one shape and one row pitch, and every level is the coarse
    grid of the one before it."""
    levels = _tail_levels(levels, "mg_tail")
    desc = (_native.MgLevel * len(levels))()
    for k, (u, un, b, r) in enumerate(levels):
        pitch = _pitched(f"levels[{k}].u", u)
        for name, t in (("un", un), ("b", b), ("r", r)):
            if t is None:
                continue
            if _pitched(f"levels[{k}].{name}", t) != pitch or t.shape != u.shape:
                raise ValueError(f"levels[{k}]: {name} must have u's shape and row pitch")
            _same_kind("u", u, name, t)
        if k:
            _same_kind("levels[0].u", levels[0][0], f"levels[{k}].u", u)
            _coarse_of(levels[k - 1][0], u, f"levels[{k - 1}].u", f"levels[{k}].u")
        h, w = u.shape
        if h < 3 or w < 3:
            raise ValueError(f"levels[{k}]: need at least 3 rows and 3 columns")
        desc[k] = _native.MgLevel(u.data_ptr(), un.data_ptr(), b.data_ptr(), None if r is None else r.data_ptr(), h, w,
                                  pitch)
    _check_dtype(levels[0][0], "mg_tail")
    return desc


def _tail_launch(desc, dtype, nu1, nu2, coarse_sweeps, omega, stream) -> None:
    L = _native.lib()
    fn = L.mpx_mg_tail_f64 if dtype == torch.float64 else L.mpx_mg_tail_f32
    _native.check(fn(desc, len(desc), nu1, nu2, coarse_sweeps, omega, stream))


def _tail_on_cpu(levels, nu1, nu2, coarse_sweeps, omega, single_point, relax, residual, restrict, prolong_add_) -> None:
    """The fused tail's sequence with the launched operators, on the caller's
    buffers: sweeps ping-pong between u and un, starting from u."""
    cur = [[u, un] for u, un, _, _ in levels]

    def sweep(k, om):
        relax(cur[k][0], cur[k][1], om, levels[k][2])
        cur[k].reverse()

    n = len(levels)
    for k in range(n - 1):
        for _ in range(nu1):
            sweep(k, omega)
        residual(cur[k][0], levels[k][3], rhs=levels[k][2])
        restrict(levels[k][3], levels[k + 1][2])
        levels[k + 1][0].zero_()
    if single_point(levels[-1][0]):
        sweep(n - 1, 1.0)
    else:
        for _ in range(coarse_sweeps):
            sweep(n - 1, omega)
    for k in range(n - 2, -1, -1):
        prolong_add_(cur[k + 1][0], cur[k][0])
        for _ in range(nu2):
            sweep(k, omega)


def mg_tail(levels, nu1: int, nu2: int, coarse_sweeps: int, omega: float) -> None:
    """The V-cycle from ``levels[0]`` down to the coarsest level and back up, as
    ``PoissonMultigrid._vcycle`` runs it for a level k >= 1. ``levels``: a
    sequence of ``(u, un, b, r_or_None)``, finest first, each the coarse grid
    of the one before it; the four tensors of a level share one shape and one
    row pitch; only the last level may go without ``r``. Per level but the
    last: ``nu1`` damped sweeps with the level's ``b``, the residual into
    ``r``, full weighting into the next level's ``b``, the next level's ``u``
    <- 0 (its H x W elements), the next level, prolongation added in place,
    ``nu2`` sweeps. The last level: ``coarse_sweeps`` sweeps, or one undamped
    sweep when it is 3 x 3.

    Where the results lie: sweeps ping-pong between a level's ``u`` and ``un``,
    starting from ``u`` (for a level below ``levels[0]``, from the zeroed
    ``u``), so a level's iterate ends in ``un`` if it ran an odd number of
    sweeps (``tail_sweeps``), in ``u`` otherwise; the other of the two and
    ``r`` are scratch. Rows 0 and H - 1 of ``un`` are never written: as for
    ``jacobi_relax`` they are input, the level's boundary values (zeros below
    ``levels[0]``). ``b`` of every level below ``levels[0]`` holds the
    restricted residual.

    GPU tensors: one launch of one workgroup on the current stream, nothing
    allocated, no synchronisation; bit-identical to the launched operators.
    CPU float64 tensors: the same sequence with the CPU operators."""
    nu1, nu2, coarse_sweeps, omega = _tail_params(nu1, nu2, coarse_sweeps, omega)
    desc = _tail_desc(levels)
    levels = [tuple(lv) for lv in levels]
    u0 = levels[0][0]
    if u0.is_cuda:
        _tail_launch(desc, u0.dtype, nu1, nu2, coarse_sweeps, omega, _native.stream_of(u0))
        return
    _tail_on_cpu(levels, nu1, nu2, coarse_sweeps, omega, lambda t: tuple(t.shape) == (3, 3),
                 lambda u, un, om, b: jacobi_relax(u, un, 1, u.shape[0] - 1, om, rhs=b), mg_residual, mg_restrict,
                 mg_prolong_add_)
