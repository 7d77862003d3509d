"""Geometric multigrid V-cycle for the 3-D Poisson problem -Laplace(u) = f in a
box on one device, in ``SlabJacobi3D``'s layout and discretisation at world
size 1 (b = h^2 f, Dirichlet values on all six faces of the
(planes + 2, ny, nx) buffer; the fixed point satisfies
6 u - (sum of the six neighbours) = b).

Level 0 is the (planes + 2, ny, nx) grid. A level (D, H, W) has the coarse
level (Dc, Hc, Wc) with D = 2 Dc - 1, H = 2 Hc - 1, W = 2 Wc - 1 while D - 1,
H - 1 and W - 1 are all even and the coarse grid keeps an interior. One
V(nu1, nu2) cycle at level l:

  1. nu1 damped Jacobi sweeps (``ops.jacobi3d_relax``);
  2. the residual r = b + sum(neighbours) - 6 u (``ops.mg3_residual``);
  3. full weighting of r into level l+1's right-hand side (``ops.mg3_restrict``);
  4. level l+1's u <- 0 (the error equation has zero Dirichlet values);
  5. the cycle on level l+1;
  6. trilinear interpolation of level l+1's u added to u (``ops.mg3_prolong_add_``);
  7. nu2 damped Jacobi sweeps.

The coarsest level runs ``coarse_sweeps`` sweeps, or, with a single interior
point, one undamped sweep (the exact solve up to rounding). Every operator has
one defined rounding order, so a GPU fp64 cycle is bit-identical to the CPU
cycle. With ``tail_points`` the levels of at most that many points run in one
kernel of one workgroup (``ops.mg3_tail``), bit-identical to their launches.
All buffers are allocated in the constructor, with the row pitch rounded
up to 16 bytes so the odd widths take the vector kernels; ``cycle()``
allocates nothing.

Full multigrid (``fmg()``) solves from scratch instead of cycling on level 0,
as ``PoissonMultigrid.fmg`` does in 2-D:

  1. level 0's b is restricted down the hierarchy (``ops.mg3_restrict``) and
     level 0's Dirichlet values are injected into every level (level k's point
     (K, J, I) is level 0's (2^k K, 2^k J, 2^k I));
  2. the coarsest level is solved from a zero interior by the V-cycle's
     coarsest treatment;
  3. level by level up to level 0: the coarser level's solution is
     interpolated into the level's interior (``ops.mg3_prolong_cubic``: the
     solution, not a correction, so the interpolant must be of higher order
     than the discretisation; with the V-cycle's trilinear one the algebraic
     error stays 7 to 21 times the discretisation error) and
     ``cycles_per_level`` V-cycles start there with the level's restricted b.

The default is two cycles per level, not the 2-D solver's one: the 3-D V(2,2)
cycle contracts by 0.15 to 0.26 per cycle (2-D: 0.11 to 0.15), and with one
cycle per level the algebraic error is 0.9 to 2.6 times the discretisation
error and grows with the grid, while with two it stays near 0.14 of it at
every size. ``fmg()`` uses the constructor's buffers and allocates nothing on
the device.
"""

from __future__ import annotations

import math
from typing import Callable, List, Optional, Tuple

import torch

from .. import _native, ops
from ..ops.multigrid3d import _tail3_desc, _tail3_launch


class _Level3:
    """Buffers of one grid level: pitched (D, H, W) views u, un, b, r."""

    def __init__(self, d: int, h: int, w: int, dtype, device, with_r: bool):
        nv = 16 // torch.empty((), dtype=dtype).element_size()
        pitch = (w + nv - 1) // nv * nv
        self.d, self.h, self.w = d, h, w
        self._bufs = []

        def grid() -> torch.Tensor:
            buf = torch.zeros((d, h, pitch), dtype=dtype, device=device)
            self._bufs.append(buf)
            return buf[:, :, :w]

        self.u, self.un, self.b = grid(), grid(), grid()
        self.r = grid() if with_r else None

    def zero_u(self) -> None:
        """u <- 0 on the whole backing buffer (one contiguous fill)."""
        self.u._base.zero_()


class PoissonMultigrid3D:
    """V-cycle solver for 6 u - (sum of the six neighbours) = b on a
    (planes + 2, ny, nx) grid with Dirichlet boundary values.

    ``levels``: the list of level shapes, finest first. ``cycle()`` runs one
    V-cycle and returns the fused max|s - u| of level 0's last post-smoothing
    sweep (``last_residual``, ``SlabJacobi3D.last_residual``'s meaning);
    ``solve(tol)`` cycles until it is at most ``tol``. ``cycles`` counts the
    cycles run. float64 on CPU tensors, float64 / float32 on the GPU.

    ``tail_points``: the finest level k >= 1 with at most that many points
    (D * H * W) and every level below it run as one kernel (``tail_level``:
    its index, or None); 0: every level is launched; None: the measured
    default on the GPU (``DEFAULT_TAIL_POINTS``), 0 on CPU tensors. The results
    do not depend on it. ``launches_per_cycle``: the launches of one cycle,
    the fill of a coarse u counted as one.

    The
    default omega = 6/7 is the damping with the best smoothing factor (5/7) of
    the 7-point Jacobi iteration."""

    # tail_points=None on the GPU: the threshold with the shortest measured cycle, per dtype (profiles/multigrid3d.md)
    DEFAULT_TAIL_POINTS = {torch.float64: 4913, torch.float32: 4913}

    def __init__(self, planes: int, ny: int, nx: int, dtype=torch.float64, device=None, nu1: int = 2, nu2: int = 2,
                 omega: float = 6.0 / 7.0, coarse_sweeps: int = 50, max_levels: Optional[int] = None,
                 tail_points: Optional[int] = None):
        if planes < 1 or ny < 3 or nx < 3:
            raise ValueError("need at least 1 interior plane, 3 rows and 3 columns")
        if nu1 < 0 or nu2 < 1:
            raise ValueError("need nu1 >= 0 and nu2 >= 1 (the residual comes from the last post-smoothing sweep)")
        if coarse_sweeps < 1:
            raise ValueError("need coarse_sweeps >= 1")
        omega = float(omega)
        if not (math.isfinite(omega) and omega > 0.0):
            raise ValueError("omega must be finite and positive")
        if max_levels is not None and max_levels < 1:
            raise ValueError("max_levels must be at least 1")
        if tail_points is not None and tail_points < 0:
            raise ValueError("tail_points must be at least 0")
        self.device = torch.device("cpu" if device is None else device)
        if self.device.type != "cuda" and dtype != torch.float64:
            raise ValueError("the CPU model is float64")
        if dtype not in (torch.float64, torch.float32):
            raise ValueError("PoissonMultigrid3D supports float64/float32")
        self.planes, self.ny, self.nx, self.dtype = planes, ny, nx, dtype
        self.nu1, self.nu2, self.omega, self.coarse_sweeps = int(nu1), int(nu2), omega, int(coarse_sweeps)
        self.levels: List[Tuple[int, int, int]] = self.level_shapes(planes, ny, nx, max_levels)
        # a level's r feeds the restriction, so the coarsest level has none
        self._lv = [_Level3(d, h, w, dtype, self.device, with_r=k + 1 < len(self.levels))
                    for k, (d, h, w) in enumerate(self.levels)]
        self.resid = torch.zeros(1, dtype=dtype, device=self.device)
        self.cycles = 0
        self.last_residual: Optional[float] = None
        if tail_points is None:
            tail_points = self.DEFAULT_TAIL_POINTS[dtype] if self.device.type == "cuda" else 0
        self.tail_points = int(tail_points)
        self.tail_level: Optional[int] = next(
            (k for k in range(1, len(self.levels)) if math.prod(self.levels[k]) <= self.tail_points), None)
        self._tail_sweeps: List[int] = []
        self._tail_desc = None
        self._fmg_ready = False
        self._fmg_desc: dict = {}  # fmg(): the tail descriptors of the levels below tail_level
        if self.tail_level is not None:
            tail = self._lv[self.tail_level:]
            self._tail_sweeps = ops.tail_sweeps(len(tail), self.nu1, self.nu2, self.coarse_sweeps,
                                                math.prod(self.levels[-1]) == 27)
            if self.device.type == "cuda":
                # validated once; _tail() only refreshes the u / un pointers (host memory only)
                self._tail_desc = _tail3_desc([(lv.u, lv.un, lv.b, lv.r) for lv in tail])

    @property
    def launches_per_cycle(self) -> int:
        """Kernel launches of one cycle (the fill of a coarse u counts as one;
        the zeroing of the residual word does not)."""
        n = len(self.levels)
        if n == 1:
            return self.nu1 + self.nu2
        launched = n - 1 if self.tail_level is None else self.tail_level
        total = launched * (self.nu1 + self.nu2 + 4)
        if self.tail_level is not None:
            return total + 1
        return total + (1 if math.prod(self.levels[-1]) == 27 else self.coarse_sweeps)

    @staticmethod
    def level_shapes(planes: int, ny: int, nx: int, max_levels: Optional[int] = None) -> List[Tuple[int, int, int]]:
        shapes = [(planes + 2, ny, nx)]
        while max_levels is None or len(shapes) < max_levels:
            if any((s - 1) % 2 for s in shapes[-1]):
                break
            coarse = tuple((s + 1) // 2 for s in shapes[-1])
            if min(coarse) < 3:
                break
            shapes.append(coarse)
        return shapes

    # ------------------------------------------------------------------ setup
    @property
    def u(self) -> torch.Tensor:
        """Level 0's current iterate, a (D, H, W) view."""
        return self._lv[0].u

    @property
    def rhs(self) -> torch.Tensor:
        return self._lv[0].b

    def set_boundary(self, z0: float = 1.0, z1: float = 0.0, y0: float = 0.0, y1: float = 0.0, x0: float = 0.0,
                     x1: float = 0.0) -> None:
        """Dirichlet faces in ``SlabJacobi3D.set_boundary``'s order: x faces
        first, then y, then z (later assignments win on the shared edges)."""
        f = self._lv[0]
        for t in (f.u, f.un):
            t[:, :, 0] = x0
            t[:, :, -1] = x1
            t[:, 0, :] = y0
            t[:, -1, :] = y1
            t[0] = z0
            t[-1] = z1

    def _coords(self):
        z = torch.arange(0, self.planes, device=self.device).view(-1, 1, 1)
        y = torch.arange(1, self.ny - 1, device=self.device).view(1, -1, 1)
        x = torch.arange(1, self.nx - 1, device=self.device).view(1, 1, -1)
        return z, y, x

    def fill(self, fn: Optional[Callable[..., torch.Tensor]] = None, seed: int = 0) -> None:
        """Interior initial values: fn(plane_index, row_index, col_index) or
        seeded noise (``SlabJacobi3D.fill``'s values at world size 1)."""
        f = self._lv[0]
        if fn is None:
            g = torch.Generator(device="cpu").manual_seed(seed)
            vals = torch.rand((self.planes, self.ny - 2, self.nx - 2), generator=g, dtype=torch.float64).to(self.device)
        else:
            vals = torch.as_tensor(fn(*self._coords()), device=self.device)
        f.u[1:-1, 1:-1, 1:-1] = vals.to(self.dtype)
        f.un.copy_(f.u)

    def set_rhs(self, fn: Optional[Callable[..., torch.Tensor]] = None, tensor: Optional[torch.Tensor] = None) -> None:
        """Right-hand side b = h^2 f: ``fn(plane_index, row_index, col_index)``
        over the interior, or ``tensor``, the owned planes as (planes, ny, nx)."""
        if (fn is None) == (tensor is None):
            raise ValueError("set_rhs takes exactly one of fn and tensor")
        b = self._lv[0].b
        if tensor is not None:
            if tuple(tensor.shape) != (self.planes, self.ny, self.nx):
                raise ValueError(f"rhs tensor must hold the owned planes, shape {(self.planes, self.ny, self.nx)}")
            b[1:-1] = tensor.to(self.device, self.dtype)
        else:
            b[1:-1, 1:-1, 1:-1] = torch.as_tensor(fn(*self._coords()), device=self.device).to(self.dtype)

    # ------------------------------------------------------------------ cycle
    def _relax(self, lv: _Level3, omega: float, track: bool = False) -> None:
        ops.jacobi3d_relax(lv.u, lv.un, 1, lv.d - 1, omega, self.resid if track else None, rhs=lv.b)
        lv.u, lv.un = lv.un, lv.u

    def _tail(self, k: Optional[int] = None) -> None:
        """Levels ``k`` (default and at least ``tail_level``) and below in one
        kernel; leaves the level objects as their launches would (u and un
        swapped after an odd number of sweeps)."""
        k = self.tail_level if k is None else k
        tail = self._lv[k:]
        desc = self._tail_desc if k == self.tail_level else self._fmg_desc.get(k)
        if desc is None:
            ops.mg3_tail([(lv.u, lv.un, lv.b, lv.r) for lv in tail], self.nu1, self.nu2, self.coarse_sweeps, self.omega)
        else:
            for d, lv in zip(desc, tail):
                d.u, d.un = lv.u.data_ptr(), lv.un.data_ptr()
            _tail3_launch(desc, self.dtype, self.nu1, self.nu2, self.coarse_sweeps, self.omega,
                          _native.stream_of(tail[0].u))
        for lv, n in zip(tail, self._tail_sweeps[k - self.tail_level:]):
            if n & 1:
                lv.u, lv.un = lv.un, lv.u

    def _vcycle(self, k: int) -> None:
        if k == self.tail_level:
            self._tail()
            return
        lv = self._lv[k]
        if k + 1 == len(self._lv) and k > 0:
            if (lv.d, lv.h, lv.w) == (3, 3, 3):
                self._relax(lv, 1.0)
            else:
                for _ in range(self.coarse_sweeps):
                    self._relax(lv, self.omega)
            return
        for _ in range(self.nu1):
            self._relax(lv, self.omega)
        if k + 1 < len(self._lv):
            nx = self._lv[k + 1]
            ops.mg3_residual(lv.u, lv.r, rhs=lv.b)
            ops.mg3_restrict(lv.r, nx.b)
            nx.zero_u()
            self._vcycle(k + 1)
            ops.mg3_prolong_add_(nx.u, lv.u)
        for s in range(self.nu2):
            self._relax(lv, self.omega, track=(k == 0 and s == self.nu2 - 1))

    def cycle(self) -> float:
        """One V-cycle; one host read (the residual)."""
        self.resid.zero_()
        self._vcycle(0)
        self.cycles += 1
        self.last_residual = float(self.resid.item())
        return self.last_residual

    # -------------------------------------------------------------------- fmg
    def _fmg_setup(self) -> None:
        """First call of ``fmg()`` on the GPU: the descriptors of the tails that
        start below ``tail_level`` (host memory)."""
        self._fmg_ready = True
        if self._tail_desc is not None:
            for k in range(self.tail_level + 1, len(self._lv)):
                self._fmg_desc[k] = _tail3_desc([(lv.u, lv.un, lv.b, lv.r) for lv in self._lv[k:]])

    def _fmg_cycle(self, k: int) -> None:
        """One V-cycle that starts at level k: one launch at or below ``tail_level``."""
        if self.tail_level is not None and k >= self.tail_level:
            self._tail(k)
        else:
            self._vcycle(k)

    def fmg(self, cycles_per_level: int = 2) -> float:
        """Full multigrid: solves from scratch for level 0's ``b`` and the
        Dirichlet values found on the six faces of level 0's ``u`` (they may
        vary over a face). Level 0's interior is ignored and overwritten.
        Every level, coarsest first, gets the tricubic interpolation of the
        level below it (the coarsest: zeros) and then ``cycles_per_level``
        V-cycles that start there. Returns ``last_residual`` of level 0's last
        cycle, the one host read; ``cycles`` grows by ``cycles_per_level``.
        The levels below level 0 are left as ``cycle()`` expects them, so
        cycles may follow.

        ``cycles_per_level`` defaults to 2 where ``PoissonMultigrid.fmg``
        takes 1: the 3-D V(2,2) cycle contracts by 0.15 to 0.26 per cycle, too
        weak for one. With one cycle per level the algebraic error is 0.9 to
        2.6 times the discretisation error of the 7-point scheme and grows
        with the grid; with two it is about 0.14 of it at every size (smooth
        solutions, a hierarchy that reaches a small coarsest grid: a 3 x 3 x 3
        one is solved exactly, any other gets ``coarse_sweeps`` sweeps per
        cycle). With one level ``fmg()`` zeroes the interior and runs the
        cycles."""
        cpl = int(cycles_per_level)
        if cpl < 1:
            raise ValueError("cycles_per_level must be at least 1")
        lvs, n = self._lv, len(self._lv)
        if not self._fmg_ready:
            self._fmg_setup()
        # 1. right-hand sides, restricted straight into the levels' b (its boundary is
        # never read or written): a cycle that starts at level k overwrites b below
        # level k only, and the levels take their turn from the coarsest up
        for k in range(1, n):
            ops.mg3_restrict(lvs[k - 1].b, lvs[k].b)
        # 2. Dirichlet values by injection. The z and y faces into both buffers of a
        # level (a launched sweep never writes planes 0 and D - 1 of its output,
        # the tail kernel neither those nor rows 0 and H - 1); the x faces into u
        # only: every sweep copies them through
        f = lvs[0]
        f.un[::f.d - 1].copy_(f.u[::f.d - 1])
        f.un[:, ::f.h - 1].copy_(f.u[:, ::f.h - 1])
        for k in range(1, n):
            lv, s = lvs[k], 1 << k
            zf, yf, xf = f.u[::f.d - 1, ::s, ::s], f.u[::s, ::f.h - 1, ::s], f.u[::s, ::s, ::f.w - 1]
            for t in (lv.u, lv.un):
                t[::lv.d - 1].copy_(zf)
                t[:, ::lv.h - 1].copy_(yf)
            lv.u[:, :, ::lv.w - 1].copy_(xf)
        # 3. the coarsest level from a zero interior
        lvs[-1].u[1:-1, 1:-1, 1:-1].zero_()
        for c in range(cpl):
            if n == 1:
                self.resid.zero_()
            self._fmg_cycle(n - 1)
        # 4. up the hierarchy
        for k in range(n - 2, -1, -1):
            lv, nx = lvs[k], lvs[k + 1]
            ops.mg3_prolong_cubic(nx.u, lv.u)
            # from here level k + 1 holds error equations: zero Dirichlet values. The
            # cycle zeroes its u as a whole and the sweeps copy u's columns to un,
            # which leaves the two planes and the two rows of un
            nx.un[::nx.d - 1].zero_()
            nx.un[:, ::nx.h - 1].zero_()
            for c in range(cpl):
                if k == 0:
                    self.resid.zero_()
                self._fmg_cycle(k)
        self.cycles += cpl
        self.last_residual = float(self.resid.item())
        return self.last_residual

    def solve(self, tol: float, max_cycles: int = 50) -> int:
        """Cycle until ``last_residual <= tol`` or ``max_cycles`` cycles have
        run; returns the number of cycles run by this call."""
        n = 0
        while n < max_cycles:
            n += 1
            if self.cycle() <= tol:
                break
        return n
