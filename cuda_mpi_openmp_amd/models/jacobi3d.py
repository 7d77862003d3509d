"""3-D Jacobi solver on a plane-slab decomposed box: the Dirichlet problem for
the Laplace equation by default, the Poisson equation -Laplace(u) = f once a
right-hand side is set (``SlabJacobi3D.set_rhs``, b = h^2 f). It mirrors
``SlabJacobi`` one dimension up: the global (global_planes, ny, nx) volume is
split over z, each rank stores its planes with one halo plane below and above,
and a sweep is the 7-point kernel of ``ops.jacobi3d_sweep``.

Halo transport: the two-sided exchange of ``parallel.HaloExchange`` on the
buffers viewed as (buffer_planes, ny * nx) — a plane is one buffer row, so the
2-D transport moves it unchanged. Per iteration and rank, overlapped form:
  1. sweep the two slab-edge planes (the only planes a neighbour needs);
  2. start the halo exchange of those planes;
  3. sweep the interior planes while the exchange is in flight;
  4. wait for the halos, swap u <-> u_new.
With the native RCCL tier the step runs in order (sweep, then exchange). Every
``check_every`` iterations the sweeps fold max|s - u| into a device scalar and
one all-reduce(MAX) produces the global residual. Device-signalled peer halos
and HIP graphs are not implemented for planes.

Chebyshev acceleration (``accel="chebyshev"``) is the 2-D solver's schedule
with the box's Jacobi spectral radius.

Global boundary: Dirichlet. Plane 0 of rank 0's buffer is the z = 0 face, the
last buffer plane of the last rank the opposite face; rows 0 / ny - 1 and
columns 0 / nx - 1 of every plane are fixed. A decomposed run is bit-identical
to a one-rank run.
"""

from __future__ import annotations

import math
from typing import Callable, Optional

import torch
import torch.distributed as dist

from .. import ops
from ..parallel.collectives import all_reduce_max, gather_slabs
from ..parallel.dist import DistContext
from ..parallel.halo import HaloExchange
from ..parallel.slab import Slab


class SlabJacobi3D:
    """Jacobi iteration on this rank's plane slab:
    u <- ((((zm + zp) + (ym + yp)) + (xm + xp)) [+ b]) / 6.

    ``accel="chebyshev"``: Golub-Varga acceleration exactly as in
    ``SlabJacobi``, with
    rho = (cos(pi / (global_planes + 1)) + cos(pi / (ny - 1)) + cos(pi / (nx - 1))) / 3:
    step 1 of a sequence is the plain sweep, step 2 uses
    omega = 1 / (1 - rho^2 / 2), step k >= 3 omega_k = 1 / (1 - rho^2 omega_{k-1} / 4),
    computed in Python floats from the step count and the global geometry only,
    so every rank passes the same bits. ``fill``, ``set_boundary``, ``set_rhs``,
    a halo re-synchronisation, a checkpoint without history and
    ``restart_acceleration()`` restart the sequence."""

    def __init__(self, ctx: DistContext, global_planes: int, ny: int, nx: int, dtype=torch.float64,
                 check_every: int = 10, overlap: bool | str = "auto", halo: str = "auto",
                 accel: Optional[str] = None):
        if nx < 3 or ny < 3:
            raise ValueError("need at least 3 rows and 3 columns")
        if ny * nx >= 2 ** 31:
            raise ValueError("a plane must hold fewer than 2^31 points")
        if accel not in (None, "chebyshev"):
            raise ValueError(f"unknown acceleration {accel!r} (None or 'chebyshev')")
        if halo not in ("auto", "peer", "rccl", "none"):
            raise ValueError(f"unknown halo transport {halo!r}")
        if halo == "peer":
            raise ValueError("device-signalled peer halos are not implemented for plane slabs: use halo='rccl'")
        self.accel = accel
        self.rho: Optional[float] = None
        if accel is not None:
            self.rho = (math.cos(math.pi / (global_planes + 1)) + math.cos(math.pi / (ny - 1))
                        + math.cos(math.pi / (nx - 1))) / 3.0
        self.omega: Optional[float] = None
        self.accel_step = 0
        self._un_is_history = False  # load_checkpoint restored the previous iterate into un
        self.ctx = ctx
        self.ny, self.nx = ny, nx
        self.dtype = dtype
        self.check_every = max(1, int(check_every))
        self.overlap = (ctx.native is None) if overlap == "auto" else bool(overlap)
        # "none": benchmarking ablation only (wrong answer, same per-rank work)
        self.no_halo = halo == "none"
        if self.no_halo:
            self.overlap = False
        self.slab = Slab(global_planes, ctx.world, ctx.rank, halo_up=1, halo_down=1)
        self.halo = HaloExchange(self.slab, ctx)
        shape = (self.slab.buffer_rows, ny, nx)
        dev = ctx.device
        self.u = torch.zeros(shape, dtype=dtype, device=dev)
        self.un = torch.zeros(shape, dtype=dtype, device=dev)
        # persistent (buffer_planes, ny * nx) views for the halo exchange: a plane is one row
        self._rows = {t.data_ptr(): t.view(shape[0], ny * nx) for t in (self.u, self.un)}
        self.resid = torch.zeros(1, dtype=dtype, device=dev)
        self.rhs: Optional[torch.Tensor] = None  # (buffer_planes, ny, nx) once set_rhs has run
        self.iteration = 0
        self.last_residual: Optional[float] = None
        self._halos_valid = False  # u's halo planes hold the neighbours' current planes

    # ------------------------------------------------------------------ setup
    def set_boundary(self, z0: float = 1.0, z1: float = 0.0, y0: float = 0.0, y1: float = 0.0, x0: float = 0.0,
                     x1: float = 0.0) -> None:
        """Dirichlet faces: x faces first, then y, then z on the ranks that own a
        global face (later assignments win on the shared edges)."""
        for t in (self.u, self.un):
            t[:, :, 0] = x0
            t[:, :, -1] = x1
            t[:, 0, :] = y0
            t[:, -1, :] = y1
            if not self.slab.has_up:
                t[0] = z0
            if not self.slab.has_down:
                t[-1] = z1
        self._halos_valid = False
        self.restart_acceleration()

    def _coords(self):
        s = self.slab
        dev = self.u.device
        z = torch.arange(s.row0, s.row0 + s.rows, device=dev).view(-1, 1, 1)
        y = torch.arange(1, self.ny - 1, device=dev).view(1, -1, 1)
        x = torch.arange(1, self.nx - 1, device=dev).view(1, 1, -1)
        return z, y, x

    def fill(self, fn: Optional[Callable[..., torch.Tensor]] = None, seed: int = 0) -> None:
        """Interior initial values: fn(global_plane_index, row_index, col_index)
        (broadcastable index tensors) or seeded noise."""
        s = self.slab
        if fn is None:
            g = torch.Generator(device="cpu").manual_seed(seed + 7919 * self.ctx.rank)
            vals = torch.rand((s.rows, self.ny - 2, self.nx - 2), generator=g, dtype=torch.float64).to(self.u.device)
        else:
            vals = torch.as_tensor(fn(*self._coords()), device=self.u.device)
        self.u[1:1 + s.rows, 1:-1, 1:-1] = vals.to(self.dtype)
        self.un.copy_(self.u)
        self._halos_valid = False
        self.restart_acceleration()

    def set_rhs(self, fn: Optional[Callable[..., torch.Tensor]] = None,
                tensor: Optional[torch.Tensor] = None) -> None:
        """Right-hand side b = h^2 f on this rank's planes: ``fn(z, y, x)`` with
        ``fill``'s conventions, or ``tensor``, this rank's owned planes as
        (planes, ny, nx). Halo planes and boundary elements are never read."""
        if (fn is None) == (tensor is None):
            raise ValueError("set_rhs takes exactly one of fn and tensor")
        s = self.slab
        if tensor is not None and tuple(tensor.shape) != (s.rows, self.ny, self.nx):
            raise ValueError(f"rhs tensor must hold this rank's owned planes, shape {(s.rows, self.ny, self.nx)}")
        self.restart_acceleration()
        if self.rhs is None:
            self.rhs = torch.zeros_like(self.u)
        if tensor is not None:
            self.rhs[1:1 + s.rows] = tensor.to(self.u.device, self.dtype)
        else:
            vals = torch.as_tensor(fn(*self._coords()), device=self.u.device)
            self.rhs[1:1 + s.rows, 1:-1, 1:-1] = vals.to(self.dtype)

    @property
    def transport(self) -> Optional[str]:
        if not self.ctx.is_distributed:
            return None
        if self.no_halo:
            return "none (ablation: no halo exchange)"
        return "native-rccl" if self.ctx.native is not None else "torch.distributed"

    def restart_acceleration(self) -> None:
        """The next step is step 1 of the Chebyshev sequence again: a plain
        sweep that ignores ``un``. No-op without ``accel``."""
        self.accel_step = 0
        self.omega = None
        self._un_is_history = False

    def _next_omega(self) -> Optional[float]:
        """omega of the step about to run; None for the plain step (k = 1, or
        no acceleration). A function of k and the global geometry only."""
        if self.accel is None or self.accel_step == 0:
            return None
        if self.accel_step == 1:
            return 1.0 / (1.0 - self.rho * self.rho / 2.0)
        return 1.0 / (1.0 - self.rho * self.rho * self.omega / 4.0)

    def _reset_un(self) -> None:
        """un <- u before the first sweep after a (re)initialisation (un's fixed
        faces are never swept), which restarts the Chebyshev sequence, unless
        load_checkpoint has just put the previous iterate there: then only the
        halo planes are refreshed."""
        if self._un_is_history:
            self.un[0].copy_(self.u[0])
            self.un[-1].copy_(self.u[-1])
            self._un_is_history = False
            return
        self.un.copy_(self.u)
        self.restart_acceleration()

    # ------------------------------------------------------------------ halos
    @property
    def _host_staged(self) -> bool:
        """GPU slabs on a gloo control plane (several ranks rehearsed on one
        GPU): gloo reads a send buffer from the host with no stream order, so
        the edge planes go through host copies, which wait for the sweeps."""
        return self.ctx.is_distributed and self.u.is_cuda and self.ctx.backend != "nccl"

    def _halo_start(self, t: torch.Tensor) -> None:
        if not self._host_staged:
            self.halo.start(self._rows[t.data_ptr()])
            return
        s, rank = self.slab, self.ctx.rank
        p2p, self._staged_recvs = [], []
        for has, peer, own, halo in ((s.has_up, rank - 1, 1, 0), (s.has_down, rank + 1, s.rows, s.rows + 1)):
            if has:
                p2p.append(dist.P2POp(dist.isend, t[own].cpu(), peer))  # .cpu(): after the edge sweeps
                h = torch.empty((self.ny, self.nx), dtype=self.dtype)
                p2p.append(dist.P2POp(dist.irecv, h, peer))
                self._staged_recvs.append((halo, h))
        self._staged_works = dist.batch_isend_irecv(p2p) if p2p else []

    def _halo_wait(self, t: torch.Tensor) -> None:
        if not self._host_staged:
            self.halo.wait()
            return
        for w in self._staged_works:
            w.wait()
        for k, h in self._staged_recvs:
            t[k].copy_(h)
        self._staged_works, self._staged_recvs = [], []

    def _halo_exchange(self, t: torch.Tensor) -> None:
        if self._host_staged:
            self._halo_start(t)
            self._halo_wait(t)
        else:
            self.halo.exchange(self._rows[t.data_ptr()])

    def sync_halos(self) -> None:
        """Exchange u's slab-edge planes (needed once after (re)initialisation;
        afterwards every step refreshes the halos of the planes it computes)."""
        if not self.no_halo:
            self._halo_exchange(self.u)
        self._reset_un()
        self._halos_valid = True

    @property
    def owned(self) -> torch.Tensor:
        return self.u[1:1 + self.slab.rows]

    # ------------------------------------------------------------------ stepping
    def _sweep(self, k0: int, k1: int, track: bool, omega: Optional[float] = None) -> None:
        if k1 <= k0:
            return
        if self.u.is_cuda:
            ops.jacobi3d_sweep(self.u, self.un, k0, k1, self.resid if track else None, rhs=self.rhs, omega=omega)
        else:
            r = ops.jacobi3d_sweep(self.u, self.un, k0, k1, rhs=self.rhs, omega=omega)
            if track:
                self.resid.fill_(max(float(self.resid.item()), r))

    def step(self) -> Optional[float]:
        if not self._halos_valid:
            self.sync_halos()
        track = (self.iteration + 1) % self.check_every == 0
        n = self.slab.rows
        if track:
            self.resid.zero_()
        w = self._next_omega()  # None: the plain sweeps, exactly as without accel
        if self.ctx.is_distributed and self.overlap and not self.no_halo:
            for k in ([1] if n == 1 else [1, n]):
                self._sweep(k, k + 1, track, w)
            self._halo_start(self.un)    # waits for the edge planes only
            self._sweep(2, n, track, w)  # interior overlaps the transfer
            self._halo_wait(self.un)
        else:
            self._sweep(1, n + 1, track, w)
            if not self.no_halo:
                self._halo_exchange(self.un)
        self.u, self.un = self.un, self.u
        self.iteration += 1
        if self.accel is not None:
            self.omega = 1.0 if w is None else w
            self.accel_step += 1
        if track:
            all_reduce_max(self.resid, self.ctx)
            self.last_residual = float(self.resid.item())
            return self.last_residual
        return None

    def run(self, iters: int, tol: Optional[float] = None) -> int:
        """``iters`` iterations (fewer once the residual drops below ``tol``)."""
        for _ in range(iters):
            r = self.step()
            if tol is not None and r is not None and r < tol:
                break
        return self.iteration

    # ------------------------------------------------------------------ I/O
    def gather(self) -> Optional[torch.Tensor]:
        return gather_slabs(self.owned.contiguous(), self.slab, self.ctx)

    def save_checkpoint(self, prefix: str) -> str:
        """One file per rank: owned planes (+ halos), iteration, residual and,
        when one is set, the right-hand side. An accelerated solver also stores
        the previous iterate (``u_prev``) and ``accel`` = {step, omega, rho}, so
        a resumed run continues the Chebyshev sequence bit for bit."""
        path = f"{prefix}.rank{self.ctx.rank}.pt"
        ck = {"u": self.u.cpu(), "iteration": self.iteration, "residual": self.last_residual,
              "global_planes": self.slab.global_rows, "world": self.ctx.world, "ny": self.ny, "nx": self.nx}
        if self.rhs is not None:
            ck["rhs"] = self.rhs.cpu()
        if self.accel is not None:
            # a pending re-synchronisation restarts the sequence anyway
            live = self._halos_valid and self.accel_step > 0
            ck["u_prev"] = self.un.cpu()
            ck["accel"] = {"step": self.accel_step if live else 0, "omega": self.omega if live else None,
                           "rho": self.rho}
        torch.save(ck, path)
        return path

    def load_checkpoint(self, prefix: str) -> None:
        ck = torch.load(f"{prefix}.rank{self.ctx.rank}.pt", weights_only=True)
        if (ck["global_planes"], ck["world"], ck["ny"], ck["nx"]) != (self.slab.global_rows, self.ctx.world, self.ny,
                                                                     self.nx):
            raise ValueError("checkpoint geometry does not match this solver")
        self.u.copy_(ck["u"].to(self.u.device, self.dtype))
        self.un.copy_(self.u)
        if "rhs" in ck:  # checkpoints without one leave this solver's rhs alone
            if self.rhs is None:
                self.rhs = torch.zeros_like(self.u)
            self.rhs.copy_(ck["rhs"].to(self.u.device, self.dtype))
        self.iteration = int(ck["iteration"])
        self.last_residual = ck["residual"]
        self._halos_valid = False
        self.restart_acceleration()  # checkpoints without history load as a restart
        if self.accel is not None and "u_prev" in ck and "accel" in ck and int(ck["accel"]["step"]) > 0:
            # sync_halos must not clobber the previous iterate in un's owned planes
            self.un.copy_(ck["u_prev"].to(self.u.device, self.dtype))
            self.accel_step = int(ck["accel"]["step"])
            self.omega = float(ck["accel"]["omega"])
            self._un_is_history = True
