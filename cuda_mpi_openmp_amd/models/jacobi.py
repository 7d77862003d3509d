"""2-D Jacobi solver on a row-slab decomposed grid: the Laplace equation by
default, the Poisson equation -Laplace(u) = f once a right-hand side is set
(``SlabJacobi.set_rhs``, b = h^2 f; every transport, graphs and checkpoints
carry it) — the distributed-stencil north star of BASELINE.json ("MPI -> RCCL 2D Jacobi
stencil, 16384^2 grid domain-decomposed across 8 MI355X, halo exchange over
xGMI"). The reference has no such solver; this is its MI355X-native
form.

Halo transports (``halo=``):

* ``"peer"`` (GPU, default when available): one-sided and device-signalled.
  Each rank IPC-maps its neighbours' mailboxes (completed-iteration word and
  two parity slots of their edge rows; the slabs are never shared, so they
  may be any size) once; every iteration is ONE sweep kernel whose slab-edge
  waves wait on the neighbours' counters, read their edge rows over xGMI,
  write this rank's new edge rows write-through into its mailbox and publish
  its counter (native/src/kernels/jacobi.hip, ``parallel.peer.
  JacobiPeerLink``). No exchange kernel, no host round trip per iteration.
* ``"rccl"``: two-sided send/recv of the edge rows (below).

RCCL transport, per iteration and rank:
  1. sweep the two slab-edge rows (the only rows a neighbour needs);
  2. post the halo exchange of those freshly computed rows over RCCL
     (point-to-point on the xGMI link between neighbouring GPUs);
  3. sweep the interior rows while the exchange is in flight;
  4. wait for the halos, swap u <-> u_new.
Every ``check_every`` iterations the sweeps also fold max|u_new - u| into a
device scalar and one 8-byte all-reduce(MAX) produces the global residual (the
small-message latency over xGMI is paid once per check, not per iteration).

Chebyshev acceleration (``accel="chebyshev"``): the semi-iterative three-term
recurrence u_{k+1} = u_{k-1} + omega_{k+1} (J(u_k) - u_{k-1}) over the same
sweeps (J: the plain or Poisson Jacobi update). The iterate before last is
what ``un`` holds when a sweep starts, so the sweep reads one more word per
point and allocates nothing; only u's edge rows cross ranks, as before. The
iteration count to a fixed tolerance drops from O(N^2) to O(N).

Global boundary: Dirichlet. Row 0 of rank 0's buffer is the top boundary, the
last buffer row of the last rank the bottom boundary; columns 0 and cols-1 are
fixed. A decomposed run is bit-identical to a one-rank run.
"""

from __future__ import annotations

import ctypes
import math
from typing import Callable, Optional

import torch

from .. import ops
from ..parallel.collectives import all_reduce_max, gather_slabs
from ..parallel.dist import DistContext
from ..parallel.fault import FaultInjected, fault_hook as _fault_hook  # noqa: F401 (re-export)
from ..parallel.halo import HaloExchange
from ..parallel.slab import Slab


class SlabJacobi:
    """Jacobi iteration on this rank's row slab. Laplace by default:
    u <- ((up + down) + (left + right)) / 4. With a right-hand side
    (``set_rhs``: b = h^2 f for -Laplace(u) = f) it solves the Poisson problem:
    u <- (((up + down) + (left + right)) + b) / 4, whose fixed point satisfies
    4 u - (sum of the neighbours) = b. The right-hand side is local to each
    rank (never exchanged); a solver that never sets one launches exactly the
    Laplace sweeps.

    ``accel="chebyshev"``: Chebyshev (Golub-Varga) acceleration. With k the
    1-based count of steps since the last (re)start and
    rho = (cos(pi / (global_rows + 1)) + cos(pi / (cols - 1))) / 2, the Jacobi
    spectral radius of the grid:

    * k = 1 is the plain sweep (``un``'s contents are ignored; nominal omega 1);
    * k = 2 uses omega = 1 / (1 - rho^2 / 2);
    * k >= 3 uses omega_k = 1 / (1 - rho^2 omega_{k-1} / 4);

    and a step k >= 2 writes p + omega (s - p), s the plain step's value and p
    the iterate before last (``ops.jacobi_sweep(omega=)``). omega is computed
    in Python floats from k and the global geometry alone, so every rank
    passes the same bits and a decomposed run stays bit-identical to a
    one-rank run. ``rho``, ``omega`` (the last one used, None before the first
    step) and ``accel_step`` (steps since the last (re)start) are attributes.
    Whatever replaces ``un``'s history restarts the sequence: ``fill``,
    ``set_boundary``, ``set_rhs``, a halo re-synchronisation after a host
    write (``_halos_valid = False``), a checkpoint without history, or
    ``restart_acceleration()``. The residual keeps its meaning, max|s - u|."""

    def __init__(self, ctx: DistContext, global_rows: int, cols: int, dtype=torch.float64, check_every: int = 10,
                 overlap: bool | str = "auto", halo: str = "auto", accel: Optional[str] = None):
        if cols < 3:
            raise ValueError("need at least 3 columns")
        if accel not in (None, "chebyshev"):
            raise ValueError(f"unknown acceleration {accel!r} (None or 'chebyshev')")
        self.accel = accel
        self.rho: Optional[float] = None
        if accel is not None:
            self.rho = 0.5 * (math.cos(math.pi / (global_rows + 1)) + math.cos(math.pi / (cols - 1)))
        self.omega: Optional[float] = None
        self.accel_step = 0
        self._un_is_history = False  # load_checkpoint restored the previous iterate into un
        self.ctx = ctx
        self.cols = cols
        self.dtype = dtype
        self.check_every = max(1, int(check_every))
        # "auto": in order with the native RCCL tier (a cross-queue join costs
        # ~10 us on MI355X, more than the 1-row halo transfer it would hide;
        # profiles/comm_step.md), overlapped on torch.distributed
        self.overlap = (ctx.native is None) if overlap == "auto" else bool(overlap)
        self.slab = Slab(global_rows, ctx.world, ctx.rank, halo_up=1, halo_down=1)
        self.halo = HaloExchange(self.slab, ctx)
        shape = (self.slab.buffer_rows, cols)
        dev = ctx.device
        if halo not in ("auto", "peer", "rccl", "none"):
            raise ValueError(f"unknown halo transport {halo!r}")
        # "none": benchmarking ablation only — ranks sweep their slabs with no
        # halo exchange at all (wrong answer, same per-rank work): the
        # difference to "peer" is the cost of the device-side ordering and the
        # xGMI halo reads
        self.no_halo = halo == "none"
        if self.no_halo:
            self.overlap = False
        self.peer = None
        if halo not in ("rccl", "none") and ctx.is_distributed and dev.type == "cuda":
            # only a small mailbox per rank is IPC-shared (its iteration word and
            # two parity slots of its edge rows: parallel.peer.Mailbox), so the
            # u / u_new slabs may be any size
            from ..parallel.peer import try_jacobi_peer

            self.u = torch.zeros(shape, dtype=dtype, device=dev)
            self.un = torch.zeros(shape, dtype=dtype, device=dev)
            es = self.u.element_size()
            nv = 16 // es
            layout_ok = cols % nv == 0 and self.u.data_ptr() % 16 == 0 and self.un.data_ptr() % 16 == 0
            self.peer = try_jacobi_peer(ctx, self.slab, [self.u, self.un], layout_ok)
            if self.peer is None and halo == "peer":
                raise RuntimeError("peer halo transport unavailable (IPC mapping failed or cols not a multiple of "
                                   f"{nv})")
        else:
            if halo == "peer" and ctx.is_distributed:
                raise RuntimeError("peer halos need GPU ranks (IPC-mapped device memory)")
            self.u = torch.zeros(shape, dtype=dtype, device=dev)
            self.un = torch.zeros(shape, dtype=dtype, device=dev)
        self.resid = torch.zeros(1, dtype=dtype, device=dev)
        self.rhs: Optional[torch.Tensor] = None  # (buffer_rows, cols) once set_rhs has run
        self.iteration = 0
        self.last_residual: Optional[float] = None
        self._halos_valid = False  # u's halo rows hold the neighbours' current rows
        self._graphs: dict = {}  # (u pointer at cycle start, check_every) -> StepGraph of one cycle

    # ------------------------------------------------------------------ setup
    def set_boundary(self, top: float = 1.0, bottom: float = 0.0, left: float = 0.0, right: float = 0.0) -> None:
        for t in (self.u, self.un):
            t[:, 0] = left
            t[:, -1] = right
            if not self.slab.has_up:
                t[0, :] = top
            if not self.slab.has_down:
                t[-1, :] = bottom
        self.restart_acceleration()

    def fill(self, fn: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None, seed: int = 0) -> None:
        """Interior initial values: fn(global_row_index, col_index) or seeded noise."""
        self._quiesce()
        s = self.slab
        rows = torch.arange(s.row0, s.row0 + s.rows, device=self.u.device).unsqueeze(1)
        cols = torch.arange(1, self.cols - 1, device=self.u.device).unsqueeze(0)
        if fn is None:
            g = torch.Generator(device="cpu").manual_seed(seed + 7919 * self.ctx.rank)
            vals = torch.rand((s.rows, self.cols - 2), generator=g, dtype=torch.float64).to(self.u.device)
        else:
            vals = fn(rows, cols)
        self.u[1:1 + s.rows, 1:-1] = vals.to(self.dtype)
        self.un.copy_(self.u)
        self._halos_valid = False

    def set_rhs(self, fn: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None,
                tensor: Optional[torch.Tensor] = None) -> None:
        """Right-hand side b = h^2 f of -Laplace(u) = f on this rank's rows:
        ``fn(global_row_index, col_index)`` with ``fill``'s conventions (interior
        columns), or ``tensor``, this rank's owned rows as (rows, cols). The
        buffer has u's shape; its halo rows and boundary columns are never
        read for a result. The cached cycle graphs hold the Laplace launches
        (or none), so they are dropped."""
        if (fn is None) == (tensor is None):
            raise ValueError("set_rhs takes exactly one of fn and tensor")
        s = self.slab
        if tensor is not None and tuple(tensor.shape) != (s.rows, self.cols):
            raise ValueError(f"rhs tensor must hold this rank's owned rows, shape {(s.rows, self.cols)}")
        self._quiesce()
        self._graphs.clear()
        self.restart_acceleration()
        if self.rhs is None:
            self.rhs = torch.zeros((s.buffer_rows, self.cols), dtype=self.dtype, device=self.u.device)
        if tensor is not None:
            self.rhs[1:1 + s.rows] = tensor.to(self.u.device, self.dtype)
        else:
            rows = torch.arange(s.row0, s.row0 + s.rows, device=self.u.device).unsqueeze(1)
            cols = torch.arange(1, self.cols - 1, device=self.u.device).unsqueeze(0)
            vals = torch.as_tensor(fn(rows, cols), device=self.u.device)
            self.rhs[1:1 + s.rows, 1:-1] = vals.to(self.dtype)

    @property
    def transport(self) -> Optional[str]:
        if not self.ctx.is_distributed:
            return None
        if self.no_halo:
            return "none (ablation: no halo exchange)"
        if self.peer is not None:
            return "xgmi-peer-signalled"
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
        rows and columns are never swept). That loses the previous iterate, so
        the Chebyshev sequence restarts, unless load_checkpoint has just put
        the previous iterate there: then only the halo rows are refreshed."""
        if self._un_is_history:
            self.un[0].copy_(self.u[0])
            self.un[-1].copy_(self.u[-1])
            self._un_is_history = False
            return
        self.un.copy_(self.u)
        self.restart_acceleration()

    def _quiesce(self) -> None:
        """Peer mode, before any host write to the IPC-shared buffers: every
        rank's queued sweeps have finished (a neighbour's last untracked sweep
        may still be reading our edge rows or waiting on our iteration word)."""
        if self.peer is not None:
            torch.cuda.synchronize(self.u.device)
            self.ctx.barrier()

    def sync_halos(self) -> None:
        """Exchange u's slab-edge rows (needed once after (re)initialisation;
        afterwards every step refreshes the halos of the rows it computes).
        Peer mode: publish the buffers and reset every rank's iteration word.
        The captured cycle graphs hold the previous descriptor (the neighbours'
        buffer parity) by value, so they are dropped here."""
        if self.peer is not None or self.no_halo:
            if self.peer is not None:
                self._quiesce()
                self._graphs.clear()
            self._reset_un()
            if self.peer is not None:
                self.peer.publish(self.u, self.iteration)
            self._halos_valid = True
            return
        self.halo.exchange(self.u)
        self._reset_un()
        self._halos_valid = True

    def check_peer(self) -> None:
        """Raise when a device-side halo wait gave up (a neighbour stalled)."""
        if self.peer is not None and self.peer.timed_out():
            raise RuntimeError(f"rank {self.ctx.rank}: peer halo wait timed out at iteration ~{self.iteration}")

    @property
    def owned(self) -> torch.Tensor:
        return self.u[1:1 + self.slab.rows]

    # ------------------------------------------------------------------ stepping
    def _sweep(self, r0: int, r1: int, track: bool, omega: Optional[float] = None) -> None:
        if r1 <= r0:
            return
        if self.u.is_cuda:
            ops.jacobi_sweep(self.u, self.un, r0, r1, self.resid if track else None, rhs=self.rhs, omega=omega)
        else:
            r = ops.jacobi_sweep(self.u, self.un, r0, r1, rhs=self.rhs, omega=omega)
            if track:
                self.resid.fill_(max(float(self.resid.item()), r))

    def step(self) -> Optional[float]:
        corrupt = _fault_hook(self.ctx.rank, self.iteration)
        if not self._halos_valid:
            self.sync_halos()
        if corrupt:  # injected silent error: one value off by one.
            # Host-exchanged halos (RCCL / gloo): the received halo row itself — a
            # cross-rank halo error. Peer mailboxes: the neighbour reads
            # this rank's edge row from the mailbox slot the previous sweep wrote,
            # which the host cannot change without racing that read, so the error
            # goes into this rank's first owned row instead: it is wrong here at
            # once and reaches the upper neighbour one sweep later, through the
            # mailbox row this sweep writes (the update spreads it to the adjacent
            # columns). Either way the N-rank == one-device check must fail.
            row = 1 if self.peer is not None else 0 if self.slab.has_up else self.slab.rows + 1
            self.u[row, self.cols // 2] += 1.0
        track = (self.iteration + 1) % self.check_every == 0
        self._advance(track)
        if track:
            self.last_residual = float(self.resid.item())
            self.check_peer()
            return self.last_residual
        return None

    def _advance(self, track: bool) -> None:
        """One iteration's device work (sweeps, halo exchange, swap and, when
        tracking, the residual all-reduce) with no host synchronisation, so it
        can be captured into a HIP graph."""
        s = self.slab
        n = s.rows
        if track:
            self.resid.zero_()
        w = self._next_omega()  # None: the plain sweeps, exactly as without accel
        if self.peer is not None:
            from .. import _native

            if w is not None:  # p is local too: same descriptor, same counters
                _native.check(_native.lib().mpx_jacobi_peer_sweep_accel(
                    int(self.dtype == torch.float64), self.u.data_ptr(),
                    None if self.rhs is None else self.rhs.data_ptr(), self.un.data_ptr(), self.cols, self.cols, n, w,
                    self.resid.data_ptr() if track else None, ctypes.byref(self.peer.desc),
                    _native.stream_of(self.u)))
            elif self.rhs is not None:  # b is local: same descriptor, same counters
                _native.check(_native.lib().mpx_jacobi_peer_sweep_rhs(
                    int(self.dtype == torch.float64), self.u.data_ptr(), self.rhs.data_ptr(), self.un.data_ptr(),
                    self.cols, self.cols, n, self.resid.data_ptr() if track else None,
                    ctypes.byref(self.peer.desc), _native.stream_of(self.u)))
            else:
                _native.check(_native.lib().mpx_jacobi_peer_sweep(
                    int(self.dtype == torch.float64), self.u.data_ptr(), self.un.data_ptr(), self.cols, self.cols, n,
                    self.resid.data_ptr() if track else None, ctypes.byref(self.peer.desc),
                    _native.stream_of(self.u)))
        elif self.ctx.is_distributed and self.overlap:
            edge = [1] if n == 1 else [1, n]
            for r in edge:
                self._sweep(r, r + 1, track, w)
            self.halo.start(self.un)      # RCCL waits for the edge rows only
            self._sweep(2, n, track, w)   # interior overlaps the transfer (same omega)
            self.halo.wait()
        else:
            self._sweep(1, n + 1, track, w)
            if not self.no_halo:
                self.halo.exchange(self.un)
        self.u, self.un = self.un, self.u
        self.iteration += 1
        if self.accel is not None:
            self.omega = 1.0 if w is None else w
            self.accel_step += 1
        if track:
            all_reduce_max(self.resid, self.ctx)

    def run(self, iters: int, tol: Optional[float] = None, graph: bool = False) -> int:
        """``iters`` iterations (fewer once the residual drops below ``tol``).

        ``graph=True`` (GPU): the iterations run as replays of one HIP graph of
        a whole residual cycle — check_every iterations, doubled to an even
        count so u/un are back in place at the end of every replay — with the
        host reading the residual once per replay. Launch-bound sweeps (small
        slabs, many ranks) no longer wait on the host's per-launch cost.
        Falls back to eager steps when the step cannot be captured.

        With ``accel`` the steps always run eagerly: omega is a by-value kernel
        argument that changes every iteration, so a replayed cycle would carry
        stale values. ``graph=True`` is accepted and captures nothing."""
        done = 0
        if graph and self.u.is_cuda and self.accel is None:
            done = self._run_graph(iters, tol)
            if done < 0:  # tolerance reached inside the graphed part
                return self.iteration
        for _ in range(iters - done):
            r = self.step()
            if tol is not None and r is not None and r < tol:
                break
        return self.iteration

    def _cycle_graph(self):
        """The HIP graph of one residual cycle (check_every iterations) starting
        from the current u/un roles; with an odd check_every the roles
        alternate between cycles, so two graphs exist. Captured once, reused
        by every later run() (capture + instantiate cost milliseconds)."""
        from ..utils.graphs import try_step_graph

        key = (self.u.data_ptr(), self.check_every)
        if key in self._graphs:
            return self._graphs[key]
        state = (self.u, self.un, self.iteration)
        it = [0]

        def body():  # the last iteration of the cycle tracks the residual, as in step()
            it[0] += 1
            self._advance(it[0] == self.check_every)

        g = try_step_graph(body, self.check_every, self.u.device, warmup=0)
        self.u, self.un, self.iteration = state  # the capture recorded the cycle, it did not run it
        self._graphs[key] = g
        return g

    def _run_graph(self, iters: int, tol: Optional[float]) -> int:
        if not self._halos_valid:
            self.sync_halos()
        # align to a cycle boundary eagerly, so every replay starts a cycle
        done = 0
        while self.iteration % self.check_every and done < iters:
            r = self.step()
            done += 1
            if tol is not None and r is not None and r < tol:
                return -1
        while iters - done >= self.check_every:
            g = self._cycle_graph()
            if g is None:
                return done
            _fault_hook(self.ctx.rank, self.iteration)
            g.replay()
            if self.check_every % 2:
                self.u, self.un = self.un, self.u
            self.iteration += self.check_every
            done += self.check_every
            self.last_residual = float(self.resid.item())
            self.check_peer()
            if tol is not None and self.last_residual < tol:
                return -1
        return done

    # ------------------------------------------------------------------ I/O
    def gather(self) -> Optional[torch.Tensor]:
        return gather_slabs(self.owned.contiguous(), self.slab, self.ctx)

    def save_checkpoint(self, prefix: str) -> str:
        """One file per rank: owned rows (+ halos), iteration, residual and,
        when one is set, the right-hand side. An accelerated solver also stores
        the previous iterate (``u_prev``) and ``accel`` = {step, omega, rho}, so
        a resumed run continues the Chebyshev sequence bit for bit."""
        path = f"{prefix}.rank{self.ctx.rank}.pt"
        ck = {"u": self.u.cpu(), "iteration": self.iteration, "residual": self.last_residual,
              "global_rows": self.slab.global_rows, "world": self.ctx.world, "cols": self.cols}
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

    def close(self) -> None:
        """Collective in peer mode: unmap the neighbours' mailboxes and free this
        rank's once no rank can still be reading it."""
        if self.peer is not None:
            self.peer.close(collective=True)
            self.peer = None

    def load_checkpoint(self, prefix: str) -> None:
        ck = torch.load(f"{prefix}.rank{self.ctx.rank}.pt", weights_only=True)
        if (ck["global_rows"], ck["world"], ck["cols"]) != (self.slab.global_rows, self.ctx.world, self.cols):
            raise ValueError("checkpoint geometry does not match this solver")
        self._quiesce()
        self._graphs.clear()
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
            # sync_halos must not clobber the previous iterate in un's owned rows
            self.un.copy_(ck["u_prev"].to(self.u.device, self.dtype))
            self.accel_step = int(ck["accel"]["step"])
            self.omega = float(ck["accel"]["omega"])
            self._un_is_history = True
