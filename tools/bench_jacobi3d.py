#!/usr/bin/env python3
"""3-D Jacobi (7-point stencil) on a Z x Y x X box, plane-slab decomposed over N
ranks (strong scaling), residual all-reduce every --check-every iterations.
Halos: two-sided exchange of the slab-edge planes (--halo rccl; native RCCL
tier when available) or none (ablation, wrong answer).

  python tools/bench_jacobi3d.py [--size 512 | --dims Z Y X] [--fp32] [--rhs] [--accel]
  python tools/bench_jacobi3d.py --gpus 8      (launches the 8 ranks itself)
  MPX_DIST_BACKEND=gloo python tools/bench_jacobi3d.py --device cpu --gpus 2 --size 12

Prints one JSON line on rank 0 (max time over ranks): ms per sweep, points/s
and the effective TB/s at 2 + rhs + accel words per point. With N > 1 ranks
the final field is gathered and compared bit for bit with ONE device running
the same warmup + iters iterations from the same initial field ("verified"); a
mismatch exits 3.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_mpi_openmp_amd.parallel.timing import aligned_start, clock_ns, gather_span, start_delay  # noqa: E402
from cuda_mpi_openmp_amd import parallel  # noqa: E402
from cuda_mpi_openmp_amd.models import SlabJacobi3D  # noqa: E402


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=512, help="a cube: Z = Y = X")
    p.add_argument("--dims", type=int, nargs=3, metavar=("Z", "Y", "X"), default=None)
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--check-every", type=int, default=10)
    p.add_argument("--fp32", action="store_true")
    p.add_argument("--halo", choices=["rccl", "none"], default="rccl",
                   help="none = ablation without any halo exchange (wrong answer; isolates the exchange cost)")
    p.add_argument("--device", default="auto", choices=["auto", "cuda", "cpu"])
    p.add_argument("--rhs", action="store_true", help="Poisson sweep with a seeded right-hand side (off: Laplace)")
    p.add_argument("--accel", action="store_true", help="Chebyshev acceleration (off: plain Jacobi)")
    p.add_argument("--no-verify", action="store_true", help="skip the N-rank == one-device comparison")
    p.add_argument("--gpus", type=int, default=None,
                   help="ranks to run (self-launched when no torchrun environment); default WORLD_SIZE or 1")
    a = p.parse_args()
    from cuda_mpi_openmp_amd.parallel import launch

    if a.gpus is not None:
        rc = launch.relaunch_if_needed(os.path.abspath(__file__), sys.argv[1:], a.gpus, a.device)
        if rc is not None:
            return rc
    ctx = parallel.init(device=a.device)
    if a.gpus is not None:
        launch.check_world(a.gpus, ctx.world)
    dt = torch.float32 if a.fp32 else torch.float64
    nz, ny, nx = a.dims if a.dims else (a.size, a.size, a.size)
    accel = "chebyshev" if a.accel else None
    sol = SlabJacobi3D(ctx, nz, ny, nx, dtype=dt, check_every=a.check_every, halo=a.halo, accel=accel)
    sol.set_boundary(z0=1.0)
    sol.fill(seed=0)
    if a.rhs:
        sol.set_rhs(tensor=rhs_planes(ctx.rank, sol.slab.rows, ny, nx))
    sync = (lambda: torch.cuda.synchronize(ctx.device)) if ctx.device.type == "cuda" else (lambda: None)
    sol.run(a.warmup)
    sync()
    ctx.barrier()
    aligned_start(ctx)  # every rank leaves at one agreed instant of the shared clock
    start_delay(ctx.rank)
    t0 = clock_ns()
    sol.run(a.iters)
    sync()
    t1 = clock_ns()
    ctx.barrier()
    span = gather_span(t0, t1, ctx)  # collective: every rank
    verified = None
    if ctx.world > 1 and not a.no_verify and a.halo != "none":  # the ablation is wrong by design
        got = sol.gather()
        if ctx.rank == 0:
            verified = one_device_equal(got, (nz, ny, nx), a, dt, ctx)
        verified = parallel.broadcast_object(verified, ctx)
    if ctx.rank == 0:
        ms = span.job_s * 1e3 / a.iters
        es = 4 if a.fp32 else 8
        pts = nz * ny * nx
        words = 2 + bool(a.rhs) + bool(a.accel)
        print(json.dumps({
            "metric": "3-D Jacobi sweep time, box plane-slab decomposed over N ranks",
            "value": round(ms, 5), "unit": "ms/sweep", "higher_is_better": False, "scaling": "strong",
            "n_gpus": ctx.world, "iters": a.iters, "warmup": a.warmup, "dims": [nz, ny, nx],
            "dtype": "fp32" if a.fp32 else "fp64", "check_every": a.check_every,
            "gpoints_per_s": round(pts / (ms * 1e-3) / 1e9, 3),
            "rhs": bool(a.rhs), "accel": accel, "words_per_point": words,
            "TBps_effective": round(words * pts * es / (ms * 1e-3) / 1e12, 6),
            "residual": sol.last_residual,
            "transport": sol.transport,
            "halo": ("overlap" if sol.overlap else "inorder") if ctx.world > 1 else None,
            **span.fields(a.iters),
            "verified": verified,
            "verified_what": "gathered N-rank field == one-device run of the same iterations (bit-exact)"
            if verified is not None else None}), flush=True)
    parallel.shutdown()
    return 3 if verified is False else 0


def rhs_planes(rank: int, planes: int, ny: int, nx: int) -> torch.Tensor:
    """Rank `rank`'s planes of the seeded source term, b in [-2^-10, 2^-10)."""
    g = torch.Generator(device="cpu").manual_seed(104729 + 7919 * rank)
    return (torch.rand((planes, ny, nx), generator=g, dtype=torch.float64) * 2.0 - 1.0) * 2.0 ** -10


def one_device_equal(got, dims, a, dt, ctx) -> bool:
    """Rank 0: rebuild every rank's initial field (SlabJacobi3D.fill(seed=0)
    draws rank r's planes from seed 7919 * r), run warmup + iters iterations on
    this device alone, compare with the gathered N-rank field."""
    from cuda_mpi_openmp_amd.parallel.slab import Slab

    nz, ny, nx = dims
    ref = SlabJacobi3D(parallel.DistContext(device=ctx.device), nz, ny, nx, dtype=dt, check_every=a.check_every,
                       accel="chebyshev" if a.accel else None)
    ref.set_boundary(z0=1.0)
    parts = []
    for r in range(ctx.world):
        sr = Slab(nz, ctx.world, r, 1, 1)
        g = torch.Generator(device="cpu").manual_seed(0 + 7919 * r)
        parts.append(torch.rand((sr.rows, ny - 2, nx - 2), generator=g, dtype=torch.float64))
    ref.fill(fn=lambda z, y, x: torch.cat(parts))
    if a.rhs:
        ref.set_rhs(tensor=torch.cat([rhs_planes(r, Slab(nz, ctx.world, r, 1, 1).rows, ny, nx)
                                      for r in range(ctx.world)]))
    ref.run(a.warmup + a.iters)
    same = bool(torch.equal(got.to(ref.u.device), ref.owned))
    del ref
    return same


if __name__ == "__main__":
    sys.exit(main())
