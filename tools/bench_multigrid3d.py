#!/usr/bin/env python3
"""Geometric multigrid V-cycle for the 3-D Poisson problem on one MI355X
(models.PoissonMultigrid3D): the time of one V(2,2) cycle, the per-kernel times
at level 0, the solve to a tolerance, and the Chebyshev-accelerated
SlabJacobi3D solve of the same problem in the same session.

  python tools/bench_multigrid3d.py [--planes 255] [--ny 257] [--nx 257] [--fp32]
                                    [--tol 1e-8] [--reps 20] [--no-solve] [--no-kernels]
                                    [--tail-points N] [--tail-table] [--fmg]

Per-kernel times: device events around single launches, median over --reps
launches that rotate through buffer sets larger than the 256 MiB Infinity
Cache together, so no launch finds its input cached. The rates count the words
the algorithm needs per fine point: relax 3, residual 3, restrict 1 + 1/8,
prolong-add 2 + 1/8, prolong_cubic 1 + 1/8. ``rhs_sweep_even`` is ops.jacobi3d_sweep(rhs=) on the
contiguous (planes + 1, ny - 1, nx - 1) grid, whose even width takes the
wave-strip kernel: the yardstick for ``relax``. ``below_level2_share`` is the
time of the sub-cycle from level 2 down over the whole cycle. ``walk`` is
ops.mg3_walk() (MPX_MG3_WALK="rows,restrict_planes,prolong_planes,min_waves"
replaces it for A/B runs); ``cubic_walk`` is ops.mg3_cubic_walk()
(MPX_MG3_CUBIC_WALK="planes").

``--tail-points N``: the levels of at most N points run as one kernel (0: every
level launched; default: the model's measured threshold); the JSON line carries
``tail_points``, ``tail_level`` and ``launches_per_cycle``. ``--tail-table``: per
level, the sub-cycle from that level down, launched and fused (``tail_table``).

``--fmg``: full multigrid (``fmg()``, two cycles per level, and ``fmg(1)``) on
the manufactured problem u = sin(3x + 0.4) e^y cos(2z), b = 12 h^2 u, next to
``solve(tol)`` from a zero interior and ``cycle()`` in the same process (key
``fmg``): times, rho = max|u_fmg - u_h| / max|u_h - u| with u_h the fp64 model
cycled 30 times, the error against u, and the launches of one ``fmg()``.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_mpi_openmp_amd import ops, parallel  # noqa: E402
from cuda_mpi_openmp_amd.models import PoissonMultigrid3D, SlabJacobi3D  # noqa: E402

MALL_BYTES = 256 << 20


def problem_rhs(planes: int, ny: int, nx: int) -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(11)
    return (torch.rand((planes, ny, nx), generator=g, dtype=torch.float64) * 2.0 - 1.0) * 0.01


def setup(sol, rhs):
    sol.set_boundary(z0=1.0)
    sol.fill(seed=3)
    sol.set_rhs(tensor=rhs)


def median_us(launch, nsets: int, reps: int, dev) -> float:
    """Median device time of launch(k), k rotating through the buffer sets."""
    for k in range(nsets):  # warm every set: code objects, page tables
        launch(k)
    torch.cuda.synchronize(dev)
    pairs = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(i % nsets)
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize(dev)
    return statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3


def kernel_times(planes, ny, nx, dt, reps, dev):
    d, h, w = planes + 2, ny, nx
    es = 4 if dt == torch.float32 else 8
    shapes = PoissonMultigrid3D.level_shapes(planes, ny, nx, 2)
    nsets = max(2, -(-2 * MALL_BYTES // (d * h * w * es)))
    sets = [PoissonMultigrid3D(planes, ny, nx, dtype=dt, device=dev, max_levels=2) for _ in range(nsets)]
    for s in sets:  # the times do not depend on the values
        for lv in s._lv:
            for t in (lv.u, lv.b, lv.r):
                if t is not None:
                    t.uniform_(-1.0, 1.0)
    out, pts = {}, (d - 2) * (h - 2) * (w - 2)
    f = [s._lv[0] for s in sets]
    out["relax"] = (median_us(lambda k: ops.jacobi3d_relax(f[k].u, f[k].un, 1, d - 1, 6.0 / 7.0, rhs=f[k].b), nsets, reps,
                              dev), 3)
    r = [lv.r if lv.r is not None else lv.un for lv in f]  # a single level keeps no r: any grid serves as output
    out["residual"] = (median_us(lambda k: ops.mg3_residual(f[k].u, r[k], rhs=f[k].b), nsets, reps, dev), 3)
    if len(shapes) == 2:
        c = [s._lv[1] for s in sets]
        out["restrict"] = (median_us(lambda k: ops.mg3_restrict(f[k].r, c[k].b), nsets, reps, dev), 1.125)
        out["prolong_add"] = (median_us(lambda k: ops.mg3_prolong_add_(c[k].u, f[k].u), nsets, reps, dev), 2.125)
        if min(shapes[1]) >= 3:
            out["prolong_cubic"] = (median_us(lambda k: ops.mg3_prolong_cubic(c[k].u, f[k].u), nsets, reps, dev), 1.125)
    del sets, f
    de, he, we = d - 1, h - 1, w - 1  # the even box next to it: the wave-strip kernel
    ev = [[torch.rand((de, he, we), dtype=dt, device=dev) for _ in range(3)] for _ in range(nsets)]
    out["rhs_sweep_even"] = (median_us(lambda k: ops.jacobi3d_sweep(ev[k][0], ev[k][1], 1, de - 1, rhs=ev[k][2]), nsets,
                                       reps, dev), 3)
    res = {}
    for name, (us, words) in out.items():
        n = (de - 2) * (he - 2) * (we - 2) if name == "rhs_sweep_even" else pts
        res[name] = {"us": round(us, 2), "TBps": round(words * n * es / (us * 1e-6) / 1e12, 3)}
    return res


def tail_table(planes, ny, nx, dt, reps, max_points, dev):
    """Per level k >= 1 of at most ``max_points`` points: the median time of the
    sub-cycle from level k down, launched (``tail_points=0``) and as one kernel
    (the tail starting at k), each between two device synchronisations."""
    def sub_cycle_us(m, k):
        ts = []
        for i in range(reps + 3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            m._vcycle(k)
            torch.cuda.synchronize(dev)
            if i >= 3:
                ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e6

    launched = PoissonMultigrid3D(planes, ny, nx, dtype=dt, device=dev, tail_points=0)
    rows_out = []
    for k in range(1, len(launched.levels)):
        points = 1
        for n in launched.levels[k]:
            points *= n
        if points > max_points:
            continue
        fused = PoissonMultigrid3D(planes, ny, nx, dtype=dt, device=dev, tail_points=points)
        assert fused.tail_level == k
        for m in (launched, fused):
            setup(m, problem_rhs(planes, ny, nx))
            m.cycle()
        a, b = sub_cycle_us(launched, k), sub_cycle_us(fused, k)
        rows_out.append({"level": k, "shape": list(launched.levels[k]), "points": points, "launched_us": round(a, 1),
                         "fused_us": round(b, 1), "launches": launched.launches_per_cycle - fused.launches_per_cycle + 1})
        del fused
    return rows_out


def manufactured(planes, ny, nx):
    """u = sin(3x + 0.4) e^y cos(2z) on the grid of spacing h = 1 / (nx - 1), and h: -Laplace(u) = 12 u."""
    h = 1.0 / (nx - 1)
    z = torch.arange(planes + 2, dtype=torch.float64).view(-1, 1, 1) * h
    y = torch.arange(ny, dtype=torch.float64).view(1, -1, 1) * h
    x = torch.arange(nx, dtype=torch.float64).view(1, 1, -1) * h
    return torch.sin(3.0 * x + 0.4) * torch.exp(y) * torch.cos(2.0 * z), h


def fmg_launches(m, cpl):
    """Launches of one fmg(cpl), counted as ``launches_per_cycle`` counts: a
    fill or a copy is one launch, the zeroing of the residual word none."""
    n, tail = len(m.levels), m.tail_level

    def cycle_from(k):
        if tail is not None and k >= tail:
            return 1
        bottom = 1 if tail is not None else (1 if m.levels[-1] == (3, 3, 3) else m.coarse_sweeps)
        if k == n - 1:
            return bottom if n > 1 else m.nu1 + m.nu2
        launched = (n - 1 if tail is None else tail) - k
        return launched * (m.nu1 + m.nu2 + 4) + bottom

    total = (n - 1) + 2 + 5 * (n - 1) + 1  # restrictions of b, the injected faces, the coarsest interior
    total += cpl * cycle_from(n - 1)
    for k in range(n - 1):
        total += 3 + cpl * cycle_from(k)  # the prolongation and the two fills of the coarser un
    return total


def fmg_report(planes, ny, nx, dt, reps, tol, tail_points, dev):
    exact, h = manufactured(planes, ny, nx)
    exact = exact.to(dev)
    rhs = (12.0 * h * h * exact)[1:-1]

    def problem(dtype):
        m = PoissonMultigrid3D(planes, ny, nx, dtype=dtype, device=dev, tail_points=tail_points)
        m.set_rhs(tensor=rhs)
        m.u.copy_(exact)
        m.u[1:-1, 1:-1, 1:-1] = 0.0
        m._lv[0].un.copy_(m.u)
        return m

    def timed(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e3

    def err(m, ref):
        return float((m.u.to(torch.float64) - ref).abs().max())

    out = {}
    m = problem(dt)
    for _ in range(2):
        m.fmg()
    out["fmg_ms"] = round(timed(m.fmg, reps), 4)
    ufmg = m.u.to(torch.float64).clone()
    out["fmg_residual"] = m.last_residual
    out["fmg_error"] = err(m, exact)
    out["fmg_launches"] = fmg_launches(m, 2)
    m.fmg(1)
    out["fmg1_ms"] = round(timed(lambda: m.fmg(1), reps), 4)
    ufmg1 = m.u.to(torch.float64).clone()
    out["fmg1_error"] = err(m, exact)
    out["fmg1_launches"] = fmg_launches(m, 1)
    out["cycle_ms"] = round(timed(m.cycle, reps), 4)
    out["launches_per_cycle"] = m.launches_per_cycle
    del m
    # solve(tol) from a zero interior: the second solve, on kernels and buffers already warm
    for k in range(2):
        s = problem(dt)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        n = s.solve(tol)
        torch.cuda.synchronize(dev)
        out.update({"solve_ms": round((time.perf_counter() - t0) * 1e3, 3), "solve_cycles": n,
                    "solve_residual": s.last_residual, "solve_error": err(s, exact)})
        del s
    # the discrete solution in fp64, whatever the dtype timed
    d = problem(torch.float64)
    for _ in range(30):
        d.cycle()
    disc = err(d, exact)
    out.update({"discretisation_error": disc, "uh_residual": d.last_residual,
                "rho": round(float((ufmg - d.u).abs().max()) / disc, 4),
                "rho1": round(float((ufmg1 - d.u).abs().max()) / disc, 4)})
    out["fmg_over_cycle"] = round(out["fmg_ms"] / out["cycle_ms"], 3)
    return out


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--planes", type=int, default=255)
    p.add_argument("--ny", type=int, default=257)
    p.add_argument("--nx", type=int, default=257)
    p.add_argument("--fp32", action="store_true")
    p.add_argument("--tol", type=float, default=1e-8)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--no-solve", action="store_true", help="skip the solves (multigrid and Chebyshev Jacobi)")
    p.add_argument("--no-kernels", action="store_true", help="skip the per-kernel times")
    p.add_argument("--tail-points", type=int, default=None,
                   help="levels of at most this many points run as one kernel (0: none; default: the model's)")
    p.add_argument("--tail-table", action="store_true",
                   help="time the sub-cycle from every level of at most --tail-table-max points down, launched and fused")
    p.add_argument("--tail-table-max", type=int, default=274625)
    p.add_argument("--no-cycle", action="store_true", help="skip the cycle time")
    p.add_argument("--fmg", action="store_true",
                   help="full multigrid on the manufactured problem next to solve(tol) and cycle() (key fmg)")
    p.add_argument("--max-jacobi-iters", type=int, default=100000)
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_multigrid3d: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    dt = torch.float32 if a.fp32 else torch.float64
    planes, ny, nx = a.planes, a.ny, a.nx
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731

    kern = None if a.no_kernels else kernel_times(planes, ny, nx, dt, a.reps, dev)
    levels = PoissonMultigrid3D.level_shapes(planes, ny, nx)
    rhs = None if (a.no_cycle and a.no_solve) else problem_rhs(planes, ny, nx)

    plan = {"tail_points": a.tail_points, "tail_level": None, "launches_per_cycle": None}  # filled in from a model
    cycle_ms, share = None, None
    if not a.no_cycle:
        # one V-cycle: host clock around cycle() (it ends in the residual read)
        mg = PoissonMultigrid3D(planes, ny, nx, dtype=dt, device=dev, tail_points=a.tail_points)
        setup(mg, rhs)
        for _ in range(3):
            mg.cycle()
        sync()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            mg.cycle()
            ts.append(time.perf_counter() - t0)
        cycle_ms = statistics.median(ts) * 1e3
        if len(mg.levels) > 2 and (mg.tail_level is None or mg.tail_level >= 2):
            ts = []
            for _ in range(a.reps):
                sync()
                t0 = time.perf_counter()
                mg._vcycle(2)
                sync()
                ts.append(time.perf_counter() - t0)
            share = statistics.median(ts) * 1e3 / cycle_ms
        plan = {"tail_points": mg.tail_points, "tail_level": mg.tail_level, "launches_per_cycle": mg.launches_per_cycle}
        del mg

    table = tail_table(planes, ny, nx, dt, a.reps, a.tail_table_max, dev) if a.tail_table else None

    solve = {}
    if not a.no_solve:
        s = PoissonMultigrid3D(planes, ny, nx, dtype=dt, device=dev, tail_points=a.tail_points)
        setup(s, rhs)
        plan = {"tail_points": s.tail_points, "tail_level": s.tail_level, "launches_per_cycle": s.launches_per_cycle}
        sync()
        t0 = time.perf_counter()
        n = s.solve(a.tol)
        sync()
        solve = {"solve_ms": round((time.perf_counter() - t0) * 1e3, 3), "cycles": n, "residual": s.last_residual}
        j = SlabJacobi3D(parallel.DistContext(device=dev), planes, ny, nx, dtype=dt, check_every=100, accel="chebyshev")
        setup(j, rhs)
        j.run(200)  # warm
        setup(j, rhs)
        j.iteration = 0
        sync()
        t0 = time.perf_counter()
        j.run(a.max_jacobi_iters, tol=a.tol)
        sync()
        solve.update({"jacobi_solve_ms": round((time.perf_counter() - t0) * 1e3, 3), "jacobi_iterations": j.iteration,
                      "jacobi_residual": j.last_residual})
        solve["jacobi_over_multigrid"] = round(solve["jacobi_solve_ms"] / solve["solve_ms"], 2)
        solve["max_abs_difference"] = float((s.u - j.u).abs().max())

    fmg = fmg_report(planes, ny, nx, dt, a.reps, a.tol, a.tail_points, dev) if a.fmg else None

    print(json.dumps({
        "metric": "3-D Poisson multigrid V(2,2) cycle time on one MI355X",
        "value": None if cycle_ms is None else round(cycle_ms, 4), "unit": "ms/cycle", "higher_is_better": False,
        "grid": [planes + 2, ny, nx], "dtype": "fp32" if a.fp32 else "fp64", "levels": len(levels),
        "coarsest": list(levels[-1]), "reps": a.reps, "tol": a.tol, "walk": ops.mg3_walk(),
        "cubic_walk": ops.mg3_cubic_walk(),
        "below_level2_share": None if share is None else round(share, 3),
        **plan, "tail_table": table, "level0_kernels": kern, "fmg": fmg, **solve}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
