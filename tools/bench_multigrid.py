#!/usr/bin/env python3
"""Geometric multigrid V-cycle for the 2-D Poisson problem on one MI355X
(models.PoissonMultigrid): the time of one V(2,2) cycle, the per-kernel times at
level 0, the solve to a tolerance, and the Chebyshev-accelerated SlabJacobi
solve of the same problem in the same session.

  python tools/bench_multigrid.py [--rows 2047] [--cols 2049] [--fp32]
                                  [--tol 1e-8] [--reps 20] [--no-solve]
                                  [--tail-points N] [--tail-table] [--fmg]

Per-kernel times: device events around single launches, median over --reps
launches that rotate through buffer sets larger than the 256 MiB Infinity
Cache together, so no launch finds its input cached. The rates count the words
the algorithm needs per fine point: relax 3, residual 3, restrict 1.25,
prolong-add 2.25, prolong-cubic 1.25. ``rhs_sweep_even`` is ops.jacobi_sweep(rhs=) on the
(rows + 2, cols - 1) grid, whose even width takes the wave-strip kernel: the
gap to ``relax`` is what the odd width costs. ``below_level2_share`` is the
time of the sub-cycle from level 2 down over the whole cycle (launch-bound).

``--tail-points N``: the levels of at most N points run as one kernel (0: every
level launched; default: the model's measured threshold); the JSON line carries
``tail_points``, ``tail_level`` and ``launches_per_cycle``. ``--tail-table``: per
level, the sub-cycle from that level down, launched and fused (``tail_table``).

``--fmg``: full multigrid on the manufactured problem u = sin(3x + 0.4) e^y
(-Laplace(u) = 8 u, nonzero Dirichlet values, h = 1 / (cols - 1)), under the
key ``fmg``: the time of ``fmg()`` (median over --reps calls, host clock, each
ends in the residual read), max|u_fmg - u|, and rho = max|u_fmg - u_h| /
max|u_h - u| with u_h from 25 fp64 cycles; next to it, in the same session,
``solve(tol)`` of the same problem from a zero interior (time, cycles and its
max|u - exact|), one ``cycle()``, and ``fmg()`` of the level-1 grid alone
(``below_level0_ms``: what ``fmg()`` spends below level 0, but for one
restriction and the boundary injection).

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
from cuda_mpi_openmp_amd.models import PoissonMultigrid, SlabJacobi  # noqa: E402

MALL_BYTES = 256 << 20


def problem_rhs(rows: int, cols: int) -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(11)
    return (torch.rand((rows, cols), generator=g, dtype=torch.float64) * 2.0 - 1.0) * 0.01


def setup(sol, rows, cols):
    sol.set_boundary(top=1.0)
    sol.fill(seed=3)
    sol.set_rhs(tensor=problem_rhs(rows, cols))


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


def kernel_times(rows, cols, dt, reps, dev):
    h, w = rows + 2, cols
    es = 4 if dt == torch.float32 else 8
    shapes = PoissonMultigrid.level_shapes(rows, cols, 2)
    nsets = max(2, -(-2 * MALL_BYTES // (h * w * es)))
    sets = [PoissonMultigrid(rows, cols, dtype=dt, device=dev, max_levels=2) for _ in range(nsets)]
    for s in sets:  # the times do not depend on the values
        for lv in s._lv:
            for t in (lv.u, lv.b, lv.r):
                if t is not None:
                    t.uniform_(-1.0, 1.0)
    out, pts = {}, (h - 2) * (w - 2)
    f = [s._lv[0] for s in sets]
    out["relax"] = (median_us(lambda k: ops.jacobi_relax(f[k].u, f[k].un, 1, h - 1, 0.8, rhs=f[k].b), nsets, reps, dev), 3)
    out["residual"] = (median_us(lambda k: ops.mg_residual(f[k].u, f[k].r, rhs=f[k].b), nsets, reps, dev), 3)
    if len(shapes) == 2:
        c = [s._lv[1] for s in sets]
        out["restrict"] = (median_us(lambda k: ops.mg_restrict(f[k].r, c[k].b), nsets, reps, dev), 1.25)
        out["prolong_add"] = (median_us(lambda k: ops.mg_prolong_add_(c[k].u, f[k].u), nsets, reps, dev), 2.25)
        out["prolong_cubic"] = (median_us(lambda k: ops.mg_prolong_cubic(c[k].u, f[k].u), nsets, reps, dev), 1.25)
    del sets, f
    we = w - 1  # the even width next to it: the wave-strip kernel
    ev = [[torch.rand((h, we), dtype=dt, device=dev) for _ in range(3)] for _ in range(nsets)]
    out["rhs_sweep_even"] = (median_us(lambda k: ops.jacobi_sweep(ev[k][0], ev[k][1], 1, h - 1, rhs=ev[k][2]), nsets, reps,
                                       dev), 3)
    res = {}
    for name, (us, words) in out.items():
        n = (h - 2) * (we - 2) if name == "rhs_sweep_even" else pts
        res[name] = {"us": round(us, 2), "TBps": round(words * n * es / (us * 1e-6) / 1e12, 3)}
    return res


def tail_table(rows, cols, dt, reps, max_points, dev):
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

    launched = PoissonMultigrid(rows, cols, dtype=dt, device=dev, tail_points=0)
    rows_out = []
    for k in range(1, len(launched.levels)):
        points = 1
        for n in launched.levels[k]:
            points *= n
        if points > max_points:
            continue
        fused = PoissonMultigrid(rows, cols, dtype=dt, device=dev, tail_points=points)
        assert fused.tail_level == k
        for m in (launched, fused):
            setup(m, rows, cols)
            m.cycle()
        a, b = sub_cycle_us(launched, k), sub_cycle_us(fused, k)
        rows_out.append({"level": k, "shape": list(launched.levels[k]), "points": points, "launched_us": round(a, 1),
                         "fused_us": round(b, 1), "launches": launched.launches_per_cycle - fused.launches_per_cycle + 1})
        del fused
    return rows_out


def manufactured(rows, cols):
    """u = sin(3x + 0.4) e^y on the (rows + 2, cols) grid, h = 1 / (cols - 1); and h."""
    h = 1.0 / (cols - 1)
    y = torch.arange(rows + 2, dtype=torch.float64).unsqueeze(1) * h
    x = torch.arange(cols, dtype=torch.float64).unsqueeze(0) * h
    return torch.sin(3.0 * x + 0.4) * torch.exp(y), h


def fmg_report(rows, cols, dt, reps, tol, tail_points, dev):
    def problem(r, c, dtype):
        m = PoissonMultigrid(r, c, dtype=dtype, device=dev, tail_points=tail_points)
        u, h = manufactured(r, c)
        u = u.to(dev)
        m.set_rhs(tensor=(8.0 * h * h * u)[1:-1])
        m.u.copy_(u)
        m.u[1:-1, 1:-1] = 0.0
        m._lv[0].un.copy_(m.u)
        return m, u

    def timed(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e3

    out = {}
    m, exact = problem(rows, cols, dt)
    for _ in range(3):
        m.fmg()
    out["fmg_ms"] = round(timed(m.fmg, reps), 4)
    ufmg = m.u.to(torch.float64).clone()
    out["fmg_residual"] = m.last_residual
    out["fmg_error"] = float((ufmg - exact).abs().max())
    m.fmg(2)
    out["fmg2_ms"] = round(timed(lambda: m.fmg(2), reps), 4)
    out["fmg2_error"] = float((m.u.to(torch.float64) - exact).abs().max())
    ufmg2 = m.u.to(torch.float64).clone()
    out["cycle_ms"] = round(timed(m.cycle, reps), 4)
    del m
    # solve(tol) from a zero interior: the second solve, on kernels and buffers already warm
    for k in range(2):
        s, _ = problem(rows, cols, dt)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        n = s.solve(tol)
        torch.cuda.synchronize(dev)
        out.update({"solve_ms": round((time.perf_counter() - t0) * 1e3, 3), "solve_cycles": n,
                    "solve_residual": s.last_residual, "solve_error": float((s.u.to(torch.float64) - exact).abs().max())})
        del s
    if len(PoissonMultigrid.level_shapes(rows, cols)) > 1:
        c, _ = problem((rows + 2 + 1) // 2 - 2, (cols + 1) // 2, dt)
        for _ in range(3):
            c.fmg()
        out["below_level0_ms"] = round(timed(c.fmg, reps), 4)
        del c
    # the discrete solution in fp64, whatever the dtype timed
    d, _ = problem(rows, cols, torch.float64)
    for _ in range(25):
        d.cycle()
    uh = d.u
    disc = float((uh - exact).abs().max())
    out.update({"discretisation_error": disc, "uh_residual": d.last_residual,
                "rho": round(float((ufmg - uh).abs().max()) / disc, 4),
                "rho2": round(float((ufmg2 - uh).abs().max()) / disc, 4)})
    out["fmg_over_cycle"] = round(out["fmg_ms"] / out["cycle_ms"], 3)
    return out


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=2047)
    p.add_argument("--cols", type=int, default=2049)
    p.add_argument("--fp32", action="store_true")
    p.add_argument("--tol", type=float, default=1e-8)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--no-solve", action="store_true", help="skip the solves (multigrid and Chebyshev Jacobi)")
    p.add_argument("--no-kernels", action="store_true", help="skip the per-kernel times")
    p.add_argument("--tail-points", type=int, default=None,
                   help="levels of at most this many points run as one kernel (0: none; default: the model's)")
    p.add_argument("--tail-table", action="store_true",
                   help="time the sub-cycle from every level of at most --tail-table-max points down, launched and fused")
    p.add_argument("--tail-table-max", type=int, default=263169)
    p.add_argument("--fmg", action="store_true",
                   help="full multigrid on the manufactured problem next to solve(tol) and cycle() (key fmg)")
    p.add_argument("--max-jacobi-iters", type=int, default=200000)
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_multigrid: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    dt = torch.float32 if a.fp32 else torch.float64
    rows, cols = a.rows, a.cols
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731

    kern = None if a.no_kernels else kernel_times(rows, cols, dt, a.reps, dev)

    # one V-cycle: host clock around cycle() (it ends in the residual read)
    mg = PoissonMultigrid(rows, cols, dtype=dt, device=dev, tail_points=a.tail_points)
    setup(mg, rows, cols)
    for _ in range(3):
        mg.cycle()
    sync()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        mg.cycle()
        ts.append(time.perf_counter() - t0)
    cycle_ms = statistics.median(ts) * 1e3
    share = None
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

    table = tail_table(rows, cols, dt, a.reps, a.tail_table_max, dev) if a.tail_table else None

    solve = {}
    if not a.no_solve:
        s = PoissonMultigrid(rows, cols, dtype=dt, device=dev, tail_points=a.tail_points)
        setup(s, rows, cols)
        sync()
        t0 = time.perf_counter()
        n = s.solve(a.tol)
        sync()
        solve = {"solve_ms": round((time.perf_counter() - t0) * 1e3, 3), "cycles": n, "residual": s.last_residual}
        j = SlabJacobi(parallel.DistContext(device=dev), rows, cols, dtype=dt, check_every=100, accel="chebyshev")
        setup(j, rows, cols)
        j.run(200)  # warm
        setup(j, rows, cols)
        j.iteration = 0
        sync()
        t0 = time.perf_counter()
        j.run(a.max_jacobi_iters, tol=a.tol)
        sync()
        solve.update({"jacobi_solve_ms": round((time.perf_counter() - t0) * 1e3, 3), "jacobi_iterations": j.iteration,
                      "jacobi_residual": j.last_residual})
        solve["jacobi_over_multigrid"] = round(solve["jacobi_solve_ms"] / solve["solve_ms"], 2)
        solve["max_abs_difference"] = float((s.u - j.u).abs().max())

    fmg = fmg_report(rows, cols, dt, a.reps, a.tol, a.tail_points, dev) if a.fmg else None

    print(json.dumps({
        "metric": "2-D Poisson multigrid V(2,2) cycle time on one MI355X",
        "value": round(cycle_ms, 4), "unit": "ms/cycle", "higher_is_better": False,
        "grid": [rows + 2, cols], "dtype": "fp32" if a.fp32 else "fp64", "levels": len(mg.levels),
        "coarsest": list(mg.levels[-1]), "reps": a.reps, "tol": a.tol,
        "below_level2_share": None if share is None else round(share, 3),
        **plan, "tail_table": table, "level0_kernels": kern, "fmg": fmg, **solve}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
