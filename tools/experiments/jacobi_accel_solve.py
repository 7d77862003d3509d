#!/usr/bin/env python3
"""Iterations and wall time to a residual (max|s - u|) below a tolerance on a
manufactured n x n Poisson problem, plain Jacobi against Chebyshev acceleration,
one device, fp64:

  python tools/experiments/jacobi_accel_solve.py [n] [tol] [plain_wall_limit_s] [out.json]

u* is seeded noise on the grid, b = 4 u* - (sum of the neighbours), the start is
u* on the boundary and 0 inside. The accelerated solver runs eager steps with
the residual checked every 100 iterations; the plain solver replays HIP graphs
of 1000-iteration cycles. The plain run stops at the wall limit when it has not
converged by then and reports the residual it reached."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cuda_mpi_openmp_amd import parallel  # noqa: E402
from cuda_mpi_openmp_amd.models import SlabJacobi  # noqa: E402


def main() -> None:
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    tol = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-8
    limit = float(sys.argv[3]) if len(sys.argv) > 3 else 120.0
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(20)
    us = torch.rand((n, n), generator=g, dtype=torch.float64).to(dev)
    b = torch.zeros_like(us)
    b[1:-1, 1:-1] = 4.0 * us[1:-1, 1:-1] - ((us[:-2, 1:-1] + us[2:, 1:-1]) + (us[1:-1, :-2] + us[1:-1, 2:]))
    out = []
    for accel, every, chunk in (("chebyshev", 100, 100), (None, 1000, 20000)):
        sol = SlabJacobi(parallel.DistContext(device=dev), n - 2, n, check_every=every, accel=accel)
        start = us.clone()
        start[1:-1, 1:-1] = 0.0
        sol.u.copy_(start)
        sol.un.copy_(sol.u)
        sol.set_rhs(tensor=b[1:-1])
        sol.run(every, graph=accel is None)  # warm-up: first launches, graph capture
        torch.cuda.synchronize()
        sol.u.copy_(start)
        sol._halos_valid = False
        sol.iteration = 0
        t0 = time.perf_counter()
        reached = False
        while not reached and time.perf_counter() - t0 < limit:
            sol.run(chunk, tol=tol, graph=accel is None)
            reached = sol.last_residual is not None and sol.last_residual < tol
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        rec = {"n": n, "tol": tol, "accel": accel, "iterations": sol.iteration, "reached": reached,
               "residual": sol.last_residual, "wall_s": round(el, 3),
               "us_per_iteration": round(el * 1e6 / max(sol.iteration, 1), 2),
               "max_error": float((sol.u - us).abs().max())}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del sol
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
