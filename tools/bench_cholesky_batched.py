#!/usr/bin/env python3
"""Batched fp64 Cholesky of small SPD matrices on one MI355X
(ops.cholesky_factor_batched_ / ops.cholesky_solve_batched_): the time of one
call against the three other ways to do the same work on the same tensors in
the same session:

  loop   the Python loop over ops.cholesky_factor_ / ops.cholesky_solve_, one
         matrix at a time (all there was before the batched kernels);
  torch  torch.linalg.cholesky / torch.cholesky_solve on the whole batch;
  lu     ops.lu_factor_batched_ / ops.lu_solve_batched_ on the same matrices.

  python tools/bench_cholesky_batched.py [--batches 64,1024,16384] [--sizes 4,8,16,32,64]
                                         [--nrhs 1,16] [--reps 7] [--loop-reps 3]
                                         [--no-loop] [--no-torch] [--no-lu]

Every figure is device time between two events around the call(s) on a fresh
copy of the same batch A = G G^T + n I, G standard normal (the copy is outside
the events), the median over --reps (--loop-reps for the loop, which takes
seconds at the largest batch) after one warm-up round. ``*_over_ours`` are
ratios of times: above 1 the batched Cholesky call is faster.
``bits_equal_cpu`` compares the lower triangles of the factors, info and the
solutions of the batched GPU call with the CPU reference of the same batch.
Prints one JSON line per (batch, n).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_mpi_openmp_amd import ops  # noqa: E402


def timed(fn, reset, reps, dev):
    """Median device ms of fn() over reps, reset() before each, after one warm-up round."""
    out = []
    for i in range(reps + 1):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        if i:
            out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="64,1024,16384")
    p.add_argument("--sizes", default="4,8,16,32,64")
    p.add_argument("--nrhs", default="1,16")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--loop-reps", type=int, default=3)
    p.add_argument("--no-loop", action="store_true")
    p.add_argument("--no-torch", action="store_true")
    p.add_argument("--no-lu", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_cholesky_batched: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    for batch in (int(s) for s in a.batches.split(",")):
        for n in (int(s) for s in a.sizes.split(",")):
            gen = torch.Generator(device=dev).manual_seed(1000 * n + batch)
            g = torch.randn((batch, n, n), generator=gen, dtype=torch.float64, device=dev)
            a0 = g @ g.transpose(1, 2) + n * torch.eye(n, dtype=torch.float64, device=dev)
            a0 = torch.tril(a0) + torch.tril(a0, -1).transpose(1, 2)
            work = a0.clone()
            out = {"metric": "batched fp64 Cholesky on one MI355X", "batch": batch, "n": n, "unit": "ms",
                   "higher_is_better": False, "reps": a.reps, "loop_reps": a.loop_reps}

            def reset():
                work.copy_(a0)

            out["factor_ms"] = timed(lambda: ops.cholesky_factor_batched_(work), reset, a.reps, dev)
            out["value"] = out["factor_ms"]
            if not a.no_loop:
                out["factor_loop_ms"] = timed(lambda: [ops.cholesky_factor_(work[m]) for m in range(batch)], reset,
                                              a.loop_reps, dev)
                out["factor_loop_over_ours"] = out["factor_loop_ms"] / out["factor_ms"]
            if not a.no_torch:
                out["factor_torch_ms"] = timed(lambda: torch.linalg.cholesky(work), reset, a.reps, dev)
                out["factor_torch_over_ours"] = out["factor_torch_ms"] / out["factor_ms"]
            if not a.no_lu:
                out["factor_lu_ms"] = timed(lambda: ops.lu_factor_batched_(work), reset, a.reps, dev)
                out["factor_lu_over_ours"] = out["factor_lu_ms"] / out["factor_ms"]
            l, info = ops.cholesky_factor_batched(a0)
            c_l, c_info = ops.cholesky_factor_batched(a0.cpu())
            equal = torch.equal(torch.tril(l).cpu(), torch.tril(c_l)) and torch.equal(info.cpu(), c_info)
            if not a.no_torch:
                t_l = torch.linalg.cholesky(a0)
            if not a.no_lu:
                lu, piv, _ = ops.lu_factor_batched(a0)
            for nrhs in (int(s) for s in a.nrhs.split(",")):
                b0 = torch.randn((batch, n, nrhs), generator=gen, dtype=torch.float64, device=dev)
                bw = b0.clone()

                def reset_b():
                    bw.copy_(b0)

                key = f"solve{nrhs}"
                out[f"{key}_ms"] = timed(lambda: ops.cholesky_solve_batched_(l, bw), reset_b, a.reps, dev)
                if not a.no_loop:
                    out[f"{key}_loop_ms"] = timed(
                        lambda: [ops.cholesky_solve_(l[m], bw[m]) for m in range(batch)], reset_b, a.loop_reps, dev)
                    out[f"{key}_loop_over_ours"] = out[f"{key}_loop_ms"] / out[f"{key}_ms"]
                if not a.no_torch:
                    out[f"{key}_torch_ms"] = timed(lambda: torch.cholesky_solve(bw, t_l), reset_b, a.reps, dev)
                    out[f"{key}_torch_over_ours"] = out[f"{key}_torch_ms"] / out[f"{key}_ms"]
                if not a.no_lu:
                    out[f"{key}_lu_ms"] = timed(lambda: ops.lu_solve_batched_(lu, piv, bw), reset_b, a.reps, dev)
                    out[f"{key}_lu_over_ours"] = out[f"{key}_lu_ms"] / out[f"{key}_ms"]
                x = ops.cholesky_solve_batched(l, b0)
                equal = equal and torch.equal(x.cpu(), ops.cholesky_solve_batched(c_l, b0.cpu()))
            out["bits_equal_cpu"] = bool(equal)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
            del a0, work, l, g
    return 0


if __name__ == "__main__":
    sys.exit(main())
