#!/usr/bin/env python3
"""Dense fp64 Cholesky on one MI355X (ops.cholesky_factor_): the time of the
factorisation, its phases, the symmetric update kernel alone against its byte
and flop counts, the solve, and torch.linalg.cholesky, torch.cholesky_solve and
this package's LU (ops.lu_factor_) on the same matrix in the same session.

  python tools/bench_cholesky.py [--sizes 1024,2048,4096,8192] [--reps 5] [--no-phases]

The matrix is G G^T + n I with G standard normal.

factor_ms / torch_ms / lu_ms: device events around one call on a fresh copy of
the matrix (the copy is outside the events), the three alternating, median over
--reps after one warm-up call each. ``gflops`` is n^3 / 3 over factor_ms;
``launches`` is the number of kernels one factorisation queues.

phases_ms: the factorisation run phase by phase through mpx_chol_phase_f64 with
device events around every phase of every panel, summed per phase: ``diag``
(one workgroup), ``panel`` (L21 by substitution), ``update`` (the MFMA kernel).
The events add their own overhead, and the one-call factorisation factors every
diagonal block but the first inside the update before it, beside the other
tiles: ``phases_sum_ms`` is larger than factor_ms.
``phases_match_factor`` compares the lower triangles bit for bit.

update: the first panel step's update, the lower triangle of C (M x M,
M = n - 64) -= L21 L21^T with K = 64, alone: median device time, the bytes it
must move (the lower triangle of C read and written, the panel read once:
8 (M (M + 1) + M K)) and its M (M + 1) K flops. Below n = 4096 C fits the
256 MiB Infinity Cache, so only the largest sizes measure HBM.

solve: ops.cholesky_solve_ and torch.cholesky_solve with 1 and 64 right-hand
sides, fresh copies of B outside the events, alternating, median.

Prints one JSON line per size.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_mpi_openmp_amd import _native, ops  # noqa: E402

NB = 64  # chol.hip's panel width


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def alternate(runs, reset, reps, dev):
    """median ms of every (name, fn) of ``runs``, alternating, ``reset`` before each and outside the events"""
    times = {k: [] for k, _ in runs}
    for i in range(reps + 1):  # the first round warms all
        for k, fn in runs:
            reset()
            pair = event_ms(fn)
            torch.cuda.synchronize(dev)
            if i:
                times[k].append(pair[0].elapsed_time(pair[1]))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def phase_times(a0, dev):
    L = _native.lib()
    n = a0.shape[0]
    a = a0.clone()
    info = torch.empty(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    names = ("diag", "panel", "update")
    events = {k: [] for k in names}
    for j0 in range(0, n, NB):
        for ph, name in enumerate(names):
            if ph and n - j0 <= NB:
                continue  # nothing below the last block
            events[name].append(event_ms(lambda: _native.check(L.mpx_chol_phase_f64(
                a.data_ptr(), n, n, info.data_ptr(), j0, ph, stream))))
    torch.cuda.synchronize(dev)
    out = {k: round(sum(x.elapsed_time(y) for x, y in v), 3) for k, v in events.items()}
    return out, a, sum(len(v) for v in events.values())


def update_alone(a0, reps, dev):
    """The update of the first panel step on its own (the operands' values do not matter for the time)."""
    L = _native.lib()
    n = a0.shape[0]
    a = a0.clone()
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    a[:, :NB] *= 1e-3  # keep the repeated C -= L21 L21^T bounded

    def run():
        _native.check(L.mpx_chol_phase_f64(a.data_ptr(), n, n, info.data_ptr(), 0, 2, stream))

    run()
    torch.cuda.synchronize(dev)
    pairs = [event_ms(run) for _ in range(max(reps, 5))]
    torch.cuda.synchronize(dev)
    us = statistics.median(x.elapsed_time(y) for x, y in pairs) * 1e3
    m = n - NB
    nbyte = 8 * (m * (m + 1) + m * NB)
    flop = m * (m + 1) * NB
    return {"us": round(us, 1), "bytes": nbyte, "TBps": round(nbyte / (us * 1e-6) / 1e12, 3),
            "TFps": round(flop / (us * 1e-6) / 1e12, 2)}


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="1024,2048,4096,8192")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--no-phases", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_cholesky: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    for n in (int(s) for s in a.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        a0 = torch.randn((n, n), generator=g, dtype=torch.float64, device=dev)
        a0 = a0 @ a0.T
        a0.diagonal().add_(float(n))
        work = a0.clone()
        res = alternate([("factor_ms", lambda: ops.cholesky_factor_(work)),
                         ("torch_ms", lambda: torch.linalg.cholesky(work)),
                         ("lu_ms", lambda: ops.lu_factor_(work))], lambda: work.copy_(a0), a.reps, dev)
        panels = (n + NB - 1) // NB
        out = {"metric": "dense fp64 Cholesky factorisation time on one MI355X", "n": n, "nb": NB, "reps": a.reps,
               "value": res["factor_ms"], "unit": "ms", "higher_is_better": False, **res,
               "gflops": round(n ** 3 / 3.0 / (res["factor_ms"] * 1e-3) / 1e9, 1),
               "torch_over_ours": round(res["torch_ms"] / res["factor_ms"], 3),
               "lu_over_ours": round(res["lu_ms"] / res["factor_ms"], 3),
               "launches": 2 * (panels - 1) + 1}
        # the same matrix, the two factorisations: the residual of each on the lower triangle, relative to |A|
        l, info = ops.cholesky_factor(a0)
        out["info"] = int(info.item())
        low = torch.tril(l)
        out["residual_ours"] = float(torch.tril(a0 - low @ low.T).abs().max() / a0.abs().max())
        tl = torch.linalg.cholesky(a0)
        out["residual_torch"] = float(torch.tril(a0 - tl @ tl.T).abs().max() / a0.abs().max())
        del low
        solve = {}
        for nrhs in (1, 64):
            b0 = torch.randn((n, nrhs), generator=g, dtype=torch.float64, device=dev)
            b = b0.clone()
            r = alternate([("ours_ms", lambda: ops.cholesky_solve_(l, b)),
                           ("torch_ms", lambda: torch.cholesky_solve(b, tl))], lambda: b.copy_(b0), a.reps, dev)
            r["torch_over_ours"] = round(r["torch_ms"] / r["ours_ms"], 3)
            solve[f"nrhs{nrhs}"] = r
        out["solve"] = solve
        del tl
        if not a.no_phases and n > NB:
            ph, fa, count = phase_times(a0, dev)
            out["phases_ms"] = ph
            out["phases_sum_ms"] = round(sum(ph.values()), 3)
            out["phase_launches"] = count
            out["phases_match_factor"] = bool(torch.equal(torch.tril(fa), torch.tril(l)))
            out["update"] = update_alone(a0, a.reps, dev)
            del fa
        print(json.dumps(out), flush=True)
        del a0, work, l
    return 0


if __name__ == "__main__":
    sys.exit(main())
