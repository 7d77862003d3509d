#!/usr/bin/env python3
"""Dense fp64 Householder QR on one MI355X (ops.qr_factor_): the time of the
factorisation, its phases, the W = V^T C and C -= V Z kernels alone against
their flop counts beside the LU's update, the application of Q^T, least
squares, and torch.geqrf, torch.ormqr and this package's LU (ops.lu_factor_, at
the same n) in the same session.

  python tools/bench_qr.py [--shapes 1024x1024,...,65536x256] [--reps 5] [--no-phases]

The matrix is standard normal.

factor_ms / torch_ms / lu_ms: device events around one call on a fresh copy of
the matrix (the copy is outside the events), alternating, median over --reps
after one warm-up call each; lu_ms is ops.lu_factor_ on the leading n x n
block. ``gflops`` is 2 n^2 (m - n / 3) over factor_ms; ``launches`` is the
number of kernels one factorisation queues.

phases_ms: the factorisation run phase by phase through mpx_qr_phase_f64 with
device events around every phase of every panel, summed per phase: ``panel``
(one launch per column), ``w`` (V^T C and V^T V on the MFMA), ``tz`` (T and
Z = T^T W), ``apply`` (C -= V Z on the MFMA). The events add their own
overhead. ``phases_match_factor`` compares the results bit for bit.

kernels: the first panel step's W and apply launches alone, median device time
and rate: W is 2 (m)(64)(n - 64 + 64) flops (the V^T V tile included), apply
2 (m)(64)(n - 64); ``lu_update`` is the LU's update on the same trailing
matrix (mpx_lu_phase_f64, phase 3; square shapes only), 2 (n - 64)^2 64 flops.

apply_qt / lstsq: ops.qr_mul_q_(transpose=True) on 64 right-hand sides against
torch.ormqr, and ops.lstsq on 1 right-hand side against torch.linalg.lstsq.

Prints one JSON line per shape.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_mpi_openmp_amd import _native, ops  # noqa: E402

NB = 64  # qr.hip's panel width


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


def launches(m, n):
    total = 1
    for j0 in range(0, n, NB):
        jb = min(NB, n - j0)
        total += sum(1 for j in range(jb + 1) if m - (j0 + j) > 0)
        if n - j0 - jb > 0:
            total += 4
    return total


def phase_times(a0, dev):
    L = _native.lib()
    m, n = a0.shape
    a = a0.clone()
    tau = torch.empty(n, dtype=torch.float64, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = int(L.mpx_qr_workspace_bytes(m, n, 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    names = ("panel", "w", "tz", "apply")
    events = {k: [] for k in names}
    for j0 in range(0, n, NB):
        for ph, name in enumerate(names):
            if ph and n - j0 <= NB:
                continue  # nothing right of the last panel
            events[name].append(event_ms(lambda: _native.check(L.mpx_qr_phase_f64(
                a.data_ptr(), m, n, n, tau.data_ptr(), info.data_ptr(), j0, ph, ws.data_ptr(), nbytes, stream))))
    torch.cuda.synchronize(dev)
    return {k: round(sum(x.elapsed_time(y) for x, y in v), 3) for k, v in events.items()}, a, tau


def kernels_alone(a0, reps, dev):
    """The W and apply launches of the first panel step on their own (the values do not matter for the time)."""
    L = _native.lib()
    m, n = a0.shape
    a = a0.clone()
    a[:, :NB] *= 1e-3  # keep the repeated C -= V Z bounded
    tau = torch.zeros(n, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = int(L.mpx_qr_workspace_bytes(m, n, 0))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        pairs = [event_ms(fn) for _ in range(max(reps, 5))]
        torch.cuda.synchronize(dev)
        return statistics.median(x.elapsed_time(y) for x, y in pairs) * 1e3

    def phase(ph):
        return lambda: _native.check(L.mpx_qr_phase_f64(a.data_ptr(), m, n, n, tau.data_ptr(), info.data_ptr(), 0, ph,
                                                        ws.data_ptr(), nbytes, stream))

    out = {}
    us = timed(phase(1))
    out["w"] = {"us": round(us, 1), "TFps": round(2.0 * m * NB * n / (us * 1e-6) / 1e12, 2)}
    phase(2)()
    us = timed(phase(3))
    out["apply"] = {"us": round(us, 1), "TFps": round(2.0 * m * NB * (n - NB) / (us * 1e-6) / 1e12, 2)}
    if m == n and n - NB > 256 and int(L.mpx_lu_panel_width()) == NB:
        piv = torch.arange(n, dtype=torch.int32, device=dev)
        lbytes = int(L.mpx_lu_workspace_bytes(n))
        lws = torch.zeros(lbytes, dtype=torch.uint8, device=dev)
        us = timed(lambda: _native.check(L.mpx_lu_phase_f64(a.data_ptr(), n, n, piv.data_ptr(), info.data_ptr(), 0, 3,
                                                            lws.data_ptr(), lbytes, stream)))
        out["lu_update"] = {"us": round(us, 1), "TFps": round(2.0 * (n - NB) ** 2 * NB / (us * 1e-6) / 1e12, 2)}
    return out


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="1024x1024,2048x2048,4096x4096,8192x8192,65536x256,16384x1024")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--no-phases", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_qr: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    for m, n in (tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")):
        g = torch.Generator(device=dev).manual_seed(m + n)
        a0 = torch.randn((m, n), generator=g, dtype=torch.float64, device=dev)
        work = a0.clone()
        sq = a0[:n].clone()
        res = alternate([("factor_ms", lambda: ops.qr_factor_(work)),
                         ("torch_ms", lambda: torch.geqrf(work)),
                         ("lu_ms", lambda: ops.lu_factor_(sq))],
                        lambda: (work.copy_(a0), sq.copy_(a0[:n])), a.reps, dev)
        flops = 2.0 * n * n * (m - n / 3.0)
        out = {"metric": "dense fp64 Householder QR factorisation time on one MI355X", "m": m, "n": n, "nb": NB,
               "reps": a.reps, "value": res["factor_ms"], "unit": "ms", "higher_is_better": False, **res,
               "gflops": round(flops / (res["factor_ms"] * 1e-3) / 1e9, 1),
               "torch_gflops": round(flops / (res["torch_ms"] * 1e-3) / 1e9, 1),
               "torch_over_ours": round(res["torch_ms"] / res["factor_ms"], 3),
               "lu_over_ours": round(res["lu_ms"] / res["factor_ms"], 3),
               "launches": launches(m, n)}
        qr, tau, info = ops.qr_factor(a0)
        out["info"] = int(info.item())
        tq, ttau = torch.geqrf(a0)
        r, tr = torch.triu(qr[:n]), torch.triu(tq[:n])
        out["r_diff_vs_torch"] = float((r - tr).abs().max() / tr.abs().max())
        b0 = torch.randn((m, 64), generator=g, dtype=torch.float64, device=dev)
        b = b0.clone()
        ap = alternate([("ours_ms", lambda: ops.qr_mul_q_(qr, tau, b, transpose=True)),
                        ("torch_ms", lambda: torch.ormqr(tq, ttau, b, left=True, transpose=True))],
                       lambda: b.copy_(b0), a.reps, dev)
        ap["torch_over_ours"] = round(ap["torch_ms"] / ap["ours_ms"], 3)
        out["apply_qt_nrhs64"] = ap
        b1 = b0[:, :1].contiguous()
        ls = alternate([("ours_ms", lambda: ops.lstsq(a0, b1)),
                        ("torch_ms", lambda: torch.linalg.lstsq(a0, b1))], lambda: None, a.reps, dev)
        ls["torch_over_ours"] = round(ls["torch_ms"] / ls["ours_ms"], 3)
        out["lstsq_nrhs1"] = ls
        del tq, b, b0
        if not a.no_phases and n > NB:
            ph, fa, ftau = phase_times(a0, dev)
            out["phases_ms"] = ph
            out["phases_sum_ms"] = round(sum(ph.values()), 3)
            out["phases_match_factor"] = bool(torch.equal(fa, qr) and torch.equal(ftau, tau))
            out["kernels"] = kernels_alone(a0, a.reps, dev)
            del fa
        print(json.dumps(out), flush=True)
        del a0, work, sq, qr
    return 0


if __name__ == "__main__":
    sys.exit(main())
