#!/usr/bin/env python3
"""Dense fp64 LU with partial pivoting on one MI355X (ops.lu_factor_): the time
of the factorisation, its phases, the trailing-update kernel alone against its
byte and flop counts, and torch.linalg.lu_factor on the same matrices in the
same session.

  python tools/bench_lu.py [--sizes 1024,2048,4096,8192] [--reps 5] [--no-phases] [--no-torch]

factor_ms / torch_ms: device events around one call on a fresh copy of the same
standard-normal matrix (the copy is outside the events), the two alternating,
median over --reps after one warm-up call each. ``gflops`` is (2/3) n^3 over
factor_ms.

phases_ms: the factorisation run phase by phase through mpx_lu_phase_f64 with
device events around every phase of every panel, summed per phase: ``panel``
(one launch per panel column), ``laswp`` (the interchanges outside the panel),
``trsm`` (U12), ``update`` (the MFMA kernel), and ``tail`` (the last <= 256
rows: one workgroup; their interchanges left of the block are left out, so
``phases_match_factor`` compares U and the pivots). The events add their own
overhead: ``phases_sum_ms`` is larger than factor_ms.

update: the first panel step's update, C ((n - nb) x (n - nb)) -= A B with
K = nb, alone: median device time, the bytes it must move (C read and written,
A and B read once: 8 (2 M N + (M + N) K)) and its 2 M N K flops. Below
n = 4096 C fits the 256 MiB Infinity Cache, so only the largest sizes measure
HBM.

MPX_LU_NB=16|32 in the environment narrows the panel (default 64); ``nb``
reports the width in use. Prints one JSON line per size.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_mpi_openmp_amd import _native, ops  # noqa: E402

TAIL_ROWS = 256  # lu.hip's kTailRows


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def phase_times(a0, nb, dev):
    L = _native.lib()
    n = a0.shape[0]
    a = a0.clone()
    piv = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = int(L.mpx_lu_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    names = ("panel", "laswp", "trsm", "update")
    events = {k: [] for k in names + ("tail",)}
    j0 = 0
    while n - j0 > TAIL_ROWS:
        for ph, name in enumerate(names):
            events[name].append(event_ms(lambda: _native.check(L.mpx_lu_phase_f64(
                a.data_ptr(), n, n, piv.data_ptr(), info.data_ptr(), j0, ph, ws.data_ptr(), nbytes, stream))))
        j0 += nb

    def tail():
        sub = a[j0:, j0:]
        _, p, _ = ops.lu_factor_(sub)
        piv[j0:] = p + j0

    events["tail"].append(event_ms(tail))
    torch.cuda.synchronize(dev)
    out = {k: round(sum(x.elapsed_time(y) for x, y in v), 3) for k, v in events.items()}
    return out, a, piv


def update_alone(a0, nb, reps, dev):
    """The update of the first panel step on its own (the operands' values do not matter for the time)."""
    L = _native.lib()
    n = a0.shape[0]
    a = a0.clone()
    piv = torch.zeros(n, dtype=torch.int32, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = int(L.mpx_lu_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    a[:nb] *= 1e-3  # keep the repeated C -= A B bounded

    def run():
        _native.check(L.mpx_lu_phase_f64(a.data_ptr(), n, n, piv.data_ptr(), info.data_ptr(), 0, 3, ws.data_ptr(),
                                         nbytes, stream))

    run()
    torch.cuda.synchronize(dev)
    pairs = [event_ms(run) for _ in range(max(reps, 5))]
    torch.cuda.synchronize(dev)
    us = statistics.median(x.elapsed_time(y) for x, y in pairs) * 1e3
    m = n - nb
    nbyte = 8 * (2 * m * m + 2 * m * nb)
    flop = 2 * m * m * nb
    return {"us": round(us, 1), "bytes": nbyte, "TBps": round(nbyte / (us * 1e-6) / 1e12, 3),
            "TFps": round(flop / (us * 1e-6) / 1e12, 2)}


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="1024,2048,4096,8192")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--no-phases", action="store_true")
    p.add_argument("--no-torch", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        print("bench_lu: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    nb = int(_native.lib().mpx_lu_panel_width())
    for n in (int(s) for s in a.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        a0 = torch.randn((n, n), generator=g, dtype=torch.float64, device=dev)
        work = a0.clone()

        def ours():
            ops.lu_factor_(work)

        def theirs():
            torch.linalg.lu_factor(work)

        runs = [("factor_ms", ours)] + ([] if a.no_torch else [("torch_ms", theirs)])
        times = {k: [] for k, _ in runs}
        for i in range(a.reps + 1):  # the first round warms both
            for k, fn in runs:
                work.copy_(a0)
                pair = event_ms(fn)
                torch.cuda.synchronize(dev)
                if i:
                    times[k].append(pair[0].elapsed_time(pair[1]))
        res = {k: round(statistics.median(v), 3) for k, v in times.items()}
        out = {"metric": "dense fp64 LU factorisation time on one MI355X", "n": n, "nb": nb, "reps": a.reps,
               "value": res["factor_ms"], "unit": "ms", "higher_is_better": False, **res,
               "gflops": round(2.0 / 3.0 * n ** 3 / (res["factor_ms"] * 1e-3) / 1e9, 1)}
        if not a.no_torch:
            out["torch_over_ours"] = round(res["torch_ms"] / res["factor_ms"], 3)
            # the same matrix, the two factorisations: the residual of each, relative to |A|
            lu, piv, _ = ops.lu_factor(a0)
            perm, low, up = ops.lu_unpack(lu, piv)
            out["residual_ours"] = float((a0[perm] - low @ up).abs().max() / a0.abs().max())
            tl, tp = torch.linalg.lu_factor(a0)
            pm, l2, u2 = torch.lu_unpack(tl, tp)
            out["residual_torch"] = float((a0 - pm @ l2 @ u2).abs().max() / a0.abs().max())
            del lu, low, up, tl, pm, l2, u2
        if not a.no_phases and n > TAIL_ROWS:
            ph, fa, fp = phase_times(a0, nb, dev)
            out["phases_ms"] = ph
            out["phases_sum_ms"] = round(sum(ph.values()), 3)
            lu, piv, _ = ops.lu_factor(a0)
            out["phases_match_factor"] = bool(torch.equal(torch.triu(fa), torch.triu(lu)) and torch.equal(fp, piv))
            out["update"] = update_alone(a0, nb, a.reps, dev)
            del fa, lu
        print(json.dumps(out), flush=True)
        del a0, work
    return 0


if __name__ == "__main__":
    sys.exit(main())
