#!/usr/bin/env python3
"""Chebyshev-accelerated Jacobi sweeps at n^2 against the plain sweeps of the
same library, timed through raw ctypes:

  python tools/experiments/jbench_accel.py LIBMPX_SO [n] [out.json]

Variants, interleaved in every round: laplace (2 words per point), rhs (3, the
baseline of the accelerated Laplace sweep, which also moves 3), accel (3) and
rhs_accel (4; baseline rhs x 4/3). Method of jbench_rhs.py: two rotated buffer
sets, 7 interleaved rounds of 6 launches after two warm-up launches, medians
with the min-max spread; with the residual the timed window includes the memset
of the residual word. Before timing, the production accelerated entries must
equal the tuning entry at R = 8 bit for bit, and 4096 rows are compared with
the plain torch expression on the device. The accelerated sweeps update un in
place (un <- un + omega (s - un), omega = 1.7: a contraction, the values stay
bounded over the repeats)."""
import ctypes
import json
import os
import statistics
import sys

import torch

OMEGA = 1.7


def main() -> None:
    lib_path = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
    L = ctypes.CDLL(lib_path, mode=ctypes.RTLD_GLOBAL)
    T = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(lib_path)), "libmpx_tune.so"), mode=ctypes.RTLD_GLOBAL)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for nm in ("mpx_jacobi_f64", "mpx_jacobi_f32"):
        getattr(L, nm).argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
    for nm in ("mpx_jacobi_rhs_f64", "mpx_jacobi_rhs_f32"):
        getattr(L, nm).argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, vp]
    for nm in ("mpx_jacobi_accel_f64", "mpx_jacobi_accel_f32"):
        getattr(L, nm).argtypes = [vp, vp, vp, ci, ci, ci, ci, cd, vp, vp]
    T.mpx_jacobi_accel_variant.argtypes = [vp, vp, vp, ci, ci, ci, ci, cd, vp, ci, ci, vp]
    dev = torch.device("cuda:0")
    out = []

    def chk(rc):
        assert rc == 0, rc

    for dt in (torch.float64, torch.float32):
        f64 = dt == torch.float64
        sets = []
        for k in range(2):
            g = torch.Generator(device=dev).manual_seed(k)
            u = torch.rand((n + 2, n), dtype=dt, device=dev, generator=g)
            b = (torch.rand((n + 2, n), dtype=dt, device=dev, generator=g) * 2 - 1) * 2.0 ** -10
            sets.append((u, b, torch.rand((n + 2, n), dtype=dt, device=dev, generator=g)))
        res = torch.zeros(1, dtype=dt, device=dev)
        lap = L.mpx_jacobi_f64 if f64 else L.mpx_jacobi_f32
        rhs = L.mpx_jacobi_rhs_f64 if f64 else L.mpx_jacobi_rhs_f32
        acc = L.mpx_jacobi_accel_f64 if f64 else L.mpx_jacobi_accel_f32
        var = {
            "laplace": lambda s, r: chk(lap(s[0].data_ptr(), s[2].data_ptr(), n, n, 1, n + 1, r, None)),
            "rhs": lambda s, r: chk(rhs(s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), n, n, 1, n + 1, r, None)),
            "accel": lambda s, r: chk(acc(s[0].data_ptr(), None, s[2].data_ptr(), n, n, 1, n + 1, OMEGA, r, None)),
            "rhs_accel": lambda s, r: chk(acc(s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), n, n, 1, n + 1, OMEGA,
                                              r, None)),
        }
        # correctness first: production == tuning entry at R = 8 == torch, on set 0
        u0, b0, p0 = sets[0]
        keep = p0.clone()
        w = torch.tensor(OMEGA, dtype=dt, device=dev)
        m = min(n, 4096)
        for with_b in (False, True):
            bp = b0.data_ptr() if with_b else None
            p0.copy_(keep)
            chk(acc(u0.data_ptr(), bp, p0.data_ptr(), n, n, 1, n + 1, OMEGA, None, None))
            prod = p0.clone()
            p0.copy_(keep)
            chk(T.mpx_jacobi_accel_variant(u0.data_ptr(), bp, p0.data_ptr(), n, n, 1, n + 1, OMEGA, None, int(f64), 8,
                                           None))
            torch.cuda.synchronize()
            assert torch.equal(prod, p0), "production and tuning entry differ"
            s = (u0[0:m, 1:-1] + u0[2:m + 2, 1:-1]) + (u0[1:m + 1, :-2] + u0[1:m + 1, 2:])
            if with_b:
                s = s + b0[1:m + 1, 1:-1]
            s = s * 0.25
            pk = keep[1:m + 1, 1:-1]
            assert torch.equal(prod[1:m + 1, 1:-1], pk + w * (s - pk)), "differs from the torch expression"
            assert torch.equal(prod[0], keep[0]) and torch.equal(prod[n + 1], keep[n + 1])
            del prod, s, pk
        p0.copy_(keep)
        del keep
        times = {}
        s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 6
        for _ in range(7):
            for name, fn in var.items():
                for with_res in (False, True):
                    r = res.data_ptr() if with_res else None
                    fn(sets[0], r)
                    fn(sets[1], r)
                    s_ev.record()
                    for i in range(reps):
                        if with_res:
                            res.zero_()
                        fn(sets[i & 1], r)
                    e_ev.record()
                    e_ev.synchronize()
                    times.setdefault((name, with_res), []).append(s_ev.elapsed_time(e_ev) * 1e3 / reps)
        es = 8 if f64 else 4
        words = {"laplace": 2, "rhs": 3, "accel": 3, "rhs_accel": 4}
        for (name, with_res), ts in times.items():
            us = statistics.median(ts)
            rec = {"dtype": "fp64" if f64 else "fp32", "variant": name, "residual": with_res,
                   "us_median": round(us, 1), "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                   "TBps": round(words[name] * n * n * es / us / 1e6, 3)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del sets
        torch.cuda.empty_cache()
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
