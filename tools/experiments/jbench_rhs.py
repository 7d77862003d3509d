#!/usr/bin/env python3
"""Laplace and Poisson (rhs) Jacobi sweeps at n^2, timed through raw ctypes on a
given libmpx.so, so that a build of an earlier commit (no rhs symbols: only
its Laplace sweep is timed) runs under the same script:

  python tools/experiments/jbench_rhs.py LIBMPX_SO TAG [n] [out.json]

Two rotated buffer sets (each buffer alone exceeds the 256 MB MALL at
16384^2), 7 interleaved rounds of 6 launches after two warm-up launches,
medians; with the residual the timed window includes the memset of the
residual word. The rhs forms are the production entry and the tuning entry at
R = 8 with plain (nt0) / non-temporal (nt1) loads of b (libmpx_tune.so next
to the library); they must agree bit for bit, and 4096 rows are compared
with the plain torch expression on the device. Bandwidth is analytic: 2
words per point for Laplace, 3 with an rhs."""
import ctypes
import json
import os
import statistics
import sys

import torch


def main() -> None:
    lib_path, tag = sys.argv[1], sys.argv[2]
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 16384
    L = ctypes.CDLL(lib_path, mode=ctypes.RTLD_GLOBAL)
    has_rhs = hasattr(L, "mpx_jacobi_rhs_f64")
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for nm in ("mpx_jacobi_f64", "mpx_jacobi_f32"):
        getattr(L, nm).argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
    if has_rhs:
        T = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(lib_path)), "libmpx_tune.so"),
                        mode=ctypes.RTLD_GLOBAL)
        for nm in ("mpx_jacobi_rhs_f64", "mpx_jacobi_rhs_f32"):
            getattr(L, nm).argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, vp]
        T.mpx_jacobi_rhs_variant.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, ci, ci, ci, vp]
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
            sets.append((u, b, torch.empty_like(u)))
        res = torch.zeros(1, dtype=dt, device=dev)
        lap = L.mpx_jacobi_f64 if f64 else L.mpx_jacobi_f32
        var = {"laplace": lambda s, r: chk(lap(s[0].data_ptr(), s[2].data_ptr(), n, n, 1, n + 1, r, None))}
        if has_rhs:
            rhs = L.mpx_jacobi_rhs_f64 if f64 else L.mpx_jacobi_rhs_f32
            var["rhs"] = lambda s, r: chk(rhs(s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), n, n, 1, n + 1, r,
                                              None))
            for nt in (0, 1):
                var[f"rhs_R8_nt{nt}"] = lambda s, r, nt=nt: chk(T.mpx_jacobi_rhs_variant(
                    s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), n, n, 1, n + 1, r, int(f64), 8, nt, None))
            s0, outs = sets[0], {}
            for name, fn in var.items():
                s0[2].zero_()
                fn(s0, None)
                torch.cuda.synchronize()
                outs[name] = s0[2][1:n + 1].clone()
            assert torch.equal(outs["rhs"], outs["rhs_R8_nt0"]) and torch.equal(outs["rhs"], outs["rhs_R8_nt1"])
            assert not torch.equal(outs["rhs"], outs["laplace"])
            m = min(n, 4096)
            u0, b0 = s0[0], s0[1]
            want = (((u0[0:m, 1:-1] + u0[2:m + 2, 1:-1]) + (u0[1:m + 1, :-2] + u0[1:m + 1, 2:]))
                    + b0[1:m + 1, 1:-1]) * 0.25
            assert torch.equal(outs["rhs"][0:m, 1:-1], want)
            del outs, want
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
        for (name, with_res), ts in times.items():
            words = 2 if name == "laplace" else 3
            us = statistics.median(ts)
            rec = {"lib": tag, "dtype": "fp64" if f64 else "fp32", "variant": name, "residual": with_res,
                   "us_median": round(us, 1), "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                   "TBps": round(words * n * n * es / us / 1e6, 3)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del sets
        torch.cuda.empty_cache()
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
