"""lab5 key-value sort timing on one GPU, lab5_bench.py's method (median of
event-timed runs, the input restored outside the events, every result
checked), four ways in one process:
  (a) ops.sort      stable pairs sort, AUTO: values + int32 indices, out of place
  (b) ops.argsort   the permutation only
  (c) ops.sort_     keys only: the yardstick for the payload's cost (pairs move
                    twice the bytes per pass; far above 2x points at spills or
                    lost occupancy)
  (d) torch.sort(x, stable=True) into a preallocated out=(values, int64 indices):
                    what (a) replaces
(a) and (b) include their scratch copy of the keys and their allocations from
torch's caching allocator, as a caller pays them. One JSON line per (dtype, n).
PAIRS_LOGN=20,24,26 / PAIRS_ITERS=7 / PAIRS_VARIANTS=20,21,22 narrow or widen a run
(variants: the in-place pairs sort with an iota payload through libmpx_tune)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cuda_mpi_openmp_amd import _native, ops  # noqa: E402

ITERS = int(os.environ.get("PAIRS_ITERS", "7"))


def gpu_ms(fn, src):
    """Median ms of fn(work) on a fresh copy of src; returns fn's last result."""
    work = src.clone()
    for _ in range(3):
        work.copy_(src)
        out = fn(work)
    ts = []
    for _ in range(ITERS):
        work.copy_(src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(work)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2], out, work


def variant_argsort(x, variant, idx, ws):
    dt = 0 if x.dtype == torch.int32 else 1
    _native.check(_native.tune_lib().mpx_sort_pairs_variant(x.data_ptr(), idx.data_ptr(), x.numel(), dt, 1,
                                                            ws.data_ptr(), ws.numel(), variant, _native.stream_of(x)))
    return idx


def main():
    dev = torch.device("cuda:0")
    lgs = [int(v) for v in os.environ.get("PAIRS_LOGN", "20,24,26").split(",")]
    variants = [int(v) for v in os.environ.get("PAIRS_VARIANTS", "").split(",") if v]
    for dt in (torch.int32, torch.float32):
        for lg in lgs:
            n = 1 << lg
            src = (torch.randint(-2**31, 2**31 - 1, (n,), dtype=dt, device=dev) if dt == torch.int32
                   else torch.randn(n, device=dev))
            rvals, ridx = torch.empty_like(src), torch.empty(n, dtype=torch.int64, device=dev)
            t_torch, _, _ = gpu_ms(lambda x: torch.sort(x, stable=True, out=(rvals, ridx)), src)
            ref_idx = ridx.to(torch.int32)
            t_sort, (vals, idx), _ = gpu_ms(ops.sort, src)
            # random data has no NaN / signed zero: torch's order and the total order agree
            ok = torch.equal(vals.view(torch.int32), rvals.view(torch.int32)) and torch.equal(idx, ref_idx)
            t_arg, idx2, work = gpu_ms(ops.argsort, src)
            ok = ok and torch.equal(idx2, ref_idx) and torch.equal(work, src)
            t_keys, _, work = gpu_ms(ops.sort_, src)
            ok = ok and torch.equal(work.view(torch.int32), rvals.view(torch.int32))
            rec = {"workload": "lab5_sort_pairs", "dtype": str(dt).split(".")[-1], "n": n, "iters": ITERS,
                   "sort_pairs_ms": round(t_sort, 3), "argsort_ms": round(t_arg, 3), "sort_keys_only_ms": round(t_keys, 3),
                   "torch_sort_stable_ms": round(t_torch, 3), "pairs_over_keys": round(t_sort / t_keys, 2),
                   "torch_over_pairs": round(t_torch / t_sort, 2), "verified": bool(ok)}
            if variants:
                L = _native.lib()
                ws = torch.empty(int(L.mpx_sort_pairs_workspace_bytes(n, 0)), dtype=torch.uint8, device=dev)
                vidx = torch.empty(n, dtype=torch.int32, device=dev)
                rec["inplace_argsort_variants"] = {}
                for v in variants:
                    ms, out, _ = gpu_ms(lambda x, v=v: variant_argsort(x, v, vidx, ws), src)
                    rec["inplace_argsort_variants"][str(v)] = {"ms": round(ms, 3), "ok": bool(torch.equal(out, ref_idx))}
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
