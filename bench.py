#!/usr/bin/env python3
"""Flagship benchmark — lab2 2-D convolution of 4096x4096 RGBA8 images.

Metric (BASELINE.json): "Gpixel/s lab2 2D conv 4096x4096 + GPU/CPU speedup, at
1/2/4/8 MI355X". Configuration: 5x5 filter (``sobel5`` gradient magnitude on
fp32 luminance) on the hand-written gfx950 wave-streaming kernel (register
windows shifted across lanes with DPP, no LDS, no barriers), synthetic random
RGBA8 data.

Scaling is WEAK by default: every rank owns one 4096x4096 row slab of a global
(4096*N) x 4096 image. ``--layout strong`` keeps ONE global 4096x4096 image
and splits it into N row slabs (4096/N rows per rank: 512 at N = 8), same
rotation, verification and job-span timing, recorded as ``scaling: "strong"``;
at N = 1 both layouts are the same run. The strong layout also gathers every
rotated slab's N-rank output and compares it with a one-device convolution of
the whole frame (``verified_one_device``). One step = read the slab's 2+2 halo rows from the
neighbouring ranks over xGMI + convolve every owned row. Halo transport
(``--halo``): ``peer`` maps the neighbours' slabs once (IPC) and the conv
kernel loads their boundary rows over xGMI on every step — one launch per
step; ``rccl`` runs a grouped RCCL send/recv first (libmpx native tier, in
order on the compute stream); ``auto`` = peer when every rank can map and
verify its neighbours, else rccl.

HBM-honest timing: the timed steps cycle over ``--rotate`` (default 6)
independent image/output slab pairs per rank — a 6 x 128 MiB working set, 3x
the 256 MB Infinity Cache (MALL) — so every step streams its image from HBM
like a stream of distinct frames would. The same K steps re-convolving one
resident input (cache-assisted; the second stream writes a twin output) are
reported as ``value_warm_cache``, and on one stream and one pair (the round-1
methodology) as ``value_warm_cache_1stream``.

``value`` is the whole-job pixel throughput N * 4096^2 * K / job span, where
the job span is max(t_end) - min(t_start) over the ranks on the node's shared
CLOCK_MONOTONIC (parallel/timing.py): start skew between ranks is charged.
``max_rank_span_ms`` (the slowest rank's own span) and the skews ride along.
``host_enqueue_ms_per_step`` (rank 0) is the host time to enqueue the timed
steps, beside the step time: it shows the GPU, not the host, sets the rate.
``config.host_wait`` names the host wait policy (``MPX_HIP_WAIT``).

``value_streaming`` (``--stream``, on by default) times the same K steps with
an input that changes every step: the filter is iterated (step k convolves
step k-1's output) over the same rotated working set, so for N > 1 every step
needs halo rows the neighbours produced in the previous step — ordered on the
device by step words the conv kernel's own slab-edge waves wait on and
publish (peer, one dispatch per step) or by in-order RCCL send/recv.
Verified after the timed region: the gathered N-rank result of every rotated
slab equals a one-device whole-image run of the same frame sequence, and each
rank's last step equals the CPU reference on its halo-filled input. Every output pixel of every rotated pair on every rank is
compared bit-exactly with the OpenMP CPU reference after the timed region
(``verified_bit_exact``); the GPU/CPU speedup compares one GPU's per-image
time with that CPU reference on the same 4096^2 image (``speedup_vs_cpu``).

A plain run does only what the headline needs: set-up, warm-up, the K timed
steps over the rotated pairs, then the result line (``metric``, ``value``,
``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step`` and the run's
configuration). Everything else described above — the sustained, steady and
cache-resident rates, the streaming phase, the clock sampler, the bit-exact
verification against the CPU reference and the CPU baselines — runs only with
``--full``.

``--dump-outputs DIR`` writes what the last timed step computed: rank r's
output slab of that step as ``DIR/out_rank<r>.npy`` (float32, rows x W x 4) —
the whole slab when it fits the 64 MB budget shared by all ranks, else a
fixed seeded choice of its rows (the slab's first and last two among them) —
and the rows' indices within the slab as ``DIR/rows_rank<r>.npy`` (float64).
The inputs are seeded, so two builds run with the same arguments can be
compared output for output.

Run:  python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
  With --gpus N > 1 and no torchrun environment, bench.py launches N ranks
  itself (torch.distributed.run, one process per GPU) before touching the GPU,
  and fails (exit 2) when fewer than N GPUs are visible. Under
  ``MPX_DIST_BACKEND=gloo`` the N ranks may share GPUs (one-GPU rehearsal).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BASELINE_METRIC = "Gpixel/s lab2 2D conv 4096x4096 + GPU/CPU speedup, at 1/2/4/8 MI355X"
# best large-bucket Roberts run on the RTX A6000, ~0.78 Mpx / 0.17866 ms
BASELINE_GPIXEL_PER_S = 4.4
BASELINE_NOTE = ("estimate: A6000 Roberts 2x2 on a ~0.78 Mpx image, one cold launch (BASELINE.md) vs MI355X "
                 "5x5 sobel5 on 4096^2 slabs, warm steps streaming from HBM; not like-for-like — the harness's "
                 "same-methodology comparison is in profiles/harness_vs_baseline.md")


def _sig(v: float) -> float:
    """Six significant digits (a tiny CPU dry run must not round to 0)."""
    return float(f"{v:.6g}")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--warmup-ms", type=float, default=0.0,
                   help="after the --warmup steps, keep running untimed steps until at least this much "
                        "back-to-back step time has elapsed; 0 (default) = exactly --warmup steps. A/B on MI355X "
                        "(profiles/lab2_conv.md, round 4): 30 ms of settling LOWERS the timed steps' rate (the "
                        "board holds a lower clock under sustained load), so the driver's W is kept as given and "
                        "the sustained rate is reported separately (value_sustained)")
    p.add_argument("--sustain-ms", type=float, default=50.0,
                   help="value_sustained: the same K rotated steps timed again after this much continuous load "
                        "(0 = skip)")
    p.add_argument("--size", type=int, default=4096,
                   help="image side: per GPU slab (weak layout) or of the one global image (strong layout)")
    p.add_argument("--steady-ms", type=float, default=300.0,
                   help="value_steady: after this much continuous load, --steady-windows windows of the same K "
                        "rotated steps, with the board's clock / power sampled over them on every rank (0 = skip)")
    p.add_argument("--steady-windows", type=int, default=5)
    p.add_argument("--layout", choices=["weak", "strong"], default="weak",
                   help="weak: a size x size slab per rank; strong: one size x size image split over the ranks")
    p.add_argument("--filter", default="sobel5")
    p.add_argument("--rotate", type=int, default=6,
                   help="independent image/output slab pairs cycled by the timed steps (working set > MALL)")
    p.add_argument("--overlap", choices=["auto", "on", "off", "pipeline"], default="auto",
                   help="halo transfer overlapped with the interior rows (on), in order before one full launch "
                        "(off), exchanged one step ahead on the comm stream with double-buffered input (pipeline; "
                        "native RCCL tier), or the measured-faster choice for the transport in use (auto)")
    p.add_argument("--halo", choices=["auto", "peer", "rccl"], default="auto",
                   help="halo transport for N > 1: one-sided xGMI loads from IPC-mapped neighbour slabs (peer), "
                        "RCCL send/recv (rccl), or peer when available (auto)")
    p.add_argument("--streams", type=int, default=2,
                   help="HIP streams the rotated static steps alternate over (pair i always on stream i %% S): "
                        "independent frames overlap one kernel's tail with the next one's start; 1 = one stream. "
                        "Only where steps are independent (one rank or static peer halos)")
    p.add_argument("--stream-streams", type=int, default=0,
                   help="HIP streams for the streaming phase's slab sequences (each sequence stays on one stream); "
                        "0 = --streams (the static phase's streams, reused: N = 1 586 -> 652-663 Gpixel/s)")
    p.add_argument("--graph", type=int, default=0,
                   help="capture this many steps into one HIP graph and replay it (0 = eager launches; "
                        "in-order and peer halo modes)")
    p.add_argument("--watchdog", type=float, default=None,
                   help="abort (exit 75) when no step completes for this many seconds; default 300 s for N > 1")
    p.add_argument("--clocks", type=float, default=0.0,
                   help="sample the board's clocks / power / temperature at this rate (Hz) on every rank's GPU and "
                        "report their medians per timed phase under clocks (utils/clocks.py; 0 = off: the sampler "
                        "thread shares the host with the enqueue loop)")
    p.add_argument("--no-warm", action="store_true", help="skip the cache-resident (single pair) comparison run")
    p.add_argument("--stream", dest="stream", action="store_true", default=True,
                   help="also time the streaming (iterated-filter) run: value_streaming (default on)")
    p.add_argument("--no-stream", dest="stream", action="store_false")
    p.add_argument("--strict-streaming", action="store_true",
                   help="exit 3 when the streaming phase failed (a device-side halo wait gave up); by default the "
                        "verified static headline is still reported, with status \"streaming_failed\"")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-verify", action="store_true")
    p.add_argument("--device", default="auto", choices=["auto", "cuda", "cpu"])
    p.add_argument("--full", action="store_true",
                   help="after the headline's timed steps also run everything else this benchmark measures and "
                        "checks: value_sustained, value_steady, value_warm_cache*, the streaming phase, --clocks, "
                        "the bit-exact verification against the CPU reference and the CPU baselines (each still "
                        "under its own option above). Without it only the headline is measured")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's output slab (or a fixed seeded choice of its rows; at most "
                        "64 MB over all ranks) as DIR/out_rank<r>.npy, float32, with the rows' indices in "
                        "DIR/rows_rank<r>.npy")
    a = p.parse_args(argv)
    if not a.full:  # a plain run: set-up, warm-up, the timed steps, the result line
        a.sustain_ms = a.steady_ms = a.clocks = 0.0
        a.stream = False
        a.no_warm = a.no_cpu_baseline = a.no_verify = True
    return a


def main() -> int:
    args = parse_args()
    from cuda_mpi_openmp_amd.parallel import launch

    rc = launch.relaunch_if_needed(os.path.abspath(__file__), sys.argv[1:], args.gpus, args.device)
    if rc is not None:
        return rc
    return run(args)


def run(args) -> int:
    import torch
    import torch.distributed as dist

    from cuda_mpi_openmp_amd import ops, parallel
    from cuda_mpi_openmp_amd.models.edge import SlabEdgeDetector
    from cuda_mpi_openmp_amd.parallel import launch
    from cuda_mpi_openmp_amd.parallel.timing import aligned_start, clock_ns, gather_span, start_delay
    from cuda_mpi_openmp_amd.utils.streams import wait_policy_in_force

    ctx = parallel.init(device=args.device)
    launch.check_world(args.gpus, ctx.world)
    n = ctx.world
    sampler = None
    phases = {}  # phase name -> this rank's (t0, t1) on CLOCK_MONOTONIC
    if args.clocks > 0 and ctx.device.type == "cuda":
        from cuda_mpi_openmp_amd.utils.clocks import ClockSampler

        sampler = ClockSampler(hz=args.clocks, bdf=device_id(ctx.device)).start()

    def sync():
        if ctx.device.type == "cuda":
            torch.cuda.synchronize(ctx.device)

    overlap = {"auto": "auto", "on": True, "off": False, "pipeline": "pipeline"}[args.overlap]
    strong = args.layout == "strong"
    global_rows = args.size if strong else args.size * n
    args.global_rows = global_rows
    dets = []
    for r in range(max(1, args.rotate)):
        d = SlabEdgeDetector(ctx, global_rows, args.size, args.filter, overlap=overlap, halo=args.halo)
        d.fill_random(seed=1234 + 7919 * r + ctx.rank)
        dets.append(d)
    sync()
    ctx.barrier()

    cyc = [0]
    nstreams = 1
    if args.streams > 1 and ctx.device.type == "cuda" and all(d.independent_steps for d in dets) and args.graph == 0:
        if len(dets) % args.streams:
            raise SystemExit(f"--streams {args.streams} must divide --rotate {len(dets)}")
        nstreams = args.streams
    streams = hip_streams(ctx.device, nstreams) if nstreams > 1 else []
    handles = [s.cuda_stream for s in streams]
    if streams:  # every stream starts after the set-up work of the current one
        for s in streams:
            s.wait_stream(torch.cuda.current_stream(ctx.device))

    def rot_step():
        i = cyc[0] % len(dets)
        if handles:
            dets[i].step(handles[i % nstreams])  # pair i always on the same stream: no cross-stream reuse
        else:
            dets[i].step()
        cyc[0] += 1

    wd_s = args.watchdog if args.watchdog is not None else (300.0 if n > 1 else 0.0)
    watchdog = parallel.Watchdog(ctx, wd_s, what="benchmark step")
    for _ in range(max(args.warmup, len(dets))):  # every pair has run (code objects, peer maps) before timing
        rot_step()
        watchdog.beat()
    for d in dets:
        d.finish()
    sync()
    ctx.barrier()
    warm_info = settle(rot_step, len(dets), args.warmup_ms, ctx, sync, watchdog, parallel,
                       lambda: [d.finish() for d in dets])

    graph = None
    d0 = dets[0]
    single_stream = not ctx.is_distributed or d0.peer is not None or not (d0.pipeline or d0.overlap)
    if args.graph > 0 and ctx.device.type == "cuda" and single_stream:
        from cuda_mpi_openmp_amd.utils.graphs import try_step_graph

        if args.graph % len(dets):
            # a graph of a partial rotation would replay only a subset of the
            # pairs and shrink the working set back into the MALL
            raise SystemExit(f"--graph {args.graph} must be a multiple of --rotate {len(dets)}")
        cyc[0] = 0
        graph = try_step_graph(rot_step, args.graph, ctx.device)
        sync()
        ctx.barrier()

    issue_s = {}  # step function -> host enqueue time of its last timed run

    def timed(step_fn, k: int):
        """Exactly k steps bracketed by barrier + device sync on both sides.
        Every rank reads the node's shared CLOCK_MONOTONIC when it leaves the
        opening barrier + sync (t0) and at its own closing device sync (t1);
        the returned Span (parallel/timing.py) gives the job's time
        max(t1) - min(t0), which charges start skew between ranks, and the
        slowest rank's own span beside it (VERDICT r4 Next #1)."""
        ctx.barrier()
        sync()
        aligned_start(ctx)  # every rank leaves at one agreed instant of the shared clock
        start_delay(ctx.rank)  # MPX_BENCH_START_DELAY test hook (no-op unless set)
        t0 = clock_ns()
        done = 0
        if graph is not None and step_fn is rot_step:  # every replay runs args.graph complete steps
            while done + args.graph <= k:
                graph.replay()
                done += args.graph
        for _ in range(k - done):
            step_fn()
        for d in dets:
            d.finish()
        issued = (clock_ns() - t0) / 1e9  # host time to enqueue the k steps
        sync()
        t1 = clock_ns()
        ctx.barrier()
        issue_s[step_fn] = issued
        phases[timed.phase] = (t0, t1)
        return gather_span(t0, t1, ctx)

    def prime_window():
        """One untimed window of the same K steps between a settle loop and
        the windows it precedes: the settle loop retires thousands of queued
        launches at once, and the first window after it measured 6-25 % slow
        in every round-6 run (with or without the clock sampler) while the
        next ones did not; the load stays continuous (profiles/lab2_conv.md)."""
        cyc[0] = 0
        timed.phase = "prime"
        timed(rot_step, args.steps)
        phases.pop("prime", None)
        watchdog.beat()

    # ---- timed region: exactly `steps` steps over the rotated pairs ----
    timed.issue_s = issue_s
    timed.phase = "timed"
    cyc[0] = 0
    span = timed(rot_step, args.steps)
    enqueue_ms = issue_s[rot_step] * 1e3 / max(1, args.steps)
    watchdog.beat()
    elapsed = span.job_s  # the job's time: first rank's start to last rank's end
    if args.dump_outputs:  # what the last timed step returned (pair (K - 1) % rotate)
        dump_outputs(args.dump_outputs, dets[(args.steps - 1) % len(dets)].out, ctx)

    # the same K steps after >= sustain_ms of continuous load (the clock the
    # board holds under sustained load): reported beside `value`, not instead
    sustained = None
    if args.sustain_ms > 0 and graph is None:
        settle(rot_step, len(dets), args.sustain_ms, ctx, sync, watchdog, parallel, lambda: [d.finish() for d in dets])
        prime_window()
        cyc[0] = 0
        timed.phase = "sustained"
        sustained = timed(rot_step, args.steps).job_s
        watchdog.beat()

    # steady state (VERDICT r5 Next #4): the same K rotated steps in several
    # windows after >= steady_ms of load, with the board's clocks and power
    # sampled over exactly those windows (a sampler of their own, started
    # after the headline phase so it cannot disturb it, in a child process so
    # its reads never hold this process's GIL)
    steady = None
    if args.steady_ms > 0 and graph is None:
        ssam = None
        if ctx.device.type == "cuda":
            from cuda_mpi_openmp_amd.utils.clocks import ProcessClockSampler

            ssam = ProcessClockSampler(hz=100, bdf=device_id(ctx.device)).start()
        settle(rot_step, len(dets), args.steady_ms, ctx, sync, watchdog, parallel, lambda: [d.finish() for d in dets])
        prime_window()
        wins = []
        for wi in range(max(1, args.steady_windows)):
            cyc[0] = 0
            timed.phase = f"steady{wi}"
            wins.append(timed(rot_step, args.steps).job_s)
            watchdog.beat()
        t_lo = min(phases[f"steady{wi}"][0] for wi in range(len(wins)))
        t_hi = max(phases[f"steady{wi}"][1] for wi in range(len(wins)))
        for wi in range(len(wins)):
            phases.pop(f"steady{wi}", None)
        mine = None
        if ssam is not None:
            from cuda_mpi_openmp_amd.utils.clocks import key_fields

            ssam.stop()
            # the windows last a few ms (K steps each): at 100 Hz they hold 0-1
            # samples, so the record spans the last 100 ms of the settle load
            # (the same rotated steps, back to back) plus the windows
            mine = key_fields(ssam.summary(t_lo - 100_000_000, t_hi, pad_ns=3_000_000))
            mine.update(source=ssam.source, error=ssam.error)
        steady = {"wins": wins, "clocks": parallel.all_gather_object(mine, ctx)}

    warm = warm1 = None
    if not args.no_warm:
        # one input re-convolved: cache-resident, so it gets the resident-input
        # load policy (plain loads; profiles/lab2_conv.md). In the timed
        # phase's regime (steps alternating over the streams) the second
        # stream's steps write a twin output slab: 64 MiB in + 2 x 64 MiB out
        # stay in the MALL. The round-1 methodology (one stream, one pair) is
        # value_warm_cache_1stream.
        d0.cache_resident(True)
        wcyc = [0]

        def warm_step():
            if wcyc[0] % 2:
                d0.step_twin(handles[1])
            else:
                d0.step(handles[0])
            wcyc[0] += 1
        if len(handles) >= 2:
            for _ in range(2):  # the twin launch is built and warmed before timing
                warm_step()
            timed.phase = "warm_cache"
            warm = timed(warm_step, args.steps).job_s
            watchdog.beat()
        timed.phase = "warm_cache_1stream"
        warm1 = timed(d0.step, args.steps).job_s
        d0.cache_resident(False)
        watchdog.beat()
        if warm is None:
            warm, warm1 = warm1, None

    ms_per_step = elapsed * 1e3 / max(1, args.steps)
    pixels = global_rows * args.size * args.steps
    value = pixels / elapsed / 1e9

    ok, checked, one_device = True, 0, None
    if not args.no_verify:
        for d in dets:
            good, cnt = verify_full(d, ops)
            ok &= good
            checked += cnt
        ok = parallel.max_over_ranks(0.0 if ok else 1.0, ctx) == 0.0
        checked = int(parallel.all_reduce_sum_host(float(checked), ctx))
        if strong:
            one_device = verify_one_device(dets, args, ctx, ops, parallel)
            ok &= one_device

    # ---- streaming: the same K steps with a real inter-rank dependency ----
    stream_rec = None
    if args.stream:
        graph = None
        timed.phase = "streaming"
        try:
            stream_rec = run_streaming(args, ctx, n, timed, watchdog, sync, ops, parallel)
        except StreamingTimeout as e:
            # every rank raises together (the check is collective): the
            # secondary streaming figure is recorded as failed; the static
            # headline stands on its own verification. Wrong pixels are not
            # caught here — they fail the run (verified_bit_exact_streaming).
            stream_rec = {"value_streaming": None, "streaming_error": str(e), "verified_bit_exact_streaming": None,
                          "transport_streaming": None}
            if ctx.rank == 0:
                print(f"[bench] streaming phase failed: {e}", file=sys.stderr)
        ok &= stream_rec.get("verified_bit_exact", True) is not False

    watchdog.stop()
    clocks = None
    if sampler is not None:
        from cuda_mpi_openmp_amd.utils.clocks import key_fields

        sampler.stop()
        # a K-step phase lasts well under one sample period: widen each window by
        # 3 ms on both sides so it holds the samples around it
        mine_clk = {ph: key_fields(sampler.summary(a, b, pad_ns=3_000_000)) for ph, (a, b) in phases.items()}
        mine_clk["sampler"] = {"source": sampler.source, "error": sampler.error, "hz": sampler.rate_hz()}
        clocks = parallel.all_gather_object(mine_clk, ctx)
    cpu_ms = None
    if ctx.rank == 0 and not args.no_cpu_baseline:
        cpu_ms = cpu_baseline_ms(d0, args.size, ops)

    seen = {"torch_distributed": dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1,
            "rccl_native": ctx.native.size() if ctx.native is not None else None}
    # which physical GPU each rank ran on (PCI domain:bus:device), so an N-GPU
    # record shows N distinct devices
    rank_devices = parallel.all_gather_object(device_id(ctx.device), ctx)
    # an N-GPU record must come from N distinct GPUs unless ranks share devices
    # on purpose (one-GPU rehearsals, CPU dry runs): ADVICE r3
    rehearsal = (ctx.device.type != "cuda" or os.environ.get("MPX_DIST_BACKEND") == "gloo"
                 or os.environ.get("MPX_DIST_CONTRACT") == "nccl")
    shared_devices = n > 1 and len(set(rank_devices)) < n and not rehearsal
    if shared_devices and ctx.rank == 0:
        print(f"[bench] {n} ranks ran on {len(set(rank_devices))} distinct device(s) {rank_devices}; an {n}-GPU "
              f"record needs {n} GPUs", file=sys.stderr)
    ok &= not shared_devices
    stream_failed = stream_rec is not None and stream_rec.get("streaming_error") is not None
    # what a CI gate reads: the static headline may stand while the
    # streaming protocol failed — that is never "ok"
    status = "failed" if not ok else "streaming_failed" if stream_failed else "ok"
    if ctx.rank == 0:
        rec = {
            "status": status,
            "metric": BASELINE_METRIC,
            "value": _sig(value),
            "unit": "Gpixel/s",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 5),
            "host_enqueue_ms_per_step": round(enqueue_ms, 5),
            "warmup_steps_run": warm_info["steps"],
            "warmup_ms": warm_info["ms"],
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": round(value / BASELINE_GPIXEL_PER_S, 2),
            "vs_baseline_note": BASELINE_NOTE,
            "dtype": "fp32",
            "data": (f"synthetic (uniform random RGBA8, {len(dets)} independent {args.size}x{args.size} images "
                     f"cycled by the timed steps, each split into {n} row slab(s))" if strong else
                     f"synthetic (uniform random RGBA8, {len(dets)} independent {args.size}x{args.size} slabs per GPU "
                     f"cycled by the timed steps)"),
            "config": {
                "model": f"lab2 2D convolution {args.size}x{args.size} image, "
                         f"{d0.filter.k}x{d0.filter.k} filter ({d0.filter.name}"
                         f"{', separable 1x5+5x1 passes' if d0.filter.separable else ''}, band-streaming HIP kernel)",
                "global_batch": 1 if strong else n,
                "layout": args.layout,
                "rows_per_rank": [d0.slab.rows_of(r) for r in range(n)],
                "seq_len": args.size,
                "parallelism": f"slab{n}" + (("+halo-peer-fused" if d0.peer is not None else "+halo-pipelined"
                                              if d0.pipeline else "+halo-overlap" if d0.overlap else "+halo-inorder")
                                             if n > 1 else ""),
                "transport": d0.transport if n > 1 else None,
                "peer_probe": (None if n == 1 or args.halo == "rccl" or ctx.device.type != "cuda" else "ok" if d0.peer is not None else "fallback"),
                "image_hw": [global_rows, args.size],
                "halo_rows": [d0.filter.halo_up, d0.filter.halo_down],
                "graph_steps": args.graph if graph is not None else 0,
                "streams": nstreams,
                "host_wait": wait_policy_in_force(ctx.device) if ctx.device.type == "cuda" else None,
                "rotate": len(dets),
                "working_set_MiB_per_gpu": round(len(dets) * 2 * d0.slab.rows * args.size * 4 / 2**20, 1),
            },
            "world_size_seen": seen,
            "rank_devices": rank_devices,
            "distinct_devices": len(set(rank_devices)),
            "rehearsal": rehearsal,
            **span.fields(args.steps),
            "full": args.full,
            # a plain run compares nothing (null); --full: every pixel against the CPU reference
            "verified_bit_exact": (ok and (args.no_verify or checked == len(dets) * global_rows * args.size)
                                   if args.full else None),
            "verified_pixels": checked,
            "verified_one_device": one_device,
            "device": str(torch.cuda.get_device_name(ctx.device)) if ctx.device.type == "cuda" else "cpu",
        }
        if clocks is not None:
            rec["clocks"] = clocks  # one entry per rank
        if sustained is not None:
            rec["value_sustained"] = _sig(pixels / sustained / 1e9)
            rec["ms_per_step_sustained"] = round(sustained * 1e3 / max(1, args.steps), 5)
            rec["sustain_ms"] = args.sustain_ms
        if steady is not None:
            w = steady["wins"]
            rec["value_steady"] = _sig(pixels * len(w) / sum(w) / 1e9)
            rec["value_steady_windows"] = [_sig(pixels / x / 1e9) for x in w]
            rec["steady_ms"] = args.steady_ms
            rec["steady_clocks"] = steady["clocks"]  # per rank: gfxclk / power medians, last 100 ms of load + windows
        if warm is not None:
            rec["value_warm_cache"] = _sig(pixels / warm / 1e9)
            rec["ms_per_step_warm_cache"] = round(warm * 1e3 / max(1, args.steps), 5)
        if warm1 is not None:
            rec["value_warm_cache_1stream"] = _sig(pixels / warm1 / 1e9)
            rec["ms_per_step_warm_cache_1stream"] = round(warm1 * 1e3 / max(1, args.steps), 5)
        if stream_rec is not None:
            rec.update(stream_rec)
        if cpu_ms is not None:
            rec["cpu_ms_per_image"] = round(cpu_ms["median"], 3)
            rec["cpu_ms_per_image_min"] = round(cpu_ms["min"], 3)
            rec["cpu_runs"] = cpu_ms["runs"]
            rec["cpu_threads"] = ops.vector._native.lib().mpx_cpu_threads()
            rec["gpu_ms_per_image"] = round(ms_per_step, 5)
            rec["speedup_vs_cpu"] = round(cpu_ms["median"] / ms_per_step, 1)
            if cpu_ms.get("serial_o0_ms") is not None:
                # the published methodology (reference README.md:11, lab2 report p.8-9): one thread, gcc -O0,
                # clock(); the same image and filter as the GPU steps
                rec["cpu_serial_o0_ms_per_image"] = round(cpu_ms["serial_o0_ms"], 3)
                rec["speedup_vs_cpu_serial_o0"] = round(cpu_ms["serial_o0_ms"] / ms_per_step, 1)
        print(json.dumps(rec), flush=True)
    for d in dets:
        d.close()
    parallel.shutdown()
    if not ok:
        return 1
    return 3 if (stream_failed and args.strict_streaming) else 0


def hip_streams(device, k: int) -> list:
    """The first k streams of the process-wide compute set (created by
    parallel.init before any communicator): both phases overlap their frames on
    the SAME streams, each on a hardware queue of its own. Two fresh streams
    made after the static phase's had landed on one queue (rocprofv3
    queue_id), which serialised the streaming phase's frames."""
    from cuda_mpi_openmp_amd.utils.streams import compute_streams

    return compute_streams(device, k)


class StreamingTimeout(RuntimeError):
    """A device-side halo wait of the streaming phase gave up on some rank
    (raised on every rank together, after the collective check)."""


def _inject_stream_timeout(rank: int) -> bool:
    """MPX_BENCH_INJECT_STREAM_TIMEOUT="r[,r...]": the named ranks report a
    device-side halo wait that gave up in the timed streaming steps (tests of
    the collective failure path, tests/test_bench_contract.py)."""
    spec = os.environ.get("MPX_BENCH_INJECT_STREAM_TIMEOUT", "")
    return any(t.strip() == str(rank) for t in spec.split(",") if t.strip())


def run_streaming(args, ctx, n, timed, watchdog, sync, ops, parallel) -> dict:
    """value_streaming: K timed steps of the iterated filter over the rotated
    slabs (each step's halo rows were produced by the neighbours' previous
    step), then the N-rank == one-device check of every rotated slab."""
    import torch

    from cuda_mpi_openmp_amd.models.edge import SlabEdgeDetector, stream_reference

    seeds = [1234 + 7919 * r for r in range(max(1, args.rotate))]
    sdets = []
    for sd in seeds:
        d = SlabEdgeDetector(ctx, args.global_rows, args.size, args.filter, halo=args.halo, stream=True)
        d.fill_random(seed=sd + ctx.rank)
        sdets.append(d)
    cyc = [0]

    def step():
        sdets[cyc[0] % len(sdets)].step()
        cyc[0] += 1

    # each slab's frame sequence stays on one stream; different slabs' sequences
    # are independent and overlap on the static phase's streams (device-signalled
    # or no halos only: host-ordered RCCL exchanges keep one stream)
    want = args.stream_streams or args.streams
    ns = want if (want > 1 and ctx.device.type == "cuda" and len(sdets) % want == 0
                  and all(d.independent_steps for d in sdets)) else 1
    shandles = hip_streams(ctx.device, ns) if ns > 1 else []
    for st in shandles:
        st.wait_stream(torch.cuda.current_stream(ctx.device))
    shandles = [st.cuda_stream for st in shandles]
    if shandles:
        def step():  # noqa: F811 - the multi-stream form of the step above
            i = cyc[0] % len(sdets)
            sdets[i].step(shandles[i % ns])
            cyc[0] += 1
    for _ in range(max(args.warmup, len(sdets))):
        step()
        watchdog.beat()
    sync()
    ctx.barrier()
    settle(step, len(sdets), args.warmup_ms, ctx, sync, watchdog, parallel, lambda: None)
    cyc[0] = 0
    span = timed(step, args.steps)
    enqueue_ms = timed.issue_s[step] * 1e3 / max(1, args.steps)
    watchdog.beat()
    elapsed = span.job_s
    # a device-side halo wait that gave up on ANY rank fails every rank here,
    # before the gathers below (a rank raising alone would leave the others
    # blocked in them until the watchdog fires: ADVICE r3)
    bad = [d.stream_timed_out() for d in sdets]
    if _inject_stream_timeout(ctx.rank):
        bad[0] = True
    if parallel.max_over_ranks(1.0 if any(bad) else 0.0, ctx) > 0:
        for d in sdets:
            d.close()
        raise StreamingTimeout(f"rank {ctx.rank}: streaming halo wait timed out during the timed steps "
                           f"({'this rank' if any(bad) else 'on another rank'}; slabs {[i for i, b in enumerate(bad) if b]})")
    rec = {"value_streaming": _sig(args.global_rows * args.size * args.steps / elapsed / 1e9),
           "streams_streaming": ns,
           "ms_per_step_streaming": round(elapsed * 1e3 / max(1, args.steps), 5),
           "host_enqueue_ms_per_step_streaming": round(enqueue_ms, 5),
           **span.fields(args.steps, "_streaming"),
           "transport_streaming": sdets[0].transport if n > 1 else None}
    if not args.no_verify:
        ok, checked = True, 0
        for sd, d in zip(seeds, sdets):
            good, cnt = verify_full(d, ops)  # this rank's last step vs the CPU reference
            ok &= good
            got = parallel.gather_slabs(d.stream_out.contiguous(), d.slab, ctx)
            if ctx.rank == 0:  # the whole job vs one device running the same frames on the whole image
                full0 = torch.cat([regen_slab(sd + r, d.slab.rows_of(r), args.size, ctx.device) for r in range(n)])
                ref = stream_reference(full0, d.filter, d._sk)
                same = torch.equal(got.to(ref.device), ref)
                ok &= same
                checked += ref.shape[0] * ref.shape[1] if same else 0
        ok = parallel.max_over_ranks(0.0 if ok else 1.0, ctx) == 0.0
        rec["verified_streaming"] = "N-rank result == one-device result of the same frame sequence (every pixel)"
        rec["verified_bit_exact_streaming"] = ok
        rec["verified_pixels_streaming"] = int(parallel.broadcast_object(checked, ctx))
        rec["verified_bit_exact"] = None if ok else False
    for d in sdets:
        d.close()
    if rec.get("verified_bit_exact") is None:
        rec.pop("verified_bit_exact", None)
    return rec


DUMP_BYTES = 48 << 20  # float32 rows over all ranks; with the row indices well inside 64 MB


def dump_outputs(path: str, out, ctx) -> None:
    """--dump-outputs: this rank's output slab of the last timed step as
    float32, whole when the ranks' slabs fit DUMP_BYTES together, else a fixed
    seeded choice of its rows (always with the first and last two: the image
    border and the halo rows' consumers), plus the chosen rows' indices."""
    import numpy as np
    import torch

    os.makedirs(path, exist_ok=True)
    rows = out.shape[0]
    keep = max(1, min(rows, DUMP_BYTES // ctx.world // (out[0].numel() * 4)))
    idx = torch.arange(rows)
    if keep < rows:
        g = torch.Generator().manual_seed(4096 + ctx.rank)
        edge = torch.tensor(sorted({0, 1, rows - 2, rows - 1} & set(range(rows))))
        pick = torch.randperm(rows, generator=g)
        idx = torch.cat([edge, pick[~torch.isin(pick, edge)]])[:keep].sort().values
    vals = out.index_select(0, idx.to(out.device)).to("cpu").to(torch.float32)
    np.save(os.path.join(path, f"out_rank{ctx.rank}.npy"), vals.numpy())
    np.save(os.path.join(path, f"rows_rank{ctx.rank}.npy"), idx.to(torch.float64).numpy())


def device_id(dev) -> str:
    """PCI location of a GPU ("dddd:bb:dd"), or "cpu"."""
    from cuda_mpi_openmp_amd.parallel.dist import device_pci

    return device_pci(dev)


def regen_slab(seed: int, rows: int, size: int, device):
    """Rank r's initial frame (SlabEdgeDetector.fill_random with its seed)."""
    import torch

    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return torch.randint(0, 256, (rows, size, 4), dtype=torch.uint8, device=device, generator=g)


def settle(step_fn, chunk: int, warmup_ms: float, ctx, sync, watchdog, parallel, finish) -> dict:
    """Time-based warm-up: after the fixed warm-up steps, run untimed steps
    until at least ``warmup_ms`` of back-to-back step time has elapsed. The step
    count is derived from one timed probe chunk and agreed across ranks (max),
    so RCCL halo sends/recvs stay matched. Returns {"steps", "ms"}."""
    if warmup_ms <= 0:
        return {"steps": 0, "ms": 0.0}
    t0 = time.perf_counter()
    steps = 0
    rest = chunk
    for _ in range(16):  # rounds: each agrees across ranks on how many more steps to run
        for i in range(rest):
            step_fn()
            if i % 256 == 255:
                watchdog.beat()
        steps += rest
        finish()
        sync()
        elapsed = (time.perf_counter() - t0) * 1e3
        need = parallel.max_over_ranks(warmup_ms - elapsed, ctx)
        watchdog.beat()
        if need <= 0:
            break
        per_step = elapsed / steps
        # every rank must run the same count (halo sends / recvs stay matched)
        rest = int(parallel.max_over_ranks(float(max(1, min(200000, int(need / max(per_step, 1e-3)) + 1))), ctx))
    ctx.barrier()
    return {"steps": steps, "ms": round((time.perf_counter() - t0) * 1e3, 2)}


def cpu_baseline_ms(det, size: int, ops, runs: int = 5) -> dict:
    """CPU reference on the rank's first size x size image (rank 0 only):
    the OpenMP -O3 build, median and min of ``runs`` calls, plus the serial
    gcc -O0 program (labs/lab2/src/cpu_exe, the published methodology) on the
    same image written as a .data file, when it is built."""
    import statistics
    import subprocess
    import tempfile

    import torch

    img = det.own[:size].to("cpu").contiguous()
    if img.shape[0] < size:  # strong layout: this rank owns a fraction of the image; time a whole frame
        g = torch.Generator().manual_seed(99)
        img = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, generator=g)
    out = torch.empty_like(img)
    ops.conv(img, det.filter, out)  # first touch of the output pages outside the timing
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ops.conv(img, det.filter, out)
        ts.append((time.perf_counter() - t0) * 1e3)
    res = {"median": statistics.median(ts), "min": min(ts), "runs": runs, "serial_o0_ms": None}
    exe = os.path.join(ROOT, "labs", "lab2", "src", "cpu_exe")
    if os.path.exists(exe) and os.environ.get("MPX_BENCH_SERIAL_CPU", "1") != "0":
        from cuda_mpi_openmp_amd.harness.core import parse_timing
        from cuda_mpi_openmp_amd.utils.imgdata import encode_data

        with tempfile.TemporaryDirectory() as td:
            src, dst = os.path.join(td, "in.data"), os.path.join(td, "out.data")
            with open(src, "wb") as f:
                f.write(encode_data(img.numpy()))
            r = subprocess.run([exe, "--op", det.filter.name], input=f"{src}\n{dst}\n", capture_output=True,
                               text=True, timeout=600)
            if r.returncode == 0:
                res["serial_o0_ms"] = parse_timing(r.stdout.splitlines()[0] if r.stdout else "")
    return res


def verify_one_device(dets, args, ctx, ops, parallel) -> bool:
    """Strong layout: every rotated image's gathered N-rank output equals one
    device convolving the whole frame (regenerated from the ranks' seeds)."""
    import torch

    ok = True
    n = ctx.world
    for r_i, d in enumerate(dets):
        got = parallel.gather_slabs(d.out.contiguous(), d.slab, ctx)
        if ctx.rank == 0:
            seed = 1234 + 7919 * r_i
            full = torch.cat([regen_slab(seed + r, d.slab.rows_of(r), args.size, ctx.device) for r in range(n)])
            ref = ops.conv(full, d.filter)
            ok &= bool(torch.equal(got.to(ref.device), ref))
    return parallel.max_over_ranks(0.0 if ok else 1.0, ctx) == 0.0


def verify_full(det, ops):
    """Every owned output row of one detector against the OpenMP CPU reference
    run on the same halo-filled input (bit-exact). Returns (ok, pixels checked)."""
    import torch

    s = det.slab
    buf = det.halo_filled().to("cpu")
    out_cpu = torch.empty((s.rows, det.w, 4), dtype=torch.uint8)
    ops.conv_rows(buf, out_cpu, det.filter, src_row0=s.own_offset, out_row0=0, oy0=0, oy1=s.rows, y_lo=s.y_lo,
                  y_hi=s.y_hi)
    good = bool(torch.equal(out_cpu, (det.stream_out if det.stream else det.out).to("cpu")))
    return good, s.rows * det.w


if __name__ == "__main__":
    sys.exit(main())
