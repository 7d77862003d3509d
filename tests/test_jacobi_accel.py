"""Chebyshev acceleration of the Jacobi tier, from the kernels to SlabJacobi.

With s the value of the plain sweep (Laplace, or Poisson with a right-hand side
b) and p the iterate before last, which ``un`` holds on entry, a step is

    un = p + omega * (s - p)

a subtract, a multiply and an add, each rounded, with omega rounded once to the
working dtype. GPU fp32, GPU fp64, the CPU library and the dtype-preserving
torch expression (``ref.jacobi(..., keep_dtype=True, omega=, prev=)``) agree bit
for bit; no kernel comparison here carries a tolerance. The method is the one
of test_jacobi_rhs.py, except that ``un`` is pre-filled with a seeded random
previous iterate instead of a sentinel: rows [r0, r1) must equal the reference,
every other row must keep its bits, and the residual word must equal the
maximum of the per-row reference residuals max|s - u| (independent of omega).

Halo rows, boundary columns and pitch padding of p and b hold NaN: they are
don't-care and must reach no output and no residual. omega is drawn from the
real schedule of the case's geometry (omega_2, omega_9) plus the arbitrary 1.7.
"""

from __future__ import annotations

import ctypes
import functools
import math
import os
import socket
import traceback

import pytest
import torch
import torch.multiprocessing as mp

from cuda_mpi_openmp_amd import _native, ops, parallel
from cuda_mpi_openmp_amd.models import SlabJacobi
from cuda_mpi_openmp_amd.ops import reference as ref

FIELDS = {"uniform": dict(scale=1.0, offset=0.0), "flat": dict(scale=2.0 ** -10, offset=0.5)}
DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector
NAN = float("nan")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _schedule(global_rows: int, cols: int, n: int):
    """(rho, [omega_1 .. omega_n]) of the issue's recurrence; omega_1 = 1 is the
    nominal value of the plain first step."""
    rho = 0.5 * (math.cos(math.pi / (global_rows + 1)) + math.cos(math.pi / (cols - 1)))
    om = [1.0, 1.0 / (1.0 - rho * rho / 2.0)]
    while len(om) < n:
        om.append(1.0 / (1.0 - rho * rho * om[-1] / 4.0))
    return rho, om[:n]


def _omegas(height: int, cols: int):
    """omega_2 and omega_9 of the geometry (a width below 3 has no schedule: 3
    stands in) and one arbitrary value."""
    _, om = _schedule(height - 2, max(cols, 3), 9)
    return (om[1], om[8], 1.7)


@functools.lru_cache(maxsize=None)
def _case(dtype, height: int, cols: int, field: str = "uniform"):
    """(u, b, p, per-row residuals without b, with b) on the CPU, computed once
    and never modified. b and p carry NaN in their halo rows and boundary
    columns. rowres[k] is max_j |s - c| of row k + 1."""
    kw = FIELDS[field]
    g = torch.Generator().manual_seed(9000 * cols + 10 * height + len(field))
    u = (torch.rand((height, cols), generator=g, dtype=torch.float64) * kw["scale"] + kw["offset"]).to(dtype)
    b = ((torch.rand((height, cols), generator=g, dtype=torch.float64) * 2.0 - 1.0) * kw["scale"]).to(dtype)
    p = (torch.rand((height, cols), generator=g, dtype=torch.float64) * kw["scale"] + kw["offset"]).to(dtype)
    for t in (b, p):
        t[0] = t[-1] = NAN
        t[:, 0] = t[:, -1] = NAN
    rowres = []
    for rhs in (None, b):
        plain = ref.jacobi(u, 1, height - 1, keep_dtype=True, rhs=rhs)
        if cols > 2:
            rowres.append((plain[1:-1, 1:-1] - u[1:-1, 1:-1]).abs().amax(dim=1))
        else:
            rowres.append(torch.zeros(height - 2, dtype=dtype))
    return u, b, p, rowres[0], rowres[1]


@functools.lru_cache(maxsize=None)
def _want(dtype, height: int, cols: int, field: str, with_rhs: bool, omega: float) -> torch.Tensor:
    """The full-height torch reference of one accelerated sweep."""
    u, b, p, _, _ = _case(dtype, height, cols, field)
    w = ref.jacobi(u, 1, height - 1, keep_dtype=True, rhs=b if with_rhs else None, omega=omega, prev=p)
    assert w.dtype == dtype and not bool(torch.isnan(w).any())
    return w


def _expected_res(rowres: torch.Tensor, r0: int, r1: int) -> float:
    return float(rowres[r0 - 1:r1 - 1].max()) if r1 > r0 else 0.0


def _assert_sweep(un, res, want, p, rowres, r0, r1, tag):
    """un started as a copy of p: rows [r0, r1) hold the reference, every other
    row its old bits (NaN included), the residual word the per-row maximum."""
    assert _same_bits(un[r0:r1], want[r0:r1]), f"output differs: {tag}"
    assert _same_bits(un[:r0], p[:r0]) and _same_bits(un[r1:], p[r1:]), f"rows outside the range written: {tag}"
    if res is not None:
        got, exp = float(res.item()), _expected_res(rowres, r0, r1)
        assert got == exp, f"residual {got!r} != {exp!r}: {tag}"


def _abi(u, b, un, cols, pitch, r0, r1, omega, res):
    L = _native.lib()
    fn = L.mpx_jacobi_accel_f64 if u.dtype == torch.float64 else L.mpx_jacobi_accel_f32
    _native.check(fn(u.data_ptr(), None if b is None else b.data_ptr(), un.data_ptr(), cols, pitch, r0, r1, omega,
                     None if res is None else res.data_ptr(), _native.stream_of(u)))


def _variant(u, b, un, cols, pitch, r0, r1, omega, res, R):
    _native.check(_native.tune_lib().mpx_jacobi_accel_variant(
        u.data_ptr(), None if b is None else b.data_ptr(), un.data_ptr(), cols, pitch, r0, r1, omega,
        None if res is None else res.data_ptr(), int(u.dtype == torch.float64), R, _native.stream_of(u)))


# ---------------------------------------------------------------------------
# 1. CPU library and ops.jacobi_sweep(omega=) on CPU tensors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [3, 5, 64])
def test_cpu_library_equals_the_torch_expression(cols):
    height = 20
    u, b, p, rr_lap, rr_rhs = _case(torch.float64, height, cols)
    L = _native.lib()
    for with_rhs in (False, True):
        rowres = rr_rhs if with_rhs else rr_lap
        for omega in _omegas(height, cols):
            want = _want(torch.float64, height, cols, "uniform", with_rhs, omega)
            for r0, r1 in ((1, height - 1), (1, 2), (4, 11), (height - 2, height - 1), (6, 6)):
                tag = (cols, with_rhs, omega, r0, r1)
                un = p.clone()
                r = L.mpx_cpu_jacobi_accel_f64(u.data_ptr(), b.data_ptr() if with_rhs else None, un.data_ptr(), cols,
                                               cols, r0, r1, omega)
                _assert_sweep(un, None, want, p, rowres, r0, r1, tag)
                assert r == _expected_res(rowres, r0, r1), tag
                un2 = p.clone()
                res = torch.zeros(1, dtype=torch.float64)
                r2 = ops.jacobi_sweep(u.clone(), un2, r0, r1, res, rhs=b.clone() if with_rhs else None, omega=omega)
                assert r2 == r
                _assert_sweep(un2, res, want, p, rowres, r0, r1, ("ops",) + tag)


@pytest.mark.parametrize("cols,pad", [(5, 1), (64, 3)])
def test_cpu_library_pitch_wider_than_cols(cols, pad):
    """NaN in the padding of u, b and p reaches nothing; un's padding keeps its bits."""
    height, pitch = 20, cols + pad
    u, b, p, rr_lap, rr_rhs = _case(torch.float64, height, cols)
    up, bp, pp = (torch.full((height, pitch), NAN, dtype=torch.float64) for _ in range(3))
    up[:, :cols], bp[:, :cols], pp[:, :cols] = u, b, p
    omega = _omegas(height, cols)[0]
    for with_rhs in (False, True):
        want = _want(torch.float64, height, cols, "uniform", with_rhs, omega)
        rowres = rr_rhs if with_rhs else rr_lap
        for r0, r1 in ((1, height - 1), (3, 9)):
            un = pp.clone()
            r = _native.lib().mpx_cpu_jacobi_accel_f64(up.data_ptr(), bp.data_ptr() if with_rhs else None,
                                                       un.data_ptr(), cols, pitch, r0, r1, omega)
            assert _same_bits(un[:, cols:], pp[:, cols:]), "padding written"
            assert not bool(torch.isnan(un[r0:r1, :cols]).any())
            _assert_sweep(un[:, :cols], None, want, p, rowres, r0, r1, (cols, pitch, with_rhs, r0, r1))
            assert r == _expected_res(rowres, r0, r1)


# ---------------------------------------------------------------------------
# 2. argument errors: nothing is written
# ---------------------------------------------------------------------------
def test_argument_errors():
    u = torch.zeros((6, 8), dtype=torch.float64)
    un = torch.full_like(u, -7.0)
    u32 = torch.zeros((6, 8), dtype=torch.float32)
    un32 = torch.full_like(u32, -7.0)
    L = _native.lib()
    bad = (0.0, -1.5, float("nan"), float("inf"), -float("inf"))
    for w in bad:
        with pytest.raises(ValueError):
            ops.jacobi_sweep(u, un, 1, 5, omega=w)
        assert L.mpx_jacobi_accel_f64(u.data_ptr(), None, un.data_ptr(), 8, 8, 1, 5, w, None, None) != 0
        assert L.mpx_jacobi_accel_f64(u.data_ptr(), u.data_ptr(), un.data_ptr(), 8, 8, 1, 5, w, None, None) != 0
        assert L.mpx_jacobi_accel_f32(u32.data_ptr(), None, un32.data_ptr(), 8, 8, 1, 5, w, None, None) != 0
        assert math.isnan(L.mpx_cpu_jacobi_accel_f64(u.data_ptr(), None, un.data_ptr(), 8, 8, 1, 5, w))
        assert _native.tune_lib().mpx_jacobi_accel_variant(u.data_ptr(), None, un.data_ptr(), 8, 8, 1, 5, w, None, 1, 8,
                                                           None) != 0
    # positive doubles that are 0 or infinite once rounded to float
    for w in (1e-60, 1e60):
        assert L.mpx_jacobi_accel_f32(u32.data_ptr(), None, un32.data_ptr(), 8, 8, 1, 5, w, None, None) != 0
    with pytest.raises(_native.MpxError):
        _native.check(L.mpx_jacobi_accel_f64(u.data_ptr(), None, un.data_ptr(), 8, 8, 1, 5, 0.0, None, None))
    # null u / un, bad geometry
    assert L.mpx_jacobi_accel_f64(None, None, un.data_ptr(), 8, 8, 1, 5, 1.5, None, None) != 0
    assert L.mpx_jacobi_accel_f32(None, None, un32.data_ptr(), 8, 8, 1, 5, 1.5, None, None) != 0
    assert L.mpx_jacobi_accel_f64(u.data_ptr(), None, None, 8, 8, 1, 5, 1.5, None, None) != 0
    assert L.mpx_jacobi_accel_f64(u.data_ptr(), None, un.data_ptr(), 8, 7, 1, 5, 1.5, None, None) != 0
    assert L.mpx_jacobi_peer_sweep_accel(1, None, None, un.data_ptr(), 8, 8, 4, 1.5, None, None, None) != 0
    assert L.mpx_jacobi_peer_sweep_accel(1, u.data_ptr(), None, un.data_ptr(), 8, 8, 4, 1.5, None, None, None) != 0
    assert math.isnan(L.mpx_cpu_jacobi_accel_f64(None, None, un.data_ptr(), 8, 8, 1, 5, 1.5))
    assert math.isnan(L.mpx_cpu_jacobi_accel_f64(u.data_ptr(), None, un.data_ptr(), 8, 7, 1, 5, 1.5))
    assert _native.tune_lib().mpx_jacobi_accel_variant(None, None, un.data_ptr(), 8, 8, 1, 5, 1.5, None, 1, 8, None) != 0
    assert bool((un == -7.0).all()) and bool((un32 == -7.0).all())
    # the oracle wants omega and prev together
    with pytest.raises(ValueError):
        ref.jacobi(u, 1, 5, omega=1.5)
    with pytest.raises(ValueError):
        SlabJacobi(parallel.DistContext(), 4, 8, accel="sor")
    with pytest.raises(ValueError):
        SlabJacobi(parallel.DistContext(), 4, 8, accel=True)
    plain = SlabJacobi(parallel.DistContext(), 4, 8)
    assert plain.accel is None and plain.rho is None and plain.omega is None and plain.accel_step == 0


# ---------------------------------------------------------------------------
# 3. symbols
# ---------------------------------------------------------------------------
def test_accel_variant_is_a_tuning_entry_only():
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert hasattr(_native.tune_lib(), "mpx_jacobi_accel_variant")
    assert not hasattr(raw, "mpx_jacobi_accel_variant"), "mpx_jacobi_accel_variant exported by libmpx"
    for name in ("mpx_jacobi_accel_f64", "mpx_jacobi_accel_f32", "mpx_jacobi_peer_sweep_accel",
                 "mpx_cpu_jacobi_accel_f64"):
        assert hasattr(raw, name), name


# ---------------------------------------------------------------------------
# 4. the schedule
# ---------------------------------------------------------------------------
def _problem_solver(device, dtype, rows, cols, accel, seed=5, rhs_seed=None):
    sol = SlabJacobi(parallel.DistContext(device=device), rows, cols, dtype=dtype, check_every=5, accel=accel)
    sol.set_boundary(top=1.0, left=0.5, right=0.25)
    sol.fill(seed=seed)
    if rhs_seed is not None:
        g = torch.Generator().manual_seed(rhs_seed)
        sol.set_rhs(tensor=torch.rand((rows, cols), generator=g, dtype=torch.float64) - 0.5)
    return sol


def _assert_next_step_is_plain(sol):
    """The next step must be the plain sweep of u (whatever un holds)."""
    n = sol.slab.rows
    want = ref.jacobi(sol.u, 1, n + 1, keep_dtype=True, rhs=sol.rhs)
    sol.step()
    assert _same_bits(sol.u.cpu(), want)
    assert sol.accel_step == 1 and sol.omega == 1.0


def test_schedule_and_restarts():
    rows, cols = 14, 16
    rho, om = _schedule(rows, cols, 20)
    acc = _problem_solver("cpu", torch.float64, rows, cols, "chebyshev")
    plain = _problem_solver("cpu", torch.float64, rows, cols, None)
    assert acc.rho == rho and acc.omega is None and acc.accel_step == 0
    acc.step()
    plain.step()
    assert _same_bits(acc.u, plain.u), "step 1 is the plain sweep"
    assert acc.omega == 1.0 and acc.accel_step == 1
    for k in range(2, 21):
        prev, cur = acc.un.clone(), acc.u.clone()  # un holds the iterate before u
        acc.step()
        assert acc.omega == om[k - 1] and acc.accel_step == k, k
        want = ref.jacobi(cur, 1, rows + 1, keep_dtype=True, omega=om[k - 1], prev=prev)
        assert _same_bits(acc.u, want), k
    plain.run(19)
    assert not torch.equal(acc.u, plain.u)
    acc.restart_acceleration()
    assert acc.omega is None and acc.accel_step == 0
    _assert_next_step_is_plain(acc)
    acc.run(4)
    assert acc.accel_step == 5 and acc.omega == om[4]
    acc.fill(seed=11)
    _assert_next_step_is_plain(acc)
    acc.run(4)
    g = torch.Generator().manual_seed(3)
    acc.set_rhs(tensor=torch.rand((rows, cols), generator=g, dtype=torch.float64) - 0.5)
    assert acc.accel_step == 0
    _assert_next_step_is_plain(acc)
    acc.run(3)
    acc.u[3, 4] += 0.125  # a host write followed by _halos_valid = False
    acc._halos_valid = False
    _assert_next_step_is_plain(acc)
    acc.run(3)
    acc.set_boundary(top=2.0)
    _assert_next_step_is_plain(acc)


# ---------------------------------------------------------------------------
# 5. convergence on the manufactured problem
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _manufactured(h: int = 16, w: int = 16):
    """u* random on an h x w grid, boundary included, and
    b = 4 u* - (sum of the neighbours) in fp64: u* is the fixed point."""
    g = torch.Generator().manual_seed(20)
    us = torch.rand((h, w), generator=g, dtype=torch.float64)
    b = torch.zeros_like(us)
    b[1:-1, 1:-1] = 4.0 * us[1:-1, 1:-1] - ((us[:-2, 1:-1] + us[2:, 1:-1]) + (us[1:-1, :-2] + us[1:-1, 2:]))
    return us, b


def _manufactured_solver(device, dtype, accel, h=16, w=16) -> SlabJacobi:
    us, b = _manufactured(h, w)
    sol = SlabJacobi(parallel.DistContext(device=device), h - 2, w, dtype=dtype, check_every=10, accel=accel)
    start = us.clone()
    start[1:-1, 1:-1] = 0.0  # boundary from u*, interior from 0
    sol.u.copy_(start.to(dtype))
    sol.un.copy_(sol.u)
    sol.set_rhs(tensor=b[1:-1])
    return sol


@functools.lru_cache(maxsize=None)
def _torch_iterate(dtype, iters: int, h: int = 16, w: int = 16) -> torch.Tensor:
    us, b = _manufactured(h, w)
    u = us.clone()
    u[1:-1, 1:-1] = 0.0
    u, bb = u.to(dtype), b.to(dtype)
    _, om = _schedule(h - 2, w, max(iters, 2))
    prev = u
    for k in range(1, iters + 1):
        if k == 1:
            nxt = ref.jacobi(u, 1, h - 1, keep_dtype=True, rhs=bb)
        else:
            nxt = ref.jacobi(u, 1, h - 1, keep_dtype=True, rhs=bb, omega=om[k - 1], prev=prev)
        prev, u = u, nxt
    return u


def _check_convergence(device, h, w, iters, acc_bound, plain_bound):
    us, _ = _manufactured(h, w)
    acc = _manufactured_solver(device, torch.float64, "chebyshev", h, w)
    acc.run(iters)
    err = float((acc.u.cpu() - us).abs().max())
    print(f"{h}x{w} {iters} iterations: accelerated error {err:.3e} residual {acc.last_residual:.3e}")
    assert err <= acc_bound, err
    assert acc.last_residual is not None and acc.last_residual <= acc_bound, acc.last_residual
    plain = _manufactured_solver(device, torch.float64, None, h, w)
    plain.run(iters)
    perr = float((plain.u.cpu() - us).abs().max())
    print(f"{h}x{w} {iters} iterations: plain error {perr:.3e}")
    assert perr > plain_bound, perr


def test_convergence_cpu():
    # numpy, fp64: 16 x 16 / 200: 4.4e-16 accelerated, 9.4e-3 plain; 34 x 66 / 400: 2.1e-13, 0.25
    _check_convergence("cpu", 16, 16, 200, 1e-12, 1e-3)
    _check_convergence("cpu", 34, 66, 400, 1e-10, 0.1)
    sol = _manufactured_solver("cpu", torch.float64, "chebyshev")
    sol.run(50)
    assert _same_bits(sol.u, _torch_iterate(torch.float64, 50))


# ---------------------------------------------------------------------------
# 6. three gloo CPU ranks, checkpoint in the middle, against one rank
# ---------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _global_problem(rows, cols, dtype=torch.float64):
    g = torch.Generator().manual_seed(31)
    field = torch.rand((rows, cols - 2), generator=g, dtype=torch.float64).to(dtype)
    src = (torch.rand((rows, cols), generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dtype)
    return field, src


def _setup(sol, field, src, rhs=True):
    sol.set_boundary(top=1.0, left=0.5, right=0.25)
    s = sol.slab
    sol.u[1:1 + s.rows, 1:-1] = field[s.row0:s.row0 + s.rows].to(sol.u.device)
    sol.un.copy_(sol.u)
    sol._halos_valid = False
    if rhs:
        sol.set_rhs(tensor=src[s.row0:s.row0 + s.rows])


def _cpu_ckpt_worker(rank, world, port, rows, cols, ckdir, errq):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        ctx = parallel.init(device="cpu")
        field, src = _global_problem(rows, cols)
        _, om = _schedule(rows, cols, 25)
        a = SlabJacobi(ctx, rows, cols, check_every=5, accel="chebyshev")
        _setup(a, field, src)
        a.run(10)
        assert a.accel_step == 10 and a.omega == om[9]
        a.save_checkpoint(os.path.join(ckdir, "ck"))
        ck = torch.load(os.path.join(ckdir, f"ck.rank{rank}.pt"), weights_only=True)
        assert "u_prev" in ck and torch.equal(ck["u_prev"], a.un)
        assert ck["accel"] == {"step": 10, "omega": om[9], "rho": a.rho}
        b = SlabJacobi(ctx, rows, cols, check_every=5, accel="chebyshev")
        b.set_boundary(top=1.0, left=0.5, right=0.25)
        b.load_checkpoint(os.path.join(ckdir, "ck"))
        assert b.iteration == 10 and b.accel_step == 10 and b.omega == om[9]
        b.run(15)
        assert b.accel_step == 25 and b.omega == om[24]
        got, res = b.gather(), b.last_residual
        # a checkpoint written by a plain solver loads as a restart
        c = SlabJacobi(ctx, rows, cols, check_every=5)
        _setup(c, field, src)
        c.run(3)
        c.save_checkpoint(os.path.join(ckdir, "plain"))
        pk = torch.load(os.path.join(ckdir, f"plain.rank{rank}.pt"), weights_only=True)
        assert "u_prev" not in pk and "accel" not in pk
        b.load_checkpoint(os.path.join(ckdir, "plain"))
        assert b.accel_step == 0 and b.omega is None and b.iteration == 3
        b.step()
        c.step()
        assert b.accel_step == 1 and torch.equal(b.owned, c.owned), "the first step after a restart is plain"
        if ctx.rank == 0:
            one = SlabJacobi(parallel.DistContext(), rows, cols, check_every=5, accel="chebyshev")
            _setup(one, field, src)
            one.run(25)
            assert torch.equal(got, one.owned), "three accelerated ranks differ from one rank"
            assert res == one.last_residual and res is not None
            pl = SlabJacobi(parallel.DistContext(), rows, cols, check_every=5)
            _setup(pl, field, src)
            pl.run(25)
            assert not torch.equal(pl.owned, one.owned)
        parallel.shutdown()
    except Exception:  # noqa: BLE001
        errq.put(f"rank {rank}: {traceback.format_exc()}")


def _run_ranks(target, world, *args, timeout=150, **kwargs):
    """Run `world` rank processes, bounded by `timeout` seconds in total; ranks
    still alive then are killed and reported."""
    import time

    ctx = mp.get_context("spawn")
    errq = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, errq), kwargs=kwargs) for r in range(world)]
    for p in procs:
        p.start()
    errs = []
    deadline = time.monotonic() + timeout
    while any(p.is_alive() for p in procs) and time.monotonic() < deadline:
        while not errq.empty():  # drain while waiting: a child blocks at exit until its queue is read
            errs.append(errq.get())
        time.sleep(0.1)
    hung = [r for r, p in enumerate(procs) if p.is_alive()]
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join(10)
    while not errq.empty():
        errs.append(errq.get())
    assert not hung, f"ranks {hung} still running after {timeout} s"
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


def test_three_cpu_ranks_with_checkpoint_equal_one_rank(tmp_path):
    _run_ranks(_cpu_ckpt_worker, 3, 8 * 3 + 5, 19, str(tmp_path))


# ---------------------------------------------------------------------------
# 7. every row-block shape of the production template (ACCEL = true)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_accel_production_template_every_row_block(gpu, dtype):
    """Row counts 1..3R put the tail (1..R rows) in block 0 (walking down),
    block 1 (walking up) and block 2 (down again); Laplace and RHS, with and
    without the residual word, both fields, omega cycling through the three."""
    cols = 129 * NV[dtype]  # three strips, the last one partial
    height = 54
    oms = _omegas(height, cols)
    launches = 0
    for field in FIELDS:
        u, b, p, rr_lap, rr_rhs = _case(dtype, height, cols, field)
        ud, bd, pd = u.to(gpu), b.to(gpu), p.to(gpu)
        wd = {(rhs, w): _want(dtype, height, cols, field, rhs, w).to(gpu) for rhs in (False, True) for w in oms}
        un = torch.empty_like(ud)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        for R in (1, 2, 3, 5, 8):
            for r0 in (1, 2):
                for n in range(1, 3 * R + 1):
                    r1 = r0 + n
                    assert r1 <= height - 1
                    for with_rhs, with_res in ((False, True), (True, True), (False, False), (True, False)):
                        w = oms[launches % 3]
                        un.copy_(pd)
                        res.zero_()
                        _variant(ud, bd if with_rhs else None, un, cols, cols, r0, r1, w, res if with_res else None, R)
                        _assert_sweep(un, res if with_res else None, wd[with_rhs, w], pd,
                                      rr_rhs if with_rhs else rr_lap, r0, r1,
                                      (dtype, field, R, r0, r1, with_rhs, with_res, w))
                        launches += 1
    assert launches == 2 * 2 * 4 * 3 * (1 + 2 + 3 + 5 + 8)


# ---------------------------------------------------------------------------
# 8. column edges of the wave path (production launch)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_accel_wave_path_column_edges(gpu, dtype):
    rows = 9
    for nvec in (1, 2, 61, 62, 63, 124, 125):
        cols = nvec * NV[dtype]
        oms = _omegas(rows + 2, cols)
        for fi, field in enumerate(FIELDS):
            u, b, p, rr_lap, rr_rhs = _case(dtype, rows + 2, cols, field)
            ud, bd, pd = u.to(gpu), b.to(gpu), p.to(gpu)
            for with_rhs in (False, True):
                w = oms[(fi + with_rhs) % 3]
                un = pd.clone()
                res = torch.zeros(1, dtype=dtype, device=gpu)
                ops.jacobi_sweep(ud, un, 1, rows + 1, res, rhs=bd if with_rhs else None, omega=w)
                _assert_sweep(un, res, _want(dtype, rows + 2, cols, field, with_rhs, w).to(gpu), pd,
                              rr_rhs if with_rhs else rr_lap, 1, rows + 1, (dtype, field, cols, with_rhs))


# ---------------------------------------------------------------------------
# 9. generic kernels; un off the 16-byte boundary; pitch > cols
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_accel_generic_kernels(gpu, dtype):
    height = 33 + 3
    for cols in (1, 2, 3, 5, 255, 257, 513):
        oms = _omegas(height, cols)
        u, b, p, rr_lap, rr_rhs = _case(dtype, height, cols)
        ud, bd, pd = u.to(gpu), b.to(gpu), p.to(gpu)
        un = torch.empty_like(ud)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        k = 0
        for rows in (1, 16, 17, 33):
            for r0 in (1, 2):
                for with_rhs in (False, True):
                    w = oms[k % 3]
                    k += 1
                    un.copy_(pd)
                    res.zero_()
                    ops.jacobi_sweep(ud, un, r0, r0 + rows, res, rhs=bd if with_rhs else None, omega=w)
                    _assert_sweep(un, res, _want(dtype, height, cols, "uniform", with_rhs, w).to(gpu), pd,
                                  rr_rhs if with_rhs else rr_lap, r0, r0 + rows, (dtype, cols, r0, rows, with_rhs))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_accel_unaligned_un_takes_scalar_kernel(gpu, dtype):
    rows, cols = 17, 63 * NV[dtype]
    u, b, p, rr_lap, rr_rhs = _case(dtype, rows + 2, cols)
    n = (rows + 2) * cols
    flat = torch.empty(n + 8, dtype=dtype, device=gpu)
    un = flat[1:1 + n].view(rows + 2, cols)
    ud, bd, pd = u.to(gpu), b.to(gpu), p.to(gpu)
    assert un.is_contiguous() and un.data_ptr() % 16 != 0 and ud.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
    oms = _omegas(rows + 2, cols)
    for with_rhs in (False, True):
        un.copy_(pd)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        ops.jacobi_sweep(ud, un, 1, rows + 1, res, rhs=bd if with_rhs else None, omega=oms[with_rhs])
        _assert_sweep(un, res, _want(dtype, rows + 2, cols, "uniform", with_rhs, oms[with_rhs]).to(gpu), pd,
                      rr_rhs if with_rhs else rr_lap, 1, rows + 1, (dtype, with_rhs))
    # the wave template itself refuses such a un
    with pytest.raises(_native.MpxError, match="vector layout"):
        _variant(ud, None, un, cols, cols, 1, rows + 1, 1.7, None, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_accel_pitch_wider_than_cols(gpu, dtype):
    nv = NV[dtype]
    rows, cols, pitch = 19, 63 * nv, 63 * nv + nv
    u, b, p, rr_lap, rr_rhs = _case(dtype, rows + 2, cols)
    ud, bd, pp = (torch.full((rows + 2, pitch), NAN, dtype=dtype, device=gpu) for _ in range(3))
    ud[:, :cols], bd[:, :cols], pp[:, :cols] = u.to(gpu), b.to(gpu), p.to(gpu)
    pd = p.to(gpu)
    oms = _omegas(rows + 2, cols)
    for with_rhs in (False, True):
        wd = _want(dtype, rows + 2, cols, "uniform", with_rhs, oms[1]).to(gpu)
        for r0, r1 in ((1, rows + 1), (3, rows - 1)):
            un = pp.clone()
            res = torch.zeros(1, dtype=dtype, device=gpu)
            _abi(ud, bd if with_rhs else None, un, cols, pitch, r0, r1, oms[1], res)
            assert _same_bits(un[:, cols:], pp[:, cols:]), "padding written"
            assert not bool(torch.isnan(un[r0:r1, :cols]).any())
            _assert_sweep(un[:, :cols], res, wd, pd, rr_rhs if with_rhs else rr_lap, r0, r1, (dtype, with_rhs, r0, r1))


# ---------------------------------------------------------------------------
# 10. the overlapped step's launch pattern
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["wave", "generic"])
def test_accel_overlapped_step_launch_pattern(gpu, dtype, family):
    cols = 70 * NV[dtype] if family == "wave" else 257
    for n in (37, 1, 2):
        u, b, p, rr_lap, rr_rhs = _case(dtype, n + 2, cols)
        ud, bd, pd = u.to(gpu), b.to(gpu), p.to(gpu)
        w = _omegas(n + 2, cols)[1]
        for with_rhs in (False, True):
            rhs = bd if with_rhs else None
            rowres = rr_rhs if with_rhs else rr_lap
            wd = _want(dtype, n + 2, cols, "uniform", with_rhs, w).to(gpu)
            full = pd.clone()
            rfull = torch.zeros(1, dtype=dtype, device=gpu)
            ops.jacobi_sweep(ud, full, 1, n + 1, rfull, rhs=rhs, omega=w)
            _assert_sweep(full, rfull, wd, pd, rowres, 1, n + 1, (dtype, family, n, with_rhs, "full"))
            un = pd.clone()
            res = torch.zeros(1, dtype=dtype, device=gpu)
            for r in ([1] if n == 1 else [1, n]):
                ops.jacobi_sweep(ud, un, r, r + 1, res, rhs=rhs, omega=w)
            if n >= 2:
                ops.jacobi_sweep(ud, un, 2, n, res, rhs=rhs, omega=w)
            _assert_sweep(un, res, wd, pd, rowres, 1, n + 1, (dtype, family, n, with_rhs, "overlapped"))
            assert _same_bits(un, full) and _same_bits(res, rfull), (dtype, family, n, with_rhs)


# ---------------------------------------------------------------------------
# 11. SlabJacobi(accel="chebyshev") on the GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_accel_solver_gpu(gpu):
    cpu = _manufactured_solver("cpu", torch.float64, "chebyshev")
    cpu.run(60)
    sol = _manufactured_solver(gpu, torch.float64, "chebyshev")
    sol.run(60)
    assert _same_bits(sol.u.cpu(), cpu.u) and sol.last_residual == cpu.last_residual is not None
    assert sol.omega == cpu.omega and sol.accel_step == 60
    s32 = _manufactured_solver(gpu, torch.float32, "chebyshev")
    s32.run(60)
    assert _same_bits(s32.u.cpu(), _torch_iterate(torch.float32, 60))
    _check_convergence(gpu, 16, 16, 200, 1e-12, 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_accel_graph_request_runs_eager(gpu, dtype):
    rows, cols = 37, 33 * NV[dtype]
    field, src = _global_problem(rows, cols, dtype)
    sols = []
    for graph in (True, False):
        sol = SlabJacobi(parallel.DistContext(device=gpu), rows, cols, dtype=dtype, check_every=10, accel="chebyshev")
        _setup(sol, field, src)
        if graph:
            sol.run(60, graph=True)
        else:
            for _ in range(60):
                sol.step()
        torch.cuda.synchronize()
        assert sol.iteration == 60 and sol.accel_step == 60 and sol._graphs == {}
        sols.append(sol)
    assert _same_bits(sols[0].u, sols[1].u) and sols[0].last_residual == sols[1].last_residual is not None
    plain = SlabJacobi(parallel.DistContext(device=gpu), rows, cols, dtype=dtype, check_every=10)
    _setup(plain, field, src)
    plain.run(60)
    assert not torch.equal(plain.u, sols[0].u)


# ---------------------------------------------------------------------------
# 12. peer halos: ranks sharing the one GPU, gloo control plane
# ---------------------------------------------------------------------------
def _peer_accel_worker(rank, world, port, rows, cols, iters, fp64, rhs, errq):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        ctx = parallel.init(device="cuda", backend="gloo")
        dt = torch.float64 if fp64 else torch.float32
        field, src = _global_problem(rows, cols, dt)
        sol = SlabJacobi(ctx, rows, cols, dtype=dt, check_every=10, halo="peer", accel="chebyshev")
        assert sol.transport == "xgmi-peer-signalled", sol.transport
        _setup(sol, field, src, rhs=rhs)
        sol.run(iters)
        torch.cuda.synchronize()
        sol.check_peer()
        got = sol.gather()
        res = sol.last_residual
        sol.run(10)  # the continuation keeps the sequence going
        got2 = sol.gather()
        res2 = sol.last_residual
        assert sol.accel_step == iters + 10
        sol.close()
        if ctx.rank == 0:
            one = SlabJacobi(parallel.DistContext(device=ctx.device), rows, cols, dtype=dt, check_every=10,
                             accel="chebyshev")
            _setup(one, field, src, rhs=rhs)
            one.run(iters)
            assert torch.equal(got.cpu(), one.owned.cpu()), "accelerated peer halos differ from one rank"
            assert res == one.last_residual and res is not None
            one.run(10)
            assert torch.equal(got2.cpu(), one.owned.cpu()) and res2 == one.last_residual
            assert one.omega == sol.omega
            plain = SlabJacobi(parallel.DistContext(device=ctx.device), rows, cols, dtype=dt, check_every=10)
            _setup(plain, field, src, rhs=rhs)
            plain.run(iters + 10)
            assert not torch.equal(plain.owned, one.owned)
        parallel.shutdown()
    except Exception:  # noqa: BLE001
        errq.put(f"rank {rank}: {traceback.format_exc()}")


@pytest.mark.gpu
@pytest.mark.parametrize("world,fp64,rhs", [(2, True, True), (3, False, False)])
def test_accel_peer_halos_equal_one_rank(gpu, world, fp64, rhs):
    """100 iterations plus a 10-iteration continuation, bit-identical to one
    rank, residual included; 8k+5 global rows."""
    _run_ranks(_peer_accel_worker, world, 8 * 9 + 5, 132 if fp64 else 136, 100, fp64, rhs)
