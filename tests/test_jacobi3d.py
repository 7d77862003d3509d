"""3-D Jacobi: the 7-point sweep kernels, the CPU library, the torch oracle and
SlabJacobi3D.

Contract (capi.h): u / un / rhs are (planes + 2, ny, nx), x fastest; a sweep of
planes [k0, k1) writes s = ((((zm + zp) + (ym + yp)) + (xm + xp)) [+ b]) * c,
c = 1/6 rounded once to the dtype, at interior points (p + omega * (s - p) with
``omega``), copies u through at boundary elements of the swept planes and
writes nothing else; the residual is max|s - u| over the swept interior points.

Every sweep comparison is on bit patterns against ``ref.jacobi3d``; ``un`` is
pre-filled with a sentinel outside the swept planes so stray writes show.
Tolerances of the solver tests: the manufactured problem's fixed point is u*
and the Jacobi iteration contracts by rho = (cos(pi/15) * 3) / 3 ~ 0.978 per
step, e^-44 over 2000 steps, so what remains is rounding: a few ulp of values
in [0, 1] (the torch expression gives 3.0e-15 plain, 2.2e-15 accelerated in
fp64, 5.6e-7 / 1.1e-6 in fp32); 1e-12 and 1e-5 keep the 2-D tests' margins.
"""

from __future__ import annotations

import ctypes
import functools
import json
import math
import os
import socket
import subprocess
import sys
import traceback

import pytest
import torch
import torch.multiprocessing as mp

from cuda_mpi_openmp_amd import _native, ops, parallel
from cuda_mpi_openmp_amd.models import SlabJacobi3D
from cuda_mpi_openmp_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.0  # u, p in [0, 1), b in [-1, 1), omega < 2: outputs lie far above -7
OMEGA = 1.7109375  # exact in fp32 too, so both dtypes take the same value
DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector
KINDS = ["laplace", "rhs", "omega", "both"]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


@functools.lru_cache(maxsize=None)
def _case(dtype, planes2: int, ny: int, nx: int):
    """Inputs and the full-range references on the CPU, computed once and never
    modified: u, b (NaN wherever the contract says it is not read), p, and per
    kind the sweep of planes [1, planes2 - 1) plus per-plane residuals. A
    sub-range sweep equals the same planes of the full-range one."""
    g = torch.Generator().manual_seed(9000 * nx + 10 * ny + planes2)
    u = torch.rand((planes2, ny, nx), generator=g, dtype=torch.float64).to(dtype)
    b = (torch.rand((planes2, ny, nx), generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dtype)
    p = torch.rand((planes2, ny, nx), generator=g, dtype=torch.float64).to(dtype)
    b[0] = b[-1] = float("nan")
    b[:, 0] = b[:, -1] = float("nan")
    b[:, :, 0] = b[:, :, -1] = float("nan")
    want, res = {}, {}
    for kind in KINDS:
        rhs = b if kind in ("rhs", "both") else None
        acc = kind in ("omega", "both")
        want[kind] = ref.jacobi3d(u, 1, planes2 - 1, keep_dtype=True, rhs=rhs, omega=OMEGA if acc else None,
                                  prev=p if acc else None)
        assert want[kind].dtype == dtype and not bool(torch.isnan(want[kind]).any())
        s = ref.jacobi3d(u, 1, planes2 - 1, keep_dtype=True, rhs=rhs)
        res[kind] = (s[1:-1, 1:-1, 1:-1] - u[1:-1, 1:-1, 1:-1]).abs().amax(dim=(1, 2))  # omega-independent
    return u, b, p, want, res


def _un_for(p: torch.Tensor, k0: int, k1: int) -> torch.Tensor:
    """un on entry: p in the swept planes (read only with omega), the sentinel elsewhere."""
    un = torch.full_like(p, SENT)
    un[k0:k1] = p[k0:k1]
    return un


def _expected_res(planeres: torch.Tensor, k0: int, k1: int) -> float:
    return float(planeres[k0 - 1:k1 - 1].max()) if k1 > k0 else 0.0


def _kw(kind: str, b):
    return dict(rhs=b if kind in ("rhs", "both") else None, omega=OMEGA if kind in ("omega", "both") else None)


def _assert_sweep(un, res, want, planeres, k0, k1, tag):
    assert _same_bits(un[k0:k1], want[k0:k1]), f"output differs: {tag}"
    assert bool((un[:k0] == SENT).all()) and bool((un[k1:] == SENT).all()), f"planes outside the range written: {tag}"
    if res is not None:
        got, exp = float(res), _expected_res(planeres, k0, k1)
        assert got == exp, f"residual {got!r} != {exp!r}: {tag}"


# ---------------------------------------------------------------------------
# 1. the oracle against an independent triple loop in Python floats
# ---------------------------------------------------------------------------
def test_oracle_equals_a_plain_triple_loop():
    u, b, p, _, _ = _case(torch.float64, 6, 4, 5)  # 4 owned planes of 4 x 5
    c = 1.0 / 6.0
    for kind in KINDS:
        kw = _kw(kind, b)
        got = ref.jacobi3d(u, 2, 5, prev=p if kw["omega"] else None, **kw)
        exp = u.clone()
        for z in range(2, 5):
            for y in range(1, 3):
                for x in range(1, 4):
                    zz = float(u[z - 1, y, x]) + float(u[z + 1, y, x])
                    yy = float(u[z, y - 1, x]) + float(u[z, y + 1, x])
                    xx = float(u[z, y, x - 1]) + float(u[z, y, x + 1])
                    n = (zz + yy) + xx
                    if kw["rhs"] is not None:
                        n = n + float(b[z, y, x])
                    s = n * c
                    if kw["omega"] is not None:
                        pv = float(p[z, y, x])
                        d = s - pv
                        t = OMEGA * d
                        s = pv + t
                    exp[z, y, x] = s
        assert _same_bits(got, exp), kind


# ---------------------------------------------------------------------------
# 2. CPU library == oracle, every plane range
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx", [(3, 3), (4, 5), (7, 64)])
def test_cpu_library_equals_the_oracle(ny, nx):
    u, b, p, want, res = _case(torch.float64, 7, ny, nx)  # 5 owned planes
    for kind in KINDS:
        kw = _kw(kind, b)
        for k0 in range(1, 7):
            for k1 in range(k0, 7):
                un = _un_for(p, k0, k1)
                r = ops.jacobi3d_sweep(u, un, k0, k1, **kw)
                _assert_sweep(un, r, want[kind], res[kind], k0, k1, (kind, ny, nx, k0, k1))
    # the resid tensor on the CPU accumulates the max
    acc = torch.tensor([0.5 * _expected_res(res["rhs"], 1, 6)], dtype=torch.float64)
    ops.jacobi3d_sweep(u, _un_for(p, 1, 6), 1, 6, resid=acc, rhs=b)
    assert float(acc) == _expected_res(res["rhs"], 1, 6)


# ---------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------
def test_ops_refusals():
    u = torch.zeros((5, 4, 6), dtype=torch.float64)
    un = torch.zeros_like(u)
    bad = [
        lambda: ops.jacobi3d_sweep(u[0], un[0], 1, 2),                                   # 2-D
        lambda: ops.jacobi3d_sweep(u, torch.zeros((5, 4, 7), dtype=torch.float64), 1, 2),  # shapes
        lambda: ops.jacobi3d_sweep(u, un.to(torch.float32), 1, 2),                        # dtypes
        lambda: ops.jacobi3d_sweep(u.transpose(1, 2), un.transpose(1, 2), 1, 2),          # non-contiguous
        lambda: ops.jacobi3d_sweep(u, un, 0, 2),
        lambda: ops.jacobi3d_sweep(u, un, 3, 2),
        lambda: ops.jacobi3d_sweep(u, un, 1, 5),
        lambda: ops.jacobi3d_sweep(u, un, 1, 2, rhs=torch.zeros((5, 4, 5), dtype=torch.float64)),
        lambda: ops.jacobi3d_sweep(u, un, 1, 2, rhs=torch.zeros((5, 4, 6), dtype=torch.float32)),
        lambda: ops.jacobi3d_sweep(u, un, 1, 2, rhs=torch.zeros((5, 6, 4), dtype=torch.float64).transpose(1, 2)),
        lambda: ops.jacobi3d_sweep(u, un, 1, 2, rhs=[0.0]),
        lambda: ops.jacobi3d_sweep(torch.zeros((5, 2, 6), dtype=torch.float64),
                                   torch.zeros((5, 2, 6), dtype=torch.float64), 1, 2),    # ny < 3
    ]
    for w in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        bad.append(lambda w=w: ops.jacobi3d_sweep(u, un, 1, 2, omega=w))
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert not bool(un.any()), i
    with pytest.raises(ValueError):
        ops.jacobi3d_sweep(u.to(torch.float32), un.to(torch.float32), 1, 2)  # the CPU reference is fp64
    # ops.jacobi_sweep keeps refusing volumes
    with pytest.raises(ValueError):
        ops.jacobi_sweep(u, un, 1, 2)
    with pytest.raises(ValueError):
        ref.jacobi3d(u, 1, 2, omega=1.5)  # omega and prev come together


def test_c_entries_refuse_before_touching_a_pointer():
    """Null pointers, bad geometry and bad omega: nonzero (GPU entries, which
    refuse before any launch, so this needs no device) or NaN (CPU functions),
    with un untouched. 0x10 stands for a pointer that must never be read."""
    L = _native.lib()
    un = torch.full((5, 4, 6), SENT, dtype=torch.float64)
    u = torch.zeros_like(un)
    up, np_, junk = u.data_ptr(), un.data_ptr(), 0x10
    geom = [(None, np_, 6, 4, 1, 2), (up, None, 6, 4, 1, 2), (up, np_, 2, 4, 1, 2), (up, np_, 6, 2, 1, 2),
            (up, np_, 6, 4, 0, 2), (up, np_, 6, 4, 3, 2), (up, np_, 65536, 32768, 1, 2)]
    for (a, o, nx, ny, k0, k1) in geom:
        for fn in (L.mpx_jacobi3d_f64, L.mpx_jacobi3d_f32):
            assert fn(junk if a else None, None, junk if o else None, nx, ny, k0, k1, None, None) != 0
        for fn in (L.mpx_jacobi3d_accel_f64, L.mpx_jacobi3d_accel_f32):
            assert fn(junk if a else None, None, junk if o else None, nx, ny, k0, k1, 1.5, None, None) != 0
        assert math.isnan(L.mpx_cpu_jacobi3d_f64(a, None, o, nx, ny, k0, k1))
        assert math.isnan(L.mpx_cpu_jacobi3d_accel_f64(a, None, o, nx, ny, k0, k1, 1.5))
    assert b"geometry" in L.mpx_last_error() or b"null" in L.mpx_last_error()
    for w in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert L.mpx_jacobi3d_accel_f64(junk, None, junk, 6, 4, 1, 2, w, None, None) != 0
        assert L.mpx_jacobi3d_accel_f32(junk, None, junk, 6, 4, 1, 2, w, None, None) != 0
        assert math.isnan(L.mpx_cpu_jacobi3d_accel_f64(up, None, np_, 6, 4, 1, 2, w))
    assert b"omega" in L.mpx_last_error()
    for w in (1e-60, 1e60):  # finite positive doubles that round to 0 / inf in fp32
        assert L.mpx_jacobi3d_accel_f32(junk, None, junk, 6, 4, 1, 2, w, None, None) != 0
    assert bool((un == SENT).all())
    out = _native.i32_array([0, 0, 0, 0])
    assert L.mpx_jacobi3d_tile(1, 0, 0, None) != 0 and L.mpx_jacobi3d_tile(1, 0, 0, out) == 0
    T = _native.tune_lib()
    for form, ty, kz in ((4, 4, 1), (-1, 4, 1), (0, 0, 1), (2, 4, 2), (1, 3, 4), (3, 4, 0)):
        assert T.mpx_jacobi3d_variant(1, junk, None, junk, 8, 4, 1, 2, 0, 1.0, None, form, ty, kz, None) != 0
    assert T.mpx_jacobi3d_variant(1, None, None, junk, 8, 4, 1, 2, 0, 1.0, None, 0, 4, 1, None) != 0
    assert T.mpx_jacobi3d_variant(1, junk, None, junk, 8, 4, 1, 2, 1, 0.0, None, 0, 4, 1, None) != 0
    assert T.mpx_jacobi3d_variant(1, junk, None, junk, 7, 4, 1, 2, 0, 1.0, None, 0, 4, 1, None) != 0  # not the vector layout


def test_solver_refusals():
    ctx = parallel.DistContext()
    with pytest.raises(ValueError):
        SlabJacobi3D(ctx, 4, 4, 4, accel="sor")
    with pytest.raises(ValueError, match="peer"):
        SlabJacobi3D(ctx, 4, 4, 4, halo="peer")
    with pytest.raises(ValueError):
        SlabJacobi3D(ctx, 4, 4, 4, halo="carrier-pigeon")
    with pytest.raises(ValueError):
        SlabJacobi3D(ctx, 4, 2, 4)
    sol = SlabJacobi3D(ctx, 4, 4, 5)
    with pytest.raises(ValueError):
        sol.set_rhs()
    with pytest.raises(ValueError):
        sol.set_rhs(tensor=torch.zeros((4, 4, 4)))


# ---------------------------------------------------------------------------
# 4. symbols
# ---------------------------------------------------------------------------
def test_symbols():
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    for name in ("mpx_jacobi3d_f64", "mpx_jacobi3d_f32", "mpx_jacobi3d_accel_f64", "mpx_jacobi3d_accel_f32",
                 "mpx_cpu_jacobi3d_f64", "mpx_cpu_jacobi3d_accel_f64", "mpx_jacobi3d_tile"):
        assert hasattr(raw, name), name
    assert hasattr(_native.tune_lib(), "mpx_jacobi3d_variant")
    assert not hasattr(raw, "mpx_jacobi3d_variant"), "mpx_jacobi3d_variant exported by libmpx"
    for dt in DTYPES:
        for rhs in (False, True):
            for accel in (False, True):
                t = ops.jacobi3d_tile(dt, rhs=rhs, accel=accel)
                assert t["form"] in (0, 1, 2, 3) and t["ty"] >= 1 and t["kz"] >= 1 and t["min_waves"] >= 1
                assert t["form"] & 1 or t["kz"] == 1  # the rows forms walk one plane
    with pytest.raises(ValueError):
        ops.jacobi3d_tile(torch.float16)


# ---------------------------------------------------------------------------
# 5 / 13. manufactured solution, 16^3
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _manufactured():
    """u* random on 16^3, faces included, and b = 6 u* - (sum of the six
    neighbours) in fp64: u* is the fixed point of the Poisson sweep."""
    g = torch.Generator().manual_seed(23)
    us = torch.rand((16, 16, 16), generator=g, dtype=torch.float64)
    i = slice(1, -1)
    b = torch.zeros_like(us)
    b[i, i, i] = 6.0 * us[i, i, i] - (((us[:-2, i, i] + us[2:, i, i]) + (us[i, :-2, i] + us[i, 2:, i]))
                                      + (us[i, i, :-2] + us[i, i, 2:]))
    return us, b


def _manufactured_solver(device, dtype, with_rhs: bool, accel=None) -> SlabJacobi3D:
    us, b = _manufactured()
    sol = SlabJacobi3D(parallel.DistContext(device=device), 14, 16, 16, dtype=dtype, check_every=10, accel=accel)
    start = us.clone()
    start[1:-1, 1:-1, 1:-1] = 0.0  # faces from u*, interior from 0
    sol.u.copy_(start.to(dtype))
    sol.un.copy_(sol.u)
    if with_rhs:
        sol.set_rhs(tensor=b[1:-1])
    return sol


def _omegas(rho: float, steps: int):
    """The Golub-Varga schedule, written out independently: None (plain), then
    1 / (1 - rho^2 / 2), then 1 / (1 - rho^2 w / 4)."""
    out, w = [], None
    for k in range(1, steps + 1):
        if k == 1:
            w = None
        elif k == 2:
            w = 1.0 / (1.0 - rho * rho / 2.0)
        else:
            w = 1.0 / (1.0 - rho * rho * w / 4.0)
        out.append(w)
    return out


RHO16 = (math.cos(math.pi / 15) + math.cos(math.pi / 15) + math.cos(math.pi / 15)) / 3.0


@functools.lru_cache(maxsize=None)
def _torch_iterate(dtype, iters: int, accel: bool) -> torch.Tensor:
    """The oracle iterated on the manufactured problem (rhs, optionally Chebyshev)."""
    us, b = _manufactured()
    u = us.clone()
    u[1:-1, 1:-1, 1:-1] = 0.0
    u, bb = u.to(dtype), b.to(dtype)
    prev = u.clone()
    for w in (_omegas(RHO16, iters) if accel else [None] * iters):
        nxt = ref.jacobi3d(u, 1, 15, keep_dtype=True, rhs=bb, omega=w, prev=prev if w is not None else None)
        prev, u = u, nxt
    return u


def _check_manufactured_fp64(device):
    us, _ = _manufactured()
    sol = _manufactured_solver(device, torch.float64, True)
    sol.run(2000)
    err = float((sol.u.cpu() - us).abs().max())
    print(f"manufactured 16^3 fp64 on {device}: 2000 plain steps, error {err:.3e}, residual {sol.last_residual:.3e}")
    assert err <= 1e-12, err
    assert sol.last_residual is not None and sol.last_residual <= 1e-12, sol.last_residual
    acc = _manufactured_solver(device, torch.float64, True, accel="chebyshev")
    acc.run(200)
    err = float((acc.u.cpu() - us).abs().max())
    print(f"manufactured 16^3 fp64 on {device}: 200 Chebyshev steps, error {err:.3e}")
    assert err <= 1e-12, err
    lap = _manufactured_solver(device, torch.float64, False)
    lap.run(2000)
    assert float((lap.u.cpu() - us).abs().max()) > 1e-2, "the faces alone must not give u*"


def test_manufactured_solution_cpu():
    _check_manufactured_fp64(torch.device("cpu"))
    for accel in (False, True):
        sol = _manufactured_solver(torch.device("cpu"), torch.float64, True, accel="chebyshev" if accel else None)
        sol.run(50)
        assert _same_bits(sol.u, _torch_iterate(torch.float64, 50, accel)), accel


# ---------------------------------------------------------------------------
# 6. three gloo CPU ranks, checkpoint in the middle, against one rank
# ---------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _global_problem(planes, ny, nx, dtype=torch.float64):
    g = torch.Generator().manual_seed(37)
    field = torch.rand((planes, ny - 2, nx - 2), generator=g, dtype=torch.float64).to(dtype)
    src = (torch.rand((planes, ny, nx), generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dtype)
    return field, src


def _setup(sol, field, src, rhs=True):
    sol.set_boundary(z0=1.0, z1=0.125, y0=0.5, y1=0.75, x0=0.25, x1=0.375)
    s = sol.slab
    sol.fill(fn=lambda z, y, x: field[s.row0:s.row0 + s.rows])
    if rhs:
        sol.set_rhs(tensor=src[s.row0:s.row0 + s.rows])


def _cpu_ckpt_worker(rank, world, port, planes, ny, nx, ckdir, errq):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        ctx = parallel.init(device="cpu")
        field, src = _global_problem(planes, ny, nx)
        mk = lambda c, **kw: SlabJacobi3D(c, planes, ny, nx, check_every=5, **kw)  # noqa: E731
        a = mk(ctx, accel="chebyshev")
        assert [a.slab.rows_of(r) for r in range(world)] == [4, 4, 3]
        _setup(a, field, src)
        a.run(10)
        a.save_checkpoint(os.path.join(ckdir, "ck"))
        ck = torch.load(os.path.join(ckdir, f"ck.rank{rank}.pt"), weights_only=True)
        assert torch.equal(ck["rhs"], a.rhs) and torch.equal(ck["u_prev"], a.un) and ck["accel"]["step"] == 10
        b = mk(ctx, accel="chebyshev")  # a fresh solver: nothing but the checkpoint
        b.load_checkpoint(os.path.join(ckdir, "ck"))
        assert b.iteration == 10 and b.accel_step == 10 and b.omega == a.omega
        b.run(15)
        got, res = b.gather(), b.last_residual
        if ctx.rank == 0:
            one = mk(parallel.DistContext(), accel="chebyshev")
            _setup(one, field, src)
            one.run(25)
            assert _same_bits(got, one.owned), "three ranks differ from one rank"
            assert res == one.last_residual and res is not None
            lap = mk(parallel.DistContext(), accel="chebyshev")
            _setup(lap, field, src, rhs=False)
            lap.run(25)
            assert not torch.equal(lap.owned, one.owned)
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
    _run_ranks(_cpu_ckpt_worker, 3, 11, 6, 8, str(tmp_path))


# ---------------------------------------------------------------------------
# 7. the Chebyshev schedule
# ---------------------------------------------------------------------------
def test_schedule_and_restarts(tmp_path):
    ctx = parallel.DistContext()
    sol = SlabJacobi3D(ctx, 9, 7, 12, accel="chebyshev", check_every=1)
    rho = (math.cos(math.pi / 10) + math.cos(math.pi / 6) + math.cos(math.pi / 11)) / 3.0
    assert sol.rho == rho
    assert SlabJacobi3D(ctx, 9, 7, 12).rho is None
    field, src = _global_problem(9, 7, 12)
    _setup(sol, field, src)

    def assert_next_step_is_plain(tag):
        assert sol.accel_step == 0 and sol.omega is None, tag
        sol.sync_halos()
        sol.un[1:-1].fill_(123.0)  # a plain step must ignore whatever un's owned planes hold
        before = sol.u.clone()
        sol.step()
        assert sol.omega == 1.0 and sol.accel_step == 1, tag
        assert _same_bits(sol.u, ref.jacobi3d(before, 1, 10, rhs=sol.rhs)), tag

    assert_next_step_is_plain("first step")
    want = _omegas(rho, 6)
    for k in range(2, 7):
        prev, cur = sol.un.clone(), sol.u.clone()
        sol.step()
        assert sol.omega == want[k - 1] and sol.accel_step == k
        assert _same_bits(sol.u, ref.jacobi3d(cur, 1, 10, rhs=sol.rhs, omega=want[k - 1], prev=prev)), k
    s = sol.slab
    sol.fill(fn=lambda z, y, x: field[s.row0:s.row0 + s.rows])
    assert_next_step_is_plain("fill")
    sol.step()
    sol.set_boundary(z0=0.5)
    assert_next_step_is_plain("set_boundary")
    sol.step()
    sol.set_rhs(tensor=src * 0.5)
    assert_next_step_is_plain("set_rhs")
    sol.step()
    sol.restart_acceleration()
    assert_next_step_is_plain("restart_acceleration")
    # a checkpoint written by a solver without acceleration carries no history
    plain = SlabJacobi3D(ctx, 9, 7, 12)
    _setup(plain, field, src)
    plain.run(3)
    plain.save_checkpoint(str(tmp_path / "plain"))
    sol.step()
    sol.load_checkpoint(str(tmp_path / "plain"))
    assert sol.iteration == 3 and _same_bits(sol.u, plain.u)
    assert_next_step_is_plain("reload without history")


# ---------------------------------------------------------------------------
# 8. the bench tool
# ---------------------------------------------------------------------------
def test_bench_tool_two_cpu_ranks():
    cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_jacobi3d.py"), "--device", "cpu", "--gpus", "2",
           "--size", "12", "--iters", "6", "--warmup", "2", "--rhs", "--accel"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert rec["verified"] is True and rec["n_gpus"] == 2 and rec["dims"] == [12, 12, 12]
    assert rec["rhs"] is True and rec["accel"] == "chebyshev" and rec["words_per_point"] == 4
    assert rec["value"] > 0 and rec["gpoints_per_s"] > 0 and rec["TBps_effective"] > 0
    assert rec["transport"] == "torch.distributed"


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _gpu_case(gpu, dtype, planes2, ny, nx):
    u, b, p, want, res = _case(dtype, planes2, ny, nx)
    return u.to(gpu), b.to(gpu), p.to(gpu), want, res


def _gpu_sweep_check(gpu, dtype, planes2, ny, nx, k0, k1, kinds=KINDS, tag=()):
    u, b, p, want, res = _gpu_case(gpu, dtype, planes2, ny, nx)
    for kind in kinds:
        un = _un_for(p, k0, k1)
        r = torch.zeros(1, dtype=dtype, device=gpu)
        ops.jacobi3d_sweep(u, un, k0, k1, resid=r, **_kw(kind, b))
        _assert_sweep(un.cpu(), r.cpu(), want[kind], res[kind], k0, k1, (kind, dtype, ny, nx, k0, k1) + tuple(tag))
        un = _un_for(p, k0, k1)
        ops.jacobi3d_sweep(u, un, k0, k1, **_kw(kind, b))  # without the residual word
        _assert_sweep(un.cpu(), None, want[kind], res[kind], k0, k1, (kind, dtype, ny, nx, k0, k1, "no resid"))


# 9. x edges of the wave path through the production launcher. One vector of
# fp64 is 2 columns, below the contract's nx >= 3, so that width exists in fp32 only.
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,nvec", [(dt, v) for dt in DTYPES for v in (1, 2, 61, 62, 63, 124, 125)
                                        if v * NV[dt] >= 3])
def test_wave_path_x_edges(gpu, dtype, nvec):
    _gpu_sweep_check(gpu, dtype, 6, 6, nvec * NV[dtype], 1, 5)


# 10. every tile tail through the variant entry, production form and tile of the kind
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["laplace", "both"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_production_tile_every_tail(gpu, dtype, kind):
    """Interior rows 1 .. 3 TY, swept planes 1 .. 2 KZ + 1 from k0 = 1 and 2, with
    and without the residual word, two strips with the last one partial."""
    t = ops.jacobi3d_tile(dtype, rhs=kind == "both", accel=kind == "both")
    form, ty, kz = t["form"], t["ty"], t["kz"]
    nx = (62 + 5) * NV[dtype]  # two strips, the last one partial
    T = _native.tune_lib()
    f64 = int(dtype == torch.float64)
    nplanes = 2 * kz + 1
    planes2 = nplanes + 3  # k0 = 2 with nplanes swept planes still leaves a halo plane
    r_all = torch.zeros(1, dtype=dtype, device=gpu)
    for rows in range(1, 3 * ty + 1):
        ny = rows + 2
        u, b, p, want, res = _gpu_case(gpu, dtype, planes2, ny, nx)
        flags, tags = [], []
        kw = _kw(kind, b)
        wd = want[kind].to(gpu)
        for k0 in (1, 2):
            for n in range(1, nplanes + 1):
                k1 = k0 + n
                for with_res in (True, False):
                    un = _un_for(p, k0, k1)
                    r_all.zero_()
                    _native.check(T.mpx_jacobi3d_variant(
                        f64, u.data_ptr(), None if kw["rhs"] is None else b.data_ptr(), un.data_ptr(), nx, ny, k0,
                        k1, int(kw["omega"] is not None), kw["omega"] or 1.0,
                        r_all.data_ptr() if with_res else None, form, ty, kz, _native.stream_of(u)))
                    ok = (_bits(un[k0:k1]) == _bits(wd[k0:k1])).all() & (un[:k0] == SENT).all() \
                        & (un[k1:] == SENT).all()
                    if with_res:
                        ok = ok & (r_all[0] == _expected_res(res[kind], k0, k1))
                    flags.append(ok)
                    tags.append((kind, rows, k0, k1, with_res))
        got = torch.stack(flags).cpu()
        assert bool(got.all()), [tags[i] for i in torch.nonzero(~got).flatten().tolist()[:8]]


# 11. generic kernels
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_generic_kernels(gpu, dtype):
    for nx in (3, 5, 255, 257):
        _gpu_sweep_check(gpu, dtype, 6, 6, nx, 2, 5)
    # an aligned width on a base pointer offset by one element, then only rhs misaligned
    nx, ny, planes2 = 16 * NV[dtype], 5, 5
    u, b, p, want, res = _case(dtype, planes2, ny, nx)

    def shifted(t, off):
        flat = torch.empty(t.numel() + 4, dtype=dtype, device=gpu)
        v = flat[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and (v.data_ptr() % 16 != 0) == (off % NV[dtype] != 0)
        return v

    for offs in ((1, 1, 1), (0, 1, 0)):  # (u and un, rhs, p)
        ud, bd = shifted(u, offs[0]), shifted(b, offs[1])
        for kind in KINDS:
            if offs == (0, 1, 0) and kind in ("laplace", "omega"):
                continue  # no rhs in these: nothing would be misaligned
            un = shifted(_un_for(p, 1, 4), offs[0])
            r = torch.zeros(1, dtype=dtype, device=gpu)
            ops.jacobi3d_sweep(ud, un, 1, 4, resid=r, **_kw(kind, bd))
            _assert_sweep(un.cpu(), r.cpu(), want[kind], res[kind], 1, 4, (kind, dtype, offs))


# 12. one production-launcher case per tile that selects the full production tile
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["laplace", "both"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_production_launcher_full_tile(gpu, dtype, kind):
    """The launcher halves its tile while the launch has fewer than min_waves
    waves; waves = strips * ceil(ny / ty) * ceil(planes / kz). One narrow strip
    (two vectors, the narrowest width both dtypes allow) and a partial last
    tile in y and z, with just enough row tiles and z blocks for min_waves
    waves at the full tile: at most 8.4 MB per buffer."""
    t = ops.jacobi3d_tile(dtype, rhs=kind == "both", accel=kind == "both")
    ty, kz, mw = t["ty"], t["kz"], t["min_waves"]
    nx = 2 * NV[dtype]
    ytiles = 64 if kz == 1 else 16
    ny = ytiles * ty - 1
    zblocks = (mw + ytiles - 1) // ytiles + 1
    planes = zblocks * kz - (1 if kz > 1 else 0)
    assert ((ny + ty - 1) // ty) * ((planes + kz - 1) // kz) >= mw
    if ty > 1:
        assert ((ny + ty // 2 - 1) // (ty // 2)) * ((planes + kz - 1) // kz) >= mw  # not by a halved tile either
    assert (planes + 2) * ny * nx * (8 if dtype == torch.float64 else 4) < 16 << 20
    _gpu_sweep_check(gpu, dtype, planes + 2, ny, nx, 1, planes + 1, kinds=(kind,))


# 13. SlabJacobi3D on one device
@pytest.mark.gpu
def test_manufactured_solution_gpu(gpu):
    _check_manufactured_fp64(gpu)
    us, _ = _manufactured()
    for dtype in DTYPES:
        sol = _manufactured_solver(gpu, dtype, True, accel="chebyshev")
        sol.run(50)
        assert _same_bits(sol.u.cpu(), _torch_iterate(dtype, 50, True)), dtype  # the sharp check
    for accel in (None, "chebyshev"):
        sol = _manufactured_solver(gpu, torch.float32, True, accel=accel)
        sol.run(1000)
        err = float((sol.u.cpu().to(torch.float64) - us).abs().max())
        print(f"manufactured 16^3 fp32 on the GPU, accel={accel}: 1000 steps, error {err:.3e}")
        assert err <= 1e-5, (accel, err)


# 14. two and three ranks sharing the one GPU over the gloo control plane
def _gpu_ranks_worker(rank, world, port, planes, ny, nx, iters, fp64, errq):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        ctx = parallel.init(device="cuda", backend="gloo")
        dt = torch.float64 if fp64 else torch.float32
        field, src = _global_problem(planes, ny, nx, dt)
        sol = SlabJacobi3D(ctx, planes, ny, nx, dtype=dt, check_every=10, halo="rccl", accel="chebyshev")
        assert sol.transport == "torch.distributed", sol.transport
        _setup(sol, field, src)
        sol.run(iters)
        torch.cuda.synchronize()
        got, res = sol.gather(), sol.last_residual
        if ctx.rank == 0:
            one = SlabJacobi3D(parallel.DistContext(device=ctx.device), planes, ny, nx, dtype=dt, check_every=10,
                               accel="chebyshev")
            _setup(one, field, src)
            one.run(iters)
            assert _same_bits(got.cpu(), one.owned.cpu()), "ranks sharing the GPU differ from one rank"
            assert res == one.last_residual and res is not None
        parallel.shutdown()
    except Exception:  # noqa: BLE001
        errq.put(f"rank {rank}: {traceback.format_exc()}")


@pytest.mark.gpu
@pytest.mark.parametrize("world,fp64", [(2, True), (3, False)])
def test_ranks_sharing_the_gpu_equal_one_rank(gpu, world, fp64):
    """20 steps with rhs + Chebyshev, uneven planes (13 over 2 or 3 ranks), a
    wave-path width: bit-identical to one rank, residual included."""
    _run_ranks(_gpu_ranks_worker, world, 13, 9, 72, 20, fp64, timeout=120)
