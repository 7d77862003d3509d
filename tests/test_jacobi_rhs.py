"""The Poisson source term of the Jacobi tier, from the kernels to SlabJacobi.

With a right-hand side b (u's shape; b = h^2 f for -Laplace(u) = f) a sweep is

    un = (((up + down) + (left + right)) + b) * 0.25

four correctly rounded adds in this association and an exact scale, so GPU
fp32, GPU fp64, the CPU library and the dtype-preserving torch expression
(``ref.jacobi(..., keep_dtype=True, rhs=b)``) agree bit for bit; no kernel
comparison here carries a tolerance. The sentinel method is the one of
test_jacobi_kernels.py: ``un`` is pre-filled with -7, rows [r0, r1) must equal
the reference, every other row must still hold the sentinel, and the residual
word must equal the maximum of the per-row reference residuals.

b is drawn per element from a seeded generator, so a ring slot holding the
wrong row of b cannot pass. Its halo rows (0 and height - 1) and boundary
columns are NaN: they are don't-care and must reach no output and no residual.
"""

from __future__ import annotations

import ctypes
import functools
import os
import socket
import traceback

import pytest
import torch
import torch.multiprocessing as mp

from cuda_mpi_openmp_amd import _native, ops, parallel
from cuda_mpi_openmp_amd.models import SlabJacobi
from cuda_mpi_openmp_amd.ops import reference as ref

SENT = -7.0  # u in [0, 1), b in [-1, 1): outputs lie in [-0.25, 1.25]
# uniform: u on [0, 1), b on [-1, 1). flat: u on [0.5, 0.5 + 2^-10), b on
# [-2^-10, 2^-10): every true difference stays around 2^-10 or below, while a
# difference taken by a lane or row that owns no output is near 0.125.
FIELDS = {"uniform": dict(scale=1.0, offset=0.0), "flat": dict(scale=2.0 ** -10, offset=0.5)}
DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


@functools.lru_cache(maxsize=None)
def _case(dtype, height: int, cols: int, field: str = "uniform"):
    """(u, b, full-height reference, per-row residuals) on the CPU, computed
    once and never modified. rowres[k] is max_j |s - c| of row k + 1."""
    kw = FIELDS[field]
    g = torch.Generator().manual_seed(7000 * cols + 10 * height + len(field))
    u = (torch.rand((height, cols), generator=g, dtype=torch.float64) * kw["scale"] + kw["offset"]).to(dtype)
    b = ((torch.rand((height, cols), generator=g, dtype=torch.float64) * 2.0 - 1.0) * kw["scale"]).to(dtype)
    b[0] = b[-1] = float("nan")  # don't-care: halo rows and boundary columns of b
    b[:, 0] = b[:, -1] = float("nan")
    want = ref.jacobi(u, 1, height - 1, keep_dtype=True, rhs=b)
    assert want.dtype == dtype and not bool(torch.isnan(want).any())
    if cols > 2:
        rowres = (want[1:-1, 1:-1] - u[1:-1, 1:-1]).abs().amax(dim=1)
    else:
        rowres = torch.zeros(height - 2, dtype=dtype)
    return u, b, want, rowres


def _expected_res(rowres: torch.Tensor, r0: int, r1: int) -> float:
    return float(rowres[r0 - 1:r1 - 1].max()) if r1 > r0 else 0.0


def _assert_sweep(un, res, want, rowres, r0, r1, tag):
    """The three assertions of a sweep of [r0, r1) into a sentinel-filled un."""
    assert _same_bits(un[r0:r1], want[r0:r1]), f"output differs: {tag}"
    assert bool((un[:r0] == SENT).all()) and bool((un[r1:] == SENT).all()), f"rows outside the range written: {tag}"
    if res is not None:
        got, exp = float(res.item()), _expected_res(rowres, r0, r1)
        assert got == exp, f"residual {got!r} != {exp!r}: {tag}"


def _abi(u, b, un, cols, pitch, r0, r1, res):
    L = _native.lib()
    fn = L.mpx_jacobi_rhs_f64 if u.dtype == torch.float64 else L.mpx_jacobi_rhs_f32
    _native.check(fn(u.data_ptr(), b.data_ptr(), un.data_ptr(), cols, pitch, r0, r1,
                     None if res is None else res.data_ptr(), _native.stream_of(u)))


def _variant(u, b, un, cols, pitch, r0, r1, res, R, nt):
    _native.check(_native.tune_lib().mpx_jacobi_rhs_variant(
        u.data_ptr(), b.data_ptr(), un.data_ptr(), cols, pitch, r0, r1, None if res is None else res.data_ptr(),
        int(u.dtype == torch.float64), R, nt, _native.stream_of(u)))


# ---------------------------------------------------------------------------
# 1. CPU library and ops.jacobi_sweep on CPU tensors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [3, 5, 64])
def test_cpu_library_equals_the_torch_expression(cols):
    height = 20
    u, b, want, rowres = _case(torch.float64, height, cols)
    L = _native.lib()
    for r0, r1 in ((1, height - 1), (1, 2), (4, 11), (height - 2, height - 1), (6, 6)):
        un = torch.full_like(u, SENT)
        r = L.mpx_cpu_jacobi_rhs_f64(u.data_ptr(), b.data_ptr(), un.data_ptr(), cols, cols, r0, r1)
        _assert_sweep(un, None, want, rowres, r0, r1, (cols, r0, r1))
        assert r == _expected_res(rowres, r0, r1), (cols, r0, r1)
        un2 = torch.full_like(u, SENT)
        res = torch.zeros(1, dtype=torch.float64)
        r2 = ops.jacobi_sweep(u.clone(), un2, r0, r1, res, rhs=b.clone())
        assert r2 == r
        _assert_sweep(un2, res, want, rowres, r0, r1, ("ops", cols, r0, r1))


@pytest.mark.parametrize("cols,pad", [(5, 1), (64, 3)])
def test_cpu_library_pitch_wider_than_cols(cols, pad):
    """NaN in the padding of u and b reaches nothing; un's padding keeps the sentinel."""
    height, pitch = 20, cols + pad
    u, b, want, rowres = _case(torch.float64, height, cols)
    up = torch.full((height, pitch), float("nan"), dtype=torch.float64)
    bp = torch.full((height, pitch), float("nan"), dtype=torch.float64)
    up[:, :cols] = u
    bp[:, :cols] = b
    for r0, r1 in ((1, height - 1), (3, 9)):
        un = torch.full_like(up, SENT)
        r = _native.lib().mpx_cpu_jacobi_rhs_f64(up.data_ptr(), bp.data_ptr(), un.data_ptr(), cols, pitch, r0, r1)
        assert bool((un[:, cols:] == SENT).all()) and not bool(torch.isnan(un).any())
        _assert_sweep(un[:, :cols], None, want, rowres, r0, r1, (cols, pitch, r0, r1))
        assert r == _expected_res(rowres, r0, r1)


# ---------------------------------------------------------------------------
# 2. a zero right-hand side is the Laplace sweep
# ---------------------------------------------------------------------------
def test_zero_rhs_equals_the_laplace_sweep():
    for cols in (3, 5, 64):
        u, _, _, _ = _case(torch.float64, 20, cols)  # non-negative: no -0 + 0 case
        lap, poi = torch.full_like(u, SENT), torch.full_like(u, SENT)
        r_lap = ops.jacobi_sweep(u, lap, 1, 19)
        r_poi = ops.jacobi_sweep(u, poi, 1, 19, rhs=torch.zeros_like(u))
        assert torch.equal(lap, poi) and r_lap == r_poi
        assert torch.equal(ref.jacobi(u, 1, 19), ref.jacobi(u, 1, 19, rhs=torch.zeros_like(u)))


# ---------------------------------------------------------------------------
# 3. argument errors, symbol visibility
# ---------------------------------------------------------------------------
def test_argument_errors():
    u = torch.zeros((6, 8), dtype=torch.float64)
    un = torch.full_like(u, SENT)
    with pytest.raises(ValueError):
        ops.jacobi_sweep(u, un, 1, 5, rhs=torch.zeros((6, 7), dtype=torch.float64))  # shape
    with pytest.raises(ValueError):
        ops.jacobi_sweep(u, un, 1, 5, rhs=torch.zeros((6, 8), dtype=torch.float32))  # dtype
    with pytest.raises(ValueError):
        ops.jacobi_sweep(u, un, 1, 5, rhs=torch.zeros((6, 8), dtype=torch.float64, device="meta"))  # device
    with pytest.raises(ValueError):
        ops.jacobi_sweep(u, un, 1, 5, rhs=torch.zeros((8, 6), dtype=torch.float64).t())  # not contiguous
    assert bool((un == SENT).all())
    L = _native.lib()
    # a null b is refused before anything is launched or dereferenced
    assert L.mpx_jacobi_rhs_f64(u.data_ptr(), None, un.data_ptr(), 8, 8, 1, 5, None, None) != 0
    assert L.mpx_jacobi_rhs_f32(u.data_ptr(), None, un.data_ptr(), 8, 8, 1, 5, None, None) != 0
    with pytest.raises(_native.MpxError):
        _native.check(L.mpx_jacobi_rhs_f64(u.data_ptr(), None, un.data_ptr(), 8, 8, 1, 5, None, None))
    assert L.mpx_jacobi_peer_sweep_rhs(1, u.data_ptr(), u.data_ptr(), un.data_ptr(), 8, 8, 4, None, None, None) != 0
    sol = SlabJacobi(parallel.DistContext(), 4, 8)
    with pytest.raises(ValueError):
        sol.set_rhs()
    with pytest.raises(ValueError):
        sol.set_rhs(tensor=torch.zeros((6, 8), dtype=torch.float64))  # buffer rows, not owned rows
    assert sol.rhs is None


def test_set_rhs_fn_follows_fill_conventions():
    """fn(global_row_index, col_index) over the interior columns; the tensor
    form takes the owned rows; a second call overwrites the same buffer."""
    rows, cols = 6, 9
    a = SlabJacobi(parallel.DistContext(), rows, cols)
    a.set_rhs(fn=lambda r, c: (100 * r + c).to(torch.float64) * 0.125)
    want = torch.zeros((rows + 2, cols), dtype=torch.float64)
    for i in range(rows):
        for j in range(1, cols - 1):
            want[1 + i, j] = (100 * i + j) * 0.125
    assert a.rhs.shape == a.u.shape and torch.equal(a.rhs, want)
    b = SlabJacobi(parallel.DistContext(), rows, cols)
    b.set_rhs(tensor=want[1:-1])
    assert torch.equal(b.rhs, want)
    buf = a.rhs
    a.set_rhs(tensor=torch.ones((rows, cols), dtype=torch.float64))
    assert a.rhs is buf and bool((a.rhs[1:-1] == 1.0).all()) and bool((a.rhs[0] == 0.0).all())
    for sol in (a, b):
        sol.fill(seed=2)
    a.set_rhs(tensor=want[1:-1])
    a.run(7)
    b.run(7)
    assert torch.equal(a.u, b.u)


def test_rhs_variant_is_a_tuning_entry_only():
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    assert hasattr(_native.tune_lib(), "mpx_jacobi_rhs_variant")
    assert not hasattr(raw, "mpx_jacobi_rhs_variant"), "mpx_jacobi_rhs_variant exported by libmpx"
    for name in ("mpx_jacobi_rhs_f64", "mpx_jacobi_rhs_f32", "mpx_jacobi_peer_sweep_rhs", "mpx_cpu_jacobi_rhs_f64"):
        assert hasattr(raw, name), name
    assert _native.tune_lib().mpx_jacobi_rhs_variant(None, None, None, 8, 8, 1, 5, None, 1, 1, 0, None) != 0


# ---------------------------------------------------------------------------
# 4 / 11. manufactured solution through SlabJacobi
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _manufactured():
    """u* random on a 16 x 16 grid (14 owned rows), boundary included, and
    b = 4 u* - (sum of the neighbours) in fp64: u* is the fixed point."""
    g = torch.Generator().manual_seed(20)
    us = torch.rand((16, 16), generator=g, dtype=torch.float64)
    b = torch.zeros_like(us)
    b[1:-1, 1:-1] = 4.0 * us[1:-1, 1:-1] - ((us[:-2, 1:-1] + us[2:, 1:-1]) + (us[1:-1, :-2] + us[1:-1, 2:]))
    return us, b


def _manufactured_solver(device, dtype, with_rhs: bool) -> SlabJacobi:
    us, b = _manufactured()
    sol = SlabJacobi(parallel.DistContext(device=device), 14, 16, dtype=dtype, check_every=10)
    start = us.clone()
    start[1:-1, 1:-1] = 0.0  # boundary from u*, interior from 0
    sol.u.copy_(start.to(dtype))
    sol.un.copy_(sol.u)
    if with_rhs:
        sol.set_rhs(tensor=b[1:-1])
    return sol


def _torch_iterate(dtype, iters: int) -> torch.Tensor:
    us, b = _manufactured()
    u = us.clone()
    u[1:-1, 1:-1] = 0.0
    u, bb = u.to(dtype), b.to(dtype)
    for _ in range(iters):
        u = ref.jacobi(u, 1, 15, keep_dtype=True, rhs=bb)
    return u


def _check_manufactured_fp64(device):
    us, _ = _manufactured()
    sol = _manufactured_solver(device, torch.float64, True)
    sol.run(2000)
    err = float((sol.u.cpu() - us).abs().max())
    # spectral radius cos(pi / 15) ~ 0.978: 2000 iterations contract by ~e^-44
    assert err <= 1e-12, err
    assert sol.last_residual is not None and sol.last_residual <= 1e-12, sol.last_residual
    lap = _manufactured_solver(device, torch.float64, False)
    lap.run(2000)
    assert float((lap.u.cpu() - us).abs().max()) > 1e-2, "the boundary alone must not give u*"


def test_manufactured_solution_cpu():
    _check_manufactured_fp64(torch.device("cpu"))
    sol = _manufactured_solver(torch.device("cpu"), torch.float64, True)
    sol.run(50)
    assert _same_bits(sol.u, _torch_iterate(torch.float64, 50))


@pytest.mark.gpu
def test_manufactured_solution_gpu(gpu):
    _check_manufactured_fp64(gpu)
    us, _ = _manufactured()
    for dtype in DTYPES:
        sol = _manufactured_solver(gpu, dtype, True)
        sol.run(50)
        assert _same_bits(sol.u.cpu(), _torch_iterate(dtype, 50)), dtype  # the sharp check
    # fp32 from the 50-iteration state on: 1000 iterations in all
    sol.run(950)
    assert sol.iteration == 1000
    err = float((sol.u.cpu().to(torch.float64) - us).abs().max())
    assert err <= 1e-5, err  # the torch fp32 iteration stalls at 7.7e-7


# ---------------------------------------------------------------------------
# 5. three gloo CPU ranks, checkpoint in the middle, against one rank
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
        a = SlabJacobi(ctx, rows, cols, check_every=5)
        _setup(a, field, src)
        a.run(10)
        a.save_checkpoint(os.path.join(ckdir, "ck"))
        ck = torch.load(os.path.join(ckdir, f"ck.rank{rank}.pt"), weights_only=True)
        assert "rhs" in ck and torch.equal(ck["rhs"], a.rhs)
        b = SlabJacobi(ctx, rows, cols, check_every=5)  # set_rhs is never called on this one
        b.set_boundary(top=1.0, left=0.5, right=0.25)
        b.load_checkpoint(os.path.join(ckdir, "ck"))
        assert b.rhs is not None and torch.equal(b.rhs, a.rhs) and b.iteration == 10
        b.run(15)
        got, res = b.gather(), b.last_residual
        # a checkpoint without an rhs leaves the solver's rhs alone
        c = SlabJacobi(ctx, rows, cols, check_every=5)
        _setup(c, field, src, rhs=False)
        c.save_checkpoint(os.path.join(ckdir, "lap"))
        assert "rhs" not in torch.load(os.path.join(ckdir, f"lap.rank{rank}.pt"), weights_only=True)
        b.load_checkpoint(os.path.join(ckdir, "lap"))
        assert b.rhs is not None and torch.equal(b.rhs, a.rhs)
        if ctx.rank == 0:
            one = SlabJacobi(parallel.DistContext(), rows, cols, check_every=5)
            _setup(one, field, src)
            one.run(25)
            assert torch.equal(got, one.owned), "three ranks with an rhs differ from one rank"
            assert res == one.last_residual and res is not None
            lap = SlabJacobi(parallel.DistContext(), rows, cols, check_every=5)
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
    _run_ranks(_cpu_ckpt_worker, 3, 8 * 3 + 5, 19, str(tmp_path))


# ---------------------------------------------------------------------------
# 6. every row-block shape of the production template (RHS = true)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rhs_production_template_every_row_block(gpu, dtype):
    """Row counts 1..3R put the tail (1..R rows) in block 0 (walking down),
    block 1 (walking up) and block 2 (down again); both fields, with and
    without the residual word, and the non-temporal form of the b loads."""
    cols = 129 * NV[dtype]  # three strips, the last one partial
    height = 54
    launches = 0
    for field in FIELDS:
        u, b, want, rowres = _case(dtype, height, cols, field)
        ud, bd, wd = u.to(gpu), b.to(gpu), want.to(gpu)
        un = torch.empty_like(ud)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        for R in (1, 2, 3, 5, 8):
            for r0 in (1, 2):
                for n in range(1, 3 * R + 1):
                    r1 = r0 + n
                    assert r1 <= height - 1
                    for with_res, nt in ((True, 0), (False, 0), (True, 1)):
                        un.fill_(SENT)
                        res.zero_()
                        _variant(ud, bd, un, cols, cols, r0, r1, res if with_res else None, R, nt)
                        _assert_sweep(un, res if with_res else None, wd, rowres, r0, r1,
                                      (dtype, field, R, r0, r1, with_res, nt))
                        launches += 1
    assert launches == 2 * 2 * 3 * 3 * (1 + 2 + 3 + 5 + 8)


# ---------------------------------------------------------------------------
# 7. column edges of the wave path (production launch)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rhs_wave_path_column_edges(gpu, dtype):
    rows = 9
    for nvec in (1, 2, 61, 62, 63, 124, 125):
        cols = nvec * NV[dtype]
        for field in FIELDS:
            u, b, want, rowres = _case(dtype, rows + 2, cols, field)
            ud = u.to(gpu)
            un = torch.full_like(ud, SENT)
            res = torch.zeros(1, dtype=dtype, device=gpu)
            ops.jacobi_sweep(ud, un, 1, rows + 1, res, rhs=b.to(gpu))
            _assert_sweep(un, res, want.to(gpu), rowres, 1, rows + 1, (dtype, field, cols))


# ---------------------------------------------------------------------------
# 8. generic kernels
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rhs_generic_kernels(gpu, dtype):
    height = 33 + 3
    for cols in (1, 2, 3, 5, 255, 257, 513):
        u, b, want, rowres = _case(dtype, height, cols)
        ud, bd, wd = u.to(gpu), b.to(gpu), want.to(gpu)
        un = torch.empty_like(ud)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        for rows in (1, 16, 17, 33):
            for r0 in (1, 2):
                un.fill_(SENT)
                res.zero_()
                ops.jacobi_sweep(ud, un, r0, r0 + rows, res, rhs=bd)
                _assert_sweep(un, res, wd, rowres, r0, r0 + rows, (dtype, cols, r0, rows))


# ---------------------------------------------------------------------------
# 9. only b off the 16-byte boundary; pitch > cols
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rhs_unaligned_b_takes_scalar_kernel(gpu, dtype):
    rows, cols = 17, 63 * NV[dtype]
    u, b, want, rowres = _case(dtype, rows + 2, cols)
    n = (rows + 2) * cols
    flat = torch.empty(n + 8, dtype=dtype, device=gpu)
    bd = flat[1:1 + n].view(rows + 2, cols)
    bd.copy_(b)
    ud = u.to(gpu)
    un = torch.full_like(ud, SENT)
    assert bd.is_contiguous() and bd.data_ptr() % 16 != 0 and ud.data_ptr() % 16 == 0 and un.data_ptr() % 16 == 0
    res = torch.zeros(1, dtype=dtype, device=gpu)
    ops.jacobi_sweep(ud, un, 1, rows + 1, res, rhs=bd)
    _assert_sweep(un, res, want.to(gpu), rowres, 1, rows + 1, dtype)
    # the wave template itself refuses such a b
    with pytest.raises(_native.MpxError, match="vector layout"):
        _variant(ud, bd, un, cols, cols, 1, rows + 1, None, 8, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rhs_pitch_wider_than_cols(gpu, dtype):
    nv = NV[dtype]
    rows, cols, pitch = 19, 63 * nv, 63 * nv + nv
    u, b, want, rowres = _case(dtype, rows + 2, cols)
    wd = want.to(gpu)
    ud = torch.full((rows + 2, pitch), float("nan"), dtype=dtype, device=gpu)
    bd = torch.full((rows + 2, pitch), float("nan"), dtype=dtype, device=gpu)
    ud[:, :cols] = u.to(gpu)
    bd[:, :cols] = b.to(gpu)
    for r0, r1 in ((1, rows + 1), (3, rows - 1)):
        un = torch.full_like(ud, SENT)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        _abi(ud, bd, un, cols, pitch, r0, r1, res)
        assert not bool(torch.isnan(un).any())
        assert bool((un[:, cols:] == SENT).all()), "padding written"
        _assert_sweep(un[:, :cols], res, wd, rowres, r0, r1, (dtype, r0, r1))


# ---------------------------------------------------------------------------
# 10. the overlapped step's launch pattern
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["wave", "generic"])
def test_rhs_overlapped_step_launch_pattern(gpu, dtype, family):
    cols = 70 * NV[dtype] if family == "wave" else 257
    for n in (37, 1, 2):
        u, b, want, rowres = _case(dtype, n + 2, cols)
        ud, bd, wd = u.to(gpu), b.to(gpu), want.to(gpu)
        full = torch.full_like(ud, SENT)
        rfull = torch.zeros(1, dtype=dtype, device=gpu)
        ops.jacobi_sweep(ud, full, 1, n + 1, rfull, rhs=bd)
        _assert_sweep(full, rfull, wd, rowres, 1, n + 1, (dtype, family, n, "full"))
        un = torch.full_like(ud, SENT)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        for r in ([1] if n == 1 else [1, n]):
            ops.jacobi_sweep(ud, un, r, r + 1, res, rhs=bd)
        if n >= 2:
            ops.jacobi_sweep(ud, un, 2, n, res, rhs=bd)
        _assert_sweep(un, res, wd, rowres, 1, n + 1, (dtype, family, n, "overlapped"))
        assert _same_bits(un, full) and _same_bits(res, rfull), (dtype, family, n)


# ---------------------------------------------------------------------------
# 12. HIP graph replays on one rank
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rhs_graph_replay_equals_eager(gpu, dtype):
    rows, cols = 37, 33 * NV[dtype]
    field, src = _global_problem(rows, cols, dtype)
    sols = []
    for graph in (True, False):
        sol = SlabJacobi(parallel.DistContext(device=gpu), rows, cols, dtype=dtype, check_every=10)
        _setup(sol, field, src)
        if graph:
            sol.run(60, graph=True)
        else:
            for _ in range(60):
                sol.step()
        torch.cuda.synchronize()
        assert sol.iteration == 60
        sols.append(sol)
    assert _same_bits(sols[0].u, sols[1].u) and sols[0].last_residual == sols[1].last_residual is not None
    lap = SlabJacobi(parallel.DistContext(device=gpu), rows, cols, dtype=dtype, check_every=10)
    _setup(lap, field, src, rhs=False)
    lap.run(60)
    assert not torch.equal(lap.u, sols[0].u)


# ---------------------------------------------------------------------------
# 13. peer halos with an rhs: ranks sharing the one GPU, gloo control plane
# ---------------------------------------------------------------------------
def _peer_rhs_worker(rank, world, port, rows, cols, iters, fp64, errq, graph=False):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        ctx = parallel.init(device="cuda", backend="gloo")
        dt = torch.float64 if fp64 else torch.float32
        field, src = _global_problem(rows, cols, dt)
        sol = SlabJacobi(ctx, rows, cols, dtype=dt, check_every=10, halo="peer")
        assert sol.transport == "xgmi-peer-signalled", sol.transport
        _setup(sol, field, src)
        sol.run(iters, graph=graph)
        torch.cuda.synchronize()
        sol.check_peer()
        got = sol.gather()
        res = sol.last_residual
        sol.run(10)  # a restart from the gathered state continues seamlessly
        got2 = sol.gather()
        res2 = sol.last_residual
        sol.close()
        if ctx.rank == 0:
            one = SlabJacobi(parallel.DistContext(device=ctx.device), rows, cols, dtype=dt, check_every=10)
            _setup(one, field, src)
            one.run(iters)
            assert torch.equal(got.cpu(), one.owned.cpu()), "peer halos with an rhs differ from one rank"
            assert res == one.last_residual and res is not None
            one.run(10)
            assert torch.equal(got2.cpu(), one.owned.cpu()) and res2 == one.last_residual
            lap = SlabJacobi(parallel.DistContext(device=ctx.device), rows, cols, dtype=dt, check_every=10)
            _setup(lap, field, src, rhs=False)
            lap.run(iters + 10)
            assert not torch.equal(lap.owned, one.owned)
        parallel.shutdown()
    except Exception:  # noqa: BLE001
        errq.put(f"rank {rank}: {traceback.format_exc()}")


@pytest.mark.gpu
@pytest.mark.parametrize("world,fp64,graph", [(2, True, False), (3, False, False), (2, True, True)])
def test_rhs_peer_halos_equal_one_rank(gpu, world, fp64, graph):
    """100 iterations plus a 10-iteration restart, bit-identical to one rank,
    residual included; 8k+5 global rows."""
    _run_ranks(_peer_rhs_worker, world, 8 * 9 + 5, 132 if fp64 else 136, 100, fp64, graph=graph)
