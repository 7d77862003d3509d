"""Full multigrid for the 3-D Poisson solver: the tricubic prolongation
``ops.mg3_prolong_cubic`` from the kernels up, and ``PoissonMultigrid3D.fmg``.

Conventions are test_multigrid_fmg.py's, one dimension up. The operator has one
rounding order, so GPU fp32, GPU fp64, the CPU library and the torch expression
``ops.reference.mg3_prolong_cubic`` agree bit for bit: no operator comparison
here carries a tolerance. Sentinels: the fine boundary and every padding
element hold NaN and must keep those bits (compared on the whole backing
buffer); the fine interior starts from values in [2, 3) that must all be
overwritten; the coarse padding holds NaN, which would reach the result if it
were read.

Layouts: "contig" (odd widths take the per-element kernels), "vec" (row pitch
rounded up to 16 bytes and one spare row per plane, so the plane stride exceeds
H * pitch: the vector kernels) and "shift" (the rounded pitch with the base
moved by one element: unaligned, per-element).

The model is checked against the definition of "solved to discretisation
accuracy": with u the solution of the differential problem, u_h the solution of
the discrete one and u_fmg the result of ``fmg()``,
rho = max|u_fmg - u_h| / max|u_h - u|. The torch expressions alone give rho =
0.056 to 0.166 with two cycles per level on the shapes used here, so the
condition rho <= 0.5 leaves a factor of 3.
"""

from __future__ import annotations

import functools

import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.models import PoissonMultigrid3D
from cuda_mpi_openmp_amd.ops import reference as ref

DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector
NAN = float("nan")
MODES = ("contig", "vec", "shift")

# coarse shapes (dc, hc, wc). Both ghosts of each dimension at every distance
# from each other: the parabola (3), two cubic ghosts that share points (4, 5,
# 6), ghosts that do not (9, 10)
SMALL = [(3, 3, 3), (4, 4, 4), (3, 4, 5), (5, 3, 4), (6, 5, 3), (4, 6, 6), (9, 10, 5), (10, 9, 4)]
# wave edges in x (128 coarse elements in fp64, 256 in fp32); several workgroups across x
WAVE_EDGES = [(4, 5, w) for w in (127, 128, 129, 130)] + [(3, 4, w) for w in (255, 256, 257, 258)]
WIDE = [(3, 6, 514), (4, 3, 1026)]
TALL_CPU = (37, 4, 3)  # more coarse planes than any walk


def _full_walk_shape():
    """The smallest narrow launch that keeps the full plane walk: a launch with
    fewer than ``min_waves`` waves shortens it. With one wave across x the
    launch has (hc - 1) * ceil((dc - 1) / planes) waves; dc - 1 is two walks
    plus one plane, so the walk down z ends in a remainder block."""
    wk = ops.mg3_cubic_walk()
    planes, need = wk["planes"], wk["min_waves"]
    dc = 2 * planes + 2
    blocks = -(-(dc - 1) // planes)
    hc = -(-need // blocks) + 1
    shape = (dc, hc, 3)
    assert (hc - 1) * blocks >= need
    assert planes == 1 or (dc - 1) % planes != 0
    assert (2 * dc - 1) * (2 * hc - 1) * 5 <= 10 ** 7
    return shape


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _place(t: torch.Tensor, mode: str, device):
    """(view, backing): t's values in a pitched view of a NaN-filled backing
    buffer on ``device``."""
    d, h, w = t.shape
    nv = NV[t.dtype]
    if mode == "contig":
        backing = t.clone().to(device)
        return backing, backing
    pitch = (w + nv - 1) // nv * nv
    if mode == "vec":
        backing = torch.full((d, h + 1, pitch), NAN, dtype=t.dtype, device=device)
        view = backing[:, :h, :w]
        assert view.stride(0) > h * pitch
    else:
        backing = torch.full((d * h * pitch + nv,), NAN, dtype=t.dtype, device=device)
        view = backing[1:1 + d * h * pitch].view(d, h, pitch)[:, :, :w]
        assert view.data_ptr() % 16 != 0
    view.copy_(t)
    return view, backing


def _rand(shape, seed, dtype, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(dtype)


def _fine(cs):
    return tuple(2 * n - 1 for n in cs)


def _inner(t: torch.Tensor) -> torch.Tensor:
    return t[1:-1, 1:-1, 1:-1]


# ---------------------------------------------------------------------------
# ops.mg3_prolong_cubic
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cubic_case(dtype, cs):
    """The coarse grid (boundary filled: it is read), the fine grid before the
    call and the torch expression's result; computed once, never modified."""
    seed = 10000 * cs[0] + 100 * cs[1] + cs[2]
    c = _rand(cs, seed, dtype)
    u = _rand(_fine(cs), seed + 1, dtype, 2.0, 3.0)
    u[0] = u[-1] = NAN
    u[:, 0] = u[:, -1] = NAN
    u[:, :, 0] = u[:, :, -1] = NAN
    want = ref.mg3_prolong_cubic(c, u)
    assert want.dtype == dtype and not bool(torch.isnan(_inner(want)).any())
    assert float(_inner(want).abs().max()) < 2.0  # nothing of the old interior is left
    assert bool(torch.isnan(want[0]).all()) and bool(torch.isnan(want[:, -1]).all())
    assert bool(torch.isnan(want[:, :, 0]).all())
    return c, u, want


def _run_cubic(device, dtype, cs, mode) -> torch.Tensor:
    """The backing buffer of the result, padding included, as a CPU tensor."""
    c, u, _ = _cubic_case(dtype, cs)
    cv, _ = _place(c, mode, device)
    uv, ub = _place(u, mode, device)
    assert ops.mg3_prolong_cubic(cv, uv) is None
    return ub.cpu()


def _check_cubic(device, dtype, cs):
    want = _cubic_case(dtype, cs)[2]
    for mode in MODES:
        got = _run_cubic(device, dtype, cs, mode)
        assert _same_bits(got, _place(want, mode, "cpu")[1]), (cs, mode, str(dtype))


@pytest.mark.parametrize("cs", SMALL + [(4, 5, 130), TALL_CPU])
def test_cpu_cubic_equals_the_torch_expression(cs):
    _check_cubic("cpu", torch.float64, cs)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cs", SMALL + WAVE_EDGES + WIDE)
def test_gpu_cubic_bit_exact(gpu, dtype, cs):
    _check_cubic(gpu, dtype, cs)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_cubic_bit_exact_on_the_full_walk(gpu, dtype):
    _check_cubic(gpu, dtype, _full_walk_shape())


@pytest.mark.gpu
@pytest.mark.parametrize("cs", [(5, 10, 130), (4, 17, 514)])
def test_gpu_cubic_fp64_equals_the_cpu_library(gpu, cs):
    for mode in MODES:
        assert _same_bits(_run_cubic(gpu, torch.float64, cs, mode), _run_cubic("cpu", torch.float64, cs, mode)), (cs, mode)


def _check_even_planes(device, dtype, cs):
    """The interior of fine plane 2K, 1 <= K <= dc - 2, is the 2-D operator's
    result for coarse plane K."""
    c, u, _ = _cubic_case(dtype, cs)
    for mode in ("contig", "vec"):
        cv, _ = _place(c, mode, device)
        uv, _ = _place(u, mode, device)
        ops.mg3_prolong_cubic(cv, uv)
        for K in range(1, cs[0] - 1):
            plane = u[2 * K].clone().to(device)
            ops.mg_prolong_cubic(cv[K], plane)
            assert _same_bits(uv[2 * K, 1:-1, 1:-1], plane[1:-1, 1:-1]), (cs, mode, K)


@pytest.mark.parametrize("cs", [(3, 3, 3), (4, 4, 4), (6, 5, 3), (9, 10, 5)])
def test_cpu_even_planes_equal_the_2d_operator(cs):
    _check_even_planes("cpu", torch.float64, cs)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cs", [(3, 3, 3), (4, 4, 4), (6, 5, 3), (9, 10, 5), (4, 5, 130)])
def test_gpu_even_planes_equal_the_2d_operator(gpu, dtype, cs):
    _check_even_planes(gpu, dtype, cs)


POLY_SHAPES = [(3, 3, 3), (3, 7, 4), (4, 4, 4), (6, 3, 5), (5, 6, 7), (4, 9, 131)]


def _poly(deg_z, deg_y, deg_x):
    """An integer-coefficient polynomial of the given degrees in z, y and x with
    a mixed term. The cubics have their roots inside the largest grid used
    (z <= 10, y <= 16, x <= 260), which keeps the values small."""
    pz = [lambda z: z * 0 + 3, lambda z: 2 * z - 5, lambda z: (z - 1) * (z - 4), lambda z: (z - 1) * (z - 3) * (z - 5)]
    py = [lambda y: y * 0 - 2, lambda y: 3 * y + 1, lambda y: (y - 2) * (y - 9), lambda y: (y - 4) * (y - 9) * (y - 14)]
    px = [lambda x: x * 0 + 5, lambda x: x - 7, lambda x: (x - 3) * (x - 100),
          lambda x: (x - 60) * (x - 130) * (x - 200)]
    return lambda z, y, x: pz[deg_z](z) * py[deg_y](y) * px[deg_x](x) + z * y * x + 11


def _poly_grid(cs):
    d, h, w = _fine(cs)
    p = _poly(*(3 if n >= 4 else 2 for n in cs))
    z = torch.arange(d, dtype=torch.float64).view(-1, 1, 1)
    y = torch.arange(h, dtype=torch.float64).view(1, -1, 1)
    x = torch.arange(w, dtype=torch.float64).view(1, 1, -1)
    full = p(z, y, x)
    # three passes yield multiples of 1/4096: exact in fp64 below 2^41
    assert float(full.abs().max()) < 2.0 ** 40
    return full


def _check_polynomials(device):
    """Coarse values sampled from a polynomial of degree <= 3 in each variable
    (<= 2 along a dimension of 3 points) at the even points of the integer grid
    come out equal to it at every fine interior point: every value and every
    intermediate of the rule is an integer or a multiple of 1/4096 below 2^41,
    so the comparison is exact, whatever the rounding order."""
    for cs in POLY_SHAPES:
        full = _poly_grid(cs)
        for mode in ("contig", "vec"):
            cv, _ = _place(full[::2, ::2, ::2].contiguous(), mode, device)
            uv, _ = _place(torch.zeros_like(full), mode, device)
            ops.mg3_prolong_cubic(cv, uv)
            assert torch.equal(_inner(uv.cpu()), _inner(full)), (cs, mode)


def test_cpu_cubic_reproduces_polynomials():
    _check_polynomials("cpu")


@pytest.mark.gpu
def test_gpu_cubic_reproduces_polynomials(gpu):
    _check_polynomials(gpu)


def test_torch_expression_reproduces_polynomials():
    for cs in POLY_SHAPES:
        full = _poly_grid(cs)
        got = ref.mg3_prolong_cubic(full[::2, ::2, ::2], torch.zeros_like(full))
        assert torch.equal(_inner(got), _inner(full)), cs
        assert not bool(got[0].any()) and not bool(got[:, -1].any()) and not bool(got[:, :, 0].any())


def _refusals(device):
    made = []

    def z(d, h, w, dt=torch.float64, dev=device):
        t = torch.zeros((d, h, w), dtype=dt, device=dev)
        made.append(t)
        return t

    ops.mg3_prolong_cubic(z(3, 3, 3), z(5, 5, 5))  # the smallest accepted
    for c, u in ((z(4, 5, 6), z(8, 9, 11)), (z(4, 5, 6), z(7, 10, 11)), (z(4, 5, 6), z(7, 9, 12)),  # wrong shape relation
                 (z(5, 4, 6), z(7, 9, 11)),
                 (z(2, 5, 6), z(3, 9, 11)), (z(4, 2, 6), z(7, 3, 11)), (z(4, 5, 2), z(7, 9, 3)),  # a coarse edge < 3
                 (z(2, 2, 2), z(3, 3, 3)),
                 (z(4, 5, 6, torch.float32), z(7, 9, 11)),  # dtype mismatch
                 (z(4, 5, 12)[:, :, ::2], z(7, 9, 11)), (z(4, 5, 6), z(7, 9, 22)[:, :, ::2]),  # non-unit x stride
                 (z(4, 5, 6)[0], z(7, 9, 11)[0]),  # 2-D tensors
                 (z(4, 5, 6).unsqueeze(0), z(7, 9, 11))):
        with pytest.raises(ValueError):
            ops.mg3_prolong_cubic(c, u)
    assert not any(bool(t.any()) for t in made)  # nothing was written


def test_cubic_refusals_cpu():
    _refusals("cpu")
    c, u = torch.zeros((4, 5, 6), dtype=torch.float32), torch.zeros((7, 9, 11), dtype=torch.float32)
    with pytest.raises(ValueError):  # the CPU reference is float64
        ops.mg3_prolong_cubic(c, u)
    assert not bool(u.any())


@pytest.mark.gpu
def test_cubic_refusals_gpu(gpu):
    _refusals(gpu)
    u = torch.zeros((7, 9, 11), dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError):  # device mismatch
        ops.mg3_prolong_cubic(torch.zeros((4, 5, 6), dtype=torch.float64), u)
    h = torch.zeros((7, 9, 11), dtype=torch.float16, device=gpu)
    with pytest.raises(ValueError):
        ops.mg3_prolong_cubic(torch.zeros((4, 5, 6), dtype=torch.float16, device=gpu), h)
    assert not bool(u.any()) and not bool(h.any())


def test_cubic_c_abi_refuses_bad_geometry():
    L = _native.lib()
    c, u = torch.ones((4, 5, 6), dtype=torch.float64), torch.zeros((7, 9, 11), dtype=torch.float64)
    cp, up = c.data_ptr(), u.data_ptr()
    good = (4, 5, 6, 6, 30, 11, 99)
    for args in ((2, 5, 6, 6, 30, 11, 99), (4, 2, 6, 6, 30, 11, 99), (4, 5, 2, 6, 30, 11, 99),  # a coarse edge < 3
                 (4, 5, 6, 5, 30, 11, 99), (4, 5, 6, 6, 30, 10, 99),  # a pitch below the width
                 (4, 5, 6, 6, 29, 11, 99), (4, 5, 6, 6, 30, 11, 98)):  # a plane stride below H * pitch
        assert L.mpx_cpu_mg3_prolong_cubic_f64(cp, up, *args) != 0, args
        assert L.mpx_mg3_prolong_cubic_f64(cp, up, *args, None) != 0, args
        assert L.mpx_mg3_prolong_cubic_f32(cp, up, *args, None) != 0, args
    assert L.mpx_cpu_mg3_prolong_cubic_f64(None, up, *good) != 0
    assert L.mpx_cpu_mg3_prolong_cubic_f64(cp, None, *good) != 0
    assert L.mpx_mg3_prolong_cubic_f64(None, up, *good, None) != 0
    assert L.mpx_mg3_prolong_cubic_f64(cp, None, *good, None) != 0
    assert L.mpx_mg3_prolong_cubic_f32(cp, None, *good, None) != 0
    assert L.mpx_mg3_cubic_walk(None) != 0
    assert not bool(u.any())
    assert L.mpx_cpu_mg3_prolong_cubic_f64(cp, up, *good) == 0 and bool(_inner(u).all())


def test_symbols_and_walk():
    L = _native.lib()
    for name in ("mpx_mg3_prolong_cubic_f64", "mpx_mg3_prolong_cubic_f32", "mpx_cpu_mg3_prolong_cubic_f64",
                 "mpx_mg3_cubic_walk"):
        assert hasattr(L, name), name
    assert callable(ops.mg3_prolong_cubic) and callable(ref.mg3_prolong_cubic)
    assert "mg3_prolong_cubic" in ops.__all__ and "mg3_cubic_walk" in ops.__all__
    wk = ops.mg3_cubic_walk()
    assert set(wk) == {"planes", "min_waves", "waves"} and all(v >= 1 for v in wk.values())
    assert wk["min_waves"] == ops.mg3_walk()["min_waves"] and wk["waves"] == ops.mg3_walk()["waves"]
    assert callable(PoissonMultigrid3D.fmg)


# ---------------------------------------------------------------------------
# PoissonMultigrid3D.fmg
# ---------------------------------------------------------------------------
def _exact(planes, ny, nx):
    """u = sin(3x + 0.4) e^y cos(2z) on the (planes + 2, ny, nx) grid of spacing
    h = 1 / (nx - 1), and h: -Laplace(u) = 12 u, nonzero Dirichlet values."""
    h = 1.0 / (nx - 1)
    z = torch.arange(planes + 2, dtype=torch.float64).view(-1, 1, 1) * h
    y = torch.arange(ny, dtype=torch.float64).view(1, -1, 1) * h
    x = torch.arange(nx, dtype=torch.float64).view(1, 1, -1) * h
    return torch.sin(3.0 * x + 0.4) * torch.exp(y) * torch.cos(2.0 * z), h


def _problem(device, dtype, planes, ny, nx, junk=0.0, **kw) -> PoissonMultigrid3D:
    """The manufactured problem: b = 12 h^2 u, u's boundary on level 0's u only,
    ``junk`` in the interior (fmg() must ignore it)."""
    m = PoissonMultigrid3D(planes, ny, nx, dtype=dtype, device=device, **kw)
    u, h = _exact(planes, ny, nx)
    m.set_rhs(tensor=(12.0 * h * h * u)[1:-1])
    start = u.clone()
    _inner(start)[:] = junk
    m.u.copy_(start.to(dtype))
    return m


@functools.lru_cache(maxsize=None)
def _discrete_solution(device, planes, ny, nx):
    """(u_h, max|u_h - u|): the fp64 model cycled 30 times, which takes the
    residual to rounding level (22 to 24 cycles reach 1e-13)."""
    m = _problem(device, torch.float64, planes, ny, nx)
    m._lv[0].un.copy_(m.u)
    for _ in range(30):
        m.cycle()
    assert m.last_residual <= 1e-13
    uh = m.u.cpu().clone()
    return uh, float((uh - _exact(planes, ny, nx)[0]).abs().max())


def _rho(device, planes, ny, nx, cycles_per_level=None):
    uh, disc = _discrete_solution(device, planes, ny, nx)
    m = _problem(device, torch.float64, planes, ny, nx, junk=5.0)
    res = m.fmg() if cycles_per_level is None else m.fmg(cycles_per_level)
    cpl = 2 if cycles_per_level is None else cycles_per_level
    assert res == m.last_residual and m.cycles == cpl
    alg = float((m.u.cpu() - uh).abs().max())
    err = float((m.u.cpu() - _exact(planes, ny, nx)[0]).abs().max())
    print(f"fmg {planes + 2}x{ny}x{nx} cycles_per_level={cpl}: rho = {alg / disc:.3f} (algebraic {alg:.3e}, "
          f"discretisation {disc:.3e}, error against u {err:.3e}), last_residual {res:.3e}")
    return alg / disc


ACCURACY_SHAPES = [(15, 17, 17), (31, 33, 33), (63, 65, 65), (31, 65, 17), (23, 41, 21)]


@pytest.mark.parametrize("planes,ny,nx", ACCURACY_SHAPES)
def test_cpu_fmg_reaches_discretisation_accuracy(planes, ny, nx):
    assert _rho("cpu", planes, ny, nx) <= 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("planes,ny,nx", ACCURACY_SHAPES + [(127, 129, 129)])
def test_gpu_fmg_reaches_discretisation_accuracy(gpu, planes, ny, nx):
    assert _rho(gpu, planes, ny, nx) <= 0.5


def test_cpu_fmg_one_cycle_per_level_is_less_accurate():
    assert _rho("cpu", 31, 33, 33, 1) > _rho("cpu", 31, 33, 33, 2)


@pytest.mark.gpu
def test_gpu_fmg_one_cycle_per_level_is_less_accurate(gpu):
    assert _rho(gpu, 63, 65, 65, 1) > _rho(gpu, 63, 65, 65, 2)


class _TorchFmg3:
    """fmg() assembled from the torch expressions, in the model's order."""

    def __init__(self, m: PoissonMultigrid3D):
        self.m = m
        self.u = [torch.zeros(s, dtype=m.dtype) for s in m.levels]
        self.b = [torch.zeros(s, dtype=m.dtype) for s in m.levels]
        self.u[0] = m.u.cpu().clone()
        self.b[0] = m.rhs.cpu().clone()
        self.last = None

    def relax(self, k, omega, track=False):
        u, d = self.u[k], self.m.levels[k][0]
        if track:
            s = ref.jacobi3d(u, 1, d - 1, keep_dtype=True, rhs=self.b[k])
            self.last = float((_inner(s) - _inner(u)).abs().max())
        self.u[k] = ref.jacobi3d(u, 1, d - 1, keep_dtype=True, rhs=self.b[k], omega=omega, prev=u)

    def vcycle(self, k):
        m, n = self.m, len(self.m.levels)
        if k + 1 == n and k > 0:
            if m.levels[k] == (3, 3, 3):
                self.relax(k, 1.0)
            else:
                for _ in range(m.coarse_sweeps):
                    self.relax(k, m.omega)
            return
        for _ in range(m.nu1):
            self.relax(k, m.omega)
        if k + 1 < n:
            r = ref.mg3_residual(self.u[k], rhs=self.b[k])
            self.b[k + 1] = ref.mg3_restrict(r)
            self.u[k + 1] = torch.zeros(m.levels[k + 1], dtype=m.dtype)
            self.vcycle(k + 1)
            self.u[k] = ref.mg3_prolong_add(self.u[k + 1], self.u[k])
        for s in range(m.nu2):
            self.relax(k, m.omega, track=(k == 0 and s == m.nu2 - 1))

    def fmg(self, cycles_per_level=2):
        n = len(self.m.levels)
        bf = [self.b[0]]
        for k in range(1, n):
            bf.append(ref.mg3_restrict(bf[-1]))
        for k in range(1, n):
            s = 1 << k
            self.u[k] = self.u[0][::s, ::s, ::s].clone()
        _inner(self.u[-1])[:] = 0
        self.b[-1] = bf[-1]
        for _ in range(cycles_per_level):
            self.vcycle(n - 1)
        for k in range(n - 2, -1, -1):
            self.u[k] = ref.mg3_prolong_cubic(self.u[k + 1], self.u[k])
            self.b[k] = bf[k]
            for _ in range(cycles_per_level):
                self.vcycle(k)
        return self.last


EQUAL_SHAPES = [((15, 17, 17), (3, 3, 3)), ((23, 41, 21), (7, 11, 6))]  # down to 3^3; coarse sweeps, cubic ghosts


def test_cpu_fmg_equals_the_torch_fmg():
    for shape, coarsest in EQUAL_SHAPES:
        c = _problem("cpu", torch.float64, *shape, junk=-3.0)
        assert c.levels[-1] == coarsest
        t = _TorchFmg3(c)
        assert c.fmg() == t.fmg() and _same_bits(c.u, t.u[0]), shape


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s, _ in EQUAL_SHAPES])
def test_gpu_fmg_fp64_equals_the_cpu_model(gpu, shape):
    g = _problem(gpu, torch.float64, *shape)
    c = _problem("cpu", torch.float64, *shape)
    assert g.fmg() == c.fmg()
    assert _same_bits(g.u, c.u)
    assert g.fmg(1) == c.fmg(1)
    assert _same_bits(g.u, c.u) and g.cycles == c.cycles == 3


@pytest.mark.gpu
def test_gpu_fmg_fp32_equals_the_torch_fmg(gpu):
    g = _problem(gpu, torch.float32, 15, 33, 65, junk=-3.0)
    t = _TorchFmg3(g)
    assert g.fmg() == t.fmg()
    assert _same_bits(g.u, t.u[0])


def _check_tail_independence(device, dtype):
    # 33 x 33 x 65 -> 17 x 17 x 33 -> 9 x 9 x 17 -> 5 x 5 x 9 -> 3 x 3 x 5
    base = _problem(device, dtype, 31, 33, 65, tail_points=0)
    assert base.tail_level is None and base.levels[0] == (33, 33, 65) and base.levels[-1] == (3, 3, 5)
    want_res, want = base.fmg(), base.u.cpu().clone()
    for points, level in ((None, None), (17 * 17 * 33, 1), (9 * 9 * 17, 2), (3 * 3 * 5, 4)):
        m = _problem(device, dtype, 31, 33, 65, tail_points=points)
        if level is not None:
            assert m.tail_level == level
        assert m.fmg() == want_res and _same_bits(m.u, want), points


def test_cpu_fmg_does_not_depend_on_the_tail():
    _check_tail_independence("cpu", torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_fmg_does_not_depend_on_the_tail(gpu, dtype):
    _check_tail_independence(gpu, dtype)


def _check_state(device, dtype, **kw):
    shape = (15, 17, 33)
    m = _problem(device, dtype, *shape, junk=2.0, **kw)
    r1, u1 = m.fmg(), m.u.cpu().clone()
    _inner(m.u)[:] = -7.0  # the interior is input to nothing
    assert m.fmg() == r1 and _same_bits(m.u, u1) and m.cycles == 4
    assert m.fmg(1) == m.last_residual and m.cycles == 5
    # the levels below level 0 were put back: a cycle from here equals a cycle of a
    # fresh solver that holds the same level 0
    fresh = PoissonMultigrid3D(*shape, dtype=dtype, device=device, **kw)
    fresh.u.copy_(m.u)
    fresh._lv[0].un.copy_(m.u)
    fresh.rhs.copy_(m.rhs)
    assert m.cycle() == fresh.cycle() and _same_bits(m.u, fresh.u)
    assert m.cycle() == fresh.cycle() and _same_bits(m.u, fresh.u)
    assert m.cycles == 7 and fresh.cycles == 2


def test_cpu_fmg_repeats_and_leaves_the_levels_ready_for_cycles():
    _check_state("cpu", torch.float64)
    _check_state("cpu", torch.float64, tail_points=9 * 9 * 17)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_fmg_repeats_and_leaves_the_levels_ready_for_cycles(gpu, dtype):
    _check_state(gpu, dtype)
    _check_state(gpu, dtype, tail_points=0)


@pytest.mark.gpu
def test_gpu_fmg_allocates_nothing_after_the_first_call(gpu):
    g = _problem(gpu, torch.float64, 31, 33, 65)
    built = torch.cuda.memory_allocated(gpu)
    g.cycle()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == built  # the constructor's memory is all cycle() has
    g.fmg()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    g.fmg()
    g.fmg(1)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before


def _check_single_level(device):
    m = _problem(device, torch.float64, 15, 17, 17, junk=9.0, max_levels=1)
    assert len(m.levels) == 1
    want = _problem(device, torch.float64, 15, 17, 17, junk=0.0, max_levels=1)
    want._lv[0].un.copy_(want.u)
    assert m.fmg(1) == want.cycle() and _same_bits(m.u, want.u) and m.cycles == 1
    with pytest.raises(ValueError):
        m.fmg(0)


def test_cpu_fmg_with_a_single_level():
    _check_single_level("cpu")


@pytest.mark.gpu
def test_gpu_fmg_with_a_single_level(gpu):
    _check_single_level(gpu)


def test_fmg_takes_boundary_values_that_vary_over_the_faces():
    """Level k's boundary is level 0's at stride 2^k. With b = 0 and the harmonic
    u = x^2 - y^2 + 3xy + z(x - 2y) both the 7-point scheme and the
    interpolation are exact on every level, and the 3 x 3 x 3 coarsest level is
    solved exactly: each level starts its cycles from u up to rounding and the
    cycles contract what error there is, so the result is u to a few hundred
    roundings of values below 8 (5e-13 allows 280 of 2^-49). The torch
    expressions alone (``_TorchFmg3``) end at u exactly on this problem: on a
    grid of spacing 1/32 the values are short dyadic fractions."""
    planes, ny, nx = 31, 33, 33
    m = PoissonMultigrid3D(planes, ny, nx, dtype=torch.float64)
    z = torch.arange(planes + 2, dtype=torch.float64).view(-1, 1, 1) / 32
    y = torch.arange(ny, dtype=torch.float64).view(1, -1, 1) / 32
    x = torch.arange(nx, dtype=torch.float64).view(1, 1, -1) / 32
    u = x * x - y * y + 3 * x * y + z * (x - 2 * y)
    start = u.clone()
    _inner(start)[:] = 0.0
    m.u.copy_(start)
    m.fmg()
    assert m.levels[-1] == (3, 3, 3)
    err = float((m.u - u).abs().max())
    print(f"harmonic boundary values: max|u_fmg - u| = {err:.3e}")
    assert err <= 5e-13
