"""Full multigrid for the 2-D Poisson solver: the cubic prolongation
``ops.mg_prolong_cubic`` from the kernels up, and ``PoissonMultigrid.fmg``.

The operator has one rounding order, so GPU fp32, GPU fp64, the CPU library and
the torch expression ``ops.reference.mg_prolong_cubic`` agree bit for bit: no
operator comparison here carries a tolerance. Sentinels: the fine boundary and
every padding element hold NaN and must keep those bits (compared on the whole
backing buffer); the fine interior starts from values that must all be
overwritten; the coarse padding holds NaN, which would reach the result if it
were read.

The model is checked against the definition of "solved to discretisation
accuracy": with u the solution of the differential problem, u_h the solution of
the discrete one and u_fmg the result of ``fmg()``,
rho = max|u_fmg - u_h| / max|u_h - u| <= 1.
"""

from __future__ import annotations

import functools

import pytest
import torch

from cuda_mpi_openmp_amd import ops
from cuda_mpi_openmp_amd.models import PoissonMultigrid
from cuda_mpi_openmp_amd.ops import reference as ref

DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector
NAN = float("nan")
MODES = ("contig", "vec", "shift")  # per-element unless the width fits; vector; unaligned base: per-element

# coarse widths: the parabola ghost, two ghosts that share points, 5, the smallest
# width whose ghosts do not; a wave edge in fp64 (128 = 64 lanes x 2) and fp32
# (256); a workgroup edge in fp64 (512) and fp32 (1024)
WIDTHS = [3, 4, 5, 6, 127, 128, 129, 130, 255, 256, 257, 258, 513, 514, 1025, 1026]
HEIGHTS = [3, 4, 5, 9, 10, 17, 18]  # both ghosts at every distance from each other; odd and even row counts
# every width with a height, every height with the widths 3, 4 and 130
CROSS = sorted({(HEIGHTS[i % len(HEIGHTS)], wc) for i, wc in enumerate(WIDTHS)}
               | {(hc, wc) for hc in HEIGHTS for wc in (3, 4, 130)})
# a launch this small walks one coarse row per lane; a launch of 8192 waves or
# more walks two, where the four interpolated rows rotate through the registers.
# The smallest such strips: an odd number of coarse row pairs (a remainder
# block) and an even one
TALL = [(4100, 3), (4101, 5)]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _place(t: torch.Tensor, mode: str, device):
    """(view, backing): t's values in a pitched view of a NaN-filled backing
    buffer on ``device``."""
    h, w = t.shape
    nv = NV[t.dtype]
    if mode == "contig":
        backing = t.clone().to(device)
        return backing, backing
    pitch = (w + nv - 1) // nv * nv
    if mode == "vec":
        backing = torch.full((h, pitch), NAN, dtype=t.dtype, device=device)
        view = backing[:, :w]
    else:
        backing = torch.full((h * pitch + nv,), NAN, dtype=t.dtype, device=device)
        view = backing[1:1 + h * pitch].view(h, pitch)[:, :w]
        assert view.data_ptr() % 16 != 0
    view.copy_(t)
    return view, backing


def _rand(shape, seed, dtype, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(dtype)


# ---------------------------------------------------------------------------
# ops.mg_prolong_cubic
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cubic_case(dtype, hc, wc):
    """The coarse grid (boundary filled: it is read), the fine grid before the
    call and the torch expression's result; computed once, never modified."""
    c = _rand((hc, wc), 1000 * hc + wc, dtype)
    u = _rand((2 * hc - 1, 2 * wc - 1), 1000 * hc + wc + 1, dtype, 2.0, 3.0)
    u[0] = u[-1] = NAN
    u[:, 0] = u[:, -1] = NAN
    want = ref.mg_prolong_cubic(c, u)
    assert want.dtype == dtype and not bool(torch.isnan(want[1:-1, 1:-1]).any())
    assert float(want[1:-1, 1:-1].abs().max()) < 2.0  # nothing of the old interior is left
    assert bool(torch.isnan(want[0]).all()) and bool(torch.isnan(want[:, -1]).all())
    return c, u, want


def _run_cubic(device, dtype, hc, wc, mode) -> torch.Tensor:
    """The backing buffer of the result, padding included, as a CPU tensor."""
    c, u, _ = _cubic_case(dtype, hc, wc)
    cv, _ = _place(c, mode, device)
    uv, ub = _place(u, mode, device)
    assert ops.mg_prolong_cubic(cv, uv) is None
    return ub.cpu()


def _check_cubic(device, dtype, hc, wc):
    want = _cubic_case(dtype, hc, wc)[2]
    for mode in MODES:
        got = _run_cubic(device, dtype, hc, wc, mode)
        assert _same_bits(got, _place(want, mode, "cpu")[1]), (hc, wc, mode, str(dtype))


@pytest.mark.parametrize("hc,wc", CROSS + TALL[:1])
def test_cpu_cubic_equals_the_torch_expression(hc, wc):
    _check_cubic("cpu", torch.float64, hc, wc)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hc,wc", CROSS + TALL)
def test_gpu_cubic_bit_exact(gpu, dtype, hc, wc):
    _check_cubic(gpu, dtype, hc, wc)


@pytest.mark.gpu
@pytest.mark.parametrize("hc,wc", [(10, 130), (17, 514)])
def test_gpu_cubic_fp64_equals_the_cpu_library(gpu, hc, wc):
    for mode in MODES:
        assert _same_bits(_run_cubic(gpu, torch.float64, hc, wc, mode),
                          _run_cubic("cpu", torch.float64, hc, wc, mode)), (hc, wc, mode)


def _poly(deg_y, deg_x):
    """An integer-coefficient polynomial of the given degrees in y and x."""
    py = [lambda y: y * 0 + 3, lambda y: 2 * y - 5, lambda y: y * y - 3 * y + 2, lambda y: y ** 3 - 4 * y * y + y + 7]
    px = [lambda x: x * 0 - 2, lambda x: 3 * x + 1, lambda x: 2 * x * x - x - 6, lambda x: x ** 3 + x * x - 9 * x + 4]
    return lambda y, x: py[deg_y](y) * px[deg_x](x) + (y if deg_y else 0) * (x if deg_x else 0) + 11


def _check_polynomials(device):
    """Coarse values sampled from a polynomial of degree <= 3 in each variable
    (<= 2 along a dimension of 3 points) at the even points of the integer grid
    come out equal to it at every fine interior point: every value and every
    intermediate of the rule is a small integer or a small multiple of 1/16,
    so the comparison is exact, whatever the rounding order."""
    for hc, wc in ((3, 3), (3, 7), (4, 4), (6, 3), (5, 6), (9, 131)):
        p = _poly(3 if hc >= 4 else 2, 3 if wc >= 4 else 2)
        i = torch.arange(2 * hc - 1, dtype=torch.float64).unsqueeze(1)
        j = torch.arange(2 * wc - 1, dtype=torch.float64).unsqueeze(0)
        full = p(i, j)
        assert float(full.abs().max()) < 2.0 ** 40
        for mode in ("contig", "vec"):
            cv, _ = _place(full[::2, ::2].contiguous(), mode, device)
            uv, _ = _place(torch.zeros_like(full), mode, device)
            ops.mg_prolong_cubic(cv, uv)
            assert torch.equal(uv.cpu()[1:-1, 1:-1], full[1:-1, 1:-1]), (hc, wc, mode)


def test_cpu_cubic_reproduces_polynomials():
    _check_polynomials("cpu")


@pytest.mark.gpu
def test_gpu_cubic_reproduces_polynomials(gpu):
    _check_polynomials(gpu)


def test_torch_expression_reproduces_polynomials():
    p = _poly(3, 3)
    i = torch.arange(9, dtype=torch.float64).unsqueeze(1)
    j = torch.arange(13, dtype=torch.float64).unsqueeze(0)
    full = p(i, j)
    got = ref.mg_prolong_cubic(full[::2, ::2], torch.zeros_like(full))
    assert torch.equal(got[1:-1, 1:-1], full[1:-1, 1:-1]) and not bool(got[0].any())


def _refusals(device):
    z = lambda h, w, dt=torch.float64, dev=device: torch.zeros((h, w), dtype=dt, device=dev)  # noqa: E731
    ops.mg_prolong_cubic(z(3, 3), z(5, 5))  # the smallest accepted
    for c, u in ((z(4, 5), z(7, 10)), (z(4, 5), z(8, 9)), (z(5, 4), z(7, 9)),  # wrong shape relation
                 (z(2, 5), z(3, 9)), (z(5, 2), z(9, 3)), (z(2, 2), z(3, 3)),  # Hc or Wc < 3
                 (z(4, 5, torch.float32), z(7, 9)),  # dtype mismatch
                 (z(4, 10)[:, ::2], z(7, 9)), (z(4, 5), z(7, 18)[:, ::2]),  # non-unit column stride
                 (z(4, 5).unsqueeze(0), z(7, 9))):
        with pytest.raises(ValueError):
            ops.mg_prolong_cubic(c, u)


def test_cubic_refusals_cpu():
    _refusals("cpu")
    with pytest.raises(ValueError):  # the CPU reference is float64
        ops.mg_prolong_cubic(torch.zeros((4, 5), dtype=torch.float32), torch.zeros((7, 9), dtype=torch.float32))


@pytest.mark.gpu
def test_cubic_refusals_gpu(gpu):
    _refusals(gpu)
    with pytest.raises(ValueError):  # device mismatch
        ops.mg_prolong_cubic(torch.zeros((4, 5), dtype=torch.float64),
                             torch.zeros((7, 9), dtype=torch.float64, device=gpu))
    with pytest.raises(ValueError):
        ops.mg_prolong_cubic(torch.zeros((4, 5), dtype=torch.float16, device=gpu),
                             torch.zeros((7, 9), dtype=torch.float16, device=gpu))


def test_cubic_c_abi_refuses_bad_geometry():
    from cuda_mpi_openmp_amd import _native

    L = _native.lib()
    c, u = torch.zeros((4, 5), dtype=torch.float64), torch.zeros((7, 9), dtype=torch.float64)
    for hc, wc, pc, pu in ((2, 5, 5, 9), (4, 2, 5, 9), (4, 5, 4, 9), (4, 5, 5, 8)):
        assert L.mpx_cpu_mg_prolong_cubic_f64(c.data_ptr(), u.data_ptr(), hc, wc, pc, pu) != 0
        assert L.mpx_mg_prolong_cubic_f64(c.data_ptr(), u.data_ptr(), hc, wc, pc, pu, None) != 0
        assert L.mpx_mg_prolong_cubic_f32(c.data_ptr(), u.data_ptr(), hc, wc, pc, pu, None) != 0
    assert L.mpx_cpu_mg_prolong_cubic_f64(None, u.data_ptr(), 4, 5, 5, 9) != 0
    assert L.mpx_mg_prolong_cubic_f64(c.data_ptr(), None, 4, 5, 5, 9, None) != 0
    assert not bool(u.any())


# ---------------------------------------------------------------------------
# PoissonMultigrid.fmg
# ---------------------------------------------------------------------------
def _exact(rows, cols):
    """u = sin(3x + 0.4) e^y on the (rows + 2, cols) grid of spacing
    h = 1 / (cols - 1), and h: -Laplace(u) = 8 u, nonzero Dirichlet values."""
    h = 1.0 / (cols - 1)
    y = torch.arange(rows + 2, dtype=torch.float64).unsqueeze(1) * h
    x = torch.arange(cols, dtype=torch.float64).unsqueeze(0) * h
    return torch.sin(3.0 * x + 0.4) * torch.exp(y), h


def _problem(device, dtype, rows, cols, junk=0.0, **kw) -> PoissonMultigrid:
    """The manufactured problem: b = 8 h^2 u, u's boundary on level 0's u only,
    ``junk`` in the interior (fmg() must ignore it)."""
    m = PoissonMultigrid(rows, cols, dtype=dtype, device=device, **kw)
    u, h = _exact(rows, cols)
    m.set_rhs(tensor=(8.0 * h * h * u)[1:-1])
    start = u.clone()
    start[1:-1, 1:-1] = junk
    m.u.copy_(start.to(dtype))
    return m


@functools.lru_cache(maxsize=None)
def _discrete_solution(device, rows, cols):
    """(u_h, max|u_h - u|): the fp64 model cycled until the residual stalls at
    rounding level (25 cycles contract it by 1e-20)."""
    m = _problem(device, torch.float64, rows, cols)
    m._lv[0].un.copy_(m.u)
    for _ in range(25):
        m.cycle()
    assert m.last_residual <= 1e-13
    uh = m.u.cpu().clone()
    return uh, float((uh - _exact(rows, cols)[0]).abs().max())


def _rho(device, rows, cols, cycles_per_level=1):
    uh, disc = _discrete_solution(device, rows, cols)
    m = _problem(device, torch.float64, rows, cols, junk=5.0)
    res = m.fmg(cycles_per_level)
    assert res == m.last_residual and m.cycles == cycles_per_level
    alg = float((m.u.cpu() - uh).abs().max())
    print(f"fmg {rows + 2}x{cols} cycles_per_level={cycles_per_level}: rho = {alg / disc:.3f} "
          f"(algebraic {alg:.3e}, discretisation {disc:.3e}), last_residual {res:.3e}")
    return alg / disc


ACCURACY_SHAPES = [(15, 17), (31, 33), (63, 65), (127, 129), (63, 129)]


@pytest.mark.parametrize("rows,cols", ACCURACY_SHAPES)
def test_cpu_fmg_reaches_discretisation_accuracy(rows, cols):
    assert _rho("cpu", rows, cols) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", ACCURACY_SHAPES + [(255, 257)])
def test_gpu_fmg_reaches_discretisation_accuracy(gpu, rows, cols):
    assert _rho(gpu, rows, cols) <= 1.0


def test_cpu_fmg_two_cycles_per_level_are_more_accurate():
    assert _rho("cpu", 63, 65, 2) < _rho("cpu", 63, 65, 1)


@pytest.mark.gpu
def test_gpu_fmg_two_cycles_per_level_are_more_accurate(gpu):
    assert _rho(gpu, 127, 129, 2) < _rho(gpu, 127, 129, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(63, 129), (47, 81)])  # coarsest 3 x 5; 4 x 6: coarse sweeps, cubic ghosts
def test_gpu_fmg_fp64_equals_the_cpu_model(gpu, rows, cols):
    g = _problem(gpu, torch.float64, rows, cols)
    c = _problem("cpu", torch.float64, rows, cols)
    assert g.fmg() == c.fmg()
    assert _same_bits(g.u, c.u)
    assert g.fmg(2) == c.fmg(2)
    assert _same_bits(g.u, c.u) and g.cycles == c.cycles == 3


class _TorchFmg:
    """fmg() assembled from the torch expressions, in the model's order."""

    def __init__(self, m: PoissonMultigrid):
        self.m = m
        self.u = [torch.zeros(s, dtype=m.dtype) for s in m.levels]
        self.b = [torch.zeros(s, dtype=m.dtype) for s in m.levels]
        self.u[0] = m.u.cpu().clone()
        self.b[0] = m.rhs.cpu().clone()
        self.last = None

    def relax(self, k, omega, track=False):
        u, h = self.u[k], self.m.levels[k][0]
        if track:
            s = ref.jacobi(u, 1, h - 1, keep_dtype=True, rhs=self.b[k])
            self.last = float((s[1:-1, 1:-1] - u[1:-1, 1:-1]).abs().max())
        self.u[k] = ref.jacobi(u, 1, h - 1, keep_dtype=True, rhs=self.b[k], omega=omega, prev=u)

    def vcycle(self, k):
        m, n = self.m, len(self.m.levels)
        if k + 1 == n and k > 0:
            if m.levels[k] == (3, 3):
                self.relax(k, 1.0)
            else:
                for _ in range(m.coarse_sweeps):
                    self.relax(k, m.omega)
            return
        for _ in range(m.nu1):
            self.relax(k, m.omega)
        if k + 1 < n:
            r = ref.mg_residual(self.u[k], rhs=self.b[k])
            self.b[k + 1] = ref.mg_restrict(r)
            self.u[k + 1] = torch.zeros(m.levels[k + 1], dtype=m.dtype)
            self.vcycle(k + 1)
            self.u[k] = ref.mg_prolong_add(self.u[k + 1], self.u[k])
        for s in range(m.nu2):
            self.relax(k, m.omega, track=(k == 0 and s == m.nu2 - 1))

    def fmg(self, cycles_per_level=1):
        n = len(self.m.levels)
        bf = [self.b[0]]
        for k in range(1, n):
            bf.append(ref.mg_restrict(bf[-1]))
        for k in range(1, n):
            s = 1 << k
            self.u[k] = self.u[0][::s, ::s].clone()
        self.u[-1][1:-1, 1:-1] = 0
        self.b[-1] = bf[-1]
        for _ in range(cycles_per_level):
            self.vcycle(n - 1)
        for k in range(n - 2, -1, -1):
            self.u[k] = ref.mg_prolong_cubic(self.u[k + 1], self.u[k])
            self.b[k] = bf[k]
            for _ in range(cycles_per_level):
                self.vcycle(k)
        return self.last


def test_cpu_fmg_equals_the_torch_fmg():
    for rows, cols in ((15, 17), (47, 81)):  # down to 3 x 3; a 4 x 6 coarsest level
        c = _problem("cpu", torch.float64, rows, cols, junk=-3.0)
        t = _TorchFmg(c)
        assert c.fmg() == t.fmg() and _same_bits(c.u, t.u[0]), (rows, cols)


@pytest.mark.gpu
def test_gpu_fmg_fp32_equals_the_torch_fmg(gpu):
    g = _problem(gpu, torch.float32, 63, 129, junk=-3.0)
    t = _TorchFmg(g)
    assert g.fmg() == t.fmg()
    assert _same_bits(g.u, t.u[0])


def _check_tail_independence(device, dtype):
    # 65 x 129 -> 33 x 65 -> 17 x 33 -> 9 x 17 -> 5 x 9 -> 3 x 5
    base = _problem(device, dtype, 63, 129, tail_points=0)
    assert base.tail_level is None
    want_res, want = base.fmg(), base.u.cpu().clone()
    for points, level in ((None, None), (33 * 65, 1), (9 * 17, 3), (3 * 5, 5)):
        m = _problem(device, dtype, 63, 129, tail_points=points)
        if level is not None:
            assert m.tail_level == level
        assert m.fmg() == want_res and _same_bits(m.u, want), points


def test_cpu_fmg_does_not_depend_on_the_tail():
    _check_tail_independence("cpu", torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_fmg_does_not_depend_on_the_tail(gpu, dtype):
    m = _problem(gpu, dtype, 63, 129)
    assert m.tail_level == 1  # the default puts five FMG levels into the tail
    _check_tail_independence(gpu, dtype)


def _check_state(device, dtype, **kw):
    m = _problem(device, dtype, 63, 129, junk=2.0, **kw)
    r1, u1 = m.fmg(), m.u.cpu().clone()
    m.u[1:-1, 1:-1] = -7.0  # the interior is input to nothing
    assert m.fmg() == r1 and _same_bits(m.u, u1) and m.cycles == 2
    # the levels below level 0 were put back: a cycle from here equals a cycle of a
    # fresh solver that holds the same level 0
    fresh = PoissonMultigrid(63, 129, dtype=dtype, device=device, **kw)
    fresh.u.copy_(m.u)
    fresh._lv[0].un.copy_(m.u)
    fresh.rhs.copy_(m.rhs)
    assert m.cycle() == fresh.cycle() and _same_bits(m.u, fresh.u)
    assert m.cycle() == fresh.cycle() and _same_bits(m.u, fresh.u)


def test_cpu_fmg_repeats_and_leaves_the_levels_ready_for_cycles():
    _check_state("cpu", torch.float64)
    _check_state("cpu", torch.float64, tail_points=17 * 33)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_fmg_repeats_and_leaves_the_levels_ready_for_cycles(gpu, dtype):
    _check_state(gpu, dtype)
    _check_state(gpu, dtype, tail_points=0)


@pytest.mark.gpu
def test_gpu_fmg_allocates_nothing_after_the_first_call(gpu):
    g = _problem(gpu, torch.float64, 63, 129)
    built = torch.cuda.memory_allocated(gpu)
    g.cycle()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == built  # the constructor's memory is all cycle() has
    g.fmg()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    g.fmg()
    g.fmg(2)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before


def _check_single_level(device):
    m = _problem(device, torch.float64, 15, 17, junk=9.0, max_levels=1)
    assert len(m.levels) == 1
    want = _problem(device, torch.float64, 15, 17, junk=0.0, max_levels=1)
    want._lv[0].un.copy_(want.u)
    assert m.fmg() == want.cycle() and _same_bits(m.u, want.u) and m.cycles == 1
    with pytest.raises(ValueError):
        m.fmg(0)


def test_cpu_fmg_with_a_single_level():
    _check_single_level("cpu")


@pytest.mark.gpu
def test_gpu_fmg_with_a_single_level(gpu):
    _check_single_level(gpu)


def test_fmg_takes_boundary_values_that_vary_along_the_edge():
    """Level k's boundary is level 0's at stride 2^k. With b = 0 and the harmonic
    u = x^2 - y^2 + 3xy both the 5-point scheme and the interpolation are exact
    on every level, and the 3 x 3 coarsest level is solved exactly: each level
    starts its cycle from u up to rounding and the cycle contracts what error
    there is, so the result is u to a few hundred roundings of values below 5
    (5e-13 allows 500)."""
    rows, cols = 31, 33
    m = PoissonMultigrid(rows, cols, dtype=torch.float64)
    y = torch.arange(rows + 2, dtype=torch.float64).unsqueeze(1) / 32
    x = torch.arange(cols, dtype=torch.float64).unsqueeze(0) / 32
    u = x * x - y * y + 3 * x * y
    start = u.clone()
    start[1:-1, 1:-1] = 0.0
    m.u.copy_(start)
    m.fmg()
    assert m.levels[-1] == (3, 3)
    assert float((m.u - u).abs().max()) <= 5e-13
