"""The coarse levels of the 3-D V-cycle in one kernel (``ops.mg3_tail``,
``PoissonMultigrid3D(tail_points=)``).

As test_multigrid_tail.py: every comparison is bitwise, the model with the tail
against the same model without it, the GPU against the CPU model,
``ops.mg3_tail`` against the launched sequence. The seeded problem is
test_multigrid3d.py's.
"""

from __future__ import annotations

import functools

import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.models import PoissonMultigrid3D

DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector
NAN = float("nan")
ALL = 10 ** 9  # tail_points that puts every level k >= 1 into the tail

# (planes, ny, nx, model keywords, what the case reaches)
CASES = [
    (7, 9, 17, {}, "(9, 9, 17), (5, 5, 9), (3, 3, 5): even coarse sweeps"),
    (7, 9, 17, {"coarse_sweeps": 7}, "a (3, 3, 5) coarsest level, odd coarse sweeps"),
    (7, 9, 17, {"nu1": 0, "nu2": 1}, "no pre-smoothing, odd sweep counts on every level"),
    (15, 17, 17, {}, "ends at 3 x 3 x 3: the undamped coarsest sweep"),
    (15, 17, 17, {"nu1": 1, "nu2": 2, "coarse_sweeps": 7}, "odd sweep counts, 3 x 3 x 3"),
    (15, 17, 17, {"nu1": 0, "nu2": 1}, "no pre-smoothing down to 3 x 3 x 3"),
    (15, 17, 17, {"max_levels": 2}, "a one-level tail"),
    (15, 17, 17, {"tail_points": 5 * 5 * 5}, "a mid-cycle entry: the tail starts at level 2"),
]
CASE_IDS = [f"{p}x{y}x{x}-" + "-".join(f"{k}{v}" for k, v in kw.items()) for p, y, x, kw, _ in CASES]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _rand(shape, seed, dtype, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(dtype)


def _problem(device, dtype, planes, ny, nx, **kw):
    """Random interior in [0, 1), z0 face 1, rhs uniform in +-0.01, seeded."""
    m = PoissonMultigrid3D(planes, ny, nx, dtype=dtype, device=device, **kw)
    m.set_boundary(z0=1.0)
    m.fill(seed=3)
    m.set_rhs(tensor=_rand((planes, ny, nx), 11, torch.float64, -0.01, 0.01))
    return m


def _cycles(device, dtype, planes, ny, nx, n=3, **kw):
    m = _problem(device, dtype, planes, ny, nx, **kw)
    res = [m.cycle() for _ in range(n)]
    return m, res


@functools.lru_cache(maxsize=None)
def _cpu_launched(planes, ny, nx, kw_items):
    """The CPU model without a tail after 3 cycles: computed once, never modified."""
    kw = dict(kw_items)
    kw["tail_points"] = 0
    return _cycles("cpu", torch.float64, planes, ny, nx, **kw)


def _assert_same_state(a, ra, b, rb, tag):
    """Residuals, level 0's u and, from a's tail level down, every u and b."""
    assert ra == rb, (tag, ra, rb)
    assert a.last_residual == b.last_residual and a.cycles == b.cycles
    assert _same_bits(a.u, b.u), tag
    first = a.tail_level if a.tail_level is not None else len(a.levels)
    for k in range(first, len(a.levels)):
        assert _same_bits(a._lv[k].u, b._lv[k].u), (tag, "u of level", k)
        assert _same_bits(a._lv[k].b, b._lv[k].b), (tag, "b of level", k)


# ---------------------------------------------------------------------------
# CPU: the sequencing and the u / un convention
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("planes,ny,nx,kw,what", CASES, ids=CASE_IDS)
def test_cpu_model_with_tail_equals_the_launched_model(planes, ny, nx, kw, what):
    want, rwant = _cpu_launched(planes, ny, nx, tuple(sorted(kw.items())))
    kw = {"tail_points": ALL, **kw}
    got, rgot = _cycles("cpu", torch.float64, planes, ny, nx, **kw)
    assert got.tail_level == (2 if kw["tail_points"] != ALL else 1), what
    _assert_same_state(got, rgot, want, rwant, what)


@pytest.mark.parametrize("kw", [{}, {"nu1": 1, "nu2": 2}, {"nu1": 0, "nu2": 1, "coarse_sweeps": 7}])
@pytest.mark.parametrize("planes,ny,nx", [(7, 9, 17), (15, 17, 17)])
def test_cpu_op_leaves_the_levels_where_the_convention_says(planes, ny, nx, kw):
    a = _problem("cpu", torch.float64, planes, ny, nx, tail_points=0, **kw)
    b = _problem("cpu", torch.float64, planes, ny, nx, tail_points=0, **kw)
    for m in (a, b):  # level 1's b and a zeroed u, as level 0 leaves them
        ops.mg3_residual(m._lv[0].u, m._lv[0].r, rhs=m._lv[0].b)
        ops.mg3_restrict(m._lv[0].r, m._lv[1].b)
        m._lv[1].zero_u()
    a._vcycle(1)  # the launched path swaps u and un itself: a._lv[k].u is the iterate
    levels = [(lv.u, lv.un, lv.b, lv.r) for lv in b._lv[1:]]
    ops.mg3_tail(levels, b.nu1, b.nu2, b.coarse_sweeps, b.omega)
    sweeps = ops.tail_sweeps(len(levels), b.nu1, b.nu2, b.coarse_sweeps, b.levels[-1] == (3, 3, 3))
    assert float(a._lv[1].u.abs().max()) > 0.0
    for k, ((u, un, rhs, _), n) in enumerate(zip(levels, sweeps), start=1):
        assert _same_bits(un if n & 1 else u, a._lv[k].u), (k, n)
        assert _same_bits(rhs, a._lv[k].b), k


def test_tail_level_and_launches_per_cycle():
    m = PoissonMultigrid3D(255, 257, 257, tail_points=0)
    assert len(m.levels) == 8 and m.levels[-1] == (3, 3, 3) and m.tail_level is None
    assert m.launches_per_cycle == 7 * 8 + 1
    m = PoissonMultigrid3D(255, 257, 257, tail_points=33 ** 3)
    assert m.levels[3] == (33, 33, 33) and m.tail_level == 3 and m.launches_per_cycle == 8 * 3 + 1
    assert PoissonMultigrid3D(255, 257, 257, tail_points=33 ** 3 - 1).tail_level == 4
    assert PoissonMultigrid3D(255, 257, 257).tail_level is None  # the default on CPU tensors is 0
    m = PoissonMultigrid3D(7, 9, 17, tail_points=0)
    assert m.levels == [(9, 9, 17), (5, 5, 9), (3, 3, 5)] and m.launches_per_cycle == 2 * 8 + 50
    assert PoissonMultigrid3D(7, 9, 17, tail_points=ALL).launches_per_cycle == 9
    m = PoissonMultigrid3D(7, 9, 17, max_levels=1, tail_points=ALL)
    assert m.tail_level is None and m.launches_per_cycle == 4
    assert set(PoissonMultigrid3D.DEFAULT_TAIL_POINTS) == {torch.float64, torch.float32}
    with pytest.raises(ValueError):
        PoissonMultigrid3D(7, 9, 17, tail_points=-1)


def _grids(shapes, dtype=torch.float64):
    return [tuple(torch.zeros(s, dtype=dtype) for _ in range(4)) for s in shapes]


def test_argument_refusals():
    good = _grids([(9, 9, 17), (5, 5, 9), (3, 3, 5)])
    ops.mg3_tail(good, 2, 2, 3, 0.8)
    ops.mg3_tail([lv[:3] + (None,) if k == 2 else lv for k, lv in enumerate(good)], 2, 2, 3, 0.8)
    for nu1, nu2, cs, om in ((-1, 2, 3, 0.8), (2, 0, 3, 0.8), (2, 2, 0, 0.8), (2, 2, 3, 0.0), (2, 2, 3, NAN),
                             (2, 2, 3, float("inf"))):
        with pytest.raises(ValueError):
            ops.mg3_tail(good, nu1, nu2, cs, om)
    wide = torch.zeros((5, 5, 10), dtype=torch.float64)[:, :, :9]  # another row pitch
    tall = torch.zeros((5, 6, 9), dtype=torch.float64)[:, :5, :]  # another plane stride
    bad_sets = [
        [],
        _grids([(3, 3, 3)] * 17),
        _grids([(9, 9, 17), (5, 5, 8)]),  # not each other's coarse grids
        _grids([(9, 9, 17), (5, 4, 9)]),
        _grids([(9, 9, 17), (4, 5, 9)]),
        _grids([(5, 5, 5), (3, 3, 3), (2, 2, 2)]),  # a level without an interior
        [good[0], good[1][:3] + (None,), good[2]],  # r missing above the last level
        [good[0], (good[1][0], wide) + good[1][2:]],
        [good[0], (good[1][0], good[1][1], tall, good[1][3])],
        [good[0], tuple(t.to(torch.float32) for t in good[1])],
        _grids([(9, 9, 17), (5, 5, 9)], dtype=torch.float32),  # the CPU reference is float64
        [tuple(torch.zeros((9, 17, 9), dtype=torch.float64).transpose(1, 2) for _ in range(4))],  # stride(2) != 1
    ]
    for bad in bad_sets:
        with pytest.raises(ValueError):
            ops.mg3_tail(bad, 2, 2, 3, 0.8)
    # the native entry points refuse the same, with nothing written
    L = _native.lib()
    bufs = _grids([(9, 9, 17), (5, 5, 9), (3, 3, 5)])
    for lv in bufs:
        for t in lv:
            t.fill_(-7.0)

    def desc(edit=None):
        d = (_native.Mg3Level * 3)()
        for k, (u, un, b, r) in enumerate(bufs):
            d[k] = _native.Mg3Level(u.data_ptr(), un.data_ptr(), b.data_ptr(), r.data_ptr(), *u.shape, u.stride(1),
                                    u.stride(0))
        if edit:
            edit(d)
        return d

    def setter(k, field, value):
        return lambda d: setattr(d[k], field, value)

    for fn in (L.mpx_mg3_tail_f64, L.mpx_mg3_tail_f32):
        assert fn(None, 3, 2, 2, 3, 0.8, None) != 0
        for n in (0, -1, 17):
            assert fn(desc(), n, 2, 2, 3, 0.8, None) != 0
        for nu1, nu2, cs, om in ((-1, 2, 3, 0.8), (2, 0, 3, 0.8), (2, 2, 0, 0.8), (2, 2, 3, 0.0), (2, 2, 3, NAN),
                                 (2, 2, 3, float("inf"))):
            assert fn(desc(), 3, nu1, nu2, cs, om, None) != 0
        for edit in (setter(0, "u", None), setter(1, "un", None), setter(2, "b", None), setter(1, "r", None),
                     setter(1, "w", 8), setter(1, "h", 4), setter(1, "d", 4), setter(2, "pitch", 4),
                     setter(1, "plane", 44), setter(0, "pitch", 16)):
            assert fn(desc(edit), 3, 2, 2, 3, 0.8, None) != 0
        assert fn(desc(setter(0, "d", 2)), 1, 2, 2, 3, 0.8, None) != 0
    assert b"invalid argument" in L.mpx_last_error()
    assert all(bool((t == -7.0).all()) for lv in bufs for t in lv)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("planes,ny,nx,kw,what", CASES, ids=CASE_IDS)
def test_gpu_model_with_tail_bit_identical(gpu, dtype, planes, ny, nx, kw, what):
    kw = {"tail_points": ALL, **kw}
    got, rgot = _cycles(gpu, dtype, planes, ny, nx, **kw)
    want, rwant = _cycles(gpu, dtype, planes, ny, nx, **{**kw, "tail_points": 0})
    assert got.tail_level == (2 if kw["tail_points"] != ALL else 1) and want.tail_level is None, what
    assert got.launches_per_cycle < want.launches_per_cycle
    _assert_same_state(got, rgot, want, rwant, what)
    if dtype == torch.float64:
        kw.pop("tail_points")
        cpu, rcpu = _cpu_launched(planes, ny, nx, tuple(sorted(kw.items())))
        _assert_same_state(got, rgot, cpu, rcpu, ("against the CPU model", what))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_gpu_default_threshold_and_single_level(gpu, dtype):
    got, rgot = _cycles(gpu, dtype, 15, 17, 17)
    want, rwant = _cycles(gpu, dtype, 15, 17, 17, tail_points=0)
    points = PoissonMultigrid3D.DEFAULT_TAIL_POINTS[dtype]
    assert got.tail_points == points
    assert got.tail_level == next((k for k, s in enumerate(got.levels) if k >= 1 and s[0] * s[1] * s[2] <= points), None)
    _assert_same_state(got, rgot, want, rwant, "default")
    one, rone = _cycles(gpu, dtype, 15, 17, 17, max_levels=1, tail_points=ALL)
    ref, rref = _cycles(gpu, dtype, 15, 17, 17, max_levels=1, tail_points=0)
    assert one.tail_level is None
    _assert_same_state(one, rone, ref, rref, "one level")


def _padded(t: torch.Tensor, device, fill):
    """(view, backing): t in a view whose row pitch exceeds its width by one
    16-byte vector and whose plane stride exceeds H * pitch by one row."""
    d, h, w = t.shape
    nv = NV[t.dtype]
    pitch = (w + nv - 1) // nv * nv + nv
    backing = torch.full((d, h + 1, pitch), fill, dtype=t.dtype, device=device)
    view = backing[:, :h, :w]
    view.copy_(t)
    return view, backing


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_gpu_op_pitch_padding_and_scratch(gpu, dtype):
    """``ops.mg3_tail`` on tensors with a padded row pitch and plane stride, NaN
    in the padding, in every ``r`` and in every element of ``un`` that a sweep
    writes (planes 1 .. D - 2; planes 0 and D - 1 of ``un`` are input, the
    boundary values): the padding keeps its bits and the results equal the
    unpadded run's and the launched sequence's."""
    shapes = PoissonMultigrid3D.level_shapes(15, 17, 33)[1:]
    assert shapes == [(9, 9, 17), (5, 5, 9), (3, 3, 5)]
    u0 = _rand(shapes[0], 5, dtype)
    b0 = _rand(shapes[0], 6, dtype, -0.01, 0.01)
    results = []
    for padded in (False, True):
        levels, backs = [], []
        for k, s in enumerate(shapes):
            init = {"u": u0 if k == 0 else torch.full(s, 7.0, dtype=dtype),
                    "un": torch.full(s, NAN, dtype=dtype),
                    "b": b0 if k == 0 else torch.full(s, 5.0, dtype=dtype),
                    "r": torch.full(s, NAN, dtype=dtype)}
            init["un"][0], init["un"][-1] = (u0[0], u0[-1]) if k == 0 else (0.0, 0.0)
            if k:  # b's boundary is never read
                init["b"][0] = init["b"][-1] = NAN
                init["b"][:, 0] = init["b"][:, -1] = NAN
                init["b"][:, :, 0] = init["b"][:, :, -1] = NAN
            pairs = {n: (_padded(t, gpu, NAN) if padded else (t.to(gpu),) * 2) for n, t in init.items()}
            levels.append(tuple(pairs[n][0] for n in ("u", "un", "b", "r")))
            backs.append({n: pairs[n][1] for n in pairs})
        ops.mg3_tail(levels, 2, 2, 6, 0.8)
        torch.cuda.synchronize()
        results.append(levels)
        for (u, un, b, r), back in zip(levels, backs):
            _, h, w = u.shape
            assert not bool(torch.isnan(u).any()) and not bool(torch.isnan(b[1:-1, 1:-1, 1:-1]).any())
            if padded:
                for name, t in back.items():
                    for pad in (t[:, :, w:], t[:, h:, :]):
                        assert pad.numel() > 0 and _same_bits(pad, torch.full(pad.shape, NAN, dtype=dtype)), name
    for k, (plain, padded) in enumerate(zip(*results)):
        assert _same_bits(plain[0], padded[0]), ("u of level", k)
        assert _same_bits(plain[2][1:-1, 1:-1, 1:-1], padded[2][1:-1, 1:-1, 1:-1]), ("b of level", k)
    m = PoissonMultigrid3D(15, 17, 33, dtype=dtype, device=gpu, tail_points=0, coarse_sweeps=6, omega=0.8)
    m._lv[1].u.copy_(u0)
    m._lv[1].un.copy_(u0)
    m._lv[1].b.copy_(b0)
    m._vcycle(1)
    for k, lv in enumerate(m._lv[1:]):
        assert _same_bits(lv.u, results[0][k][0]), ("launched u of level", k + 1)


@pytest.mark.gpu
def test_gpu_cycle_with_tail_allocates_nothing(gpu):
    g = _problem(gpu, torch.float64, 15, 17, 17, tail_points=ALL, nu1=1, nu2=2)  # odd counts: u / un swap every cycle
    assert g.tail_level == 1
    g.cycle()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    g.cycle()
    g.cycle()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before
