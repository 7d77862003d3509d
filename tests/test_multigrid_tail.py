"""The coarse levels of the 2-D V-cycle in one kernel (``ops.mg_tail``,
``PoissonMultigrid(tail_points=)``).

Every operator has one rounding order and the fused tail restates each point's
expression operation for operation, so every comparison here is bitwise: the
model with the tail against the same model without it, the GPU against the CPU
model, ``ops.mg_tail`` against the launched sequence. No tolerance anywhere.
The seeded problem is test_multigrid.py's.
"""

from __future__ import annotations

import ctypes
import functools

import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.models import PoissonMultigrid

DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector
NAN = float("nan")
ALL = 10 ** 9  # tail_points that puts every level k >= 1 into the tail

# (rows, cols, model keywords, what the case reaches)
CASES = [
    (63, 129, {}, "six levels down to (3, 5)"),
    (63, 65, {}, "ends at 3 x 3: the undamped coarsest sweep"),
    (7, 17, {"coarse_sweeps": 7}, "a (3, 5) coarsest level, odd coarse sweeps"),
    (7, 17, {"coarse_sweeps": 50}, "a (3, 5) coarsest level, even coarse sweeps"),
    (3, 2049, {}, "(5, 2049), (3, 1025): a tail level wider than the workgroup"),
    (63, 129, {"nu1": 0, "nu2": 1}, "odd sweep counts on every level, no pre-smoothing"),
    (63, 129, {"nu1": 1, "nu2": 2}, "odd sweep counts on every level"),
    (63, 129, {"max_levels": 2}, "a one-level tail"),
    (63, 129, {"tail_points": 17 * 33}, "a mid-cycle entry: the tail starts at level 2"),
]
CASE_IDS = [f"{r}x{c}-" + "-".join(f"{k}{v}" for k, v in kw.items()) for r, c, kw, _ in CASES]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _rand(shape, seed, dtype, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(dtype)


def _problem(device, dtype, rows, cols, **kw):
    """Random interior in [0, 1), top boundary 1, rhs uniform in +-0.01, seeded."""
    m = PoissonMultigrid(rows, cols, dtype=dtype, device=device, **kw)
    m.set_boundary(top=1.0)
    m.fill(seed=3)
    m.set_rhs(tensor=_rand((rows, cols), 11, torch.float64, -0.01, 0.01))
    return m


def _cycles(device, dtype, rows, cols, n=3, **kw):
    m = _problem(device, dtype, rows, cols, **kw)
    res = [m.cycle() for _ in range(n)]
    return m, res


@functools.lru_cache(maxsize=None)
def _cpu_launched(rows, cols, kw_items):
    """The CPU model without a tail after 3 cycles: computed once, never modified."""
    kw = dict(kw_items)
    kw["tail_points"] = 0
    return _cycles("cpu", torch.float64, rows, cols, **kw)


def _assert_same_state(a: PoissonMultigrid, ra, b: PoissonMultigrid, rb, tag):
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
@pytest.mark.parametrize("rows,cols,kw,what", CASES, ids=CASE_IDS)
def test_cpu_model_with_tail_equals_the_launched_model(rows, cols, kw, what):
    want, rwant = _cpu_launched(rows, cols, tuple(sorted(kw.items())))
    kw = {"tail_points": ALL, **kw}
    got, rgot = _cycles("cpu", torch.float64, rows, cols, **kw)
    assert got.tail_level == (2 if kw["tail_points"] != ALL else 1), what
    _assert_same_state(got, rgot, want, rwant, what)


def _levels_of(m: PoissonMultigrid, first: int):
    return [(lv.u, lv.un, lv.b, lv.r) for lv in m._lv[first:]]


@pytest.mark.parametrize("kw", [{}, {"nu1": 1, "nu2": 2}, {"nu1": 0, "nu2": 1, "coarse_sweeps": 7}])
@pytest.mark.parametrize("rows,cols", [(63, 129), (7, 17)])
def test_cpu_op_leaves_the_levels_where_the_convention_says(rows, cols, kw):
    """``ops.mg_tail`` on the level tensors against ``_vcycle(1)`` of the
    launched model: each level's iterate lies in ``un`` after an odd number of
    sweeps, in ``u`` otherwise, bit-identical, and so does every ``b``."""
    a = _problem("cpu", torch.float64, rows, cols, tail_points=0, **kw)
    b = _problem("cpu", torch.float64, rows, cols, tail_points=0, **kw)
    for m in (a, b):  # something to restrict: level 1's b and a zeroed u, as level 0 leaves them
        ops.mg_residual(m._lv[0].u, m._lv[0].r, rhs=m._lv[0].b)
        ops.mg_restrict(m._lv[0].r, m._lv[1].b)
        m._lv[1].zero_u()
    a._vcycle(1)  # the launched path swaps u and un itself: a._lv[k].u is the iterate
    levels = _levels_of(b, 1)
    ops.mg_tail(levels, b.nu1, b.nu2, b.coarse_sweeps, b.omega)
    sweeps = ops.tail_sweeps(len(levels), b.nu1, b.nu2, b.coarse_sweeps, b.levels[-1] == (3, 3))
    assert len(sweeps) == len(levels) and sweeps[-1] == (1 if b.levels[-1] == (3, 3) else b.coarse_sweeps)
    assert float(a._lv[1].u.abs().max()) > 0.0
    for k, ((u, un, rhs, _), n) in enumerate(zip(levels, sweeps), start=1):
        assert _same_bits(un if n & 1 else u, a._lv[k].u), (k, n)
        assert _same_bits(rhs, a._lv[k].b), k


def test_tail_level_and_launches_per_cycle():
    m = PoissonMultigrid(2047, 2049, tail_points=0)
    assert len(m.levels) == 11 and m.tail_level is None and m.launches_per_cycle == 81
    m = PoissonMultigrid(2047, 2049, tail_points=257 * 257)
    assert m.levels[3] == (257, 257) and m.tail_level == 3 and m.launches_per_cycle == 8 * 3 + 1
    assert PoissonMultigrid(2047, 2049, tail_points=257 * 257 - 1).tail_level == 4
    assert PoissonMultigrid(2047, 2049).tail_level is None  # the default on CPU tensors is 0
    assert PoissonMultigrid(2047, 2049, tail_points=8).tail_level is None  # the coarsest level has 9 points
    assert PoissonMultigrid(2047, 2049, tail_points=9).tail_level == 10
    m = PoissonMultigrid(2047, 2049, tail_points=9)
    assert m.launches_per_cycle == 81  # 80 launches above it, one undamped sweep or one tail
    m = PoissonMultigrid(63, 129, max_levels=1, tail_points=ALL)
    assert m.tail_level is None and m.launches_per_cycle == 4
    m = PoissonMultigrid(63, 129, max_levels=2, tail_points=ALL)
    assert m.tail_level == 1 and m.launches_per_cycle == 9
    assert PoissonMultigrid(63, 129, max_levels=2, tail_points=0).launches_per_cycle == 8 + 50
    assert PoissonMultigrid(63, 129, nu1=1, nu2=2, tail_points=ALL).launches_per_cycle == 8
    assert set(PoissonMultigrid.DEFAULT_TAIL_POINTS) == {torch.float64, torch.float32}
    with pytest.raises(ValueError):
        PoissonMultigrid(63, 129, tail_points=-1)


def _grids(shapes, dtype=torch.float64, device="cpu"):
    return [tuple(torch.zeros(s, dtype=dtype, device=device) for _ in range(4)) for s in shapes]


def test_argument_refusals():
    good = _grids([(9, 17), (5, 9), (3, 5)])
    ops.mg_tail(good, 2, 2, 3, 0.8)
    ops.mg_tail([lv[:3] + (None,) if k == 2 else lv for k, lv in enumerate(good)], 2, 2, 3, 0.8)  # no r on the last level
    for nu1, nu2, cs, om in ((-1, 2, 3, 0.8), (2, 0, 3, 0.8), (2, 2, 0, 0.8), (2, 2, 3, 0.0), (2, 2, 3, -1.0),
                             (2, 2, 3, NAN), (2, 2, 3, float("inf"))):
        with pytest.raises(ValueError):
            ops.mg_tail(good, nu1, nu2, cs, om)
    bad_sets = [
        [],  # no level
        _grids([(3, 3)] * 17),  # too many
        _grids([(9, 17), (5, 8), (3, 5)]),  # not each other's coarse grids
        _grids([(9, 17), (4, 9)]),
        _grids([(5, 5), (3, 3), (2, 2)]),  # a level without an interior
        [good[0], good[1][:3] + (None,), good[2]],  # r missing above the last level
        [good[0], good[1][:3]],  # not a 4-tuple
        [good[0], (good[1][0], torch.zeros((5, 10), dtype=torch.float64)[:, :9]) + good[1][2:]],  # another pitch
        [good[0], (good[1][0], good[1][1], torch.zeros((5, 8), dtype=torch.float64), good[1][3])],  # another shape
        [good[0], tuple(t.to(torch.float32) for t in good[1])],  # another dtype
        [tuple(torch.zeros((17, 9), dtype=torch.float64).t() for _ in range(4))],  # stride(1) != 1
        _grids([(9, 17), (5, 9)], dtype=torch.float32),  # the CPU reference is float64
    ]
    for bad in bad_sets:
        with pytest.raises(ValueError):
            ops.mg_tail(bad, 2, 2, 3, 0.8)
    # the native entry points refuse the same, with nothing written
    L = _native.lib()
    bufs = _grids([(9, 17), (5, 9), (3, 5)])
    for lv in bufs:
        for t in lv:
            t.fill_(-7.0)

    def desc(edit=None):
        d = (_native.MgLevel * 3)()
        for k, (u, un, b, r) in enumerate(bufs):
            d[k] = _native.MgLevel(u.data_ptr(), un.data_ptr(), b.data_ptr(), r.data_ptr(), u.shape[0], u.shape[1],
                                   u.stride(0))
        if edit:
            edit(d)
        return d

    def setter(k, field, value):
        return lambda d: setattr(d[k], field, value)

    for fn in (L.mpx_mg_tail_f64, L.mpx_mg_tail_f32):
        assert fn(None, 3, 2, 2, 3, 0.8, None) != 0
        for n in (0, -1, 17):
            assert fn(desc(), n, 2, 2, 3, 0.8, None) != 0
        for nu1, nu2, cs, om in ((-1, 2, 3, 0.8), (2, 0, 3, 0.8), (2, 2, 0, 0.8), (2, 2, 3, 0.0), (2, 2, 3, NAN),
                                 (2, 2, 3, float("inf"))):
            assert fn(desc(), 3, nu1, nu2, cs, om, None) != 0
        for edit in (setter(0, "u", None), setter(1, "un", None), setter(2, "b", None), setter(1, "r", None),
                     setter(1, "w", 8), setter(1, "h", 4), setter(2, "pitch", 4), setter(0, "pitch", 16)):
            assert fn(desc(edit), 3, 2, 2, 3, 0.8, None) != 0
        assert fn(desc(setter(0, "h", 2)), 1, 2, 2, 3, 0.8, None) != 0
    assert b"invalid argument" in L.mpx_last_error()
    assert all(bool((t == -7.0).all()) for lv in bufs for t in lv)


def test_symbols():
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    for name in ("mpx_mg_tail_f64", "mpx_mg_tail_f32", "mpx_mg3_tail_f64", "mpx_mg3_tail_f32"):
        assert hasattr(raw, name), name
    assert not hasattr(raw, "mpx_cpu_mg_tail_f64")  # the CPU twin is the composition of the CPU operators
    assert ctypes.sizeof(_native.MgLevel) == 48 and ctypes.sizeof(_native.Mg3Level) == 56
    assert callable(ops.mg_tail) and callable(ops.mg3_tail)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("rows,cols,kw,what", CASES, ids=CASE_IDS)
def test_gpu_model_with_tail_bit_identical(gpu, dtype, rows, cols, kw, what):
    kw = {"tail_points": ALL, **kw}
    got, rgot = _cycles(gpu, dtype, rows, cols, **kw)
    want, rwant = _cycles(gpu, dtype, rows, cols, **{**kw, "tail_points": 0})
    assert got.tail_level == (2 if kw["tail_points"] != ALL else 1) and want.tail_level is None, what
    assert got.launches_per_cycle < want.launches_per_cycle
    _assert_same_state(got, rgot, want, rwant, what)
    if dtype == torch.float64:
        kw.pop("tail_points")
        cpu, rcpu = _cpu_launched(rows, cols, tuple(sorted(kw.items())))
        _assert_same_state(got, rgot, cpu, rcpu, ("against the CPU model", what))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_gpu_no_tail_on_a_single_level(gpu, dtype):
    got, rgot = _cycles(gpu, dtype, 63, 129, max_levels=1, tail_points=ALL)
    want, rwant = _cycles(gpu, dtype, 63, 129, max_levels=1, tail_points=0)
    assert got.tail_level is None and got.launches_per_cycle == want.launches_per_cycle == 4
    _assert_same_state(got, rgot, want, rwant, "one level")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_gpu_default_threshold(gpu, dtype):
    """tail_points=None takes the measured default, and the results do not depend on it."""
    got, rgot = _cycles(gpu, dtype, 63, 129)
    want, rwant = _cycles(gpu, dtype, 63, 129, tail_points=0)
    points = PoissonMultigrid.DEFAULT_TAIL_POINTS[dtype]
    assert got.tail_points == points
    assert got.tail_level == next((k for k, (h, w) in enumerate(got.levels) if k >= 1 and h * w <= points), None)
    _assert_same_state(got, rgot, want, rwant, "default")


def _padded(t: torch.Tensor, device, fill):
    """(view, backing): t in a view whose pitch exceeds its width by one
    16-byte vector (and the 16-byte rounding), in a backing buffer of ``fill``."""
    h, w = t.shape
    nv = NV[t.dtype]
    pitch = (w + nv - 1) // nv * nv + nv
    backing = torch.full((h, pitch), fill, dtype=t.dtype, device=device)
    view = backing[:, :w]
    view.copy_(t)
    return view, backing


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_gpu_op_pitch_padding_and_scratch(gpu, dtype):
    """``ops.mg_tail`` on pitched tensors with NaN in the padding, in every
    ``r`` and in every element of ``un`` that a sweep writes (rows 1 .. H - 2;
    rows 0 and H - 1 of ``un`` are input, the level's boundary values, as they
    are for ``jacobi_relax``): the padding keeps its bits and the results equal
    the unpadded run's and the launched sequence's. ``u`` of the lower levels
    is pre-filled with 7 (the tail zeroes it), their ``b`` with 5 inside and
    NaN on the boundary (never read)."""
    shapes = PoissonMultigrid.level_shapes(31, 65)[1:]  # (17, 33) ... (3, 5)
    assert shapes[0] == (17, 33) and shapes[-1] == (3, 5)
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
            pairs = {n: (_padded(t, gpu, NAN) if padded else (t.to(gpu),) * 2) for n, t in init.items()}
            levels.append(tuple(pairs[n][0] for n in ("u", "un", "b", "r")))
            backs.append({n: pairs[n][1] for n in pairs})
        ops.mg_tail(levels, 2, 2, 6, 0.8)
        torch.cuda.synchronize()
        results.append(levels)
        for (u, un, b, r), back in zip(levels, backs):
            w = u.shape[1]
            assert not bool(torch.isnan(u).any()) and not bool(torch.isnan(b[1:-1, 1:-1]).any())
            if padded:
                for name, t in back.items():
                    pad = t[:, w:]
                    assert pad.numel() > 0 and bool(torch.isnan(pad).all()), name
                    assert _same_bits(pad, torch.full(pad.shape, NAN, dtype=dtype)), name
    for k, (plain, padded) in enumerate(zip(*results)):
        assert _same_bits(plain[0], padded[0]), ("u of level", k)
        assert _same_bits(plain[2][1:-1, 1:-1], padded[2][1:-1, 1:-1]), ("b of level", k)
    # and equal to the launched sequence (the model's _vcycle on the same values)
    m = PoissonMultigrid(31, 65, dtype=dtype, device=gpu, tail_points=0, coarse_sweeps=6)
    m._lv[1].u.copy_(u0)
    m._lv[1].un.copy_(u0)
    m._lv[1].b.copy_(b0)
    m._vcycle(1)
    for k, lv in enumerate(m._lv[1:]):
        assert _same_bits(lv.u, results[0][k][0]), ("launched u of level", k + 1)


@pytest.mark.gpu
def test_gpu_cycle_with_tail_allocates_nothing(gpu):
    g = _problem(gpu, torch.float64, 63, 129, tail_points=ALL, nu1=1, nu2=2)  # odd counts: u / un swap every cycle
    assert g.tail_level == 1
    g.cycle()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    g.cycle()
    g.cycle()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before
