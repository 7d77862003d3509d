"""Kernel-level tests of the Jacobi sweep: sub-ranges, residuals, fp32 bits,
pitch > cols and every row-block shape of the wave kernel.

The oracle is a dtype-preserving plain-torch expression on the CPU
(``ref.jacobi(..., keep_dtype=True)``): the sweep is three correctly rounded
adds in a fixed association and an exact scale by 0.25, with nothing to
contract, so every comparison here is bit for bit, fp32 and fp64 alike, and
no assertion carries a tolerance. A sweep is row-local, so one full-height
reference and one per-row residual vector per (dtype, cols) serve every
sub-range: ``un`` is pre-filled with a sentinel, rows [r0, r1) must equal the
reference, every other row must still hold the sentinel, and the residual word
must equal the maximum of the per-row residuals of the range.
"""

from __future__ import annotations

import functools

import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.ops import reference as ref

SENT = -7.0  # inputs are in [0, 1): no output can equal it
# Fields: uniform on [0, 1), and nearly flat on [0.5, 0.5 + 2^-10). On the flat
# one every true difference is below 2^-10, while a difference taken by a lane
# that owns no output (a strip's halo lanes see 0 for the neighbour beyond the
# wave) or from a row outside the range is near 0.125: a residual that counts
# one is wrong by two orders of magnitude, whatever the random draw.
FIELDS = {"uniform": dict(scale=1.0, offset=0.0), "flat": dict(scale=2.0 ** -10, offset=0.5)}
DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _oracle(u: torch.Tensor):
    """(full-height reference, per-row residuals) of a CPU field; rowres[k]
    is max_j |s - c| of row k + 1, 0 where a row has no interior column."""
    h, cols = u.shape
    want = ref.jacobi(u, 1, h - 1, keep_dtype=True)
    assert want.dtype == u.dtype
    if cols > 2:
        rowres = (want[1:-1, 1:-1] - u[1:-1, 1:-1]).abs().amax(dim=1)
    else:
        rowres = torch.zeros(h - 2, dtype=u.dtype)
    return want, rowres


@functools.lru_cache(maxsize=None)
def _case(dtype, height: int, cols: int, scale: float = 1.0, offset: float = 0.0):
    """A seeded field in [offset, offset + scale) with its oracle, computed
    once and never modified. For fp64 the CPU library is tied in too: its
    output and returned residual equal the torch expression's."""
    g = torch.Generator().manual_seed(1000 * cols + height)
    u = (torch.rand((height, cols), generator=g, dtype=torch.float64) * scale + offset).to(dtype)
    want, rowres = _oracle(u)
    if dtype == torch.float64:
        unc = torch.full_like(u, SENT)
        r = ops.jacobi_sweep(u.clone(), unc, 1, height - 1)
        assert _same_bits(unc[1:-1], want[1:-1])
        assert r == float(rowres.max())
    return u, want, rowres


def _expected_res(rowres: torch.Tensor, r0: int, r1: int, start: float = 0.0) -> float:
    return max(float(rowres[r0 - 1:r1 - 1].max()), start) if r1 > r0 else start


def _assert_sweep(un, res, want, rowres, r0, r1, tag, start: float = 0.0):
    """The three assertions of a sweep of [r0, r1) into a sentinel-filled un."""
    assert _same_bits(un[r0:r1], want[r0:r1]), f"output differs: {tag}"
    assert bool((un[:r0] == SENT).all()) and bool((un[r1:] == SENT).all()), f"rows outside the range written: {tag}"
    if res is not None:
        got, exp = float(res.item()), _expected_res(rowres, r0, r1, start)
        assert got == exp, f"residual {got!r} != {exp!r}: {tag}"


def _variant(T, u, un, cols, pitch, r0, r1, res, R, aux):
    _native.check(T.mpx_jacobi_variant(u.data_ptr(), un.data_ptr(), cols, pitch, r0, r1,
                                       None if res is None else res.data_ptr(), int(u.dtype == torch.float64),
                                       R, aux, _native.stream_of(u)))


def _abi(u, un, cols, pitch, r0, r1, res):
    L = _native.lib()
    fn = L.mpx_jacobi_f64 if u.dtype == torch.float64 else L.mpx_jacobi_f32
    _native.check(fn(u.data_ptr(), un.data_ptr(), cols, pitch, r0, r1, None if res is None else res.data_ptr(),
                     _native.stream_of(u)))


# ---------------------------------------------------------------------------
# 1. production instantiation <T, 2, 0, true, false, true>, every row-block shape
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_production_instantiation_every_row_block(gpu, dtype):
    """aux = 18 is the production template with an explicit R. Row counts
    1..3R put the tail (1..R rows: whole 5-row groups plus 0-4 single steps)
    in block 0 (walking down), block 1 (walking up) and block 2 (down)."""
    T = _native.tune_lib()
    cols = 129 * NV[dtype]  # three strips, the last one partial
    height = 5 + 3 * 16 + 1
    launches = 0
    for field, kw in FIELDS.items():
        u, want, rowres = _case(dtype, height, cols, **kw)
        ud, wd = u.to(gpu), want.to(gpu)
        un = torch.empty_like(ud)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        for R in (1, 2, 3, 4, 5, 6, 7, 8, 11, 16):
            for r0 in (1, 2, 5) if field == "uniform" and R in (3, 5, 8, 11) else (1,):
                for n in range(1, 3 * R + 1):
                    r1 = r0 + n
                    assert r1 <= height - 1
                    un.fill_(SENT)
                    res.zero_()
                    _variant(T, ud, un, cols, cols, r0, r1, res, R, 18)
                    _assert_sweep(un, res, wd, rowres, r0, r1, (dtype, field, R, r0, r1))
                    launches += 1
    assert launches == 3 * (2 * 63 + 2 * 27)


# ---------------------------------------------------------------------------
# 2. column edges of the wave path (production launch, R = 1 at these sizes)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_wave_path_column_edges(gpu, dtype):
    """One vector, two, one short of a strip, exactly one 62-vector strip, one
    past it, two strips, two strips and one vector."""
    rows = 9
    for nvec in (1, 2, 61, 62, 63, 124, 125):
        cols = nvec * NV[dtype]
        for field, kw in FIELDS.items():
            u, want, rowres = _case(dtype, rows + 2, cols, **kw)
            ud = u.to(gpu)
            un = torch.full_like(ud, SENT)
            res = torch.zeros(1, dtype=dtype, device=gpu)
            ops.jacobi_sweep(ud, un, 1, rows + 1, res)
            _assert_sweep(un, res, want.to(gpu), rowres, 1, rows + 1, (dtype, field, cols))


# ---------------------------------------------------------------------------
# 3. generic kernels (16 rows per lane, 256 lanes per block)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_generic_kernel_small_and_block_edges(gpu, dtype):
    height = 33 + 3
    for cols in (1, 2, 3, 5, 255, 257, 513):
        u, want, rowres = _case(dtype, height, cols)
        ud, wd = u.to(gpu), want.to(gpu)
        un = torch.empty_like(ud)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        for rows in (1, 16, 17, 33):
            for r0 in (1, 2):
                un.fill_(SENT)
                res.zero_()
                ops.jacobi_sweep(ud, un, r0, r0 + rows, res)
                _assert_sweep(un, res, wd, rowres, r0, r0 + rows, (dtype, cols, r0, rows))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["u", "un", "both"])
def test_unaligned_base_takes_scalar_kernel(gpu, dtype, which):
    """A wave-path width on a base one element past a 16-byte boundary: the
    launcher must fall back to the scalar kernel, and the result is the same."""
    rows, cols = 17, 63 * NV[dtype]
    u, want, rowres = _case(dtype, rows + 2, cols)
    n = (rows + 2) * cols

    def place(src, shifted):
        flat = torch.empty(n + 8, dtype=dtype, device=gpu)
        v = flat[1:1 + n] if shifted else flat[:n]
        v = v.view(rows + 2, cols)
        v.copy_(src)
        assert v.is_contiguous() and (v.data_ptr() % 16 != 0) == shifted
        return v

    ud = place(u, which in ("u", "both"))
    un = place(torch.full_like(u, SENT), which in ("un", "both"))
    res = torch.zeros(1, dtype=dtype, device=gpu)
    ops.jacobi_sweep(ud, un, 1, rows + 1, res)
    _assert_sweep(un, res, want.to(gpu), rowres, 1, rows + 1, (dtype, which))


# ---------------------------------------------------------------------------
# 4. the overlapped distributed step's launch pattern
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["wave", "generic"])
def test_overlapped_step_launch_pattern(gpu, dtype, family):
    """Edge rows first, then the interior, all into one residual word zeroed
    once (SlabJacobi._advance); n = 1 and n = 2 leave the interior empty."""
    cols = 70 * NV[dtype] if family == "wave" else 257
    for n in (37, 1, 2):
        u, want, rowres = _case(dtype, n + 2, cols)
        ud, wd = u.to(gpu), want.to(gpu)
        full = torch.full_like(ud, SENT)
        rfull = torch.zeros(1, dtype=dtype, device=gpu)
        ops.jacobi_sweep(ud, full, 1, n + 1, rfull)
        _assert_sweep(full, rfull, wd, rowres, 1, n + 1, (dtype, family, n, "full"))

        un = torch.full_like(ud, SENT)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        for r in ([1] if n == 1 else [1, n]):
            ops.jacobi_sweep(ud, un, r, r + 1, res)
        if n >= 2:  # the model skips r1 < r0; r0 == r1 reaches the library
            ops.jacobi_sweep(ud, un, 2, n, res)
        _assert_sweep(un, res, wd, rowres, 1, n + 1, (dtype, family, n, "overlapped"))
        assert _same_bits(un, full) and _same_bits(res, rfull), (dtype, family, n)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_range_is_a_no_op(gpu, dtype):
    for cols in (70 * NV[dtype], 257):
        u, _, _ = _case(dtype, 6, cols)
        ud = u.to(gpu)
        un = torch.full_like(ud, SENT)
        res = torch.full((1,), 0.3125, dtype=dtype, device=gpu)
        for r in (1, 3, 5):
            ops.jacobi_sweep(ud, un, r, r, res)
        ops.jacobi_sweep(ud, un, 2, 2, None)
        assert bool((un == SENT).all()) and float(res.item()) == 0.3125, (dtype, cols)


# ---------------------------------------------------------------------------
# 5. residual accumulation semantics
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["wave", "generic"])
def test_residual_accumulates_a_maximum(gpu, dtype, family):
    rows = 21
    cols = 70 * NV[dtype] if family == "wave" else 257
    # values in [0, 0.75): every difference |s - c| is below 0.75 (on [0, 1) the
    # maximum of such a field is about 0.85)
    u, want, rowres = _case(dtype, rows + 2, cols, scale=0.75)
    ud, wd = u.to(gpu), want.to(gpu)
    true_max = float(rowres.max())
    assert float(u.max()) < 0.75 and 0.0 < true_max < 0.75
    below = float(torch.tensor(true_max / 2, dtype=dtype))
    # a start above any possible difference stays; a lower one is raised to
    # exactly the true maximum; zero is the plain case
    for start in (0.75, below, 0.0):
        un = torch.full_like(ud, SENT)
        res = torch.full((1,), start, dtype=dtype, device=gpu)
        ops.jacobi_sweep(ud, un, 1, rows + 1, res)
        _assert_sweep(un, res, wd, rowres, 1, rows + 1, (dtype, family, start), start=start)
        assert float(res.item()) == (0.75 if start == 0.75 else true_max)
    # two sweeps of different ranges fold into one word
    un = torch.full_like(ud, SENT)
    res = torch.zeros(1, dtype=dtype, device=gpu)
    k = int(rowres.argmax()) + 1  # the row that holds the maximum
    lo = (1, k) if k > 1 else (k + 1, rows + 1)  # a range without it
    ops.jacobi_sweep(ud, un, k, k + 1, res)
    ops.jacobi_sweep(ud, un, lo[0], lo[1], res)
    assert float(res.item()) == true_max, (dtype, family, "max first")
    res.zero_()
    ops.jacobi_sweep(ud, un, lo[0], lo[1], res)
    assert float(res.item()) == _expected_res(rowres, lo[0], lo[1]) < true_max
    ops.jacobi_sweep(ud, un, k, k + 1, res)
    assert float(res.item()) == true_max, (dtype, family, "max last")
    # no residual word: same output
    un = torch.full_like(ud, SENT)
    ops.jacobi_sweep(ud, un, 1, rows + 1, None)
    _assert_sweep(un, None, wd, rowres, 1, rows + 1, (dtype, family, "resid=None"))


# ---------------------------------------------------------------------------
# 6. pitch > cols through the C ABI
# ---------------------------------------------------------------------------
def _pitch_cases(dtype):
    nv = NV[dtype]
    return {"wave": (63 * nv, 65 * nv), "vector": (63 * nv + 1, 64 * nv), "scalar": (63 * nv, 63 * nv + 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", ["wave", "vector", "scalar"])
def test_pitch_wider_than_cols(gpu, dtype, path):
    """NaN in the padding of u must reach no output or residual; the padding
    of un must keep its sentinel."""
    cols, pitch = _pitch_cases(dtype)[path]
    rows = 19
    u, want, rowres = _case(dtype, rows + 2, cols)
    wd = want.to(gpu)
    ud = torch.full((rows + 2, pitch), float("nan"), dtype=dtype, device=gpu)
    ud[:, :cols] = u.to(gpu)
    for r0, r1 in ((1, rows + 1), (3, rows - 1)):
        un = torch.full_like(ud, SENT)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        _abi(ud, un, cols, pitch, r0, r1, res)
        tag = (dtype, path, r0, r1)
        assert not bool(torch.isnan(un).any()), tag
        assert bool((un[:, cols:] == SENT).all()), f"padding written: {tag}"
        _assert_sweep(un[:, :cols], res, wd, rowres, r0, r1, tag)


# ---------------------------------------------------------------------------
# 7. the other tuning forms of the wave kernel
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("aux", [0, 2, 6, 10, 22, 50])
def test_tuning_forms(gpu, dtype, aux):
    """Store policy, non-temporal loads, no tail exit, non-temporal interior
    rows, 16-wave workgroups: same output (boundary columns included), same
    untouched rows, same residual, on ranges that leave a tail block."""
    T = _native.tune_lib()
    cols = 129 * NV[dtype]
    height = 40
    u, want, rowres = _case(dtype, height, cols)
    ud, wd = u.to(gpu), want.to(gpu)
    un = torch.empty_like(ud)
    res = torch.zeros(1, dtype=dtype, device=gpu)
    for R in (5, 8):
        for r0, n in ((1, 2 * R + 3), (3, R + 2), (3, 3 * R + 4), (2, 4)):
            un.fill_(SENT)
            res.zero_()
            _variant(T, ud, un, cols, cols, r0, r0 + n, res, R, aux)
            _assert_sweep(un, res, wd, rowres, r0, r0 + n, (dtype, aux, R, r0, r0 + n))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_tail_exit_residual_ignores_surplus_rows(gpu, dtype):
    """aux = 10 runs the tail as a whole 5-row group on clamped rows and drops
    the surplus stores; their differences must not reach the residual. Rows
    [0, r1) are constant 0.5 and the rows below random: the range's true
    residual comes from its last row alone and is at most 0.125, while a
    surplus step centred on the random row r1 shows as a larger value."""
    T = _native.tune_lib()
    cols = 129 * NV[dtype]
    height = 24
    for R, r0, r1 in ((5, 1, 14), (8, 1, 20), (5, 3, 10), (8, 2, 5)):
        g = torch.Generator().manual_seed(r1)
        u = torch.rand((height, cols), generator=g, dtype=torch.float64).to(dtype)
        u[:r1] = 0.5
        want, rowres = _oracle(u)
        assert 0.0 < float(rowres[:r1 - 1].max()) <= 0.125 < float(rowres[r1 - 1])
        ud = u.to(gpu)
        un = torch.full_like(ud, SENT)
        res = torch.zeros(1, dtype=dtype, device=gpu)
        _variant(T, ud, un, cols, cols, r0, r1, res, R, 10)
        _assert_sweep(un, res, want.to(gpu), rowres, r0, r1, (dtype, R, r0, r1))


# ---------------------------------------------------------------------------
# argument refusals (returned before any launch)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_refusals(gpu):
    u = torch.zeros((6, 8), dtype=torch.float64, device=gpu)
    un = torch.full_like(u, SENT)
    with pytest.raises(_native.MpxError):
        _abi(u, un, 8, 8, 3, 2, None)  # r1 < r0
    with pytest.raises(_native.MpxError):
        _abi(u, un, 8, 6, 1, 5, None)  # pitch < cols
    with pytest.raises(_native.MpxError):
        _abi(u, un, 8, 8, 0, 5, None)  # row 0 is a halo row
    with pytest.raises(_native.MpxError):
        _native.check(_native.lib().mpx_jacobi_f64(None, un.data_ptr(), 8, 8, 1, 5, None, None))
    T = _native.tune_lib()
    with pytest.raises(_native.MpxError, match="vector layout"):
        _variant(T, u, un, 7, 8, 1, 5, None, 1, 18)
    with pytest.raises(_native.MpxError):
        _variant(T, u, un, 8, 8, 1, 5, None, 1, 3)  # not a tuning form
    with pytest.raises(ValueError):
        ops.jacobi_sweep(u, un, 1, 6)  # r1 past the bottom halo row
    torch.cuda.synchronize()
    assert bool((un == SENT).all())


# ---------------------------------------------------------------------------
# CPU library (no GPU needed)
# ---------------------------------------------------------------------------
def _cpu(u, un, cols, pitch, r0, r1) -> float:
    return _native.lib().mpx_cpu_jacobi_f64(u.data_ptr(), un.data_ptr(), cols, pitch, r0, r1)


@pytest.mark.parametrize("cols", [1, 2, 3, 4, 37])
@pytest.mark.parametrize("pad", [0, 1, 5])
def test_cpu_jacobi_pitch_and_subranges(cols, pad):
    rows, pitch = 11, cols + pad
    u, want, rowres = _case(torch.float64, rows + 2, cols)
    up = torch.full((rows + 2, pitch), float("nan"), dtype=torch.float64)
    up[:, :cols] = u
    for r0, r1 in ((1, rows + 1), (1, 2), (rows, rows + 1), (2, rows), (4, 9), (5, 5)):
        un = torch.full_like(up, SENT)
        r = _cpu(up, un, cols, pitch, r0, r1)
        tag = (cols, pitch, r0, r1)
        assert not bool(torch.isnan(un).any()), tag
        assert bool((un[:, cols:] == SENT).all()), f"padding written: {tag}"
        _assert_sweep(un[:, :cols], None, want, rowres, r0, r1, tag)
        assert r == _expected_res(rowres, r0, r1), tag


def test_cpu_sweep_keeps_the_larger_residual():
    rows, cols = 9, 21
    u, want, rowres = _case(torch.float64, rows + 2, cols, scale=0.75)
    true_max = float(rowres.max())
    assert float(u.max()) < 0.75 and 0.0 < true_max < 0.75
    for start in (0.75, true_max / 2, 0.0):
        un = torch.full_like(u, SENT)
        res = torch.full((1,), start, dtype=torch.float64)
        r = ops.jacobi_sweep(u.clone(), un, 1, rows + 1, res)
        assert r == true_max
        _assert_sweep(un, res, want, rowres, 1, rows + 1, start, start=start)
    # sub-ranges fold into one word, as in the overlapped step
    un = torch.full_like(u, SENT)
    res = torch.zeros(1, dtype=torch.float64)
    for r0, r1 in ((1, 2), (rows, rows + 1), (2, rows)):
        ops.jacobi_sweep(u.clone(), un, r0, r1, res)
    _assert_sweep(un, res, want, rowres, 1, rows + 1, "overlapped")


def test_oracle_matches_a_scalar_loop():
    """The torch expression against a plain loop, fp32 through numpy scalars
    (each operation rounded to fp32), so the oracle itself is pinned."""
    import numpy as np

    for dtype, npt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        for cols in (1, 2, 3, 4, 9):
            u, want, rowres = _case(dtype, 5, cols)
            a = u.numpy()
            exp = a.copy()
            rr = np.zeros(3, dtype=npt)
            for i in range(1, 4):
                for j in range(1, cols - 1):
                    s = npt(npt(npt(a[i - 1, j] + a[i + 1, j]) + npt(a[i, j - 1] + a[i, j + 1])) * npt(0.25))
                    exp[i, j] = s
                    rr[i - 1] = max(rr[i - 1], abs(npt(s - a[i, j])))
            assert exp.tobytes() == want.numpy().tobytes(), (dtype, cols)
            assert rr.tobytes() == rowres.numpy().tobytes(), (dtype, cols)
