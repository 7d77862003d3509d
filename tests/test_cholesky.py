"""Dense Cholesky of SPD matrices (``ops.cholesky_factor`` and friends,
``DenseCholesky``): row-major fp64, lower storage.

Only the lower triangle is the factorisation's business: every matrix here
carries NaN in its strict upper triangle and a sentinel in its pitch padding,
and both must come back bit for bit. Layouts: contiguous, pitch n + 2, pitch
n + 3 (for every n one of the two is odd, which leaves every second row only
8-byte aligned).

A. Exact recovery, ``array_equal``. L has off-diagonal entries from
   {0, +-0.25, +-0.5, +-1} and a diagonal from {1, 2, 3, 4, 5, 8}; A = L L^T;
   X has integer entries in [-8, 8]; B = A X. Every intermediate of the
   factorisation and of the two substitutions is a multiple of 2^-4 far below
   2^53 * 2^-4, hence exact in any summation order, fused or not; the square
   roots are of perfect squares; every quotient is (l_ij l_jj) / l_jj or
   (l_ii y_i) / l_ii, representable, which IEEE division returns exactly and a
   multiplication by a rounded 1/3 or 1/5 does not.

B. Higham's bounds (Accuracy and Stability, ch. 10) in ``np.longdouble``, with
   u = 2^-53, gamma_m = m u / (1 - m u):
       |A - L L^T| <= gamma_{n+1} |L||L^T|          (lower triangle)
       |B - L L^T X| <= gamma_{3n} |L||L^T||X|      (elementwise)
   Derived, not tuned; LAPACK sits at 0.013-0.015 and 0.001-0.002 of them on
   these matrices.

C. Bits. The diagonal block and the first panel solve are plain VALU in the CPU
   reference's operation order, so the GPU equals the CPU reference bit for bit
   for n <= 64 (factor and solve) and in columns 0..63 of L for any n.

D. Not positive definite, all exact: family A at n = 200 with one diagonal entry
   lowered so that the reduced pivot is exactly 0 or -1, or replaced by NaN.

E. The three phases of the first panel step alone, exact.

F. Plumbing.

Sizes: the MFMA tile is 16 (1, 2, 15..17), the panel and the update tile 64
(63..65: 65 is one trailing row; 127..129), 193 is three panels (the second
update has a full off-diagonal tile and ragged diagonal ones), 257, 321, and
1100 for many tiles ragged both ways.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.models import DenseCholesky

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
LAYOUTS = {"contig": 0, "even": 2, "odd": 3}  # excess of the row pitch over the width
SENT = -7777.25
LD = np.longdouble
U53 = LD(2.0) ** -53
NRHS = (1, 3, 17, 65)


@pytest.fixture
def dev(request):
    if request.param == "cuda":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def _gamma(m):
    return LD(m) * U53 / (LD(1) - LD(m) * U53)


def _place(arr: np.ndarray, layout: str, device):
    """``arr`` as the leading columns of a sentinel-filled pitched buffer."""
    r, c = arr.shape
    back = torch.full((r, c + LAYOUTS[layout]), SENT, dtype=torch.float64, device=device)
    view = back[:, :c]
    view.copy_(torch.from_numpy(np.array(arr, dtype=np.float64)))
    return view, back


def _place_lower(arr: np.ndarray, layout: str, device):
    """The lower triangle of ``arr`` under a strict upper triangle of NaN."""
    low = np.array(arr, dtype=np.float64)
    low[np.triu_indices(low.shape[0], 1)] = np.nan
    return _place(low, layout, device)


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().copy()


def _untouched(view: torch.Tensor, back: torch.Tensor) -> bool:
    """The strict upper triangle is still NaN and the padding still the sentinel."""
    n = view.shape[0]
    upper = _np(view)[np.triu_indices(n, 1)]
    return bool(np.isnan(upper).all()) and bool((back[:, view.shape[1]:] == SENT).all())


def _padding_kept(back: torch.Tensor, c: int) -> bool:
    return bool((back[:, c:] == SENT).all())


@functools.lru_cache(maxsize=None)
def _exact_family(n: int, seed: int = 0):
    """(A, L) of yardstick A; shared, never modified."""
    rng = np.random.RandomState(1000 * seed + n)
    low = np.tril(rng.choice([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0], size=(n, n)), -1)
    low += np.diag(rng.choice([1.0, 2.0, 3.0, 4.0, 5.0, 8.0], size=n))
    a = low @ low.T
    assert np.array_equal(a * 16, np.round(a * 16)) and np.abs(a).max() < 2.0 ** 11
    for m in (a, low):
        m.setflags(write=False)
    return a, low


@functools.lru_cache(maxsize=None)
def _spd(n: int, graded: bool = False) -> np.ndarray:
    g = np.random.RandomState(7 + n).standard_normal((n, n))
    a = g @ g.T + n * np.eye(n)
    if graded:  # condition number 1e17, yet it factors: success depends on the scaled matrix
        d = 10.0 ** np.linspace(-4, 4, n)
        a = d[:, None] * a * d[None, :]
    a = np.tril(a) + np.tril(a, -1).T
    a.setflags(write=False)
    return a


def _ld_ok():
    if np.finfo(LD).eps >= 2.0 ** -60:
        pytest.skip("np.longdouble is not an extended format here")


def _factor_bound(a: np.ndarray, l: np.ndarray) -> float:
    """max over the lower triangle of |A - L L^T| / (gamma_{n+1} |L||L^T|)."""
    n = a.shape[0]
    low = np.tril(l).astype(LD)
    assert np.all(np.isfinite(np.tril(l)))
    tri = np.tril_indices(n)
    res = np.abs(a.astype(LD) - low @ low.T)[tri]
    bound = (_gamma(n + 1) * (np.abs(low) @ np.abs(low.T)))[tri]
    assert np.all(res <= bound), float(np.max(res - bound))
    return float(np.max(res / np.where(bound > 0, bound, LD(1))))


def _solve_bound(l: np.ndarray, b: np.ndarray, x: np.ndarray) -> float:
    n = l.shape[0]
    b, x = b.reshape(n, -1), x.reshape(n, -1)
    assert np.all(np.isfinite(x))
    low = np.tril(l).astype(LD)
    res = np.abs(b.astype(LD) - low @ (low.T @ x.astype(LD)))
    bound = _gamma(3 * n) * (np.abs(low) @ (np.abs(low.T) @ np.abs(x.astype(LD))))
    assert np.all(res <= bound), float(np.max(res - bound))
    return float(np.max(res / np.where(bound > 0, bound, LD(1))))


def _check_exact(n: int, layout: str, device, seed: int = 0):
    a, low = _exact_family(n, seed)
    view, back = _place_lower(a, layout, device)
    out, info = ops.cholesky_factor_(view)
    assert out.data_ptr() == view.data_ptr()
    assert info.dtype == torch.int32 and info.shape == (1,) and info.device == view.device
    assert int(info.item()) == 0
    assert np.array_equal(np.tril(_np(out)), low)
    assert _untouched(view, back)
    return out


# ---------------------------------------------------------------- A. exact recovery
EXACT_N = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193, 257, 321]
EXACT_CASES = [(n, layout) for n in EXACT_N for layout in LAYOUTS] + [(1100, "contig"), (1100, "odd")]


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n,layout", EXACT_CASES)
def test_exact_factor_and_solve(n, layout, dev):
    a = _exact_family(n)[0]
    l = _check_exact(n, layout, dev)
    rng = np.random.RandomState(n)
    for nrhs in NRHS:
        x = rng.randint(-8, 9, size=(n, nrhs)).astype(np.float64)
        bview, bback = _place(a @ x, layout, dev)
        got = ops.cholesky_solve_(l, bview)
        assert got.data_ptr() == bview.data_ptr()
        assert np.array_equal(_np(got), x), (n, nrhs)
        assert _padding_kept(bback, nrhs)
    x = rng.randint(-8, 9, size=n).astype(np.float64)
    b = torch.from_numpy(a @ x).to(dev)
    keep = b.clone()
    got = ops.cholesky_solve(l, b)
    assert got.shape == (n,) and np.array_equal(_np(got), x)
    assert torch.equal(b, keep)
    # a 1-D right-hand side that is a column of a wider buffer
    wide = torch.full((n, 3), SENT, dtype=torch.float64, device=dev)
    wide[:, 1] = keep
    ops.cholesky_solve_(l, wide[:, 1])
    assert np.array_equal(_np(wide[:, 1]), x)
    assert bool((wide[:, 0] == SENT).all()) and bool((wide[:, 2] == SENT).all())


# ---------------------------------------------------------------- B. bounds
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n,graded", [(65, False), (300, False), (129, True)])
def test_bounds(n, graded, layout, dev):
    _ld_ok()
    a = _spd(n, graded)
    view, back = _place_lower(a, layout, dev)
    l, info = ops.cholesky_factor_(view)
    assert int(info.item()) == 0
    l_np = _np(l)
    ratio = _factor_bound(a, l_np)
    assert _untouched(view, back)
    b = np.random.RandomState(n).standard_normal((n, 17))
    bview, bback = _place(b, layout, dev)
    x = ops.cholesky_solve_(l, bview)
    ratio_s = _solve_bound(l_np, b, _np(x))
    assert _padding_kept(bback, 17)
    print(f"n={n} graded={graded} {layout} {dev}: factor {ratio:.4f}, solve {ratio_s:.4f} of the bound")


# ---------------------------------------------------------------- C. bits
@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 7, 33, 64])
def test_gpu_equals_cpu_reference_up_to_one_panel(n, layout, gpu):
    a = _spd(n)
    cview, _ = _place_lower(a, layout, torch.device("cpu"))
    gview, gback = _place_lower(a, layout, gpu)
    cl, cinfo = ops.cholesky_factor_(cview)
    gl, ginfo = ops.cholesky_factor_(gview)
    assert int(cinfo.item()) == 0 and int(ginfo.item()) == 0
    assert torch.equal(torch.tril(gl).cpu(), torch.tril(cl))
    assert _untouched(gview, gback)
    for nrhs in (1, 5):
        b = np.random.RandomState(n + nrhs).standard_normal((n, nrhs))
        cb, _ = _place(b, layout, torch.device("cpu"))
        gb, gbb = _place(b, layout, gpu)
        assert torch.equal(ops.cholesky_solve_(gl, gb).cpu(), ops.cholesky_solve_(cl, cb))
        assert _padding_kept(gbb, nrhs)


@pytest.mark.gpu
def test_gpu_first_panel_equals_cpu_reference(gpu):
    n = 300
    a = _spd(n)
    cl, _ = ops.cholesky_factor(torch.from_numpy(a.copy()))
    gl, _ = ops.cholesky_factor(torch.from_numpy(a.copy()).to(gpu))
    assert torch.equal(torch.tril(gl)[:, :64].cpu(), torch.tril(cl)[:, :64])


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_runs_and_layouts_give_the_same_bits(dev):
    n = 321
    a = _spd(n)
    b = np.random.RandomState(5).standard_normal((n, 5))
    seen = []
    for layout in ("contig", "contig", "even", "odd"):
        view, back = _place_lower(a, layout, dev)
        l, _ = ops.cholesky_factor_(view)
        bview, _ = _place(b, layout, dev)
        x = ops.cholesky_solve_(l, bview)
        assert _untouched(view, back)
        seen.append((np.tril(_np(l)), _np(x)))
    for l_np, x_np in seen[1:]:
        assert np.array_equal(l_np, seen[0][0]) and np.array_equal(x_np, seen[0][1])


# ---------------------------------------------------------------- D. not positive definite
BAD_K = [0, 37, 63, 64, 96, 199]


def _spoil(a: np.ndarray, low: np.ndarray, k: int, kind: str) -> None:
    if kind == "zero":  # the reduced pivot a_kk - sum_{j < k} l_kj^2 becomes exactly 0
        a[k, k] = a[k, k] - low[k, k] ** 2
    elif kind == "minus_one":
        a[k, k] = a[k, k] - low[k, k] ** 2 - 1.0
    else:
        a[k, k] = np.nan


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["zero", "minus_one", "nan"])
@pytest.mark.parametrize("k", BAD_K)
def test_not_positive_definite(k, kind, layout, dev):
    n = 200
    a0, low = _exact_family(n)
    a = a0.copy()
    _spoil(a, low, k, kind)
    view, back = _place_lower(a, layout, dev)
    l, info = ops.cholesky_factor_(view)
    assert int(info.item()) == k + 1
    assert np.array_equal(np.tril(_np(l))[:, :k], low[:, :k])
    assert _untouched(view, back)
    full = torch.from_numpy(np.tril(a) + np.tril(a, -1).T).to(dev)
    with pytest.raises(RuntimeError, match=rf"solve_spd: the matrix is not positive definite \(column {k}\)"):
        ops.solve_spd(full, torch.ones(n, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match=rf"not positive definite \(column {k}\)"):
        DenseCholesky(full)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("first,second", [(37, 63), (37, 96), (64, 199), (63, 64)])
def test_first_bad_column_is_reported(first, second, dev):
    n = 200
    a0, low = _exact_family(n)
    a = a0.copy()
    _spoil(a, low, second, "nan")
    _spoil(a, low, first, "zero")
    view, back = _place_lower(a, "odd", dev)
    l, info = ops.cholesky_factor_(view)
    assert int(info.item()) == first + 1
    assert np.array_equal(np.tril(_np(l))[:, :first], low[:, :first])
    assert _untouched(view, back)


# ---------------------------------------------------------------- E. phases
@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gpu_phases_of_the_first_panel(layout, gpu):
    n = 200
    a, low = _exact_family(n)
    view, back = _place_lower(a, layout, gpu)
    info = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    L = _native.lib()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for phase in (0, 1, 2):
        _native.check(L.mpx_chol_phase_f64(view.data_ptr(), n, view.stride(0), info.data_ptr(), 0, phase, stream))
    torch.cuda.synchronize(gpu)
    assert int(info.item()) == 0
    got = np.tril(_np(view))
    assert np.array_equal(got[:, :64], low[:, :64])
    rest = low[64:, 64:]
    assert np.array_equal(got[64:, 64:], np.tril(rest @ rest.T))  # the Schur complement sum_{j >= 64} l_j l_j^T
    assert _untouched(view, back)
    ARG = 1
    assert L.mpx_chol_phase_f64(view.data_ptr(), n, view.stride(0), info.data_ptr(), 32, 0, stream) == ARG
    assert L.mpx_chol_phase_f64(view.data_ptr(), n, view.stride(0), info.data_ptr(), 256, 0, stream) == ARG
    assert L.mpx_chol_phase_f64(view.data_ptr(), n, view.stride(0), info.data_ptr(), 0, 3, stream) == ARG


# ---------------------------------------------------------------- F. plumbing
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_copies_views_and_streams(dev):
    n = 200
    a, low = _exact_family(n)
    t = torch.from_numpy(a.copy()).to(dev)
    keep = t.clone()
    l, info = ops.cholesky_factor(t)
    assert torch.equal(t, keep) and l.data_ptr() != t.data_ptr() and int(info.item()) == 0
    assert np.array_equal(np.tril(_np(l)), low)
    assert torch.equal(torch.triu(l, 1), torch.triu(keep, 1))  # the copy's upper triangle is the input's
    same, _ = ops.cholesky_factor_(t)
    assert same.data_ptr() == t.data_ptr() and torch.equal(same, l)
    # every second row of a taller buffer: the pitch is 2 n
    tall = torch.full((2 * n, n), SENT, dtype=torch.float64, device=dev)
    tall[::2] = keep
    out, _ = ops.cholesky_factor_(tall[::2])
    assert torch.equal(out, l) and bool((tall[1::2] == SENT).all())
    # the solution through solve_spd() and the model; A and B untouched
    x = np.random.RandomState(1).randint(-8, 9, size=(n, 3)).astype(np.float64)
    b = torch.from_numpy(a @ x).to(dev)
    bkeep = b.clone()
    assert np.array_equal(_np(ops.solve_spd(keep, b)), x) and torch.equal(b, bkeep)
    model = DenseCholesky(keep)
    assert np.array_equal(_np(model.solve(b)), x) and torch.equal(model.l, l) and model.n == n
    assert np.array_equal(_np(keep), a)
    assert np.array_equal(_np(model.solve(b[:, 0])), x[:, 0])
    if dev.type == "cuda":
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            t2 = keep.clone()
            l2, info2 = ops.cholesky_factor_(t2)
            x2 = ops.cholesky_solve(l2, b)
        side.synchronize()
        assert torch.equal(l2, l) and np.array_equal(_np(x2), x) and int(info2.item()) == 0


@pytest.mark.gpu
def test_gpu_back_to_back_on_one_stream(gpu):
    """Factorisations queued on one stream that share one info word: a matrix
    that is not positive definite, then two that are. The word is the last
    call's, and no state of one call reaches the next."""
    L = _native.lib()
    n = 321
    fam = [_exact_family(n, seed) for seed in (1, 2, 3)]
    spoilt = fam[0][0].copy()
    _spoil(spoilt, fam[0][1], 70, "minus_one")
    mats = [torch.from_numpy(m).to(gpu) for m in (spoilt, fam[1][0].copy(), fam[2][0].copy())]
    info = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    seen = []
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for m in mats:
        _native.check(L.mpx_chol_factor_f64(m.data_ptr(), n, n, info.data_ptr(), stream))
        seen.append(info.clone())  # stream-ordered copy
    torch.cuda.synchronize(gpu)
    assert [int(i.item()) for i in seen] == [71, 0, 0]
    for (a, low), m in zip(fam[1:], mats[1:]):
        assert np.array_equal(np.tril(_np(m)), low)


@pytest.mark.gpu
def test_gpu_factor_cpu_solve_and_back(gpu):
    _ld_ok()
    n = 300
    cpu = torch.device("cpu")
    a, low = _exact_family(n)
    x = np.random.RandomState(3).randint(-8, 9, size=(n, 5)).astype(np.float64)
    b = a @ x
    g_l, _ = ops.cholesky_factor(torch.from_numpy(a.copy()).to(gpu))
    c_l, _ = ops.cholesky_factor(torch.from_numpy(a.copy()))
    assert np.array_equal(_np(ops.cholesky_solve(g_l.cpu(), torch.from_numpy(b.copy()))), x)
    assert np.array_equal(_np(ops.cholesky_solve(c_l.to(gpu), torch.from_numpy(b.copy()).to(gpu))), x)
    a = _spd(n)
    b = np.random.RandomState(9).standard_normal((n, 5))
    g_l, _ = ops.cholesky_factor(torch.from_numpy(a.copy()).to(gpu))
    c_l, _ = ops.cholesky_factor(torch.from_numpy(a.copy()).to(cpu))
    _solve_bound(_np(g_l), b, _np(ops.cholesky_solve(g_l.cpu(), torch.from_numpy(b.copy()))))
    _solve_bound(_np(c_l), b, _np(ops.cholesky_solve(c_l.to(gpu), torch.from_numpy(b.copy()).to(gpu))))


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [1, 17, 200, 257])
def test_logdet_exact_family(n, dev):
    """The factor's diagonal is the constructed one exactly, so the only errors
    are the logarithms' and the sum's. With S = sum |log l_ii| (terms at most
    log 8): each log within 2 ulp of a term (2 * 2^-52 relative), n - 1
    additions in any order within (n - 1) 2^-53 S, the doubling exact, and the
    same again for the float64 reference below: |got - want| <= 2 S (n + 8) 2^-53."""
    a, low = _exact_family(n)
    l, _ = ops.cholesky_factor(torch.from_numpy(a.copy()).to(dev))
    got = ops.logdet_spd(l)
    assert got.dim() == 0 and got.dtype == torch.float64 and got.device == l.device
    logs = [math.log(v) for v in np.diag(low)]
    want = 2.0 * math.fsum(logs)
    bound = 2.0 * math.fsum(abs(v) for v in logs) * (n + 8) * 2.0 ** -53
    assert abs(float(got) - want) <= bound
    assert float(DenseCholesky(torch.from_numpy(a.copy()).to(dev)).logdet()) == float(got)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [65, 300])
def test_dense_cholesky_inverse_and_solve(n, dev):
    _ld_ok()
    a = _spd(n)
    m = DenseCholesky(torch.from_numpy(a.copy()).to(dev))
    inv = m.inverse()
    assert inv.shape == (n, n)
    _factor_bound(a, _np(m.l))
    _solve_bound(_np(m.l), np.eye(n), _np(inv))  # A inv against the identity, through A's computed factor
    b = np.random.RandomState(2).standard_normal(n)
    _solve_bound(_np(m.l), b, _np(m.solve(torch.from_numpy(b).to(dev))))


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_value_errors_and_empty_systems(dev):
    a = 4.0 * torch.eye(4, dtype=torch.float64, device=dev)
    l, info = ops.cholesky_factor(a)
    assert int(info.item()) == 0 and torch.equal(l, 2.0 * torch.eye(4, dtype=torch.float64, device=dev))
    b = torch.ones(4, dtype=torch.float64, device=dev)
    for fn in (ops.cholesky_factor, ops.cholesky_factor_, ops.logdet_spd):
        with pytest.raises(ValueError, match="fp64 only"):
            fn(a.float())
        with pytest.raises(ValueError):
            fn("a")
    with pytest.raises(ValueError, match="fp64 only"):
        ops.cholesky_solve(l, b.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.cholesky_solve_(l.float(), b)
    with pytest.raises(ValueError, match="fp64 only"):
        ops.solve_spd(a, b.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.solve_spd(a.float(), b)
    for bad in (torch.ones(4, dtype=torch.float64, device=dev), torch.ones(2, 4, 4, dtype=torch.float64, device=dev),
                torch.ones(4, 5, dtype=torch.float64, device=dev), torch.ones(5, 4, dtype=torch.float64, device=dev),
                torch.ones(4, 8, dtype=torch.float64, device=dev)[:, ::2],
                torch.ones(4, 4, dtype=torch.float64, device=dev).t(),  # stride(1) != 1
                torch.ones(1, 4, dtype=torch.float64, device=dev).expand(4, 4)):  # row stride 0 < n
        for fn in (ops.cholesky_factor_, ops.cholesky_factor, ops.logdet_spd, DenseCholesky):
            with pytest.raises(ValueError):
                fn(bad)
        with pytest.raises(ValueError):
            ops.solve_spd(bad, b)
        with pytest.raises(ValueError):
            ops.cholesky_solve(bad, b)
        with pytest.raises(ValueError):
            ops.cholesky_solve_(bad, b)
    for bad_b in (torch.ones(5, dtype=torch.float64, device=dev), torch.ones(3, 2, dtype=torch.float64, device=dev),
                  torch.ones(4, 2, 2, dtype=torch.float64, device=dev), "b"):
        with pytest.raises(ValueError):
            ops.cholesky_solve_(l, bad_b)
        with pytest.raises(ValueError):
            ops.cholesky_solve(l, bad_b)
        with pytest.raises(ValueError):
            ops.solve_spd(a, bad_b)
    with pytest.raises(ValueError):  # in place needs contiguous rows; cholesky_solve copies
        ops.cholesky_solve_(l, torch.ones(4, 6, dtype=torch.float64, device=dev)[:, ::2])
    assert ops.cholesky_solve(l, torch.ones(4, 6, dtype=torch.float64, device=dev)[:, ::2]).shape == (4, 3)
    with pytest.raises(ValueError):  # a row stride below the width
        ops.cholesky_solve_(l, torch.ones(1, 3, dtype=torch.float64, device=dev).expand(4, 3))
    with pytest.raises(ValueError):  # a 1-D right-hand side needs a positive stride
        ops.cholesky_solve_(l, torch.ones(1, dtype=torch.float64, device=dev).expand(4))
    if dev.type == "cuda":
        with pytest.raises(ValueError):
            ops.cholesky_solve(l, b.cpu())
        with pytest.raises(ValueError):
            ops.cholesky_solve_(l.cpu(), b)
        with pytest.raises(ValueError):
            ops.solve_spd(a, b.cpu())
    # empty systems are no-ops
    e_l, e_info = ops.cholesky_factor(torch.empty(0, 0, dtype=torch.float64, device=dev))
    assert e_l.shape == (0, 0) and int(e_info.item()) == 0 and e_info.device == e_l.device
    assert ops.cholesky_solve(e_l, torch.empty(0, 3, dtype=torch.float64, device=dev)).shape == (0, 3)
    assert ops.cholesky_solve(l, torch.empty(4, 0, dtype=torch.float64, device=dev)).shape == (4, 0)
    assert ops.solve_spd(e_l, torch.empty(0, dtype=torch.float64, device=dev)).shape == (0,)
    assert float(ops.logdet_spd(e_l)) == 0.0


def test_c_entry_points_refuse_bad_arguments():
    """Argument errors come back before any pointer is touched: null pointers
    throughout, no device needed."""
    L = _native.lib()
    ARG = 1  # MPX_ERR_ARG
    assert L.mpx_chol_factor_f64(None, -1, 0, None, None) == ARG
    assert L.mpx_chol_factor_f64(None, 4, 3, None, None) == ARG
    assert L.mpx_chol_factor_f64(None, 4, 4, None, None) == ARG  # null pointers
    assert b"chol" in L.mpx_last_error()
    assert L.mpx_chol_factor_f64(None, 0, 0, None, None) == 0  # n = 0: no-op
    assert L.mpx_chol_solve_f64(None, -1, 0, None, 1, 1, None) == ARG
    assert L.mpx_chol_solve_f64(None, 4, 4, None, -1, 0, None) == ARG
    assert L.mpx_chol_solve_f64(None, 4, 3, None, 1, 1, None) == ARG
    assert L.mpx_chol_solve_f64(None, 4, 4, None, 3, 2, None) == ARG
    assert L.mpx_chol_solve_f64(None, 4, 4, None, 1, 1, None) == ARG  # null pointers
    assert L.mpx_chol_solve_f64(None, 0, 0, None, 3, 3, None) == 0
    assert L.mpx_chol_solve_f64(None, 4, 4, None, 0, 0, None) == 0
    assert L.mpx_chol_phase_f64(None, -1, 0, None, 0, 0, None) == ARG
    assert L.mpx_chol_phase_f64(None, 4, 3, None, 0, 0, None) == ARG
    assert L.mpx_chol_phase_f64(None, 4, 4, None, 0, 0, None) == ARG  # null pointers
    assert L.mpx_chol_phase_f64(None, 0, 0, None, 0, 0, None) == ARG  # no panel column below n = 0
    # the CPU reference writes nothing but *info = 0 on bad arguments
    word = torch.full((1,), -1, dtype=torch.int32)
    L.mpx_cpu_chol_factor_f64(None, 4, 4, word.data_ptr())
    assert int(word.item()) == 0
    L.mpx_cpu_chol_solve_f64(None, 4, 4, None, 1, 1)
