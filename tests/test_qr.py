"""Dense Householder QR (``ops.qr_factor`` and friends, ``ops.lstsq``,
``DenseQR``): row-major fp64, m >= n, LAPACK ``geqrf`` storage (the contract is
capi.h's ``mpx_qr_factor_f64``).

Every body runs on CPU tensors (the unblocked reference) and, marked ``gpu``,
on GPU tensors (qr.hip). Layouts: contiguous, pitch n + 2, pitch n + 3; the
sentinel in the pitch padding must come back bit for bit.

Shapes (m, n), the smallest at which something changes: (1, 1), (2, 1), (5, 3)
trivial; (16, 16), (17, 15) the MFMA tile; (64, 64), (65, 64), (65, 65) one
panel and one row or column beyond it; (130, 63) a ragged panel; (129, 129),
(300, 193) three panels, ragged tiles both ways; (1100, 257) many ragged tiles;
(4200, 70) more than 64 workgroups of panel partials and a second panel of 6
columns; and one shape from ``mpx_qr_plan`` at which the W kernel sums two row
chunks.

A. Exact, ``array_equal``: upper-triangular input (tau = 0, nothing changes);
   signed scaled permutations (every reduction has a single nonzero term, so an
   unblocked fp64 Householder written here from the contract's rule is exact
   arithmetic and must be matched bit for bit; ``lstsq`` returns the exact
   integers); exactly zero columns (``info``, the first of two, the column
   stays zero, the columns left of it are those of the narrower matrix, the
   solvers raise); invariants on random data (scaling by 2^+-20, column
   nesting, two runs and three layouts, independent columns of B with a NaN
   column among them, a NaN in column j leaves the columns left of it alone,
   the phases one by one give the factorisation's bits).

B. Bounds in ``np.longdouble``, u = 2^-53, mu = max(m n, 16) u (Higham's
   gamma~_{mn} with its constant taken as 1), on Gaussian matrices and on
   Gaussian matrices with columns scaled by 10^linspace(-8, 8, n):
     1. columnwise backward error  ||a_j - (Q R)_j|| <= mu ||a_j||, Q rebuilt
        from the stored v and tau in extended precision;
     2. orthogonality  max |Q^T Q - I| <= mu;
     3. the same two for ``qr_unpack``'s Q;
     4. least squares optimality  ||A^T (b - A x)|| <= 2 mu ||A||_F (||b|| + ||A||_F ||x||)
        (first-order consequence of Higham, Accuracy and Stability, Thm 20.3);
     5. consistent integer systems  ||x - X|| <= 2 kappa_2(A) mu ||X||;
   with 1, 3, 17 and 65 right-hand sides and the 1-D form. The bounds are
   ceilings that catch a wrong or narrow-precision kernel, not accuracy claims.
   LAPACK through numpy on exactly these matrices: backward error 3.5 u to
   7.8 u, orthogonality 2.0 u to 6.8 u, optimality 0.035 of its bound at (5, 3)
   falling to 1.4e-7 at (1100, 257), forward error 0.035 at (5, 3) and 1.9e-5
   at (1100, 257). Measured here as multiples of u, Gaussian / column-scaled
   (``test_bounds_factor`` prints them), backward error then orthogonality:
     (m, n)        GPU                           CPU reference
     (1, 1)        0.00/0.00    0.00/0.00       0.00/0.00    0.00/0.00
     (2, 1)        0.50/0.23    0.27/1.92       0.50/0.23    0.27/1.92
     (5, 3)        1.47/1.80    3.25/3.42       1.47/1.80    3.25/3.42
     (16, 16)      3.86/4.59    3.72/4.22       3.86/4.59    3.72/4.22
     (17, 15)      4.58/5.14    3.59/4.46       4.58/5.14    3.59/4.46
     (64, 64)      5.50/6.15    4.77/4.72       5.95/6.19    5.75/5.28
     (65, 64)      4.89/4.62    3.99/4.64       6.49/7.01    4.40/6.68
     (65, 65)      10.84/7.02   4.28/5.99       6.78/6.87    6.25/4.86
     (130, 63)     4.93/4.94    4.27/4.01       6.31/8.12    7.23/9.59
     (129, 129)    11.69/10.28  5.61/4.62       9.15/8.01    6.73/8.68
     (300, 193)    11.73/12.38  4.78/4.29       9.55/9.47    11.64/8.40
     (1100, 257)   14.25/13.41  3.99/4.98       11.98/12.75  21.93/22.86
     (4200, 70)    4.68/4.74    4.42/4.54       7.74/7.56    36.17/42.76
     (1124, 70)    8.05/7.13    5.37/4.30       7.11/6.71    19.71/22.35
   (the reference sums a tall column's rows one after the other, the GPU in
   groups of 16, then waves, then workgroups). ``qr_unpack``'s Q on the GPU:
   backward error up to 18.2 u, orthogonality up to 9.4 u. Least squares:
   optimality 0.028 (GPU) and 0.037 (CPU reference) of its bound at (5, 3),
   1.4e-7 and 1.3e-7 at (1100, 257); forward error 0.056 and 0.041 at (5, 3),
   1.1e-5 and 1.2e-5 at (1100, 257).

C. Conventions against LAPACK (``np.linalg.qr(a, mode="raw")``) on the
   Gaussian matrices:  ||R - R_lapack||_F <= 4 kappa_2(A) mu ||A||_F, equal signs
   on R's diagonal, tau to the same relative size; the same GPU against the CPU
   reference. This pins the sign rule, v_j[j] = 1 and the storage.

D. Plumbing: streams, CPU and GPU factors crossed, ``DenseQR``, empty shapes,
   every argument check.

test_qr_exact.py goes on from here: exact families whose sums have many terms,
m > 16384, the operand alignment classes and ``qr_solve_r_`` alone.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.models import DenseLU, DenseQR

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
LAYOUTS = {"contig": 0, "even": 2, "odd": 3}  # excess of the row pitch over the width
SENT = -7777.25
LD = np.longdouble
U53 = LD(2.0) ** -53
NRHS = (1, 3, 17, 65)


def _plan(m, n):
    out = (ctypes.c_int32 * 4)()
    assert _native.lib().mpx_qr_plan(m, n, out) == 0
    return list(out)


def _chunk_shape():
    """A shape whose first panel's W = V^T C sums two row chunks and has columns right of the panel."""
    chunk = _plan(4096, 70)[1]
    m = chunk + 100
    assert _plan(m, 70)[2] >= 2
    return m, 70


SHAPES = [(1, 1), (2, 1), (5, 3), (16, 16), (17, 15), (64, 64), (65, 64), (65, 65), (130, 63), (129, 129), (300, 193),
          (1100, 257), (4200, 70), _chunk_shape()]
MID = [(5, 3), (65, 64), (130, 63), (300, 193)]


@pytest.fixture
def dev(request):
    if request.param == "cuda":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def _place(arr: np.ndarray, layout: str, device):
    """``arr`` as the leading columns of a sentinel-filled pitched buffer."""
    r, c = arr.shape
    back = torch.full((r, c + LAYOUTS[layout]), SENT, dtype=torch.float64, device=device)
    view = back[:, :c]
    view.copy_(torch.from_numpy(np.array(arr, dtype=np.float64)))
    return view, back


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().copy()


def _factor(arr: np.ndarray, layout: str, device):
    """(qr, tau, info) as numpy / int of ``qr_factor_`` on a pitched buffer whose padding must survive."""
    view, back = _place(arr, layout, device)
    out, tau, info = ops.qr_factor_(view)
    assert out.data_ptr() == view.data_ptr() and tau.shape == (arr.shape[1],) and info.dtype == torch.int32
    assert bool((back[:, arr.shape[1]:] == SENT).all())
    return _np(out), _np(tau), int(info.item())


def _ld_ok():
    if np.finfo(LD).eps >= 2.0 ** -60:
        pytest.skip("np.longdouble is not an extended format here")


@functools.lru_cache(maxsize=None)
def _gauss(m: int, n: int, scaled: bool = False) -> np.ndarray:
    a = np.random.RandomState(11 + 7 * m + n).standard_normal((m, n))
    if scaled:
        a = a * 10.0 ** np.linspace(-8, 8, n)[None, :]
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _factored(m: int, n: int, scaled: bool, devname: str):
    """The factorisation of ``_gauss`` on a device; shared, never modified. The
    layout rotates with the shape (the layouts give the same bits: section A)."""
    layout = list(LAYOUTS)[(m + n) % 3]
    out = _factor(_gauss(m, n, scaled), layout, torch.device(devname))
    for x in out[:2]:
        x.setflags(write=False)
    return out


def _householder(a: np.ndarray):
    """Unblocked fp64 Householder by the contract's rule: (qr, tau, info)."""
    a = np.array(a, dtype=np.float64)
    m, n = a.shape
    tau = np.zeros(n)
    info = 0
    for j in range(n):
        alpha = a[j, j]
        sigma = float(np.sum(a[j + 1:, j] * a[j + 1:, j]))
        if sigma == 0.0:
            if alpha == 0.0 and info == 0:
                info = j + 1
            continue
        beta = -np.copysign(np.sqrt(alpha * alpha + sigma), alpha)
        tau[j] = (beta - alpha) / beta
        v = a[j + 1:, j] / (alpha - beta)
        w = tau[j] * (a[j, j + 1:] + v @ a[j + 1:, j + 1:])
        a[j, j + 1:] -= w
        a[j + 1:, j + 1:] -= np.outer(v, w)
        a[j + 1:, j] = v
        a[j, j] = beta
    return a, tau, info


def _q_ld(qr: np.ndarray, tau: np.ndarray) -> np.ndarray:
    """The thin Q = H_0 .. H_{n-1} I[:, :n] from the stored v and tau, in extended precision."""
    m, n = qr.shape
    q = np.eye(m, n, dtype=LD)
    for j in range(n - 1, -1, -1):
        v = np.concatenate([[LD(1)], qr[j + 1:, j].astype(LD)])
        q[j:, j:] -= LD(tau[j]) * np.outer(v, v @ q[j:, j:])
    return q


def _mu(m, n):
    return LD(max(m * n, 16)) * U53


def _col_norms(x):
    return np.sqrt(np.sum(x * x, axis=0))


def _backward_ratio(a: np.ndarray, q: np.ndarray, r: np.ndarray) -> float:
    """max_j ||a_j - (Q R)_j|| / ||a_j|| in units of u."""
    al = a.astype(LD)
    return float(np.max(_col_norms(al - q @ r) / _col_norms(al)) / U53)


def _orth_ratio(q: np.ndarray) -> float:
    return float(np.max(np.abs(q.T @ q - np.eye(q.shape[1], dtype=LD))) / U53)


# ---------------------------------------------------------------- A. exact
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m,n", MID + [(200, 200)])
def test_upper_triangular_input_is_left_alone(m, n, layout, dev):
    rng = np.random.RandomState(m + n)
    a = np.zeros((m, n))
    a[:n] = np.triu(rng.standard_normal((n, n)))
    a[np.arange(n), np.arange(n)] = np.where(np.arange(n) % 2 == 0, -1.5, 2.25) * (1 + np.arange(n))
    qr, tau, info = _factor(a, layout, dev)
    assert info == 0 and np.array_equal(tau, np.zeros(n)) and np.array_equal(qr, a)


@functools.lru_cache(maxsize=None)
def _signed_permutation(m: int, n: int):
    rng = np.random.RandomState(3 * m + n)
    rows = rng.permutation(m)[:n]  # distinct, spread over the workgroups, panels and row chunks
    diag = np.arange(0, n, 5)  # every fifth nonzero on the diagonal (sigma = 0, tau = 0) where those rows are free
    if not set(diag.tolist()) & set(np.delete(rows, diag).tolist()):
        rows[diag] = diag
    assert len(set(rows.tolist())) == n
    a = np.zeros((m, n))
    a[rows, np.arange(n)] = rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.randint(-8, 9, size=n)
    expect = _householder(a)
    a.setflags(write=False)
    return a, expect


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m,n", [(5, 3), (65, 65), (130, 63), (300, 193), (4200, 70), _chunk_shape()])
def test_signed_scaled_permutations(m, n, layout, dev):
    a, (eqr, etau, einfo) = _signed_permutation(m, n)
    assert einfo == 0 and set(np.unique(etau)) <= {0.0, 1.0}
    assert set(np.unique(np.tril(eqr, -1))) <= {0.0, 1.0, -1.0}
    qr, tau, info = _factor(a, layout, dev)
    assert info == 0 and np.array_equal(tau, etau) and np.array_equal(qr, eqr)
    x = np.random.RandomState(m).randint(-8, 9, size=(n, 3)).astype(np.float64)
    b = a @ x
    assert np.array_equal(_np(ops.lstsq(torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b).to(dev))), x)
    assert np.array_equal(_np(ops.lstsq(torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b[:, 1].copy()).to(dev))),
                          x[:, 1])


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("zero", [(0,), (63,), (64,), (129,), (63, 64), (64, 129)])
def test_zero_columns(zero, dev):
    m, n = 200, 130
    a = np.array(_gauss(m, n))
    a[:, list(zero)] = 0.0
    qr, tau, info = _factor(a, "odd", dev)
    z = zero[0]
    assert info == z + 1  # the first of two
    for c in zero:
        assert np.array_equal(qr[:, c], np.zeros(m)) and tau[c] == 0.0
    if z:
        lqr, ltau, linfo = _factor(a[:, :z], "odd", dev)
        assert linfo == 0 and np.array_equal(qr[:, :z], lqr) and np.array_equal(tau[:z], ltau)
    t = torch.from_numpy(a).to(dev)
    b = torch.ones(m, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match=rf"lstsq: .*column {z}\b"):
        ops.lstsq(t, b)
    with pytest.raises(RuntimeError, match=rf"DenseQR: .*column {z}\b"):
        DenseQR(t)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("m,n", [(17, 15), (130, 63), (300, 193)])
def test_power_of_two_scaling(m, n, dev):
    a = _gauss(m, n)
    qr, tau, info = _factor(a, "contig", dev)
    low = np.tril_indices(m, -1, n)
    for s in (2.0 ** 20, 2.0 ** -20):
        sqr, stau, sinfo = _factor(a * s, "contig", dev)
        assert sinfo == info == 0 and np.array_equal(stau, tau)
        assert np.array_equal(sqr[low], qr[low]) and np.array_equal(np.triu(sqr[:n]), np.triu(qr[:n]) * s)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_column_nesting(layout, dev):
    m, n = 300, 193
    a = _gauss(m, n)
    qr, tau, _ = _factor(a, layout, dev)
    for k in (1, 63, 64, 65, 127, 128, 129, 192):
        kqr, ktau, _ = _factor(a[:, :k], layout, dev)
        assert np.array_equal(kqr, qr[:, :k]) and np.array_equal(ktau, tau[:k]), k


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("m,n", SHAPES)
def test_runs_and_layouts_give_the_same_bits(m, n, dev):
    a = _gauss(m, n)
    first = _factor(a, "contig", dev)
    for layout in ("contig", "even", "odd"):
        again = _factor(a, layout, dev)
        assert again[2] == first[2] == 0
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]), layout


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("m,n", [(130, 63), (300, 193)])
def test_columns_of_b_are_independent(m, n, dev):
    a = _gauss(m, n)
    qr, tau, _ = ops.qr_factor(torch.from_numpy(np.array(a)).to(dev))
    b = np.random.RandomState(5).standard_normal((m, 17))
    b[:, 5] = np.nan
    b[3, 9] = np.inf
    tb = torch.from_numpy(b).to(dev)
    ta = torch.from_numpy(np.array(a)).to(dev)
    full = {tr: _np(ops.qr_mul_q(qr, tau, tb, transpose=tr)) for tr in (False, True)}
    xs = _np(ops.lstsq(ta, tb))
    assert xs.shape == (n, 17)
    for tr in (False, True):
        assert np.isnan(full[tr][:, 5]).all()
    for j in (0, 4, 5, 6, 9, 16):
        one = tb[:, j].clone()
        for tr in (False, True):
            assert np.array_equal(_np(ops.qr_mul_q(qr, tau, one, transpose=tr)), full[tr][:, j], equal_nan=True)
            assert np.array_equal(_np(ops.qr_mul_q(qr, tau, tb[:, j:j + 1], transpose=tr))[:, 0], full[tr][:, j],
                                  equal_nan=True)
        assert np.array_equal(_np(ops.lstsq(ta, one)), xs[:, j], equal_nan=True)
    assert np.isfinite(xs[:, [0, 4, 6, 16]]).all()


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("j", [0, 5, 64, 70, 192])
def test_nan_stays_right_of_its_column(j, dev):
    m, n = 300, 193
    a = np.array(_gauss(m, n))
    qr, tau, _ = _factor(a, "even", dev)
    a[m // 2, j] = np.nan
    nqr, ntau, _ = _factor(a, "even", dev)
    assert np.array_equal(nqr[:, :j], qr[:, :j]) and np.array_equal(ntau[:j], tau[:j])
    assert np.isnan(ntau[j]) and np.isnan(nqr[j, j])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m,n", [(65, 65), (300, 193), _chunk_shape()])
def test_gpu_phases_give_the_factorisation(m, n, layout, gpu):
    a = _gauss(m, n)
    qr, tau, info = _factor(a, layout, gpu)
    L = _native.lib()
    view, back = _place(a, layout, gpu)
    ptau = torch.full((n,), SENT, dtype=torch.float64, device=gpu)
    pinfo = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    nbytes = int(L.mpx_qr_workspace_bytes(m, n, 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for j0 in range(0, n, _plan(m, n)[3]):
        for phase in range(4):
            _native.check(L.mpx_qr_phase_f64(view.data_ptr(), m, n, back.stride(0), ptau.data_ptr(), pinfo.data_ptr(),
                                             j0, phase, ws.data_ptr(), nbytes, stream))
    torch.cuda.synchronize(gpu)
    assert int(pinfo.item()) == info and np.array_equal(_np(ptau), tau) and np.array_equal(_np(view), qr)
    assert bool((back[:, n:] == SENT).all())


# ---------------------------------------------------------------- B. bounds
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("m,n", SHAPES)
def test_bounds_factor(m, n, scaled, dev):
    _ld_ok()
    a = _gauss(m, n, scaled)
    qr, tau, info = _factored(m, n, scaled, str(dev))
    assert info == 0 and np.isfinite(qr).all() and np.isfinite(tau).all()
    q = _q_ld(qr, tau)
    r = np.triu(qr[:n]).astype(LD)
    back, orth = _backward_ratio(a, q, r), _orth_ratio(q)
    print(f"qr bounds {dev.type} ({m}, {n}) scaled={scaled}: backward {back:.2f} u, orthogonality {orth:.2f} u, "
          f"mu = {max(m * n, 16)} u")
    assert back <= max(m * n, 16) and orth <= max(m * n, 16)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("m,n", SHAPES)
def test_bounds_unpack(m, n, scaled, dev):
    _ld_ok()
    a = _gauss(m, n, scaled)
    qr, tau, _ = _factored(m, n, scaled, str(dev))
    q, r = ops.qr_unpack(torch.from_numpy(np.array(qr)).to(dev), torch.from_numpy(np.array(tau)).to(dev))
    assert q.shape == (m, n) and r.shape == (n, n)
    assert np.array_equal(_np(r), np.triu(qr[:n]))
    ql = _np(q).astype(LD)
    back, orth = _backward_ratio(a, ql, _np(r).astype(LD)), _orth_ratio(ql)
    print(f"qr unpack {dev.type} ({m}, {n}) scaled={scaled}: backward {back:.2f} u, orthogonality {orth:.2f} u")
    assert back <= max(m * n, 16) and orth <= max(m * n, 16)


def _rhs_forms(b: np.ndarray):
    """1, 3, 17 and 65 right-hand sides and the 1-D form."""
    return [b[:, :k] for k in NRHS] + [b[:, 0]]


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("m,n", SHAPES)
def test_bounds_least_squares(m, n, dev):
    _ld_ok()
    a = _gauss(m, n)
    al = a.astype(LD)
    fro = np.sqrt(np.sum(al * al))
    mu = _mu(m, n)
    ta = torch.from_numpy(np.array(a)).to(dev)
    b = np.random.RandomState(m + 3 * n).standard_normal((m, max(NRHS)))
    worst = 0.0
    for bb in _rhs_forms(b):
        x = _np(ops.lstsq(ta, torch.from_numpy(np.ascontiguousarray(bb)).to(dev)))
        assert x.shape == (n,) + bb.shape[1:] and np.isfinite(x).all()
        xl, bl = x.astype(LD).reshape(n, -1), bb.astype(LD).reshape(m, -1)
        lhs = _col_norms(al.T @ (bl - al @ xl))
        rhs = 2 * mu * fro * (_col_norms(bl) + fro * _col_norms(xl))
        worst = max(worst, float(np.max(lhs / rhs)))
        assert np.all(lhs <= rhs)
    # consistent integer systems
    kappa = LD(np.linalg.cond(a))
    xi = np.random.RandomState(n).randint(-8, 9, size=(n, max(NRHS))).astype(np.float64)
    bi = np.asarray(al @ xi.astype(LD), dtype=np.float64)  # rounded once
    fwd = 0.0
    for k, bb in zip(list(NRHS) + [None], _rhs_forms(bi)):
        x = _np(ops.lstsq(ta, torch.from_numpy(np.ascontiguousarray(bb)).to(dev))).astype(LD).reshape(n, -1)
        want = xi[:, :k] if k else xi[:, :1]
        err = _col_norms(x - want.astype(LD))
        lim = 2 * kappa * mu * np.maximum(_col_norms(want.astype(LD)), LD(1e-300))
        fwd = max(fwd, float(np.max(err / lim)))
        assert np.all(err <= lim)
    print(f"qr lstsq {dev.type} ({m}, {n}): optimality {worst:.3g} of its bound, forward error {fwd:.3g} of its bound")


# ---------------------------------------------------------------- C. conventions
def _convention_check(a, got, ref):
    m, n = a.shape
    mu = float(_mu(m, n))
    kappa = float(np.linalg.cond(a))
    r, rr = np.triu(got[0][:n]), np.triu(ref[0][:n])
    assert np.linalg.norm(r - rr) <= 4 * kappa * mu * np.linalg.norm(a)
    assert np.array_equal(np.sign(np.diagonal(r)), np.sign(np.diagonal(rr)))
    assert np.abs(got[1] - ref[1]).max() <= 4 * kappa * mu * max(np.abs(ref[1]).max(), 1.0)
    if m == n:
        assert got[1][-1] == 0.0 and ref[1][-1] == 0.0


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("m,n", SHAPES)
def test_conventions_against_lapack(m, n, dev):
    a = _gauss(m, n)
    h, t = np.linalg.qr(np.array(a), mode="raw")
    _convention_check(a, _factored(m, n, False, str(dev)), (h.T, t))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", SHAPES)
def test_gpu_against_cpu_reference(m, n, gpu):
    a = _gauss(m, n)
    got, ref = _factored(m, n, False, str(gpu)), _factored(m, n, False, "cpu")
    _convention_check(a, got, ref)
    # v below the diagonal: the same vectors to the same size (v_j[j] = 1 implied, |v_i| <= 1)
    low = np.tril_indices(m, -1, n)
    assert np.abs(got[0][low] - ref[0][low]).max(initial=0.0) <= 4 * float(np.linalg.cond(a)) * float(_mu(m, n))


# ---------------------------------------------------------------- D. plumbing
@pytest.mark.gpu
def test_gpu_two_streams_with_their_own_workspaces(gpu):
    shapes = [(300, 193), (1100, 257)]
    want = [_factor(_gauss(m, n), "contig", gpu) for m, n in shapes]
    streams = [torch.cuda.Stream(device=gpu) for _ in shapes]
    outs = []
    for (m, n), s in zip(shapes, streams):
        t = torch.from_numpy(np.array(_gauss(m, n))).to(gpu)
        s.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(s):
            outs.append(ops.qr_factor_(t))
    for s in streams:
        s.synchronize()
    for (qr, tau, info), w in zip(outs, want):
        assert np.array_equal(_np(qr), w[0]) and np.array_equal(_np(tau), w[1]) and int(info.item()) == w[2]


def _ls_within_bound(a, b, x):
    al, bl, xl = a.astype(LD), b.astype(LD).reshape(a.shape[0], -1), x.astype(LD).reshape(a.shape[1], -1)
    fro = np.sqrt(np.sum(al * al))
    lhs = _col_norms(al.T @ (bl - al @ xl))
    return bool(np.all(lhs <= 2 * _mu(*a.shape) * fro * (_col_norms(bl) + fro * _col_norms(xl))))


@pytest.mark.gpu
def test_gpu_and_cpu_factors_crossed(gpu):
    _ld_ok()
    m, n = 300, 193
    a = _gauss(m, n)
    b = np.random.RandomState(2).standard_normal((m, 3))
    cpu = torch.device("cpu")
    fact = {d: ops.qr_factor(torch.from_numpy(np.array(a)).to(d)) for d in (cpu, gpu)}
    for src, dst in ((cpu, gpu), (gpu, cpu)):
        qr, tau = fact[src][0].to(dst), fact[src][1].to(dst)
        y = ops.qr_mul_q(qr, tau, torch.from_numpy(b).to(dst), transpose=True)
        x = ops.qr_solve_r_(qr, y[:n].clone())
        assert _ls_within_bound(a, b, _np(x))
        back = _np(ops.qr_mul_q(qr, tau, y))  # Q Q^T b = b
        assert np.abs(back - b).max() <= float(_mu(m, n)) * np.abs(b).max() * 4


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_dense_qr_model(dev):
    _ld_ok()
    m, n = 130, 63
    a = _gauss(m, n)
    t = torch.from_numpy(np.array(a)).to(dev)
    keep = t.clone()
    model = DenseQR(t)
    qr, tau, info = ops.qr_factor(t)
    assert torch.equal(t, keep) and qr.data_ptr() != t.data_ptr() and int(info.item()) == 0
    assert torch.equal(model.qr, qr) and torch.equal(model.tau, tau) and (model.m, model.n) == (m, n)
    q, r = ops.qr_unpack(qr, tau)
    assert torch.equal(model.q(), q) and torch.equal(model.r(), r)
    b = torch.from_numpy(np.random.RandomState(4).standard_normal((m, 3))).to(dev)
    bkeep = b.clone()
    assert torch.equal(model.solve(b), ops.lstsq(t, b)) and torch.equal(b, bkeep)
    assert torch.equal(model.solve(b[:, 0]), ops.lstsq(t, b[:, 0]))
    assert _ls_within_bound(a, _np(b), _np(model.solve(b)))
    for tr in (False, True):
        assert torch.equal(model.mul_q(b, transpose=tr), ops.qr_mul_q(qr, tau, b, transpose=tr))
    same = ops.qr_mul_q_(qr, tau, b, transpose=True)
    assert same.data_ptr() == b.data_ptr() and torch.equal(b, model.mul_q(bkeep, transpose=True))
    with pytest.raises(ValueError, match="square"):
        model.logabsdet()
    sq = torch.from_numpy(np.array(_gauss(65, 65))).to(dev)
    sign, logabs = DenseLU(sq).slogdet()
    got = DenseQR(sq).logabsdet()
    assert got.dim() == 0 and abs(float(got) - float(logabs)) <= 1e-10 * max(1.0, abs(float(logabs)))
    # every second row of a taller buffer: the pitch is 2 n
    tall = torch.full((2 * m, n), SENT, dtype=torch.float64, device=dev)
    tall[::2] = keep
    out, otau, _ = ops.qr_factor_(tall[::2])
    assert torch.equal(out, qr) and torch.equal(otau, tau) and bool((tall[1::2] == SENT).all())


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_empty_shapes(dev):
    def z(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=dev)

    for m, n in ((0, 0), (5, 0)):
        qr, tau, info = ops.qr_factor_(z(m, n))
        assert qr.shape == (m, n) and tau.shape == (0,) and int(info.item()) == 0
        b = torch.ones((m, 2), dtype=torch.float64, device=dev)
        assert torch.equal(ops.qr_mul_q(qr, tau, b), b) and torch.equal(ops.qr_mul_q(qr, tau, b, True), b)
        q, r = ops.qr_unpack(qr, tau)
        assert q.shape == (m, 0) and r.shape == (0, 0)
        assert ops.lstsq(z(m, n), b).shape == (0, 2) and ops.lstsq(z(m, n), b[:, 0]).shape == (0,)
    a = torch.from_numpy(np.array(_gauss(5, 3))).to(dev)
    qr, tau, _ = ops.qr_factor(a)
    assert ops.qr_mul_q(qr, tau, z(5, 0)).shape == (5, 0)  # k = 0
    assert ops.lstsq(a, z(5, 0)).shape == (3, 0)
    assert ops.qr_solve_r_(qr, z(3, 0)).shape == (3, 0)
    assert DenseQR(z(0, 0)).solve(z(0, 2)).shape == (0, 2)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_value_errors(dev):
    def z(*shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device=dev)

    a = torch.from_numpy(np.array(_gauss(5, 3))).to(dev)
    qr, tau, _ = ops.qr_factor(a)
    for fn in (ops.qr_factor, ops.qr_factor_):
        with pytest.raises(ValueError, match="must be a tensor"):
            fn(None)
        with pytest.raises(ValueError, match="float64"):
            fn(z(5, 3, dtype=torch.float32))
        with pytest.raises(ValueError, match="2-D"):
            fn(z(5))
        with pytest.raises(ValueError, match="m >= n"):
            fn(z(3, 5))
        with pytest.raises(ValueError, match="contiguous rows"):
            fn(z(3, 5).T)
        with pytest.raises(ValueError, match="row stride of at least n"):
            fn(z(1, 3).expand(5, 3))
    with pytest.raises(ValueError, match="tau must be a float64 vector of 3"):
        ops.qr_mul_q(qr, tau[:2], z(5))
    with pytest.raises(ValueError, match="tau must be a float64 vector of 3"):
        ops.qr_unpack(qr, tau.float())
    with pytest.raises(ValueError, match="tau must be contiguous"):
        ops.qr_mul_q(qr, z(6)[::2], z(5))
    with pytest.raises(ValueError, match="B must be float64"):
        ops.qr_mul_q(qr, tau, z(5, dtype=torch.float32))
    with pytest.raises(ValueError, match=r"B must be \(m,\) or \(m, k\)"):
        ops.qr_mul_q(qr, tau, z(5, 1, 1))
    with pytest.raises(ValueError, match="B has 3 rows, QR 5"):
        ops.qr_mul_q(qr, tau, z(3))
    with pytest.raises(ValueError, match="B must have contiguous rows"):
        ops.qr_mul_q_(qr, tau, z(2, 5).T)
    with pytest.raises(ValueError, match="row stride of at least its width"):
        ops.qr_mul_q_(qr, tau, z(1, 2).expand(5, 2))
    with pytest.raises(ValueError, match="positive stride"):
        ops.qr_mul_q_(qr, tau, z(1).expand(5))
    with pytest.raises(ValueError, match="B has 5 rows, R 3"):
        ops.qr_solve_r_(qr, z(5))
    with pytest.raises(ValueError, match=r"B must be \(5,\) or \(5, k\)"):
        ops.lstsq(a, z(3))
    with pytest.raises(ValueError, match="B must be float64"):
        ops.lstsq(a, z(5, dtype=torch.float32))
    with pytest.raises(ValueError, match="m >= n"):
        ops.lstsq(z(3, 5), z(3))
    with pytest.raises(ValueError, match="m >= n"):
        DenseQR(z(3, 5))
    if dev.type == "cuda":
        with pytest.raises(ValueError, match="QR is on .* tau on cpu"):
            ops.qr_mul_q(qr, tau.cpu(), z(5))
        with pytest.raises(ValueError, match="QR is on .* B on cpu"):
            ops.qr_mul_q(qr, tau, z(5).cpu())
        with pytest.raises(ValueError, match="A is on .* B on cpu"):
            ops.lstsq(a, z(5).cpu())
    # a strided 1-D right-hand side and a pitched 2-D one are honoured in place
    wide = torch.full((5, 4), SENT, dtype=torch.float64, device=dev)
    wide[:, 1] = 1.0
    want = ops.qr_mul_q(qr, tau, torch.ones(5, dtype=torch.float64, device=dev), transpose=True)
    ops.qr_mul_q_(qr, tau, wide[:, 1], transpose=True)
    assert torch.equal(wide[:, 1], want) and bool((wide[:, [0, 2, 3]] == SENT).all())


def test_c_entry_points_refuse_bad_arguments():
    """Argument errors come back before any pointer is touched: null or made-up
    pointers throughout, no device needed."""
    L = _native.lib()
    ARG = 1  # MPX_ERR_ARG
    P = 4096  # a non-null, 16-byte aligned address that must never be touched
    need = int(L.mpx_qr_workspace_bytes(5, 3, 0))
    assert need > 0 and L.mpx_qr_workspace_bytes(5, 3, 2) >= need
    assert L.mpx_qr_workspace_bytes(0, 0, 0) == 0 and L.mpx_qr_workspace_bytes(3, 5, 0) == 0
    assert L.mpx_qr_factor_f64(P, -1, 0, 0, P, P, P, need, None) == ARG
    assert L.mpx_qr_factor_f64(P, 3, 5, 5, P, P, P, need, None) == ARG  # m < n
    assert b"m < n" in L.mpx_last_error()
    assert L.mpx_qr_factor_f64(P, 5, 3, 2, P, P, P, need, None) == ARG  # pitch < n
    assert L.mpx_qr_factor_f64(None, 5, 3, 3, P, P, P, need, None) == ARG
    assert L.mpx_qr_factor_f64(P, 5, 3, 3, None, P, P, need, None) == ARG
    assert L.mpx_qr_factor_f64(P, 5, 3, 3, P, None, P, need, None) == ARG
    assert L.mpx_qr_factor_f64(P, 5, 3, 3, P, P, None, need, None) == ARG
    assert L.mpx_qr_factor_f64(P, 5, 3, 3, P, P, P, need - 1, None) == ARG  # short workspace
    assert b"workspace" in L.mpx_last_error()
    assert L.mpx_qr_factor_f64(P, 5, 3, 3, P, P, P + 8, need, None) == ARG  # misaligned workspace
    assert L.mpx_qr_factor_f64(None, 0, 0, 0, None, None, None, 0, None) == 0  # empty: no-ops
    assert L.mpx_qr_factor_f64(None, 5, 0, 0, None, None, None, 0, None) == 0
    need2 = int(L.mpx_qr_workspace_bytes(5, 3, 2))
    assert L.mpx_qr_apply_f64(P, 5, 3, 3, P, P, -1, 0, 0, P, need2, None) == ARG
    assert L.mpx_qr_apply_f64(P, 3, 5, 5, P, P, 2, 2, 0, P, need2, None) == ARG  # m < n
    assert L.mpx_qr_apply_f64(P, 5, 3, 2, P, P, 2, 2, 0, P, need2, None) == ARG
    assert L.mpx_qr_apply_f64(P, 5, 3, 3, P, P, 2, 1, 0, P, need2, None) == ARG  # pitch_b < nrhs
    assert L.mpx_qr_apply_f64(None, 5, 3, 3, P, P, 2, 2, 0, P, need2, None) == ARG
    assert L.mpx_qr_apply_f64(P, 5, 3, 3, None, P, 2, 2, 0, P, need2, None) == ARG
    assert L.mpx_qr_apply_f64(P, 5, 3, 3, P, None, 2, 2, 0, P, need2, None) == ARG
    assert L.mpx_qr_apply_f64(P, 5, 3, 3, P, P, 2, 2, 0, None, need2, None) == ARG
    assert L.mpx_qr_apply_f64(P, 5, 3, 3, P, P, 2, 2, 0, P, need2 - 1, None) == ARG
    assert L.mpx_qr_apply_f64(P, 5, 3, 3, P, P, 2, 2, 0, P + 8, need2, None) == ARG
    assert L.mpx_qr_apply_f64(None, 5, 3, 3, None, None, 0, 0, 0, None, 0, None) == 0  # nrhs = 0
    assert L.mpx_qr_apply_f64(None, 0, 0, 0, None, None, 2, 2, 1, None, 0, None) == 0
    assert L.mpx_qr_rsolve_f64(P, -1, 0, P, 1, 1, None) == ARG
    assert L.mpx_qr_rsolve_f64(P, 3, 3, P, -1, 0, None) == ARG
    assert L.mpx_qr_rsolve_f64(P, 3, 2, P, 1, 1, None) == ARG
    assert L.mpx_qr_rsolve_f64(P, 3, 3, P, 2, 1, None) == ARG
    assert L.mpx_qr_rsolve_f64(None, 3, 3, P, 1, 1, None) == ARG
    assert L.mpx_qr_rsolve_f64(P, 3, 3, None, 1, 1, None) == ARG
    assert L.mpx_qr_rsolve_f64(None, 0, 0, None, 1, 1, None) == 0
    assert L.mpx_qr_rsolve_f64(None, 3, 3, None, 0, 0, None) == 0
    out = (ctypes.c_int32 * 4)()
    assert L.mpx_qr_plan(3, 5, out) == ARG and L.mpx_qr_plan(-1, -1, out) == ARG and L.mpx_qr_plan(5, 3, None) == ARG
    assert L.mpx_qr_plan(4200, 70, out) == 0 and out[0] > 0 and 4200 > 64 * out[0] and out[3] == 64
    assert L.mpx_qr_phase_f64(P, 3, 5, 5, P, P, 0, 0, P, need, None) == ARG
    assert L.mpx_qr_phase_f64(P, 5, 3, 3, P, P, 0, 0, P, need - 1, None) == ARG
    assert L.mpx_qr_phase_f64(P, 5, 3, 3, P, P, 64, 0, P, need, None) == ARG  # no panel column at 64
    assert L.mpx_qr_phase_f64(P, 5, 3, 3, P, P, 1, 0, P, need, None) == ARG
    assert L.mpx_qr_phase_f64(P, 5, 3, 3, P, P, 0, 4, P, need, None) == ARG
    # the CPU reference writes nothing but *info = 0 on bad arguments
    word = torch.full((1,), -1, dtype=torch.int32)
    L.mpx_cpu_qr_factor_f64(None, 5, 3, 3, None, word.data_ptr())
    assert int(word.item()) == 0
    word.fill_(-1)
    keep = torch.full((3, 5), 2.0, dtype=torch.float64)
    L.mpx_cpu_qr_factor_f64(keep.data_ptr(), 3, 5, 5, keep.data_ptr(), word.data_ptr())  # m < n
    assert int(word.item()) == 0 and bool((keep == 2.0).all())
    L.mpx_cpu_qr_apply_f64(None, 5, 3, 3, None, None, 1, 1, 0)
    L.mpx_cpu_qr_rsolve_f64(None, 3, 3, None, 1, 1)


@pytest.mark.gpu
def test_gpu_workspace_of_exactly_the_stated_size(gpu):
    m, n, k = 300, 193, 3
    a = _gauss(m, n)
    want = _factor(a, "contig", gpu)
    L = _native.lib()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    t = torch.from_numpy(np.array(a)).to(gpu)
    tau = torch.empty(n, dtype=torch.float64, device=gpu)
    info = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    need = int(L.mpx_qr_workspace_bytes(m, n, 0))
    guard = 64
    ws = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device=gpu)
    assert L.mpx_qr_factor_f64(t.data_ptr(), m, n, n, tau.data_ptr(), info.data_ptr(), ws.data_ptr(), need - 1,
                               stream) == 1
    _native.check(L.mpx_qr_factor_f64(t.data_ptr(), m, n, n, tau.data_ptr(), info.data_ptr(), ws.data_ptr(), need,
                                      stream))
    torch.cuda.synchronize(gpu)
    assert np.array_equal(_np(t), want[0]) and np.array_equal(_np(tau), want[1]) and int(info.item()) == 0
    assert bool((ws[need:] == 0x5A).all())
    b = torch.from_numpy(np.random.RandomState(9).standard_normal((m, k))).to(gpu)
    ref = ops.qr_mul_q(t, tau, b, transpose=True)
    need = int(L.mpx_qr_workspace_bytes(m, n, k))
    ws = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device=gpu)
    _native.check(L.mpx_qr_apply_f64(t.data_ptr(), m, n, n, tau.data_ptr(), b.data_ptr(), k, k, 1, ws.data_ptr(), need,
                                     stream))
    torch.cuda.synchronize(gpu)
    assert torch.equal(b, ref) and bool((ws[need:] == 0x5A).all())
