"""Batched Cholesky of small SPD matrices (``ops.cholesky_factor_batched`` and
friends, ``BatchedDenseCholesky``): row-major fp64, lower storage.

For n <= 64 the batched kernels use plain VALU arithmetic in the operation
order of the unblocked CPU reference, so the yardstick is the strictest one:
every member of a batch equals, with ``torch.equal``, what the single-matrix
CPU functions produce for that member alone. The single-matrix CPU results are
computed once per (n, batch) and shared. For n > 64 the batch loops over the
single-matrix MFMA kernels and inherits their yardsticks
(``tests/test_cholesky.py``: exact recovery and Higham's bounds).

Only the lower triangles are the factorisation's business: the matrices here
carry NaN in their strict upper triangles, and the layout tests surround the
members with NaN (padding, spare rows, guard members) that must come back bit
for bit.

Sizes: the padded widths are 8, 16, 32 and 64, so n covers each at its edge,
one below and one above; a wave holds 8, 4, 2 or 1 members in the
factorisation and 64 / min(nrhs, 64) in the solve, so the batch sizes leave
ragged last waves for every packing; 65 right-hand sides make two chunks.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.models import BatchedDenseCholesky, DenseCholesky

from .test_cholesky import DEVICES, NRHS, SENT, _exact_family, _factor_bound, _ld_ok, _np, _solve_bound, _spd, _spoil
from .test_cholesky import dev  # noqa: F401  (the CPU / GPU fixture)

N_ALL = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64]
B_ALL = [1, 2, 3, 7, 8, 9, 63, 64, 65, 130]
B_FOR_N = 5   # the batch of the n sweep: ragged for 8, 4 and 2 members per wave
N_FOR_B = [3, 9, 17, 33]  # one n per padded width for the batch sweep
MPX_ERR_ARG = 1
NAN = float("nan")
GUARD = int(SENT)  # what the words around info hold


# ---------------------------------------------------------------- 0. helpers
def _upper_nan(a: np.ndarray) -> np.ndarray:
    """A copy of the batch (or matrix) with NaN in every strict upper triangle."""
    out = np.array(a, dtype=np.float64)
    n = out.shape[-1]
    iu = np.triu_indices(n, 1)
    out[..., iu[0], iu[1]] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def _batch(n: int, batch: int, graded: bool = False) -> np.ndarray:
    """G G^T + n I per member, symmetric; graded: d A d as in ``_spd(graded=True)``."""
    g = np.random.RandomState(100003 * batch + 17 * n + graded).standard_normal((batch, n, n))
    a = g @ g.transpose(0, 2, 1) + n * np.eye(n)
    if graded:
        d = 10.0 ** np.linspace(-4, 4, n)
        a = d[None, :, None] * a * d[None, None, :]
    a = np.tril(a) + np.tril(a, -1).transpose(0, 2, 1)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _rhs(n: int, batch: int, nrhs: int) -> np.ndarray:
    shape = (batch, n) if nrhs == 0 else (batch, n, nrhs)  # 0: a 1-D right-hand side per member
    b = np.random.RandomState(7 * batch + n + 1000 * nrhs).standard_normal(shape)
    b.setflags(write=False)
    return b


def _t(arr: np.ndarray, device=None) -> torch.Tensor:
    t = torch.from_numpy(np.array(arr, dtype=np.float64))
    return t if device is None else t.to(device)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int64)


def _single_factor(mats: np.ndarray):
    """(tril L, info) of every member alone through the single-matrix CPU entry, stacked."""
    outs = [ops.cholesky_factor(_t(m)) for m in mats]
    n = mats.shape[1]
    low = torch.stack([torch.tril(o[0]) for o in outs]) if outs else torch.empty(0, n, n, dtype=torch.float64)
    info = torch.cat([o[1] for o in outs]) if outs else torch.empty(0, dtype=torch.int32)
    return low, info


@functools.lru_cache(maxsize=None)
def _ref_factor(n: int, batch: int, graded: bool = False):
    return _single_factor(_upper_nan(_batch(n, batch, graded)))


@functools.lru_cache(maxsize=None)
def _ref_solve(n: int, batch: int, nrhs: int):
    low, _ = _ref_factor(n, batch)
    b = _rhs(n, batch, nrhs)
    return torch.stack([ops.cholesky_solve(low[m], _t(b[m])) for m in range(batch)])


def _check_bits(n: int, batch: int, graded: bool, device):
    want_low, want_info = _ref_factor(n, batch, graded)
    assert not bool(want_info.any())  # the construction: every member is positive definite
    src = _t(_upper_nan(_batch(n, batch, graded)), device)
    keep = _bits(src)
    low, info = ops.cholesky_factor_batched(src)
    assert torch.equal(_bits(src), keep) and low.data_ptr() != src.data_ptr()
    assert info.dtype == torch.int32 and info.shape == (batch,) and info.device == src.device
    assert torch.equal(info.cpu(), want_info)
    assert torch.equal(torch.tril(low).cpu(), want_low)
    iu = np.triu_indices(n, 1)
    assert bool(np.isnan(_np(low)[:, iu[0], iu[1]]).all())  # the copy's upper triangles are the input's
    same, info2 = ops.cholesky_factor_batched_(src)
    assert same.data_ptr() == src.data_ptr() and torch.equal(info2, info)
    assert torch.equal(_bits(same), _bits(low))
    return low


# ---------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("graded", [False, True])
@pytest.mark.parametrize("n", N_ALL)
def test_factor_bits_every_n(n, graded, dev):
    _check_bits(n, B_FOR_N, graded, dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", N_FOR_B)
@pytest.mark.parametrize("batch", B_ALL)
def test_factor_bits_every_batch(batch, n, dev):
    _check_bits(n, batch, False, dev)


def _check_solve_bits(n: int, batch: int, device):
    low, _ = _ref_factor(n, batch)
    l_d = _t(_upper_nan(_np(low)), device)  # the solve reads the lower triangles only
    for nrhs in (0,) + NRHS:
        b = _t(_rhs(n, batch, nrhs), device)
        keep = b.clone()
        x = ops.cholesky_solve_batched(l_d, b)
        assert torch.equal(b, keep) and x.shape == b.shape and x.data_ptr() != b.data_ptr()
        assert torch.equal(x.cpu(), _ref_solve(n, batch, nrhs)), (n, batch, nrhs)
        same = ops.cholesky_solve_batched_(l_d, b)
        assert same.data_ptr() == b.data_ptr() and torch.equal(same, x)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", N_ALL)
def test_solve_bits_every_n(n, dev):
    _check_solve_bits(n, B_FOR_N, dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", N_FOR_B)
@pytest.mark.parametrize("batch", B_ALL)
def test_solve_bits_every_batch(batch, n, dev):
    _check_solve_bits(n, batch, dev)


# ---------------------------------------------------------------- 2. exact recovery
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", N_ALL)
def test_exact_recovery(n, dev):
    batch = 9
    fams = [_exact_family(n, seed=m) for m in range(batch)]
    a = np.stack([f[0] for f in fams])
    lows = np.stack([f[1] for f in fams])
    l, info = ops.cholesky_factor_batched_(_t(_upper_nan(a), dev))
    assert np.array_equal(_np(info), np.zeros(batch, dtype=np.int32))
    assert np.array_equal(np.tril(_np(l)), lows)
    rng = np.random.RandomState(n)
    for nrhs in NRHS:
        x = rng.randint(-8, 9, size=(batch, n, nrhs)).astype(np.float64)
        got = ops.cholesky_solve_batched(l, _t(a @ x, dev))
        assert np.array_equal(_np(got), x), (n, nrhs)
    x = rng.randint(-8, 9, size=(batch, n)).astype(np.float64)
    b = _t(np.einsum("bij,bj->bi", a, x), dev)
    got = ops.cholesky_solve_batched(l, b)
    assert got.shape == (batch, n) and np.array_equal(_np(got), x)
    got = ops.solve_spd_batched(_t(_upper_nan(a), dev), b)
    assert got.shape == (batch, n) and np.array_equal(_np(got), x)


# ---------------------------------------------------------------- 3. members do not leak into each other
N_LEAK = [7, 8, 16, 31, 32]  # a bad member shares a wave with good ones
SPOILS = [(kind, col) for kind in ("zero", "minus_one", "nan") for col in range(3)]  # col: 0, n // 2, n - 1


@functools.lru_cache(maxsize=None)
def _mixed(n: int):
    """(11 matrices with NaN upper triangles, expected info, exact factors or None, the good members)."""
    cols = (0, n // 2, n - 1)
    off = N_LEAK.index(n)  # the six spoilt slots of the five sizes cover all nine (kind, column) pairs
    plan = ["good", "bad", "good", "bad", "bad", "good", "nan", "bad", "good", "bad", "bad"]
    mats, infos, lows, good, slot = [], [], [], [], 0
    for m, what in enumerate(plan):
        a0, low = _exact_family(n, seed=20 + m)
        a = a0.copy()
        if what == "nan":
            a[:] = NAN
            infos.append(1)
            lows.append(None)
        elif what == "bad":
            kind, col = SPOILS[(2 * slot + off) % 9]
            slot += 1
            _spoil(a, low, cols[col], kind)
            infos.append(cols[col] + 1)
            lows.append(low)
        else:
            infos.append(0)
            lows.append(low)
            good.append(m)
        mats.append(a)
    mats = _upper_nan(np.stack(mats))
    mats.setflags(write=False)
    return mats, np.array(infos, dtype=np.int32), lows, good


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", N_LEAK)
def test_members_do_not_leak(n, dev):
    mats, infos, lows, good = _mixed(n)
    assert len(mats) == 11
    want_low, want_info = _single_factor(mats)
    assert np.array_equal(_np(want_info), infos)  # the construction: the members report what they were built to
    l, info = ops.cholesky_factor_batched(_t(mats, dev))
    assert np.array_equal(_np(info), infos)
    got = torch.tril(l).cpu()
    assert torch.equal(got[good], want_low[good])
    for m, k in enumerate(infos):
        if k and lows[m] is not None:  # a spoilt member: the columns before the failure are the exact factor's
            assert np.array_equal(_np(got[m])[:, :k - 1], lows[m][:, :k - 1]), m
    b = np.random.RandomState(n).standard_normal((len(mats), n, 3))
    x = ops.cholesky_solve_batched(l, _t(b, dev)).cpu()
    for m in good:
        assert torch.equal(x[m], ops.cholesky_solve(want_low[m], _t(b[m]))), m


# ---------------------------------------------------------------- 4. layouts and guards
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("extra", [0, 2, 3])
@pytest.mark.parametrize("n", [3, 8, 17, 33, 64])
def test_layouts_and_guards(n, extra, dev):
    batch, nrhs = 5, 3
    want_low, want_info = _ref_factor(n, batch)
    # two guard members, one spare row per member (batch stride > n * pitch), `extra` spare columns;
    # NaN everywhere but in the members' lower triangles
    buf = torch.full((batch + 2, n + 1, n + extra), NAN, dtype=torch.float64, device=dev)
    view = buf[1:-1, :n, :n]
    view.copy_(_t(_upper_nan(_batch(n, batch)), dev))
    before = _bits(buf)
    out, info = ops.cholesky_factor_batched_(view)
    assert out.data_ptr() == view.data_ptr()
    assert torch.equal(torch.tril(out).cpu(), want_low) and torch.equal(info.cpu(), want_info)
    inside = torch.zeros(buf.shape, dtype=torch.bool)
    inside[1:-1, :n, :n] = torch.tril(torch.ones(n, n, dtype=torch.bool))
    assert torch.equal(_bits(buf)[~inside], before[~inside])
    bbuf = torch.full((batch + 2, n + 1, nrhs + extra), NAN, dtype=torch.float64, device=dev)
    bview = bbuf[1:-1, :n, :nrhs]
    bview.copy_(_t(_rhs(n, batch, nrhs), dev))
    bbefore = _bits(bbuf)
    x = ops.cholesky_solve_batched_(out, bview)
    assert x.data_ptr() == bview.data_ptr()
    assert torch.equal(x.cpu(), _ref_solve(n, batch, nrhs))
    binside = torch.zeros(bbuf.shape, dtype=torch.bool)
    binside[1:-1, :n, :nrhs] = True
    assert torch.equal(_bits(bbuf)[~binside], bbefore[~binside])
    assert torch.equal(_bits(buf)[~inside], before[~inside])  # the solve reads the lower triangles and writes B only
    # a 1-D right-hand side per member that is a column of a wider buffer
    wide = torch.full((batch, n, 3), NAN, dtype=torch.float64, device=dev)
    wide[:, :, 1] = _t(_rhs(n, batch, 0), dev)
    ops.cholesky_solve_batched_(out, wide[:, :, 1])
    assert torch.equal(wide[:, :, 1].cpu(), _ref_solve(n, batch, 0))
    assert bool(torch.isnan(wide[:, :, 0]).all()) and bool(torch.isnan(wide[:, :, 2]).all())


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [7, 16, 33])
def test_info_guards_through_the_c_entry(n, dev):
    L = _native.lib()
    batch, guard = 9, 16
    want_low, want_info = _ref_factor(n, batch)
    a = _t(_upper_nan(_batch(n, batch)), dev)
    ibuf = torch.full((batch + 2 * guard,), GUARD, dtype=torch.int32, device=dev)
    info = ibuf[guard:guard + batch]
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            _native.check(L.mpx_chol_factor_batched_f64(a.data_ptr(), batch, n, n, n * n, info.data_ptr(),
                                                        _native.stream_of(a)))
        torch.cuda.synchronize(dev)
    else:
        L.mpx_cpu_chol_factor_batched_f64(a.data_ptr(), batch, n, n, n * n, info.data_ptr())
    assert torch.equal(torch.tril(a).cpu(), want_low) and torch.equal(info.cpu(), want_info)
    assert bool((ibuf[:guard] == GUARD).all()) and bool((ibuf[guard + batch:] == GUARD).all())


# ---------------------------------------------------------------- 5. n > 64: the single-matrix kernels in a loop
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [65, 129])
def test_fallback_above_64(n, dev):
    _ld_ok()
    batch = 3
    fams = [_exact_family(n, seed=m) for m in range(batch)]
    a = np.stack([f[0] for f in fams])
    l, info = ops.cholesky_factor_batched(_t(_upper_nan(a), dev))
    assert np.array_equal(_np(info), [0, 0, 0])
    assert np.array_equal(np.tril(_np(l)), np.stack([f[1] for f in fams]))
    x = np.random.RandomState(n).randint(-8, 9, size=(batch, n, 17)).astype(np.float64)
    assert np.array_equal(_np(ops.cholesky_solve_batched(l, _t(a @ x, dev))), x)
    x1 = x[:, :, 0].copy()
    assert np.array_equal(_np(ops.cholesky_solve_batched(l, _t(np.einsum("bij,bj->bi", a, x1), dev))), x1)
    # info per member: member 1 breaks down in the first column of the second panel
    bad = a.copy()
    _spoil(bad[1], fams[1][1], 64, "minus_one")
    l_bad, info = ops.cholesky_factor_batched(_t(_upper_nan(bad), dev))
    assert np.array_equal(_np(info), [0, 65, 0])
    for m in (0, 2):
        assert np.array_equal(np.tril(_np(l_bad[m])), fams[m][1])
    assert np.array_equal(np.tril(_np(l_bad[1]))[:, :64], fams[1][1][:, :64])
    # Higham's bounds on general SPD input (0.5 A: the same problem one binade down)
    g = np.stack([_spd(n), _spd(n, graded=True), 0.5 * _spd(n)])
    l, info = ops.cholesky_factor_batched(_t(_upper_nan(g), dev))
    assert np.array_equal(_np(info), [0, 0, 0])
    b = np.random.RandomState(n + 1).standard_normal((batch, n, 5))
    xs = ops.cholesky_solve_batched(l, _t(b, dev))
    for m in range(batch):
        _factor_bound(g[m], _np(l[m]))
        _solve_bound(_np(l[m]), b[m], _np(xs[m]))


# ---------------------------------------------------------------- 6. logdet, BatchedDenseCholesky
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [1, 8, 17, 64])
def test_logdet_exact_family(n, dev):
    """The bound of tests/test_cholesky.py::test_logdet_exact_family, per member:
    the factor's diagonal is the constructed one exactly, each log is within
    2 ulp, the sum within (n - 1) 2^-53 S, and the same again for the float64
    reference: |got - want| <= 2 S (n + 8) 2^-53 with S = sum |log l_ii|."""
    batch = 7
    fams = [_exact_family(n, seed=m) for m in range(batch)]
    a = _t(np.stack([f[0] for f in fams]), dev)
    l, _ = ops.cholesky_factor_batched(a)
    got = ops.logdet_spd_batched(l)
    assert got.shape == (batch,) and got.dtype == torch.float64 and got.device == l.device
    for m, (_, low) in enumerate(fams):
        logs = [math.log(v) for v in np.diag(low)]
        want = 2.0 * math.fsum(logs)
        bound = 2.0 * math.fsum(abs(v) for v in logs) * (n + 8) * 2.0 ** -53
        assert abs(float(got[m]) - want) <= bound, m
    assert torch.equal(BatchedDenseCholesky(a).logdet(), got)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [3, 16, 33, 64])
def test_batched_dense_cholesky_matches_dense_cholesky(n, dev):
    batch = 5
    a = _batch(n, batch)
    model = BatchedDenseCholesky(_t(a, dev))
    assert model.batch == batch and model.n == n and model.l.shape == (batch, n, n)
    inv = model.inverse()
    assert inv.shape == (batch, n, n)
    b2, b1 = _rhs(n, batch, 3), _rhs(n, batch, 0)
    x2, x1 = model.solve(_t(b2, dev)), model.solve(_t(b1, dev))
    for m in range(batch):
        single = DenseCholesky(_t(a[m]))
        assert torch.equal(torch.tril(model.l[m]).cpu(), torch.tril(single.l))
        assert torch.equal(inv[m].cpu(), single.inverse())
        assert torch.equal(x2[m].cpu(), single.solve(_t(b2[m])))
        assert torch.equal(x1[m].cpu(), single.solve(_t(b1[m])))


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_members_that_are_not_positive_definite_are_named(dev):
    n, batch = 9, 8
    fams = [_exact_family(n, seed=m) for m in range(batch)]
    a = np.stack([f[0] for f in fams])
    _spoil(a[3], fams[3][1], 4, "zero")
    _spoil(a[5], fams[5][1], 2, "nan")
    t = _t(a, dev)
    _, info = ops.cholesky_factor_batched(t)
    assert np.array_equal(_np(info), [0, 0, 0, 5, 0, 3, 0, 0])
    b = torch.ones(batch, n, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError,
                       match=r"solve_spd_batched: matrix 3 of the batch is not positive definite \(column 4\)"):
        ops.solve_spd_batched(t, b)
    with pytest.raises(RuntimeError, match=r"matrix 3 of the batch is not positive definite \(column 4\)"):
        BatchedDenseCholesky(t)
    with pytest.raises(RuntimeError, match=r"matrix 1 of the batch is not positive definite \(column 2\)"):
        ops.solve_spd_batched(t[4:], b[4:])
    with pytest.raises(RuntimeError, match=r"matrix 1 .*\(column 2\)"):
        BatchedDenseCholesky(t[4:])


# ---------------------------------------------------------------- 7. argument errors, empties
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_value_errors_and_empties(dev):
    f64 = dict(dtype=torch.float64, device=dev)
    a = 4.0 * torch.eye(4, **f64).repeat(3, 1, 1)
    l, info = ops.cholesky_factor_batched(a)
    assert not bool(info.any()) and torch.equal(l, 2.0 * torch.eye(4, **f64).repeat(3, 1, 1))
    b = torch.ones(3, 4, **f64)
    for fn in (ops.cholesky_factor_batched, ops.cholesky_factor_batched_, ops.logdet_spd_batched,
               BatchedDenseCholesky):
        with pytest.raises(ValueError, match="fp64 only"):
            fn(a.float())
        with pytest.raises(ValueError):
            fn("a")
    with pytest.raises(ValueError, match="fp64 only"):
        ops.cholesky_solve_batched(l, b.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.cholesky_solve_batched_(l.float(), b)
    with pytest.raises(ValueError, match="fp64 only"):
        ops.solve_spd_batched(a, b.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.solve_spd_batched(a.float(), b)
    wide = torch.ones(3, 4, 8, **f64)
    flat = torch.ones(64, **f64)
    for bad in (torch.ones(4, 4, **f64), torch.ones(2, 3, 4, 4, **f64), torch.ones(3, 4, 5, **f64),
                torch.ones(3, 5, 4, **f64), wide[:, :, ::2], a.transpose(1, 2),
                flat.as_strided((3, 4, 4), (16, 2, 1)),        # rows overlap
                flat.as_strided((3, 4, 4), (15, 4, 1)),        # members overlap by one element
                torch.ones(1, 4, 4, **f64).expand(3, 4, 4)):   # a batch stride of 0
        for fn in (ops.cholesky_factor_batched_, ops.cholesky_factor_batched, ops.logdet_spd_batched,
                   BatchedDenseCholesky):
            with pytest.raises(ValueError):
                fn(bad)
        with pytest.raises(ValueError):
            ops.solve_spd_batched(bad, b)
        with pytest.raises(ValueError):
            ops.cholesky_solve_batched(bad, b)
        with pytest.raises(ValueError):
            ops.cholesky_solve_batched_(bad, b)
    for bad_b in (torch.ones(3, 5, **f64), torch.ones(2, 4, **f64), torch.ones(4, **f64),
                  torch.ones(3, 4, 2, 2, **f64), torch.ones(3, 5, 2, **f64), "b"):
        with pytest.raises(ValueError):
            ops.cholesky_solve_batched_(l, bad_b)
        with pytest.raises(ValueError):
            ops.cholesky_solve_batched(l, bad_b)
        with pytest.raises(ValueError):
            ops.solve_spd_batched(a, bad_b)
    with pytest.raises(ValueError):  # in place needs contiguous rows; cholesky_solve_batched copies
        ops.cholesky_solve_batched_(l, torch.ones(3, 4, 6, **f64)[:, :, ::2])
    assert ops.cholesky_solve_batched(l, torch.ones(3, 4, 6, **f64)[:, :, ::2]).shape == (3, 4, 3)
    with pytest.raises(ValueError):  # a row stride below the width
        ops.cholesky_solve_batched_(l, torch.ones(3, 1, 2, **f64).expand(3, 4, 2))
    with pytest.raises(ValueError):  # members of B overlap
        ops.cholesky_solve_batched_(l, torch.ones(1, 4, 2, **f64).expand(3, 4, 2))
    with pytest.raises(ValueError):  # a 1-D right-hand side per member needs a positive stride
        ops.cholesky_solve_batched_(l, torch.ones(3, 1, **f64).expand(3, 4))
    if dev.type == "cuda":
        with pytest.raises(ValueError):
            ops.cholesky_solve_batched(l, b.cpu())
        with pytest.raises(ValueError):
            ops.cholesky_solve_batched_(l.cpu(), b)
        with pytest.raises(ValueError):
            ops.solve_spd_batched(a, b.cpu())
    # the single-matrix names still refuse a batch
    for fn in (ops.cholesky_factor, ops.cholesky_factor_, ops.logdet_spd, DenseCholesky):
        with pytest.raises(ValueError):
            fn(a)
    with pytest.raises(ValueError):
        ops.cholesky_solve(l, b)
    with pytest.raises(ValueError):
        ops.solve_spd(a, b)
    # empties: correctly shaped, nothing launched
    for shape in ((0, 4, 4), (3, 0, 0), (0, 0, 0)):
        e_l, e_info = ops.cholesky_factor_batched(torch.empty(shape, **f64))
        assert e_l.shape == shape and e_info.shape == shape[:1] and e_info.dtype == torch.int32
        assert e_info.device == e_l.device and not bool(e_info.any())
        e_b = torch.empty(shape[:2] + (2,), **f64)
        assert ops.cholesky_solve_batched(e_l, e_b).shape == e_b.shape
        assert ops.solve_spd_batched(torch.empty(shape, **f64), e_b).shape == e_b.shape
        assert ops.solve_spd_batched(torch.empty(shape, **f64), torch.empty(shape[:2], **f64)).shape == shape[:2]
        ld = ops.logdet_spd_batched(e_l)
        assert ld.shape == shape[:1] and ld.dtype == torch.float64
        if shape[0]:
            assert bool((ld == 0).all())
    assert ops.cholesky_solve_batched(l, torch.empty(3, 4, 0, **f64)).shape == (3, 4, 0)
    model = BatchedDenseCholesky(torch.empty(0, 4, 4, **f64))
    assert model.inverse().shape == (0, 4, 4) and model.logdet().shape == (0,)


def test_c_entry_points_refuse_bad_arguments():
    """Argument errors come back before any pointer is touched: null and
    dangling pointers, no device needed."""
    L = _native.lib()
    ARG = MPX_ERR_ARG
    wild = 0x10  # never a valid address: touching it would fault
    f = L.mpx_chol_factor_batched_f64
    assert f(wild, -1, 4, 4, 16, wild, None) == ARG
    assert f(wild, 2, -1, 4, 16, wild, None) == ARG
    assert f(wild, 2, 4, 3, 16, wild, None) == ARG            # pitch < n
    assert f(wild, 2, 4, 4, 15, wild, None) == ARG            # stride < (n - 1) pitch + n
    assert f(wild, 2, 4, 6, 21, wild, None) == ARG
    assert f(wild, 2, 4, 2 ** 62, 2 ** 62, wild, None) == ARG  # the product does not wrap
    assert f(wild, 2, 100, 2 ** 62, 2 ** 62, wild, None) == ARG  # nor above 64
    assert f(None, 2, 4, 4, 16, wild, None) == ARG
    assert f(wild, 2, 4, 4, 16, None, None) == ARG
    assert f(None, 2, 100, 100, 10000, wild, None) == ARG      # the loop above 64 checks first as well
    assert b"chol batched" in L.mpx_last_error()
    assert f(wild, 0, 4, 4, 16, wild, None) == 0               # no-ops
    assert f(wild, 2, 0, 0, 0, wild, None) == 0
    s = L.mpx_chol_solve_batched_f64
    assert s(wild, -1, 4, 4, 16, wild, 1, 1, 4, None) == ARG
    assert s(wild, 2, -1, 4, 16, wild, 1, 1, 4, None) == ARG
    assert s(wild, 2, 4, 4, 16, wild, -1, 1, 4, None) == ARG
    assert s(wild, 2, 4, 3, 16, wild, 1, 1, 4, None) == ARG    # pitch < n
    assert s(wild, 2, 4, 4, 16, wild, 3, 2, 12, None) == ARG   # pitch_b < nrhs
    assert s(wild, 2, 4, 4, 15, wild, 1, 1, 4, None) == ARG    # short stride
    assert s(wild, 2, 4, 4, 16, wild, 3, 3, 11, None) == ARG   # short stride_b
    assert s(wild, 2, 4, 2 ** 62, 2 ** 62, wild, 1, 1, 4, None) == ARG
    assert s(wild, 2, 4, 4, 16, wild, 3, 2 ** 62, 2 ** 62, None) == ARG
    assert s(None, 2, 4, 4, 16, wild, 1, 1, 4, None) == ARG
    assert s(wild, 2, 4, 4, 16, None, 1, 1, 4, None) == ARG
    # batch x nrhs beyond the blocks of one launch: one member per wave, three chunks
    assert s(wild, 2 ** 31 - 1, 4, 4, 16, wild, 129, 129, 4 * 129, None) == ARG
    assert b"chol batched solve" in L.mpx_last_error()
    assert s(wild, 0, 4, 4, 16, wild, 1, 1, 4, None) == 0
    assert s(wild, 2, 0, 0, 0, wild, 1, 1, 0, None) == 0
    assert s(wild, 2, 4, 4, 16, wild, 0, 0, 0, None) == 0
    # the CPU entries write nothing on bad arguments
    L.mpx_cpu_chol_factor_batched_f64(None, 2, 4, 4, 16, None)
    L.mpx_cpu_chol_factor_batched_f64(wild, -1, 4, 4, 16, wild)
    L.mpx_cpu_chol_factor_batched_f64(wild, 0, 4, 4, 16, wild)
    L.mpx_cpu_chol_solve_batched_f64(None, 2, 4, 4, 16, None, 1, 1, 4)
    L.mpx_cpu_chol_solve_batched_f64(wild, 0, 4, 4, 16, wild, 1, 1, 4)


# ---------------------------------------------------------------- 8. GPU only
@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 17, 64])
def test_gpu_same_bits_across_runs_and_layouts(gpu, n):
    batch = 65
    a = _t(_upper_nan(_batch(n, batch)), gpu)
    first, info = ops.cholesky_factor_batched(a)
    again, info2 = ops.cholesky_factor_batched(a)
    assert torch.equal(torch.tril(first), torch.tril(again)) and torch.equal(info, info2)
    buf = torch.full((batch, n + 2, n + 3), NAN, dtype=torch.float64, device=gpu)
    buf[:, :n, :n] = a
    padded, info3 = ops.cholesky_factor_batched_(buf[:, :n, :n])
    assert torch.equal(torch.tril(first), torch.tril(padded)) and torch.equal(info, info3)
    b = _t(_rhs(n, batch, 17), gpu)
    x = ops.cholesky_solve_batched(first, b)
    assert torch.equal(x, ops.cholesky_solve_batched(first, b))
    assert torch.equal(x, ops.cholesky_solve_batched(padded, b))


@pytest.mark.gpu
def test_gpu_side_stream_and_back_to_back(gpu):
    n, batch = 16, 130
    want = [_ref_factor(n, batch), _ref_factor(n + 1, batch)]
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        # two factorisations and two solves queued on one stream with nothing in between
        mats = [_t(_upper_nan(_batch(n, batch)), gpu), _t(_upper_nan(_batch(n + 1, batch)), gpu)]
        outs = [ops.cholesky_factor_batched_(m) for m in mats]
        xs = [ops.cholesky_solve_batched(o[0], _t(_rhs(k, batch, 3), gpu)) for o, k in zip(outs, (n, n + 1))]
    side.synchronize()
    for o, w, x, k in zip(outs, want, xs, (n, n + 1)):
        assert torch.equal(torch.tril(o[0]).cpu(), w[0]) and torch.equal(o[1].cpu(), w[1])
        assert torch.equal(x.cpu(), _ref_solve(k, batch, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 33])
def test_gpu_factors_cpu_solve_and_back(gpu, n):
    batch = 9
    a = _upper_nan(_batch(n, batch))
    b = _rhs(n, batch, 3)
    g_l, _ = ops.cholesky_factor_batched(_t(a, gpu))
    c_l, _ = ops.cholesky_factor_batched(_t(a))
    want = _ref_solve(n, batch, 3)
    assert torch.equal(ops.cholesky_solve_batched(g_l.cpu(), _t(b)), want)
    assert torch.equal(ops.cholesky_solve_batched(c_l.to(gpu), _t(b, gpu)).cpu(), want)
