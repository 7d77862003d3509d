"""Batched LU of small matrices (``ops.lu_factor_batched`` and friends,
``BatchedDenseLU``).

For n <= 64 the batched kernels use plain VALU arithmetic in the operation
order of the unblocked CPU reference, so the yardstick is the strictest one:
every member of a batch equals, with ``torch.equal``, what the single-matrix
CPU functions produce for that matrix alone. The single-matrix CPU results are
computed once per (n, batch) and shared. For n > 64 the batch loops over the
single-matrix MFMA kernels and inherits their yardsticks (``tests/test_lu.py``:
exact recovery and Higham's bounds).

Sizes: the padded widths are 8, 16, 32 and 64, so n covers each at its edge,
one below and one above; a wave holds 8, 4, 2 or 1 matrices in the
factorisation and 64 / min(nrhs, 64) in the solve, so the batch sizes leave
ragged last waves for every packing.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.models import BatchedDenseLU, DenseLU

from .test_lu import DEVICES, NRHS, _exact_family, _factor_bound, _ld_ok, _normal, _np, _solve_bound
from .test_lu import dev  # noqa: F401  (the CPU / GPU fixture)
from .test_lu_pivoting import _cancel, _tie

N_ALL = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64]
B_ALL = [1, 2, 3, 7, 8, 9, 63, 64, 65, 130]
B_FOR_N = 5   # the batch of the n sweep: ragged for 8, 4 and 2 matrices per wave
N_FOR_B = [3, 9, 17, 33]  # one n per padded width for the batch sweep
MPX_ERR_ARG = 1
NAN = float("nan")


# ---------------------------------------------------------------- 0. helpers
@functools.lru_cache(maxsize=None)
def _batch(n: int, batch: int, graded: bool = False) -> np.ndarray:
    a = np.random.RandomState(100003 * batch + 17 * n + graded).standard_normal((batch, n, n))
    if graded:
        a = a * (10.0 ** np.linspace(-8, 8, n))[None, :, None]
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


def _single_factor(mats: np.ndarray):
    """(lu, piv, info) of every matrix alone through the single-matrix CPU entry, stacked."""
    outs = [ops.lu_factor(_t(m)) for m in mats]
    n = mats.shape[1]
    lu = torch.stack([o[0] for o in outs]) if outs else torch.empty(0, n, n, dtype=torch.float64)
    piv = torch.stack([o[1] for o in outs]) if outs else torch.empty(0, n, dtype=torch.int32)
    info = torch.cat([o[2] for o in outs]) if outs else torch.empty(0, dtype=torch.int32)
    return lu, piv, info


@functools.lru_cache(maxsize=None)
def _ref_factor(n: int, batch: int, graded: bool = False):
    return _single_factor(_batch(n, batch, graded))


@functools.lru_cache(maxsize=None)
def _ref_solve(n: int, batch: int, nrhs: int):
    lu, piv, _ = _ref_factor(n, batch)
    b = _rhs(n, batch, nrhs)
    return torch.stack([ops.lu_solve(lu[m], piv[m], _t(b[m])) for m in range(batch)])


def _check_bits(n: int, batch: int, graded: bool, device):
    a = _batch(n, batch, graded)
    want_lu, want_piv, want_info = _ref_factor(n, batch, graded)
    src = _t(a, device)
    keep = src.clone()
    lu, piv, info = ops.lu_factor_batched(src)
    assert torch.equal(src, keep) and lu.data_ptr() != src.data_ptr()
    assert piv.dtype == torch.int32 and info.dtype == torch.int32
    assert piv.shape == (batch, n) and info.shape == (batch,) and piv.device == src.device
    assert torch.equal(piv.cpu(), want_piv)
    assert torch.equal(info.cpu(), want_info)
    assert torch.equal(lu.cpu(), want_lu)
    return lu, piv


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
    lu, piv, _ = _ref_factor(n, batch)
    lu_d, piv_d = lu.to(device), piv.to(device)
    for nrhs in (0,) + NRHS:
        b = _t(_rhs(n, batch, nrhs), device)
        keep = b.clone()
        x = ops.lu_solve_batched(lu_d, piv_d, b)
        assert torch.equal(b, keep) and x.shape == b.shape
        assert torch.equal(x.cpu(), _ref_solve(n, batch, nrhs)), (n, batch, nrhs)
        same = ops.lu_solve_batched_(lu_d, piv_d, b)
        assert same.data_ptr() == b.data_ptr() and torch.equal(same, x)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", N_ALL)
def test_solve_bits_every_n(n, dev):
    _check_solve_bits(n, B_FOR_N, dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [3, 33])
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
    lu, piv, info = ops.lu_factor_batched_(_t(a, dev))
    assert np.array_equal(_np(info), np.zeros(batch, dtype=np.int32))
    perm, low, up = ops.lu_unpack_batched(lu, piv)
    assert perm.dtype == torch.int64 and perm.shape == (batch, n)
    assert np.array_equal(_np(perm), np.stack([f[3] for f in fams]))
    assert np.array_equal(_np(low), np.stack([f[1] for f in fams]))
    assert np.array_equal(_np(up), np.stack([f[2] for f in fams]))
    rng = np.random.RandomState(n)
    for nrhs in NRHS:
        x = rng.randint(-4, 5, size=(batch, n, nrhs)).astype(np.float64)
        got = ops.lu_solve_batched(lu, piv, _t(a @ x, dev))
        assert np.array_equal(_np(got), x), (n, nrhs)
    x = rng.randint(-4, 5, size=(batch, n)).astype(np.float64)
    got = ops.solve_batched(_t(a, dev), _t(np.einsum("bij,bj->bi", a, x), dev))
    assert got.shape == (batch, n) and np.array_equal(_np(got), x)


# ---------------------------------------------------------------- 3. members do not leak into each other
@functools.lru_cache(maxsize=None)
def _mixed(n: int):
    """(matrices, expected info of the non-NaN members, index of the NaN member)."""
    kz = n // 2
    zero_col = np.array(_exact_family(n, seed=50)[0])
    zero_col[:, kz] = 0.0
    kc = min(n - 2, 3)
    t_late = n - 3
    members = [
        (_exact_family(n, seed=1)[0], 0),
        (zero_col, kz + 1),
        (_exact_family(n, seed=2)[0], 0),
        (_cancel(n, (kc,))[0], kc + 1),
        (_tie(n, 0, 0, 1, 1)[0], n),
        (_tie(n, 0, 1, n - 1, -1)[0], n),
        (np.full((n, n), NAN), None),
        (_tie(n, t_late, t_late, n - 2, -1)[0], n),
        (_tie(n, 2, 3, 5, 1)[0], n),
        (_exact_family(n, seed=3)[0], 0),
        (_normal(n), 0),
    ]
    mats = np.stack([np.array(m[0]) for m in members])
    mats.setflags(write=False)
    return mats, [m[1] for m in members], 6


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [7, 8, 16, 31, 32])
def test_members_do_not_leak(n, dev):
    mats, infos, nan_at = _mixed(n)
    want_lu, want_piv, want_info = _single_factor(mats)
    for m, k in enumerate(infos):  # the construction: the families report what they were built to
        assert k is None or int(want_info[m]) == k, (m, k)
    lu, piv, info = ops.lu_factor_batched(_t(mats, dev))
    assert torch.equal(piv.cpu(), want_piv)
    assert torch.equal(info.cpu(), want_info)
    others = [m for m in range(len(infos)) if m != nan_at]
    assert torch.equal(lu.cpu()[others], want_lu[others])
    b = np.random.RandomState(n).standard_normal((len(infos), n, 3))
    x = ops.lu_solve_batched(lu, piv, _t(b, dev)).cpu()
    for m in others:
        want = ops.lu_solve(want_lu[m], want_piv[m], _t(b[m]))
        # singular members divide by zero: the same values with NaN in the same places
        # (IEEE 754 leaves the sign and payload of a generated NaN open: x86 sets the sign, gfx950 does not)
        assert np.array_equal(_np(x[m]), _np(want), equal_nan=True), m


# ---------------------------------------------------------------- 4. layouts and guards
def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int64)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("extra", [0, 2, 3])
@pytest.mark.parametrize("n", [3, 8, 17, 33, 64])
def test_layouts_and_guards(n, extra, dev):
    batch, nrhs = 5, 3
    want_lu, want_piv, want_info = _ref_factor(n, batch)
    # two guard members, one spare row per member (batch stride > n * pitch), `extra` spare columns
    buf = torch.full((batch + 2, n + 1, n + extra), NAN, dtype=torch.float64, device=dev)
    view = buf[1:-1, :n, :n]
    view.copy_(_t(_batch(n, batch), dev))
    before = _bits(buf)
    out, piv, info = ops.lu_factor_batched_(view)
    assert out.data_ptr() == view.data_ptr()
    assert torch.equal(out.cpu(), want_lu) and torch.equal(piv.cpu(), want_piv) and torch.equal(info.cpu(), want_info)
    inside = torch.zeros(buf.shape, dtype=torch.bool)
    inside[1:-1, :n, :n] = True
    assert torch.equal(_bits(buf)[~inside], before[~inside])
    bbuf = torch.full((batch + 2, n + 1, nrhs + extra), NAN, dtype=torch.float64, device=dev)
    bview = bbuf[1:-1, :n, :nrhs]
    bview.copy_(_t(_rhs(n, batch, nrhs), dev))
    bbefore = _bits(bbuf)
    x = ops.lu_solve_batched_(out, piv, bview)
    assert x.data_ptr() == bview.data_ptr()
    assert torch.equal(x.cpu(), _ref_solve(n, batch, nrhs))
    binside = torch.zeros(bbuf.shape, dtype=torch.bool)
    binside[1:-1, :n, :nrhs] = True
    assert torch.equal(_bits(bbuf)[~binside], bbefore[~binside])
    # a 1-D right-hand side per member that is a column of a wider buffer
    wide = torch.full((batch, n, 3), NAN, dtype=torch.float64, device=dev)
    wide[:, :, 1] = _t(_rhs(n, batch, 0), dev)
    ops.lu_solve_batched_(out, piv, wide[:, :, 1])
    assert torch.equal(wide[:, :, 1].cpu(), _ref_solve(n, batch, 0))
    assert bool(torch.isnan(wide[:, :, 0]).all()) and bool(torch.isnan(wide[:, :, 2]).all())


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [7, 16, 33])
def test_piv_and_info_guards_through_the_c_entry(n, dev):
    L = _native.lib()
    batch, guard = 9, 16
    want_lu, want_piv, want_info = _ref_factor(n, batch)
    a = _t(_batch(n, batch), dev)
    pbuf = torch.full((batch * n + 2 * guard,), -77, dtype=torch.int32, device=dev)
    ibuf = torch.full((batch + 2 * guard,), -77, dtype=torch.int32, device=dev)
    piv, info = pbuf[guard:guard + batch * n], ibuf[guard:guard + batch]
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            _native.check(L.mpx_lu_factor_batched_f64(a.data_ptr(), batch, n, n, n * n, piv.data_ptr(), info.data_ptr(),
                                                      None, 0, _native.stream_of(a)))
        torch.cuda.synchronize(dev)
    else:
        L.mpx_cpu_lu_factor_batched_f64(a.data_ptr(), batch, n, n, n * n, piv.data_ptr(), info.data_ptr())
    assert torch.equal(a.cpu(), want_lu)
    assert torch.equal(piv.cpu().view(batch, n), want_piv) and torch.equal(info.cpu(), want_info)
    for buf, used in ((pbuf, batch * n), (ibuf, batch)):
        assert bool((buf[:guard] == -77).all()) and bool((buf[guard + used:] == -77).all())


# ---------------------------------------------------------------- 5. n > 64: the single-matrix kernels in a loop
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [65, 257])
def test_fallback_above_64(n, dev):
    _ld_ok()
    fams = [_exact_family(n, seed=m) for m in range(2)]
    a = np.stack([f[0] for f in fams])
    lu, piv, info = ops.lu_factor_batched(_t(a, dev))
    assert np.array_equal(_np(info), [0, 0])
    perm, low, up = ops.lu_unpack_batched(lu, piv)
    for m, f in enumerate(fams):
        assert np.array_equal(_np(perm[m]), f[3]) and np.array_equal(_np(low[m]), f[1])
        assert np.array_equal(_np(up[m]), f[2])
    x = np.random.RandomState(n).randint(-4, 5, size=(2, n, 17)).astype(np.float64)
    assert np.array_equal(_np(ops.lu_solve_batched(lu, piv, _t(a @ x, dev))), x)
    # Higham's bounds on general input, and info per member: member 1 has a zero column
    g = np.stack([_normal(n), _normal(n)])
    g[1, :, 40] = 0.0
    lu, piv, info = ops.lu_factor_batched(_t(g, dev))
    assert np.array_equal(_np(info), [0, 41])
    b = np.random.RandomState(n + 1).standard_normal((2, n, 5))
    xs = ops.lu_solve_batched(lu[:1], piv[:1], _t(b[:1], dev))
    for m in range(2):
        _factor_bound(g[m], _np(lu[m]), _np(piv[m]))
    _solve_bound(_np(lu[0]), _np(piv[0]), b[0], _np(xs[0]))


# ---------------------------------------------------------------- 6. slogdet, BatchedDenseLU
def _parity(perm) -> int:
    seen, parity = np.zeros(len(perm), bool), 1
    for i in range(len(perm)):
        j, length = i, 0
        while not seen[j]:
            seen[j] = True
            j = perm[j]
            length += 1
        if length and length % 2 == 0:
            parity = -parity
    return parity


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [1, 8, 17, 64])
def test_slogdet_exact_family(n, dev):
    batch = 7
    fams = [_exact_family(n, seed=m) for m in range(batch)]
    a = _t(np.stack([f[0] for f in fams]), dev)
    lu, piv, _ = ops.lu_factor_batched(a)
    sign, logabs = ops.slogdet_batched(lu, piv)
    assert sign.shape == (batch,) and logabs.shape == (batch,) and sign.dtype == torch.float64
    for m, (_, _, up, perm) in enumerate(fams):
        d = np.diag(up)
        assert float(sign[m]) == float(np.prod(np.sign(d)) * _parity(perm))
        want = float(np.sum(np.log2(np.abs(d)))) * math.log(2.0)
        assert abs(float(logabs[m]) - want) <= 1e-12 * max(1.0, abs(want))
    s2, l2 = BatchedDenseLU(a).slogdet()
    assert torch.equal(s2, sign) and torch.equal(l2, logabs)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [3, 16, 33, 64])
def test_batched_dense_lu_matches_dense_lu(n, dev):
    batch = 5
    a = _batch(n, batch)
    model = BatchedDenseLU(_t(a, dev))
    inv = model.inverse()
    assert inv.shape == (batch, n, n)
    b2, b1 = _rhs(n, batch, 3), _rhs(n, batch, 0)
    x2, x1 = model.solve(_t(b2, dev)), model.solve(_t(b1, dev))
    for m in range(batch):
        single = DenseLU(_t(a[m]))
        assert torch.equal(inv[m].cpu(), single.inverse())
        assert torch.equal(x2[m].cpu(), single.solve(_t(b2[m])))
        assert torch.equal(x1[m].cpu(), single.solve(_t(b1[m])))


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_singular_members_are_named(dev):
    n, batch = 9, 8
    a = np.array(_batch(n, batch))
    a[3, :, 4] = 0.0
    a[5, :, 2] = 0.0
    t = _t(a, dev)
    _, _, info = ops.lu_factor_batched(t)
    assert np.array_equal(_np(info), [0, 0, 0, 5, 0, 3, 0, 0])
    b = torch.ones(batch, n, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match=r"matrix 3 .*column 4"):
        ops.solve_batched(t, b)
    with pytest.raises(RuntimeError, match=r"matrix 3 .*column 4"):
        BatchedDenseLU(t)
    with pytest.raises(RuntimeError, match=r"matrix 1 .*column 2"):
        ops.solve_batched(t[4:], b[4:])


# ---------------------------------------------------------------- 7. argument errors, empties
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_value_errors_and_empties(dev):
    f64 = dict(dtype=torch.float64, device=dev)
    a = torch.eye(4, **f64).repeat(3, 1, 1)
    lu, piv, _ = ops.lu_factor_batched(a)
    b = torch.ones(3, 4, **f64)
    with pytest.raises(ValueError, match="fp64 only"):
        ops.lu_factor_batched(a.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.lu_factor_batched_(a.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.lu_solve_batched(lu, piv, b.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.solve_batched(a, b.float())
    wide = torch.ones(3, 4, 8, **f64)
    flat = torch.ones(64, **f64)
    for bad in (torch.ones(4, 4, **f64), torch.ones(2, 3, 4, 4, **f64), torch.ones(3, 4, 5, **f64),
                torch.ones(3, 5, 4, **f64), wide[:, :, ::2], a.transpose(1, 2),
                flat.as_strided((3, 4, 4), (16, 2, 1)),        # rows overlap
                flat.as_strided((3, 4, 4), (15, 4, 1)),        # members overlap by one element
                torch.ones(1, 4, 4, **f64).expand(3, 4, 4)):   # a batch stride of 0
        for fn in (ops.lu_factor_batched_, ops.lu_factor_batched):
            with pytest.raises(ValueError):
                fn(bad)
        with pytest.raises(ValueError):
            ops.solve_batched(bad, b)
        with pytest.raises(ValueError):
            ops.lu_solve_batched(bad, piv, b)
        with pytest.raises(ValueError):
            ops.slogdet_batched(bad, piv)
        with pytest.raises(ValueError):
            ops.lu_unpack_batched(bad, piv)
    for bad_b in (torch.ones(3, 5, **f64), torch.ones(2, 4, **f64), torch.ones(4, **f64),
                  torch.ones(3, 4, 2, 2, **f64), torch.ones(3, 5, 2, **f64)):
        with pytest.raises(ValueError):
            ops.lu_solve_batched_(lu, piv, bad_b)
        with pytest.raises(ValueError):
            ops.lu_solve_batched(lu, piv, bad_b)
        with pytest.raises(ValueError):
            ops.solve_batched(a, bad_b)
    with pytest.raises(ValueError):  # in place needs contiguous rows; lu_solve_batched copies
        ops.lu_solve_batched_(lu, piv, torch.ones(3, 4, 6, **f64)[:, :, ::2])
    assert ops.lu_solve_batched(lu, piv, torch.ones(3, 4, 6, **f64)[:, :, ::2]).shape == (3, 4, 3)
    with pytest.raises(ValueError):  # members of B overlap
        ops.lu_solve_batched_(lu, piv, torch.ones(1, 4, 2, **f64).expand(3, 4, 2))
    for bad_piv in (piv[:2], piv[:, :3], piv.long(), piv[0], torch.zeros(3, 8, dtype=torch.int32, device=dev)[:, ::2]):
        with pytest.raises(ValueError):
            ops.lu_solve_batched(lu, bad_piv, b)
        with pytest.raises(ValueError):
            ops.slogdet_batched(lu, bad_piv)
        with pytest.raises(ValueError):
            ops.lu_unpack_batched(lu, bad_piv)
    if dev.type == "cuda":
        with pytest.raises(ValueError):
            ops.lu_solve_batched(lu, piv, b.cpu())
        with pytest.raises(ValueError):
            ops.lu_solve_batched(lu, piv.cpu(), b)
        with pytest.raises(ValueError):
            ops.solve_batched(a, b.cpu())
        with pytest.raises(ValueError):
            ops.slogdet_batched(lu, piv.cpu())
    # the single-matrix names still refuse a batch
    with pytest.raises(ValueError):
        ops.lu_factor(a)
    # empties: correctly shaped, nothing launched
    for shape in ((0, 4, 4), (3, 0, 0), (0, 0, 0)):
        e_lu, e_piv, e_info = ops.lu_factor_batched(torch.empty(shape, **f64))
        assert e_lu.shape == shape and e_piv.shape == shape[:2] and e_piv.dtype == torch.int32
        assert e_info.shape == shape[:1] and not bool(e_info.any())
        e_b = torch.empty(shape[:2] + (2,), **f64)
        assert ops.lu_solve_batched(e_lu, e_piv, e_b).shape == e_b.shape
        assert ops.solve_batched(torch.empty(shape, **f64), e_b).shape == e_b.shape
        sign, logabs = ops.slogdet_batched(e_lu, e_piv)
        assert sign.shape == shape[:1] and logabs.shape == shape[:1]
        if shape[0]:
            assert bool((sign == 1).all()) and bool((logabs == 0).all())
        perm, low, up = ops.lu_unpack_batched(e_lu, e_piv)
        assert perm.shape == shape[:2] and low.shape == shape and up.shape == shape
    assert ops.lu_solve_batched(lu, piv, torch.empty(3, 4, 0, **f64)).shape == (3, 4, 0)
    model = BatchedDenseLU(torch.empty(0, 4, 4, **f64))
    assert model.inverse().shape == (0, 4, 4)


def test_c_entry_points_refuse_bad_arguments():
    """Argument errors come back before any pointer is touched: null and
    dangling pointers, no device needed."""
    L = _native.lib()
    ARG = MPX_ERR_ARG
    wild = 0x10  # never a valid address: touching it would fault
    assert L.mpx_lu_batched_workspace_bytes(100, 64) == 0 and L.mpx_lu_batched_workspace_bytes(100, 1) == 0
    assert L.mpx_lu_batched_workspace_bytes(0, 300) == 0
    need = L.mpx_lu_batched_workspace_bytes(2, 300)
    assert need == L.mpx_lu_workspace_bytes(300) and need > 0
    f = L.mpx_lu_factor_batched_f64
    assert f(wild, -1, 4, 4, 16, wild, wild, None, 0, None) == ARG
    assert f(wild, 2, -1, 4, 16, wild, wild, None, 0, None) == ARG
    assert f(wild, 2, 4, 3, 16, wild, wild, None, 0, None) == ARG           # pitch < n
    assert f(wild, 2, 4, 4, 15, wild, wild, None, 0, None) == ARG           # stride < (n - 1) pitch + n
    assert f(wild, 2, 4, 6, 21, wild, wild, None, 0, None) == ARG
    assert f(wild, 2, 4, 2 ** 62, 2 ** 62, wild, wild, None, 0, None) == ARG  # the product does not wrap
    assert f(None, 2, 4, 4, 16, wild, wild, None, 0, None) == ARG
    assert f(wild, 2, 4, 4, 16, None, wild, None, 0, None) == ARG
    assert f(wild, 2, 4, 4, 16, wild, None, None, 0, None) == ARG
    assert b"lu batched" in L.mpx_last_error()
    assert f(wild, 2, 300, 300, 90000, wild, wild, None, 0, None) == ARG      # n > 64 needs the workspace
    assert f(wild, 2, 300, 300, 90000, wild, wild, wild, need - 1, None) == ARG
    assert f(wild, 2, 300, 300, 90000, wild, wild, 0x18, need, None) == ARG   # not 16-byte aligned
    assert f(wild, 0, 4, 4, 16, wild, wild, None, 0, None) == 0               # no-ops
    assert f(wild, 2, 0, 0, 0, wild, wild, None, 0, None) == 0
    s = L.mpx_lu_solve_batched_f64
    assert s(wild, -1, 4, 4, 16, wild, wild, 1, 1, 4, None) == ARG
    assert s(wild, 2, -1, 4, 16, wild, wild, 1, 1, 4, None) == ARG
    assert s(wild, 2, 4, 4, 16, wild, wild, -1, 1, 4, None) == ARG
    assert s(wild, 2, 4, 3, 16, wild, wild, 1, 1, 4, None) == ARG             # pitch < n
    assert s(wild, 2, 4, 4, 16, wild, wild, 3, 2, 12, None) == ARG            # pitch_b < nrhs
    assert s(wild, 2, 4, 4, 15, wild, wild, 1, 1, 4, None) == ARG             # short stride
    assert s(wild, 2, 4, 4, 16, wild, wild, 3, 3, 11, None) == ARG            # short stride_b
    assert s(wild, 2, 4, 4, 16, wild, wild, 3, 2 ** 62, 2 ** 62, None) == ARG
    assert s(None, 2, 4, 4, 16, wild, wild, 1, 1, 4, None) == ARG
    assert s(wild, 2, 4, 4, 16, None, wild, 1, 1, 4, None) == ARG
    assert s(wild, 2, 4, 4, 16, wild, None, 1, 1, 4, None) == ARG
    assert b"lu batched solve" in L.mpx_last_error()
    assert s(wild, 0, 4, 4, 16, wild, wild, 1, 1, 4, None) == 0
    assert s(wild, 2, 0, 0, 0, wild, wild, 1, 1, 0, None) == 0
    assert s(wild, 2, 4, 4, 16, wild, wild, 0, 0, 0, None) == 0
    # the CPU entries write nothing on bad arguments
    L.mpx_cpu_lu_factor_batched_f64(None, 2, 4, 4, 16, None, None)
    L.mpx_cpu_lu_factor_batched_f64(wild, -1, 4, 4, 16, wild, wild)
    L.mpx_cpu_lu_solve_batched_f64(None, 2, 4, 4, 16, None, None, 1, 1, 4)
    L.mpx_cpu_lu_solve_batched_f64(wild, 0, 4, 4, 16, wild, wild, 1, 1, 4)


# ---------------------------------------------------------------- 8. GPU only
@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 17, 64])
def test_gpu_same_bits_across_runs_and_layouts(gpu, n):
    batch = 65
    a = _t(_batch(n, batch), gpu)
    first = ops.lu_factor_batched(a)
    again = ops.lu_factor_batched(a)
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    buf = torch.full((batch, n + 2, n + 3), NAN, dtype=torch.float64, device=gpu)
    buf[:, :n, :n] = a
    padded = ops.lu_factor_batched_(buf[:, :n, :n])
    assert all(torch.equal(x, y) for x, y in zip(first, padded))
    b = _t(_rhs(n, batch, 17), gpu)
    x = ops.lu_solve_batched(first[0], first[1], b)
    assert torch.equal(x, ops.lu_solve_batched(first[0], first[1], b))
    assert torch.equal(x, ops.lu_solve_batched(padded[0], padded[1], b))


@pytest.mark.gpu
def test_gpu_side_stream_and_back_to_back(gpu):
    n, batch = 16, 130
    want = [_ref_factor(n, batch), _ref_factor(n + 1, batch)]
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        # two factorisations and two solves queued on one stream with nothing in between
        mats = [_t(_batch(n, batch), gpu), _t(_batch(n + 1, batch), gpu)]
        outs = [ops.lu_factor_batched_(m) for m in mats]
        xs = [ops.lu_solve_batched(o[0], o[1], _t(_rhs(k, batch, 3), gpu)) for o, k in zip(outs, (n, n + 1))]
    side.synchronize()
    for o, w, x, k in zip(outs, want, xs, (n, n + 1)):
        assert torch.equal(o[0].cpu(), w[0]) and torch.equal(o[1].cpu(), w[1]) and torch.equal(o[2].cpu(), w[2])
        assert torch.equal(x.cpu(), _ref_solve(k, batch, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 33])
def test_gpu_factors_cpu_solve_and_back(gpu, n):
    batch = 9
    a = _batch(n, batch)
    b = _rhs(n, batch, 3)
    g_lu, g_piv, _ = ops.lu_factor_batched(_t(a, gpu))
    c_lu, c_piv, _ = ops.lu_factor_batched(_t(a))
    want = _ref_solve(n, batch, 3)
    assert torch.equal(ops.lu_solve_batched(g_lu.cpu(), g_piv.cpu(), _t(b)), want)
    assert torch.equal(ops.lu_solve_batched(c_lu.to(gpu), c_piv.to(gpu), _t(b, gpu)).cpu(), want)
