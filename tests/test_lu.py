"""Dense LU with partial pivoting (``ops.lu_factor`` and friends, ``DenseLU``).

The trailing update accumulates in the MFMA's order, so GPU and CPU results are
not required to agree bit for bit on general input. Correctness is pinned by
two yardsticks that do not depend on the code under test:

A. Exact recovery. ``A[perm] = L @ U`` with L unit lower (entries 0, +-0.25,
   +-0.5), U with integer entries in [-8, 8] above a diagonal of +-2^e
   (e in 0..3), and a random row order. Every quantity of the elimination is a
   small dyadic rational, so every product and sum is exact in fp64 in any
   order; at step k the true pivot row holds u_kk and every other candidate at
   most |u_kk| / 2, so partial pivoting has no ties and must find ``perm``.
   The factors, the row order and the solution of ``A X = B`` with integer X
   are compared with ``array_equal``: no tolerance.

B. Higham's componentwise backward-error bounds, evaluated in ``np.longdouble``
   (eps below 2^-60 is asserted): with u = 2^-53, gamma_m = m u / (1 - m u),
       |A[perm] - L U| <= gamma_n |L||U|,
       |B[perm] - L U X| <= gamma_3n |L||U||X|      (elementwise)
   for any summation order, each operation rounded once or fused. The
   thresholds are derived, not tuned; LAPACK's factors of a 300 x 300 normal
   matrix sit at about 0.01 of the first one. ``max|L| <= 1`` is asserted
   exactly: it holds iff every pivot was a column maximum of the computed
   values.

Every case runs on a contiguous matrix and with a row pitch of n + 2 and n + 3
(for every n one of the two pitches is odd, which leaves every second row only
8-byte aligned); the padding holds a sentinel that must survive. Sizes: the
panel width and the update tile are 64, the MFMA tile 16, one workgroup factors
a remainder of at most 256 rows, hence 15..17, 63..65, 127, 129, 256, 257, and
1100 for several update tiles in both directions, ragged on both edges.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.models import DenseLU

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


def _padding_kept(back: torch.Tensor, c: int) -> bool:
    return bool((back[:, c:] == SENT).all())


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().copy()


def _perm_of(piv) -> np.ndarray:
    perm = np.arange(len(piv))
    for k, p in enumerate(piv):
        perm[k], perm[p] = perm[p], perm[k]
    return perm


@functools.lru_cache(maxsize=None)
def _exact_family(n: int, seed: int = 0):
    """(A, L, U, perm) of yardstick A; shared, never modified."""
    rng = np.random.RandomState(1000 * seed + n)
    low = np.tril(rng.choice([0.0, 0.25, -0.25, 0.5, -0.5], size=(n, n)), -1) + np.eye(n)
    up = np.triu(rng.randint(-8, 9, size=(n, n)).astype(np.float64), 1)
    up += np.diag(rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.randint(0, 4, size=n))
    perm = rng.permutation(n)
    a = np.empty((n, n))
    a[perm] = low @ up
    for m in (a, low, up, perm):
        m.setflags(write=False)
    return a, low, up, perm


@functools.lru_cache(maxsize=None)
def _normal(n: int, graded: bool = False) -> np.ndarray:
    a = np.random.RandomState(7 + n).standard_normal((n, n))
    if graded:
        a = a * (10.0 ** np.linspace(-8, 8, n))[:, None]
    a.setflags(write=False)
    return a


def _ld_ok():
    if np.finfo(LD).eps >= 2.0 ** -60:
        pytest.skip("np.longdouble is not an extended format here")


def _factor_bound(a: np.ndarray, lu: np.ndarray, piv) -> float:
    """max over the elements of |A[perm] - L U| / (gamma_n |L||U|); asserts max|L| <= 1."""
    n = a.shape[0]
    low = (np.tril(lu, -1) + np.eye(n)).astype(LD)
    up = np.triu(lu).astype(LD)
    assert np.abs(np.tril(lu, -1)).max(initial=0.0) <= 1.0
    res = np.abs(a[_perm_of(piv)].astype(LD) - low @ up)
    bound = _gamma(n) * (np.abs(low) @ np.abs(up))
    assert np.all(res <= bound), float(np.max(res - bound))
    return float(np.max(res / np.where(bound > 0, bound, LD(1))))


def _solve_bound(lu: np.ndarray, piv, b: np.ndarray, x: np.ndarray) -> float:
    n = lu.shape[0]
    b, x = b.reshape(n, -1), x.reshape(n, -1)
    assert np.all(np.isfinite(x))
    low = (np.tril(lu, -1) + np.eye(n)).astype(LD)
    up = np.triu(lu).astype(LD)
    res = np.abs(b[_perm_of(piv)].astype(LD) - low @ (up @ x.astype(LD)))
    bound = _gamma(3 * n) * (np.abs(low) @ (np.abs(up) @ np.abs(x.astype(LD))))
    assert np.all(res <= bound), float(np.max(res - bound))
    return float(np.max(res / np.where(bound > 0, bound, LD(1))))


def _check_exact(n: int, layout: str, device, seed: int = 0):
    a, low, up, perm = _exact_family(n, seed)
    view, back = _place(a, layout, device)
    out, piv, info = ops.lu_factor_(view)
    assert out.data_ptr() == view.data_ptr()
    assert piv.dtype == torch.int32 and info.dtype == torch.int32 and piv.device == view.device
    assert int(info.item()) == 0
    p_out, l_out, u_out = ops.lu_unpack(out, piv)
    assert np.array_equal(_np(p_out), perm)
    assert np.array_equal(_np(l_out), low)
    assert np.array_equal(_np(u_out), up)
    assert _padding_kept(back, n)
    return out, piv


# ---------------------------------------------------------------- 1. exact recovery
EXACT_N = [1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 200, 256, 257, 1100]


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", EXACT_N)
def test_exact_factor_and_solve(n, layout, dev):
    a = _exact_family(n)[0]
    lu, piv = _check_exact(n, layout, dev)
    rng = np.random.RandomState(n)
    for nrhs in NRHS:
        x = rng.randint(-4, 5, size=(n, nrhs)).astype(np.float64)
        bview, bback = _place(a @ x, layout, dev)
        got = ops.lu_solve_(lu, piv, bview)
        assert got.data_ptr() == bview.data_ptr()
        assert np.array_equal(_np(got), x), (n, nrhs)
        assert _padding_kept(bback, nrhs)
    x = rng.randint(-4, 5, size=n).astype(np.float64)
    b = torch.from_numpy(a @ x).to(dev)
    keep = b.clone()
    got = ops.lu_solve(lu, piv, b)
    assert got.shape == (n,) and np.array_equal(_np(got), x)
    assert torch.equal(b, keep)
    # a 1-D right-hand side that is a column of a wider buffer
    wide = torch.full((n, 3), SENT, dtype=torch.float64, device=dev)
    wide[:, 1] = keep
    ops.lu_solve_(lu, piv, wide[:, 1])
    assert np.array_equal(_np(wide[:, 1]), x)
    assert bool((wide[:, 0] == SENT).all()) and bool((wide[:, 2] == SENT).all())


# ---------------------------------------------------------------- 2. bounds
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n,graded", [(65, False), (300, False), (129, True)])
def test_bounds(n, graded, layout, dev):
    _ld_ok()
    a = _normal(n, graded)
    view, back = _place(a, layout, dev)
    lu, piv, info = ops.lu_factor_(view)
    assert int(info.item()) == 0
    lu_np, piv_np = _np(lu), _np(piv)
    ratio = _factor_bound(a, lu_np, piv_np)
    assert _padding_kept(back, n)
    b = np.random.RandomState(n).standard_normal((n, 17))
    bview, bback = _place(b, layout, dev)
    x = ops.lu_solve_(lu, piv, bview)
    ratio_s = _solve_bound(lu_np, piv_np, b, _np(x))
    assert _padding_kept(bback, 17)
    print(f"n={n} graded={graded} {layout} {dev}: factor {ratio:.4f}, solve {ratio_s:.4f} of the bound")


# ---------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ties_take_the_lowest_row(layout, dev):
    n = 70
    a = np.random.RandomState(3).standard_normal((n, n))
    a[:, 0] = 0.5 - 0.001 * np.arange(n)
    a[:6, 0] = [1, -3, 3, 2, -3, 3]
    view, _ = _place(a, layout, dev)
    _, piv, _ = ops.lu_factor_(view)
    assert int(piv[0]) == 1
    for m in (n, 300):  # one workgroup; the partial searches of several
        big = np.random.RandomState(4).standard_normal((m, m))
        big[:, 0] = -2.0
        view, _ = _place(big, layout, dev)
        _, piv, _ = ops.lu_factor_(view)
        assert int(piv[0]) == 0
    big = np.random.RandomState(5).standard_normal((300, 300))
    big[:, 0] = 0.25
    big[[7, 150, 299], 0] = [-3, 3, -3]
    view, _ = _place(big, layout, dev)
    _, piv, _ = ops.lu_factor_(view)
    assert int(piv[0]) == 7


# ---------------------------------------------------------------- 4. identity, permutation
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_identity_and_permutation(layout, dev):
    n = 130
    view, back = _place(np.eye(n), layout, dev)
    lu, piv, info = ops.lu_factor_(view)
    assert np.array_equal(_np(lu), np.eye(n)) and np.array_equal(_np(piv), np.arange(n)) and int(info.item()) == 0
    assert _padding_kept(back, n)
    order = np.random.RandomState(11).permutation(n)
    pm = np.eye(n)[order]
    cur, want = pm.copy(), []
    for k in range(n):  # elimination never changes a permutation matrix
        p = k + int(np.argmax(np.abs(cur[k:, k])))
        want.append(p)
        cur[[k, p]] = cur[[p, k]]
    view, back = _place(pm, layout, dev)
    lu, piv, info = ops.lu_factor_(view)
    assert np.array_equal(_np(lu), np.eye(n)) and np.array_equal(_np(piv), np.array(want)) and int(info.item()) == 0
    perm, low, up = ops.lu_unpack(lu, piv)
    assert np.array_equal(pm[_np(perm)], np.eye(n))
    assert _padding_kept(back, n)


# ---------------------------------------------------------------- 5. singular input
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k", [0, 64, 96])
def test_zero_column(k, layout, dev):
    _ld_ok()
    n = 97
    a = np.random.RandomState(20 + k).standard_normal((n, n))
    a[:, k] = 0.0
    view, back = _place(a, layout, dev)
    lu, piv, info = ops.lu_factor_(view)
    assert int(info.item()) == k + 1
    if k == 0:
        assert int(piv[0]) == 0
    assert float(lu[k, k]) == 0.0
    _factor_bound(a, _np(lu), _np(piv))
    assert _padding_kept(back, n)
    with pytest.raises(RuntimeError, match=f"column {k}"):
        ops.solve(torch.from_numpy(a.copy()).to(dev), torch.ones(n, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError):
        DenseLU(torch.from_numpy(a.copy()).to(dev))


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [97, 300])
def test_zero_column_several_workgroups_and_regular(n, dev):
    a = np.random.RandomState(n).standard_normal((n, n))
    assert int(ops.lu_factor(torch.from_numpy(a.copy()).to(dev))[2].item()) == 0
    a[:, 1] = 0.0
    a[:, 70] = 0.0
    lu, piv, info = ops.lu_factor(torch.from_numpy(a).to(dev))
    assert int(info.item()) == 2 and int(piv[1]) == 1  # the first zero pivot is reported
    x = ops.solve(torch.from_numpy(_exact_family(65)[0].copy()).to(dev), torch.ones(65, dtype=torch.float64, device=dev))
    assert x.shape == (65,)


# ---------------------------------------------------------------- 6. interfaces
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_copies_views_and_streams(dev):
    n = 200
    a, low, up, perm = _exact_family(n)
    t = torch.from_numpy(a.copy()).to(dev)
    keep = t.clone()
    lu, piv, info = ops.lu_factor(t)
    assert torch.equal(t, keep) and lu.data_ptr() != t.data_ptr()
    assert np.array_equal(_np(torch.triu(lu)), up)
    same, _, _ = ops.lu_factor_(t)
    assert same.data_ptr() == t.data_ptr() and torch.equal(same, lu)
    # every second row of a taller buffer: the pitch is 2 n
    tall = torch.full((2 * n, n), SENT, dtype=torch.float64, device=dev)
    tall[::2] = keep
    out, piv2, _ = ops.lu_factor_(tall[::2])
    assert torch.equal(out, lu) and torch.equal(piv2, piv)
    assert bool((tall[1::2] == SENT).all())
    # the solution through solve(); B untouched
    x = np.random.RandomState(1).randint(-4, 5, size=(n, 3)).astype(np.float64)
    b = torch.from_numpy(a @ x).to(dev)
    bkeep = b.clone()
    assert np.array_equal(_np(ops.solve(keep, b)), x) and torch.equal(b, bkeep)
    if dev.type == "cuda":
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            t2 = keep.clone()
            lu2, piv3, _ = ops.lu_factor_(t2)
            x2 = ops.lu_solve(lu2, piv3, b)
        side.synchronize()
        assert torch.equal(lu2, lu) and np.array_equal(_np(x2), x)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [1, 17, 200, 257])
def test_slogdet_exact_family(n, dev):
    a, low, up, perm = _exact_family(n)
    lu, piv, _ = ops.lu_factor(torch.from_numpy(a.copy()).to(dev))
    sign, logabs = ops.slogdet(lu, piv)
    d = np.diag(up)
    seen, parity = np.zeros(n, bool), 1
    for i in range(n):  # parity of perm from its cycles
        j, length = i, 0
        while not seen[j]:
            seen[j] = True
            j = perm[j]
            length += 1
        if length and length % 2 == 0:
            parity = -parity
    assert float(sign) == float(np.prod(np.sign(d)) * parity)
    want = float(np.sum(np.log2(np.abs(d)))) * math.log(2.0)
    assert abs(float(logabs) - want) <= 1e-12 * max(1.0, abs(want))
    s2, l2 = DenseLU(torch.from_numpy(a.copy()).to(dev)).slogdet()
    assert float(s2) == float(sign) and float(l2) == float(logabs)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [65, 300])
def test_dense_lu_inverse_and_solve(n, dev):
    _ld_ok()
    a = _normal(n)
    m = DenseLU(torch.from_numpy(a.copy()).to(dev))
    inv = m.inverse()
    assert inv.shape == (n, n)
    _solve_bound(_np(m.lu), _np(m.piv), np.eye(n), _np(inv))
    b = np.random.RandomState(2).standard_normal(n)
    _solve_bound(_np(m.lu), _np(m.piv), b, _np(m.solve(torch.from_numpy(b).to(dev))))


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_value_errors(dev):
    a = torch.eye(4, dtype=torch.float64, device=dev)
    lu, piv, _ = ops.lu_factor(a)
    b = torch.ones(4, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="fp64 only"):
        ops.lu_factor(a.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.lu_factor_(a.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.lu_solve(lu, piv, b.float())
    with pytest.raises(ValueError, match="fp64 only"):
        ops.solve(a, b.float())
    for bad in (torch.ones(4, dtype=torch.float64, device=dev), torch.ones(2, 4, 4, dtype=torch.float64, device=dev),
                torch.ones(4, 5, dtype=torch.float64, device=dev), torch.ones(5, 4, dtype=torch.float64, device=dev),
                torch.ones(4, 8, dtype=torch.float64, device=dev)[:, ::2]):
        for fn in (ops.lu_factor_, ops.lu_factor):
            with pytest.raises(ValueError):
                fn(bad)
        with pytest.raises(ValueError):
            ops.solve(bad, b)
        with pytest.raises(ValueError):
            ops.lu_solve(bad, piv, b)
        with pytest.raises(ValueError):
            ops.slogdet(bad, piv)
        with pytest.raises(ValueError):
            ops.lu_unpack(bad, piv)
    with pytest.raises(ValueError):  # a transposed matrix has stride(1) != 1
        ops.lu_factor_(torch.ones(4, 4, dtype=torch.float64, device=dev).t())
    for bad_b in (torch.ones(5, dtype=torch.float64, device=dev), torch.ones(3, 2, dtype=torch.float64, device=dev),
                  torch.ones(4, 2, 2, dtype=torch.float64, device=dev)):
        with pytest.raises(ValueError):
            ops.lu_solve_(lu, piv, bad_b)
        with pytest.raises(ValueError):
            ops.lu_solve(lu, piv, bad_b)
    with pytest.raises(ValueError):  # in place needs contiguous rows; lu_solve copies
        ops.lu_solve_(lu, piv, torch.ones(4, 6, dtype=torch.float64, device=dev)[:, ::2])
    with pytest.raises(ValueError):
        ops.solve(a, torch.ones(5, dtype=torch.float64, device=dev))
    for bad_piv in (piv[:3], piv.long(), torch.zeros(4, 1, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError):
            ops.lu_solve(lu, bad_piv, b)
        with pytest.raises(ValueError):
            ops.slogdet(lu, bad_piv)
    if dev.type == "cuda":
        with pytest.raises(ValueError):
            ops.lu_solve(lu, piv, b.cpu())
        with pytest.raises(ValueError):
            ops.lu_solve(lu, piv.cpu(), b)
        with pytest.raises(ValueError):
            ops.solve(a, b.cpu())
    # empty systems are no-ops
    e_lu, e_piv, e_info = ops.lu_factor(torch.empty(0, 0, dtype=torch.float64, device=dev))
    assert e_lu.shape == (0, 0) and e_piv.shape == (0,) and int(e_info.item()) == 0
    assert ops.lu_solve(lu, piv, torch.empty(4, 0, dtype=torch.float64, device=dev)).shape == (4, 0)


def test_c_entry_points_refuse_bad_arguments():
    """Argument errors come back before any pointer is touched: null pointers
    throughout, no device needed."""
    L = _native.lib()
    ARG = 1  # MPX_ERR_ARG
    assert L.mpx_lu_workspace_bytes(0) == 0
    need = L.mpx_lu_workspace_bytes(1000)
    assert need > 0 and L.mpx_lu_workspace_bytes(100000) >= need
    assert L.mpx_lu_factor_f64(None, -1, 0, None, None, None, 0, None) == ARG
    assert L.mpx_lu_factor_f64(None, 4, 3, None, None, None, 0, None) == ARG
    assert L.mpx_lu_factor_f64(None, 4, 4, None, None, None, 0, None) == ARG  # short workspace, null pointers
    assert L.mpx_lu_factor_f64(None, 4, 4, None, None, None, need, None) == ARG
    assert b"lu" in L.mpx_last_error()
    assert L.mpx_lu_factor_f64(None, 0, 0, None, None, None, 0, None) == 0  # n = 0: no-op
    assert L.mpx_lu_solve_f64(None, -1, 0, None, None, 1, 1, None, 0, None) == ARG
    assert L.mpx_lu_solve_f64(None, 4, 4, None, None, -1, 0, None, 0, None) == ARG
    assert L.mpx_lu_solve_f64(None, 4, 3, None, None, 1, 1, None, 0, None) == ARG
    assert L.mpx_lu_solve_f64(None, 4, 4, None, None, 3, 2, None, 0, None) == ARG
    assert L.mpx_lu_solve_f64(None, 4, 4, None, None, 1, 1, None, 0, None) == ARG  # null pointers
    assert L.mpx_lu_solve_f64(None, 0, 0, None, None, 3, 3, None, 0, None) == 0
    assert L.mpx_lu_solve_f64(None, 4, 4, None, None, 0, 0, None, 0, None) == 0


# ---------------------------------------------------------------- 7. GPU only
@pytest.mark.gpu
def test_gpu_back_to_back_share_one_workspace(gpu):
    """Two factorisations of different matrices queued on one stream with one
    workspace: a stale counter or pivot partial of the first would break the
    second."""
    L = _native.lib()
    n = 300  # more rows than one workgroup takes: the counted panel launches run
    fam = [_exact_family(n, seed) for seed in (1, 2)]
    mats = [torch.from_numpy(f[0].copy()).to(gpu) for f in fam]
    pivs = [torch.empty(n, dtype=torch.int32, device=gpu) for _ in fam]
    infos = [torch.full((1,), -1, dtype=torch.int32, device=gpu) for _ in fam]
    nbytes = int(L.mpx_lu_workspace_bytes(n))
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=gpu)  # a dirty workspace is the caller's right
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for m, p, i in zip(mats, pivs, infos):
        _native.check(L.mpx_lu_factor_f64(m.data_ptr(), n, n, p.data_ptr(), i.data_ptr(), ws.data_ptr(), nbytes,
                                          stream))
    torch.cuda.synchronize(gpu)
    for (a, low, up, perm), m, p, i in zip(fam, mats, pivs, infos):
        assert int(i.item()) == 0
        p_out, l_out, u_out = ops.lu_unpack(m, p)
        assert np.array_equal(_np(p_out), perm) and np.array_equal(_np(l_out), low) and np.array_equal(_np(u_out), up)


@pytest.mark.gpu
def test_gpu_factors_cpu_solve_and_back(gpu):
    _ld_ok()
    n = 300
    a = _normal(n)
    b = np.random.RandomState(9).standard_normal((n, 5))
    g_lu, g_piv, _ = ops.lu_factor(torch.from_numpy(a.copy()).to(gpu))
    c_lu, c_piv, _ = ops.lu_factor(torch.from_numpy(a.copy()))
    x = ops.lu_solve(g_lu.cpu(), g_piv.cpu(), torch.from_numpy(b.copy()))
    _solve_bound(_np(g_lu), _np(g_piv), b, _np(x))
    x = ops.lu_solve(c_lu.to(gpu), c_piv.to(gpu), torch.from_numpy(b.copy()).to(gpu))
    _solve_bound(_np(c_lu), _np(c_piv), b, _np(x))
