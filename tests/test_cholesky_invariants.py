"""Dense Cholesky, second pass: what test_cholesky.py leaves open from column 64
on, where the f64 MFMA is in every element. Same conventions: NaN in the strict
upper triangle, the sentinel in the pitch padding, both back bit for bit.

1. A wide exact family, ``array_equal``. test_cholesky's exact family fits a
   24-bit significand, so a kernel that accumulated in fp32 would recover it.
   Here L has strictly lower entries m 2^-10 with integer |m| <= 2^(10+t) and a
   diagonal of powers of two (every root and every quotient (l_ij l_jj) / l_jj is
   exact); A = L L^T and B = A X are built in integers, in units of 2^-20. Every
   intermediate of the factorisation is a partial sum of sum_k l_ik l_jk, every
   intermediate of the solve one of sum_k l_ik sum_m l_mk x_m, so
       factor budget = max (|L||L^T|),   solve budget = max (|L| (|L^T||X|))
   (integers, units of 2^-20) bound them all. The tests assert
   2^45 <= budget < 2^53: below 2^53 everything is exact in fp64 in any
   summation order, fused or not; from 2^45 on nothing that keeps fewer than
   about 45 bits anywhere can return the constructed values.

2. Bit invariants on random SPD data. An element's operations depend on its own
   row, its own column and the panel origin only: not on n, on how ragged a tile
   is, or on the lane, wave or workgroup that holds it. Hence, all
   ``array_equal``: (a) chol(A[:m, :m]) is the leading block of chol(A);
   (b) a block-diagonal matrix factors block by block; (c) the phases of
   ``mpx_chol_phase_f64`` over every panel give the factorisation's bits;
   (d) chol(D A D) = D chol(A) for D a diagonal of powers of two while nothing
   leaves the normal range; (e) the columns of B are independent systems, NaN
   and infinities included; (f) 16-byte and 8-byte operand loads give the same
   bits, in every combination of L's and B's alignment; (g) the rows of a taller
   buffer below a ragged last tile are left alone.

3. The three modes of the update kernel alone against ``np.longdouble``. One
   element c - sum_{k < K} a_k b_k, summed in any order with or without FMA,
   is within gamma_{K+1} (|c| + sum |a_k||b_k|) of the exact value (each product
   rounded at most once, at most K additions on any term's path), gamma_m =
   m u / (1 - m u), u = 2^-53. A chain of S such updates of one element is the
   same sum with the stages' roundings added up: gamma_{K_1 + .. + K_S + S}.
   The long-double reference's own error is 2^-11 of these bounds. Each test
   prints its largest ratio to the bound; a sequential float64 evaluation sits
   near 0.08, a float32 one near 6e7.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops

from .test_cholesky import (DEVICES, LAYOUTS, LD, SENT, _gamma, _ld_ok, _np, _padding_kept, _place, _place_lower,
                            _spd, _untouched)
from .test_cholesky import dev  # noqa: F401  (the CPU / GPU fixture)


def _factor(a: np.ndarray, layout: str, device):
    """(tril(L), info) of ``a`` factored in place in a NaN / sentinel buffer."""
    view, back = _place_lower(a, layout, device)
    l, info = ops.cholesky_factor_(view)
    assert _untouched(view, back)
    return np.tril(_np(l)), int(info.item())


def _factor_on(a: np.ndarray, layout: str, device):
    """The factor left on the device, for a solve: (view, tril(L) as numpy)."""
    view, back = _place_lower(a, layout, device)
    l, info = ops.cholesky_factor_(view)
    assert int(info.item()) == 0 and _untouched(view, back)
    return l, np.tril(_np(l))


def _solve(l: torch.Tensor, b: np.ndarray, layout: str, device) -> np.ndarray:
    bview, bback = _place(b, layout, device)
    x = ops.cholesky_solve_(l, bview)
    assert x.data_ptr() == bview.data_ptr() and _padding_kept(bback, b.shape[1])
    return _np(x)


# ---------------------------------------------------------------- 1. the wide exact family
def _exact_f64(units: np.ndarray, scale: float) -> np.ndarray:
    out = units.astype(np.float64)
    assert np.array_equal(out.astype(np.int64), units), "the integers do not fit fp64"
    return out * scale  # a power of two


@functools.lru_cache(maxsize=None)
def _wide_family(n: int, t: int, seed: int = 0):
    """(A, L, factor budget, L in units of 2^-10); shared, never modified. The
    integer products run in int64: |l| <= 2^(10+t) units bounds every sum of n
    products by n 4^(10+t), asserted below 2^62 in Python integers (no wrap);
    n = 17 is also built from Python integers in object arrays."""
    rng = np.random.RandomState(100000 * seed + 1000 * t + n)
    lim = 2 ** (10 + t)
    li = np.tril(rng.randint(-lim, lim + 1, size=(n, n)).astype(np.int64), -1)
    li += np.diag(rng.choice([256, 512, 1024, 2048, 4096, 8192], size=n).astype(np.int64))  # 0.25 .. 8
    assert n * max(lim, 8192) ** 2 < 2 ** 62
    ai = li @ li.T
    if n <= 17:
        lo = li.astype(object)
        assert np.array_equal(lo.dot(lo.T), ai.astype(object))
    budget = int((np.abs(li) @ np.abs(li).T).max())
    a, low = _exact_f64(ai, 2.0 ** -20), _exact_f64(li, 2.0 ** -10)
    for m in (a, low, li):
        m.setflags(write=False)
    return a, low, budget, li


def _wide_rhs(n: int, t: int, nrhs: int):
    """(B, X, solve budget) for the family above: integer X in [-8, 8], B = A X."""
    _, _, _, li = _wide_family(n, t)
    xi = np.random.RandomState(7 * n + nrhs).randint(-8, 9, size=(n, nrhs)).astype(np.int64)
    assert 8 * n * n * int(np.abs(li).max()) ** 2 < 2 ** 62
    bi = li @ (li.T @ xi)
    budget = int((np.abs(li) @ (np.abs(li).T @ np.abs(xi))).max())
    return _exact_f64(bi, 2.0 ** -20), xi.astype(np.float64), budget


WIDE_N = [17, 65, 129, 193, 321]
WIDE_T = 12
# t of the solve cases: 8 gives budgets of 2^47.3 .. 2^51.9 from n = 65 on; at n = 17 the sums are
# short (2^43.9 at t = 8), and the factor's t = 12 gives 2^51.4 .. 2^52.0
SOLVE_T = {17: 12, 65: 8, 129: 8, 193: 8, 321: 8}


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", WIDE_N)
def test_wide_family_factor(n, layout, dev):
    a, low, budget, _ = _wide_family(n, WIDE_T)
    assert 2 ** 45 <= budget < 2 ** 53, f"factor budget 2^{np.log2(float(budget)):.1f}"
    got, info = _factor(a, layout, dev)
    assert info == 0
    assert np.array_equal(got, low)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", WIDE_N)
def test_wide_family_solve(n, layout, dev):
    t = SOLVE_T[n]
    a, low, _, _ = _wide_family(n, t)
    l, got = _factor_on(a, layout, dev)
    assert np.array_equal(got, low)
    for nrhs in (1, 17, 65):
        b, x, budget = _wide_rhs(n, t, nrhs)
        assert 2 ** 45 <= budget < 2 ** 53, f"solve budget 2^{np.log2(float(budget)):.1f} at nrhs = {nrhs}"
        assert np.array_equal(_solve(l, b, layout, dev), x), nrhs


# ---------------------------------------------------------------- 2a. nesting
NEST_M = [1, 63, 64, 65, 100, 128, 129, 192, 200, 257, 320]


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", ["even", "odd"])  # pitch m + 2 and m + 3: both parities at every m
def test_leading_blocks_nest(layout, dev):
    n = 321
    a = _spd(n)
    full, info = _factor(a, layout, dev)
    assert info == 0
    for m in NEST_M:
        part, info = _factor(a[:m, :m], layout, dev)
        assert info == 0
        assert np.array_equal(part, full[:m, :m]), m


# ---------------------------------------------------------------- 2b. block diagonal
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("m2", [1, 40, 64, 137])
@pytest.mark.parametrize("m", [64, 128])
def test_block_diagonal_factors_block_by_block(m, m2, dev):
    """A tile at a nonzero origin behaves like tile (0, 0), and the second
    block's first diagonal block has the same bits from the update's workgroup
    (here) and from the diagonal kernel (alone). The zero block stays zero
    (0 / d, then c - 0 * 0 in the update)."""
    a1, a2 = _spd(m), _spd(m2)
    a = np.zeros((m + m2, m + m2))
    a[:m, :m] = a1
    a[m:, m:] = a2
    for layout in ("even", "odd"):
        got, info = _factor(a, layout, dev)
        l1, info1 = _factor(a1, layout, dev)
        l2, info2 = _factor(a2, layout, dev)
        assert (info, info1, info2) == (0, 0, 0)
        assert np.array_equal(got[m:, m:], l2)
        assert np.array_equal(got[:m, :m], l1)
        assert np.array_equal(got[m:, :m], np.zeros((m2, m)))


# ---------------------------------------------------------------- 2c. phases = factorisation
def _by_phases(a: np.ndarray, layout: str, gpu):
    """(tril, info) from mpx_chol_phase_f64 over every panel, phases 0, 1, 2."""
    n = a.shape[0]
    view, back = _place_lower(a, layout, gpu)
    info = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    L = _native.lib()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for j0 in range(0, n, 64):
        for phase in (0, 1, 2):
            _native.check(L.mpx_chol_phase_f64(view.data_ptr(), n, view.stride(0), info.data_ptr(), j0, phase, stream))
    torch.cuda.synchronize(gpu)
    assert _untouched(view, back)
    return np.tril(_np(view)), int(info.item())


def _by_factor(a: np.ndarray, layout: str, gpu):
    n = a.shape[0]
    view, back = _place_lower(a, layout, gpu)
    info = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    _native.check(_native.lib().mpx_chol_factor_f64(view.data_ptr(), n, view.stride(0), info.data_ptr(), stream))
    torch.cuda.synchronize(gpu)
    assert _untouched(view, back)
    return np.tril(_np(view)), int(info.item())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("family", ["spd", "wide"])
@pytest.mark.parametrize("n", [64, 65, 129, 200, 321])
def test_gpu_phases_give_the_factorisation(n, family, layout, gpu):
    a = _spd(n) if family == "spd" else _wide_family(n, WIDE_T)[0]
    want, winfo = _by_factor(a, layout, gpu)
    got, ginfo = _by_phases(a, layout, gpu)
    assert winfo == 0 and ginfo == 0
    assert np.array_equal(got, want)
    if family == "wide":
        assert np.array_equal(got, _wide_family(n, WIDE_T)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k", [100, 195])  # the second panel; the last, ragged block (192..199)
def test_gpu_phases_report_the_same_bad_column(k, layout, gpu):
    """The reduced pivot of column k is exactly -1 (as test_cholesky's _spoil
    makes it): both paths report k + 1, which the diagonal kernels of the later
    panels must leave alone, and agree in the columns before it."""
    n = 200
    a0, low, _, _ = _wide_family(n, WIDE_T)
    a = a0.copy()
    a[k, k] = a[k, k] - low[k, k] ** 2 - 1.0
    assert a[k, k] + 1.0 == a0[k, k] - low[k, k] ** 2  # exact: multiples of 2^-20 below 2^33
    want, winfo = _by_factor(a, layout, gpu)
    got, ginfo = _by_phases(a, layout, gpu)
    assert winfo == k + 1 and ginfo == k + 1
    assert np.array_equal(got[:, :k], want[:, :k])
    assert np.array_equal(got[:, :k], low[:, :k])


# ---------------------------------------------------------------- 2d. power-of-two scaling
def _exponents(n: int, kind: str) -> np.ndarray:
    if kind == "diag":
        return np.random.RandomState(50 + n).randint(-150, 151, size=n)
    return np.full(n, 400 if kind == "up" else -400)  # A 4^400 and A 4^-400


def _in_range(v: np.ndarray, lo: int, hi: int) -> bool:
    mag = np.abs(v[v != 0])
    return bool(np.all(np.isfinite(mag)) and mag.min() > 2.0 ** lo and mag.max() < 2.0 ** hi)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("kind", ["diag", "up", "down"])
@pytest.mark.parametrize("n", [33, 64, 129, 200])  # 33, 64: plain VALU root and division; 129, 200: the MFMA
def test_power_of_two_scaling(n, kind, dev):
    """With D = diag(2^e_i): chol(D A D) = D chol(A), and the right-hand side
    D B gives D^-1 X (the forward substitution's y is the unscaled one). Every
    operation of the scaled run is the unscaled one times a power of two, so the
    identity is exact while nothing leaves the normal range: asserted below from
    the unscaled results, every nonzero |l'| in (2^-500, 2^500) (hence every
    |l'_ik l'_jk| in (2^-1000, 2^1000)), every |a'|, |b'|, |x'| in
    (2^-1000, 2^1000)."""
    e = _exponents(n, kind)
    a = _spd(n)
    b = np.random.RandomState(60 + n).standard_normal((n, 17))
    l, low = _factor_on(a, "odd", dev)
    x = _solve(l, b, "odd", dev)

    a_s = np.tril(np.ldexp(a, e[:, None] + e[None, :]))
    low_s, b_s, x_s = np.ldexp(low, e[:, None]), np.ldexp(b, e[:, None]), np.ldexp(x, -e[:, None])
    assert _in_range(low_s, -500, 500)
    for v in (a_s, b_s, x_s):
        assert _in_range(v, -1000, 1000)
    assert _in_range(low.T @ x, -400, 400)  # y, the same in both runs, and its products with l'

    a_s = a_s + np.tril(a_s, -1).T
    l2, got = _factor_on(a_s, "odd", dev)
    assert np.array_equal(got, low_s)
    assert np.array_equal(_solve(l2, b_s, "odd", dev), x_s)


# ---------------------------------------------------------------- 2e. the columns of B are independent
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [64, 129, 200])
def test_rhs_columns_are_independent(n, dev):
    nrhs = 130
    l, _ = _factor_on(_spd(n), "even", dev)
    b = np.random.RandomState(70 + n).standard_normal((n, nrhs))
    x = _solve(l, b, "odd", dev)
    assert np.all(np.isfinite(x))
    # every MFMA tile, wave quarter and workgroup edge
    for j in (0, 15, 16, 31, 32, 63, 64, 65, 129):
        assert np.array_equal(_solve(l, b[:, j:j + 1], "odd", dev)[:, 0], x[:, j]), j
    spoilt = b.copy()
    spoilt[:, 64] = np.nan
    spoilt[:, 17] = np.inf
    y = _solve(l, spoilt, "odd", dev)
    clean = np.ones(nrhs, dtype=bool)
    clean[[17, 64]] = False
    assert np.array_equal(y[:, clean], x[:, clean])
    assert not np.isfinite(y[:, ~clean]).any()


# ---------------------------------------------------------------- 2f. alignment cross product
ALIGN = ["base16", "base8", "oddpitch"]


def _place_aligned(arr: np.ndarray, align: str, device, lower: bool):
    """``arr`` in a sentinel buffer: a 16-byte aligned base with an even pitch,
    the same buffer entered one element later (every row 8 bytes off a 16-byte
    boundary), or an odd pitch. Returns (view, check) with check() true while
    everything around the lower triangle / the matrix is as it was."""
    r, c = arr.shape
    off = 1 if align == "base8" else 0
    pitch = c + 1
    pitch += (pitch % 2 == 0) if align == "oddpitch" else (pitch % 2 == 1)
    vals = np.array(arr, dtype=np.float64)
    if lower:
        vals[np.triu_indices(r, 1)] = np.nan
    back = torch.full((r, pitch), SENT, dtype=torch.float64, device=device)
    view = back[:, off:off + c]
    view.copy_(torch.from_numpy(vals))
    assert view.stride(0) % 2 == (align == "oddpitch") and view.data_ptr() % 16 == 8 * off

    def check() -> bool:
        around = bool((back[:, :off] == SENT).all()) and bool((back[:, off + c:] == SENT).all())
        return around and (not lower or bool(np.isnan(_np(view)[np.triu_indices(r, 1)]).all()))

    return view, check


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("nrhs", [17, 64])
@pytest.mark.parametrize("n", [135, 200])  # 135: a ragged K of 7 in the backward update
def test_alignment_cross_product(n, nrhs, dev):
    a = _spd(n)
    b = np.random.RandomState(80 + n + nrhs).standard_normal((n, nrhs))
    first = None
    for la in ALIGN:
        view, lcheck = _place_aligned(a, la, dev, lower=True)
        l, info = ops.cholesky_factor_(view)
        assert int(info.item()) == 0 and lcheck()
        for ba in ALIGN:
            bview, bcheck = _place_aligned(b, ba, dev, lower=False)
            x = ops.cholesky_solve_(l, bview)
            assert bcheck() and lcheck()
            seen = (np.tril(_np(l)), _np(x))
            if first is None:
                first = seen  # base16 x base16
            assert np.array_equal(seen[0], first[0]), (la, ba)
            assert np.array_equal(seen[1], first[1]), (la, ba)


# ---------------------------------------------------------------- 2g. the rows below the matrix
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [65, 135, 200])  # ragged last tiles of 1, 7 and 8 rows
def test_rows_below_the_matrix_are_kept(n, layout, dev):
    """A and B are the leading rows of buffers two rows taller: a store
    predicate that lets row n of a ragged tile through writes there, where the
    other tests have nothing to look at. Same bits as in a buffer of their own."""
    nrhs = 17
    a = _spd(n)
    b = np.random.RandomState(85 + n).standard_normal((n, nrhs))
    vals = a.copy()
    vals[np.triu_indices(n, 1)] = np.nan
    tall = torch.full((n + 2, n + LAYOUTS[layout]), SENT, dtype=torch.float64, device=dev)
    view = tall[:n, :n]
    view.copy_(torch.from_numpy(vals))
    l, info = ops.cholesky_factor_(view)
    assert int(info.item()) == 0
    assert _untouched(view, tall) and bool((tall[n:] == SENT).all())

    btall = torch.full((n + 2, nrhs + LAYOUTS[layout]), SENT, dtype=torch.float64, device=dev)
    bview = btall[:n, :nrhs]
    bview.copy_(torch.from_numpy(b))
    x = _np(ops.cholesky_solve_(l, bview))
    assert _padding_kept(btall, nrhs) and bool((btall[n:] == SENT).all())
    assert _untouched(view, tall) and bool((tall[n:] == SENT).all())

    l2, low = _factor_on(a, layout, dev)
    assert np.array_equal(np.tril(_np(l)), low)
    assert np.array_equal(_solve(l2, b, layout, dev), x)


# ---------------------------------------------------------------- 3. the update's modes alone
def _update_ratio(got: np.ndarray, c: np.ndarray, a: np.ndarray, b: np.ndarray, roundings: int, where=None) -> float:
    """Asserts |got - (c - a b)| <= gamma_roundings (|c| + |a||b|) elementwise
    (where ``where`` is true) in long double; returns the largest ratio."""
    c, a, b = c.astype(LD), a.astype(LD), b.astype(LD)
    where = np.ones(c.shape, dtype=bool) if where is None else where
    assert np.all(np.isfinite(got[where]))
    res = np.abs(got.astype(LD) - (c - a @ b))[where]
    bound = (_gamma(roundings) * (np.abs(c) + np.abs(a) @ np.abs(b)))[where]
    ratio = float(np.max(res / np.where(bound > 0, bound, LD(1))))
    assert np.all(res <= bound), ratio
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n,j0", [(65, 0), (129, 0), (200, 0), (200, 64), (321, 128)])
def test_gpu_syrk_update_alone(n, j0, layout, gpu):
    """Phase 2 alone on standard-normal data: the trailing lower triangle is
    C - A21 A21^T to the bound (K = 64), every other bit of the buffer and the
    info word are as they were."""
    _ld_ok()
    buf = np.random.RandomState(90 + n + j0).standard_normal((n, n))
    view, back = _place_lower(buf, layout, gpu)
    before = _np(back)
    info = torch.full((1,), -5, dtype=torch.int32, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    _native.check(_native.lib().mpx_chol_phase_f64(view.data_ptr(), n, view.stride(0), info.data_ptr(), j0, 2, stream))
    torch.cuda.synchronize(gpu)
    after = _np(back)
    assert int(info.item()) == -5
    r0 = j0 + 64
    inside = np.zeros(before.shape, dtype=bool)
    inside[r0:n, r0:n] = np.tri(n - r0, dtype=bool)
    assert np.array_equal(after.view(np.int64)[~inside], before.view(np.int64)[~inside])  # bits, NaN included
    a21 = buf[r0:, j0:r0]
    ratio = _update_ratio(after[r0:n, r0:n], buf[r0:, r0:], a21, a21.T, 65, where=np.tri(n - r0, dtype=bool))
    assert _untouched(view, back)
    print(f"syrk n={n} j0={j0} {layout}: {ratio:.4f} of the bound")


def _unit_block_lower(n: int, seed: int, first_column_only: bool = False) -> np.ndarray:
    """The identity in the 64-wide diagonal blocks, standard normal below them
    (or below the first one only): the substitutions on the diagonal blocks are
    then exact (x - 0 y, x / 1), and a solve is a chain of updates."""
    low = np.tril(np.random.RandomState(seed).standard_normal((n, n)), -1)
    for k0 in range(0, n, 64):
        low[k0:k0 + 64, k0:k0 + 64] = 0.0
        if first_column_only and k0:
            low[k0:, k0:] = 0.0
    return low + np.eye(n)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("r", [1, 17, 40, 64])
def test_solve_updates_alone_two_blocks(r, layout, dev):
    """n = 64 + r: the forward update (NN, K = 64) gives rows 64.. = B1 - L10 B0,
    the backward one (TN, the ragged K = r) rows 0..63 = B0 - L10^T X1 with X1
    the returned rows 64.., so that both updates' inputs are known exactly."""
    _ld_ok()
    n = 64 + r
    low = _unit_block_lower(n, 100 + r)
    lview, lback = _place_lower(low, layout, dev)
    for nrhs in (1, 17, 65):
        b = np.random.RandomState(110 + r + nrhs).standard_normal((n, nrhs))
        x = _solve(lview, b, layout, dev)
        fwd = _update_ratio(x[64:], b[64:], low[64:, :64], b[:64], 64 + 1)
        bwd = _update_ratio(x[:64], b[:64], low[64:, :64].T, x[64:], r + 1)
        print(f"r={r} nrhs={nrhs} {layout} {dev}: NN {fwd:.4f}, TN {bwd:.4f} of the bound")
    assert _untouched(lview, lback)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_solve_updates_alone_four_blocks(layout, dev):
    """n = 200 (blocks of 64, 64, 64 and 8), two forms whose stages have inputs
    that the result itself holds exactly.
    Backward chain: B is zero above the last block, so y = B, X3 = B3, and block
    p is 0 - sum_{q > p} L_qp^T X_q from the returned later blocks: 3 - p TN
    updates over one, two and three row tiles, K = 8, 64, 64 in that order.
    Forward update over several row tiles: L is zero below its diagonal blocks
    except in columns 0..63, so rows 64.. are B1 - L10 B0 by one NN update of
    136 rows, which the backward updates leave alone (c - 0 x), and rows 0..63
    are B0 - L10^T X1 by three TN updates."""
    _ld_ok()
    n, nrhs = 200, 65
    low = _unit_block_lower(n, 120)
    lview, lback = _place_lower(low, layout, dev)
    b = np.zeros((n, nrhs))
    b[192:] = np.random.RandomState(121).standard_normal((8, nrhs))
    x = _solve(lview, b, layout, dev)
    assert np.array_equal(x[192:], b[192:])
    for p, k_sum, stages in ((2, 8, 1), (1, 8 + 64, 2), (0, 8 + 64 + 64, 3)):
        rows = slice(64 * p, 64 * p + 64)
        ratio = _update_ratio(x[rows], b[rows], low[64 * p + 64:, rows].T, x[64 * p + 64:], k_sum + stages)
        print(f"n=200 block {p} {layout} {dev}: TN chain of {stages}, {ratio:.4f} of the bound")
    assert _untouched(lview, lback)

    low = _unit_block_lower(n, 122, first_column_only=True)
    lview, lback = _place_lower(low, layout, dev)
    b = np.random.RandomState(123).standard_normal((n, nrhs))
    x = _solve(lview, b, layout, dev)
    fwd = _update_ratio(x[64:], b[64:], low[64:, :64], b[:64], 64 + 1)
    bwd = _update_ratio(x[:64], b[:64], low[64:, :64].T, x[64:], 8 + 64 + 64 + 3)
    print(f"n=200 first block column {layout} {dev}: NN over three row tiles {fwd:.4f}, TN chain {bwd:.4f} of the bound")
    assert _untouched(lview, lback)


