"""The pivoting contract of the dense LU (capi.h, ``mpx_lu_factor_f64``): the
lowest row among equal magnitudes at any column, zero pivots inside the counted
panel launches, pivot folds of more than 256 partials, NaN that stays where it
is, identical bits across layouts and runs, the narrower panels of
``MPX_LU_NB`` and the phase entry of the tuning harness.

Every expected value is known before the code under test runs, and nothing
here has a tolerance: the matrices are built from chosen factors *and a chosen
interchange sequence* whose entries are small dyadic rationals, so every
quantity of the elimination is exact in fp64 in any order of summation, fused
or not. ``tests/test_lu.py`` keeps the arithmetic yardsticks (Higham bounds);
this file pins which row wins.

Pitched buffers are filled with NaN: a load that strays into the padding and
meets a zero-filled operand gives NaN, not ``finite * 0 = 0``.
"""

from __future__ import annotations

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops

from .test_lu import DEVICES, LAYOUTS, _factor_bound, _ld_ok, _normal, _np
from .test_lu import dev  # noqa: F401  (the CPU / GPU fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPX_ERR_ARG = 1


# ---------------------------------------------------------------- 0. helpers
def _place_nan(arr: np.ndarray, layout: str, device):
    """``arr`` as the leading columns of a NaN-filled pitched buffer."""
    r, c = arr.shape
    back = torch.full((r, c + LAYOUTS[layout]), float("nan"), dtype=torch.float64, device=device)
    view = back[:, :c]
    view.copy_(torch.from_numpy(np.array(arr, dtype=np.float64)))
    return view, back


def _padding_kept(back: torch.Tensor, c: int) -> bool:
    return bool(torch.isnan(back[:, c:]).all())


def _draw_factors(n: int, seed: int):
    """L and U as ``test_lu._exact_family`` draws them, and the generator."""
    rng = np.random.RandomState(1000 * seed + n)
    low = np.tril(rng.choice([0.0, 0.25, -0.25, 0.5, -0.5], size=(n, n)), -1) + np.eye(n)
    up = np.triu(rng.randint(-8, 9, size=(n, n)).astype(np.float64), 1)
    up += np.diag(rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.randint(0, 4, size=n))
    return low, up, rng


def _draw_piv(rng, n: int, top: int) -> np.ndarray:
    """Random interchanges: piv[k] in [k, top) where that is not empty, else k."""
    ks = np.arange(n)
    return (ks + np.floor(rng.random_sample(n) * np.maximum(top - ks, 1)).astype(np.int64)).astype(np.int64)


def _order_after(piv, n: int, steps: int) -> np.ndarray:
    """order[i] = the original row that sits at position i after the first ``steps`` interchanges."""
    order = np.arange(n)
    for k in range(steps):
        p = int(piv[k])
        order[k], order[p] = order[p], order[k]
    return order


def _assemble(low: np.ndarray, up: np.ndarray, piv: np.ndarray) -> np.ndarray:
    """A with ``interchanges(A) = L U``: the interchanges applied to L U in reverse order."""
    n = low.shape[0]
    a = np.empty((n, n))
    a[_order_after(piv, n, n)] = low @ up
    return a


def _freeze(*arrays):
    for m in arrays:
        m.setflags(write=False)
    return arrays


def _pivseq(n: int, seed: int = 0, forced=()):
    """(A, L, U, piv): the pivot-sequence family. At step k the pivot row holds
    u_kk (|u_kk| >= 1) and every other candidate l_ik u_kk with |l_ik| <= 1/2,
    so partial pivoting has one answer, ``piv[k]``; ``forced`` is (k, p) pairs."""
    low, up, rng = _draw_factors(n, seed)
    piv = _draw_piv(rng, n, n)
    for k, p in forced:
        assert k <= p < n
        piv[k] = p
    return _freeze(_assemble(low, up, piv), low, up, piv)


_pivseq_cached = functools.lru_cache(maxsize=None)(_pivseq)


def _tie(n: int, t: int, pq: int, ps: int, sign: int, seed: int = 0):
    """(A, L, U, piv): the tie family. The row that ends at position n - 1 is
    exactly ``sign`` times the pivot row of step t; just before step t's
    interchange the pivot row sits at position pq and its copy at ps > pq. Both
    carry the same magnitude in every column up to t (negation is exact), lose
    every earlier search (at most half the pivot), tie at column t, where pq
    must win, and the copy becomes an exact zero row parked at n - 1."""
    assert 0 <= t <= pq < ps <= n - 1 and sign in (1, -1)
    low, up, rng = _draw_factors(n, seed)
    low[n - 1, :] = 0.0
    low[n - 1, :t] = sign * low[t, :t]
    low[n - 1, t] = sign
    low[n - 1, n - 1] = 1.0
    up[n - 1, n - 1] = 0.0
    piv = _draw_piv(rng, n, n - 1)  # no step but ps (and n - 1 itself) touches n - 1
    ks = np.arange(n)
    hit = (ks >= t) & (ks < ps) & (piv == ps)  # the copy stays at ps from step t until step ps
    piv[hit] = ks[hit]
    piv[t] = pq
    piv[ps] = n - 1
    assert piv[n - 1] == n - 1
    return _freeze(_assemble(low, up, piv), low, up, piv)


_tie_cached = functools.lru_cache(maxsize=None)(_tie)


@functools.lru_cache(maxsize=None)
def _cancel(n: int, zero_rows: tuple, seed: int = 0):
    """(A, L_expected, U, piv): row k of U zero for every k of ``zero_rows`` and
    piv[k] = k, so that at step k the remaining column is exactly zero although
    no column of A is. The column is left as it is: L[k+1:, k] == 0."""
    low, up, rng = _draw_factors(n, seed)
    piv = _draw_piv(rng, n, n)
    for k in zero_rows:
        up[k, :] = 0.0
        piv[k] = k
    a = _assemble(low, up, piv)
    assert np.all(np.abs(a[:, 1:]).sum(axis=0) > 0)  # no zero column on input (column 0 has nothing above it)
    for k in zero_rows:
        low[k + 1:, k] = 0.0
    return _freeze(a, low, up, piv)


def _assert_factors(out, piv, info, low, up, piv_want, info_want, nan_last=False):
    """Packed factors, interchanges and info against the constructed ones, on
    ``out``'s device; ``nan_last``: the last column must be all NaN instead."""
    assert piv.dtype == torch.int32 and info.dtype == torch.int32
    n = low.shape[0]
    pw = torch.from_numpy(np.asarray(piv_want, dtype=np.int32)).to(piv.device)
    if not torch.equal(piv, pw):
        bad = torch.nonzero(piv != pw).flatten()
        k = int(bad[0])
        raise AssertionError(f"piv[{k}] = {int(piv[k])}, expected {int(pw[k])} ({bad.numel()} of {n} differ)")
    want = torch.from_numpy(np.tril(low, -1) + up).to(out.device)
    cols = n - 1 if nan_last else n
    if not torch.equal(out[:, :cols], want[:, :cols]):
        bad = torch.nonzero(out[:, :cols] != want[:, :cols])
        i, j = bad[0].tolist()
        raise AssertionError(f"{'L' if i > j else 'U'}[{i}, {j}] = {float(out[i, j])!r}, "
                             f"expected {float(want[i, j])!r} ({len(bad)} entries differ)")
    if nan_last:
        assert bool(torch.isnan(out[:, n - 1]).all()), "U[:, n-1] is not all NaN"
    assert int(info.item()) == info_want


def _check_tie(n, t, pq, ps, sign, layout, device, fam=None):
    a, low, up, piv = fam if fam is not None else _tie_cached(n, t, pq, ps, sign)
    # the construction, checked on the input: before step t's interchange the
    # pivot row is at pq and its exact copy (times sign) at ps
    cur = a[_order_after(piv, n, t)]
    assert np.array_equal(cur[ps], sign * cur[pq]) and np.any(cur[pq] != 0)
    view, back = _place_nan(a, layout, device)
    out, got_piv, info = ops.lu_factor_(view)
    assert out.data_ptr() == view.data_ptr()
    _assert_factors(out, got_piv, info, low, up, piv, n)
    assert int(got_piv[t]) == pq and float(out[n - 1, n - 1]) == 0.0
    assert _padding_kept(back, n)


# ---------------------------------------------------------------- 1. ties at any column
TIE_CASES = [
    pytest.param(2, 0, 0, 1, id="n2-smallest"),
    pytest.param(17, 5, 5, 16, id="n17-one-workgroup"),
    pytest.param(300, 0, 3, 9, id="n300-col0-same-16-row-group"),
    pytest.param(300, 0, 3, 40, id="n300-col0-two-waves-of-a-workgroup"),
    pytest.param(300, 0, 3, 290, id="n300-col0-first-and-last-workgroup"),
    pytest.param(300, 17, 20, 25, id="n300-midpanel-same-16-row-group"),
    pytest.param(300, 17, 30, 60, id="n300-midpanel-two-waves"),
    pytest.param(300, 17, 17, 299, id="n300-midpanel-pivot-in-place-vs-last-row"),
    pytest.param(300, 63, 70, 200, id="n300-last-panel-column-launch-62"),
    pytest.param(300, 64, 64, 65, id="n300-tail-first-column-neighbours"),
    pytest.param(300, 64, 100, 299, id="n300-tail-first-column-two-fold-waves"),
    pytest.param(300, 298, 298, 299, id="n300-last-search"),
    pytest.param(400, 130, 131, 390, id="n400-third-panel"),
    pytest.param(400, 191, 200, 399, id="n400-third-panel-last-column"),
    pytest.param(400, 192, 193, 399, id="n400-tail-first-column-c0-192"),
]
TIE_CASES_FOLD = [  # more than 64 partials: the fold crosses waves through s_v
    pytest.param(1100, 0, 5, 1030, id="n1100-col0-fold-across-waves"),
    pytest.param(1100, 3, 1000, 1099, id="n1100-col3-fold-across-waves-last-row"),
]


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("sign", [1, -1], ids=["same-sign", "negated"])
@pytest.mark.parametrize("n,t,pq,ps", TIE_CASES)
def test_tie_at_any_column_takes_the_lowest_row(n, t, pq, ps, sign, layout, dev):
    _check_tie(n, t, pq, ps, sign, layout, dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("sign", [1, -1], ids=["same-sign", "negated"])
@pytest.mark.parametrize("n,t,pq,ps", TIE_CASES_FOLD)
def test_tie_folded_across_waves(n, t, pq, ps, sign, dev):
    _check_tie(n, t, pq, ps, sign, "contig", dev)


# ---------------------------------------------------------------- 2. zero pivots in the panel launches
CANCEL_CASES = [(70, (0,)), (70, (33,)), (300, (31,)), (300, (63,)), (300, (64,)), (300, (299,)), (400, (100,)),
                (400, (191,)), (300, (20, 150))]


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n,zero_rows", CANCEL_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else f"n{v}")
def test_zero_pivot_by_exact_cancellation(n, zero_rows, layout, dev):
    """The zero pivot arises during elimination; the first one is reported, its
    column stays as it is (zeros below the diagonal) and later columns go on."""
    a, low, up, piv = _cancel(n, zero_rows)
    view, back = _place_nan(a, layout, dev)
    out, got_piv, info = ops.lu_factor_(view)
    _assert_factors(out, got_piv, info, low, up, piv, zero_rows[0] + 1)
    for k in zero_rows:
        assert int(got_piv[k]) == k and bool((out[k, k:] == 0).all()) and bool((out[k + 1:, k] == 0).all())
    assert _padding_kept(back, n)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n,k", [(300, 0), (300, 31), (300, 63), (300, 64), (400, 100), (400, 191)])
def test_zero_input_column_on_the_panel_path(n, k, layout, dev):
    """``test_lu.test_zero_column``'s check at sizes the counted panel launches factor."""
    _ld_ok()
    a = np.random.RandomState(20 + k).standard_normal((n, n))
    a[:, k] = 0.0
    view, back = _place_nan(a, layout, dev)
    lu, piv, info = ops.lu_factor_(view)
    assert int(info.item()) == k + 1
    assert int(piv[k]) == k
    assert float(lu[k, k]) == 0.0
    _factor_bound(a, _np(lu), _np(piv))
    assert _padding_kept(back, n)


# ---------------------------------------------------------------- 3. more than 256 partials
N_WIDE = 4100  # 65 workgroups search columns 0..3: 260 partials, a second trip of the fold loop


@pytest.mark.gpu
def test_gpu_fold_second_trip_finds_the_pivot(gpu):
    """Pivots forced into rows 4097..4099 at columns 0..3. With partial index
    (row - column) // 16 the winners are partials 256, 256, 255 and 256: found
    on the second trip of threads 0 and 1, and by the last thread of the first."""
    forced = ((0, 4098), (1, 4099), (2, 4097), (3, 4099))
    a, low, up, piv = _pivseq(N_WIDE, 0, forced)
    assert [(p - k) // 16 for k, p in forced] == [256, 256, 255, 256]
    view, _ = _place_nan(a, "contig", gpu)
    out, got_piv, info = ops.lu_factor_(view)
    _assert_factors(out, got_piv, info, low, up, piv, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1, -1], ids=["same-sign", "negated"])
def test_gpu_fold_tie_between_trips(gpu, sign):
    """Rows 5 and 4097 tie at column 0: partials 0 and 256, folded by one thread
    on successive trips; the earlier one must survive the second trip."""
    fam = _tie(N_WIDE, 0, 5, 4097, sign)
    assert (5 - 0) // 16 == 0 and (4097 - 0) // 16 == 256
    _check_tie(N_WIDE, 0, 5, 4097, sign, "contig", gpu, fam=fam)


# ---------------------------------------------------------------- 4. NaN containment
NAN_N = [65, 127, 300]


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", NAN_N)
def test_nan_column_stays_in_its_column(n, layout, dev):
    """NaN in the last column of A: no other column depends on it and its only
    pivot search (k = n - 1) has a single candidate."""
    a, low, up, piv = _pivseq_cached(n)
    a = a.copy()
    a[:, n - 1] = np.nan
    assert piv[n - 1] == n - 1
    view, back = _place_nan(a, layout, dev)
    out, got_piv, info = ops.lu_factor_(view)
    _assert_factors(out, got_piv, info, low, up, piv, 0, nan_last=True)
    assert _padding_kept(back, n)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", NAN_N)
def test_exact_factor_and_solve_with_nan_padding(n, layout, dev):
    a, low, up, piv = _pivseq_cached(n)
    view, back = _place_nan(a, layout, dev)
    out, got_piv, info = ops.lu_factor_(view)
    _assert_factors(out, got_piv, info, low, up, piv, 0)
    assert _padding_kept(back, n)
    rng = np.random.RandomState(n)
    for nrhs in (1, 17, 65):
        x = rng.randint(-4, 5, size=(n, nrhs)).astype(np.float64)
        bview, bback = _place_nan(a @ x, layout, dev)
        got = ops.lu_solve_(out, got_piv, bview)
        assert got.data_ptr() == bview.data_ptr()
        assert np.array_equal(_np(got), x), (n, nrhs)
        assert _padding_kept(bback, nrhs)
    assert _padding_kept(back, n)


# ---------------------------------------------------------------- 5. same bits
@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 1100])
def test_gpu_same_bits_across_runs_and_layouts(gpu, n):
    """The layouts differ only in how the update's operands are loaded (16 or 8
    bytes at a time), and nothing depends on which workgroup finishes last: two
    runs and the three layouts give identical factors, pivots and solutions."""
    a = _normal(n)
    b = np.random.RandomState(n).standard_normal((n, 17))
    results = []
    for layout in ("contig", "contig", "even", "odd"):
        view, back = _place_nan(a, layout, gpu)
        lu, piv, info = ops.lu_factor_(view)
        assert int(info.item()) == 0
        bview, bback = _place_nan(b, layout, gpu)
        x = ops.lu_solve_(lu, piv, bview)
        assert _padding_kept(back, n) and _padding_kept(bback, 17)
        results.append((layout, lu, piv, x))
    _, lu0, piv0, x0 = results[0]
    assert bool(torch.isfinite(lu0).all()) and bool(torch.isfinite(x0).all())
    for i, (layout, lu, piv, x) in enumerate(results[1:], 1):
        assert torch.equal(piv, piv0), f"run {i} ({layout}): {int((piv != piv0).sum())} pivots differ"
        assert torch.equal(lu, lu0), f"run {i} ({layout}): {int((lu != lu0).sum())} entries of LU differ"
        assert torch.equal(x, x0), f"run {i} ({layout}): {int((x != x0).sum())} entries of X differ"


# ---------------------------------------------------------------- 6. panel widths 16 and 32
def _width_child(width: int) -> None:
    """Runs in a fresh process with MPX_LU_NB=width (read once per process);
    any mismatch raises, so the process exits non-zero."""
    gpu = torch.device("cuda:0")
    got = _native.lib().mpx_lu_panel_width()
    assert got == width, f"panel width {got}, asked for {width}"
    for n in (300, 321):
        a, low, up, piv = _pivseq(n)
        for layout in LAYOUTS:
            view, back = _place_nan(a, layout, gpu)
            out, got_piv, info = ops.lu_factor_(view)
            _assert_factors(out, got_piv, info, low, up, piv, 0)
            assert _padding_kept(back, n)
            x = np.random.RandomState(n).randint(-4, 5, size=(n, 17)).astype(np.float64)
            bview, bback = _place_nan(a @ x, layout, gpu)
            assert np.array_equal(_np(ops.lu_solve_(out, got_piv, bview)), x), (n, layout)
            assert _padding_kept(bback, 17)
    for layout in LAYOUTS:
        _check_tie(300, 17, 30, 60, -1, layout, gpu)
        a, low, up, piv = _cancel(300, (31,))
        view, back = _place_nan(a, layout, gpu)
        out, got_piv, info = ops.lu_factor_(view)
        _assert_factors(out, got_piv, info, low, up, piv, 32)
        assert _padding_kept(back, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [16, 32])
def test_gpu_narrow_panels(gpu, width):
    code = f"from tests.test_lu_pivoting import _width_child; _width_child({width})"
    env = dict(os.environ, MPX_LU_NB=str(width), PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, timeout=120, capture_output=True, text=True)
    assert res.returncode == 0, f"MPX_LU_NB={width}: exit {res.returncode}\n{res.stderr[-4000:]}"


# ---------------------------------------------------------------- 7. the phase entry
@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gpu_phase_entry_does_the_work_of_the_factorisation(gpu, layout):
    """Three panel steps through ``mpx_lu_phase_f64`` leave the first 192 rows
    and columns factored and the Schur complement below, all exact."""
    L = _native.lib()
    assert L.mpx_lu_panel_width() == 64
    n, done = 400, 192
    a, low, up, piv = _pivseq_cached(n)
    view, back = _place_nan(a, layout, gpu)
    pitch = view.stride(0)
    got_piv = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    info = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    nbytes = int(L.mpx_lu_workspace_bytes(n))
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def phase(j0, ph):
        return L.mpx_lu_phase_f64(view.data_ptr(), n, pitch, got_piv.data_ptr(), info.data_ptr(), j0, ph,
                                  ws.data_ptr(), nbytes, stream)

    for j0 in (0, 64, 128):
        for ph in (0, 1, 2, 3):
            _native.check(phase(j0, ph))
    torch.cuda.synchronize(gpu)
    # position i >= 192 holds the row that the remaining interchanges take to position final[i]
    where = np.argsort(_order_after(piv, n, n))
    final = where[_order_after(piv, n, done)[done:]]
    want = np.tril(low, -1) + up
    want[done:, :done] = low[final, :done]
    want[done:, done:] = low[final, done:] @ up[done:, done:]
    assert int(info.item()) == 0
    assert np.array_equal(_np(got_piv[:done]), piv[:done])
    got = _np(view)
    assert np.array_equal(got[:done], want[:done])
    assert np.array_equal(got[done:, :done], want[done:, :done])
    assert np.array_equal(got[done:, done:], want[done:, done:])
    assert _padding_kept(back, n)
    keep = back.clone()
    for j0, ph in ((1, 0), (192, 0), (0, 4)):  # not a panel column; 208 rows left is not more than 256; no such phase
        assert phase(j0, ph) == MPX_ERR_ARG, (j0, ph)
    torch.cuda.synchronize(gpu)
    assert torch.equal(torch.nan_to_num(back, nan=-1.5), torch.nan_to_num(keep, nan=-1.5))
