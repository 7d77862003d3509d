"""Householder QR, second round (the first is test_qr.py, whose conventions and
helpers are used here): exact families whose sums have many terms, the regime
m > 16384, the operand classes of the two staging kernels, ``qr_solve_r_``
alone. Every body runs on CPU tensors (the unblocked reference) and, marked
``gpu``, on GPU tensors (qr.hip, dense_tile.hpp); everything is ``array_equal``
unless a bound is named.

Operand classes. ``qr``: contiguous, pitch n + 2, pitch n + 3, and the columns
1 .. n of a buffer with an even pitch (every row 8 bytes off a 16-byte
boundary). B: contiguous, an even pitch, an odd pitch, 8 bytes off, a strided
1-D column of a wider buffer, every second row of a taller buffer. Between them
they reach the 16-byte and the 8-byte staging of ``qr_vtc_kernel`` and of
``dense_update_kernel`` with V aligned and C not, C aligned and V not, both and
neither. Every backing buffer is filled with a sentinel and is two rows taller
than the operand: the pitch padding, the rows below row m and the unused rows of
the every-second-row buffer must come back bit for bit.

A. Block reflectors from made-up ``qr`` and ``tau``. Below the diagonal two
   entries of {+-1, +-2} per column in random rows, column 7 of every panel
   dense +-1 (its row of W sums every row of every chunk); on and above the
   diagonal integers + 0.5, which the unit-lower mask must keep out; tau from
   {0, 1/2, 1, 2, -1}, 1/2 on the dense columns; B integers in [-4, 4]. The
   expected result applies H_j = I - tau_j v_j v_j^T one after the other in
   ``np.longdouble``. The test proves that this, and the blocked algorithm of
   qr.hip in any summation order, is exact: for every sum of the sequential
   application and of the blocked one recomputed on the host (V^T V, W, T by
   the forward recursion, Z, C - V Z) log2(the largest sum of the absolute
   values of the terms) + the fraction bits of the terms is at most 50, and
   the blocked result equals the sequential one. Bits needed, Q^T / Q, as
   ``test_exact_family_is_exact`` prints them:
     (5, 3)       5.0 /  5.0   trivial
     (65, 64)    22.7 / 21.6   one full panel, one row below it
     (130, 63)   19.3 / 18.4   a ragged panel, jb = 63
     (300, 193)  29.8 / 30.6   three panels, the last ragged
     (200, 200)  42.1 / 43.7   square: the last panel has no row below it
     (1124, 70)  16.2 / 15.3   two row chunks (``mpx_qr_plan``), a panel of 6
     (16385, 70) 16.2 / 16.2   17 chunks, the last of one row
   (the seed is one at which the condition holds: other draws at (200, 200)
   need up to 57 bits and are refused by the test, not tolerated)
   with 1, 3, 64, 65, 130 right-hand sides (one column; less than a tile; one
   tile; one column more; three tiles, the last ragged) and the 1-D form, a
   ``qr`` class and a B class rotating with the case, and the full cross
   product of the classes at (300, 193) with 17 and 64 columns. GPU only: the
   factorisation's own block step, ``mpx_qr_phase_f64`` phases 1 to 3 on a
   matrix whose panel holds such a ``qr``, at j0 = 0 and j0 = 64.

B. The first reflector of the factorisation, exact with many terms: columns
   0 .. c - 1 upper triangular (tau = 0), a_cc = 0 and +-1 in exactly 4^q rows
   below it, at least one in every 16 rows from row c on (every workgroup of
   the panel kernel and every pass of every wave owns one), small integers
   right of it. Then sigma = 4^q, beta = -2^q, tau_c = 1, v_i = +-2^-q, and row
   c of R is -g / 2^q with g the integer Gram row, in the panel through the
   fold of the workgroups' partials and right of it through W, T and Z. q is
   the largest with 4^q rows below row c, at most 7. c in 0, 5, 63, 64, 70
   (first column; mid panel; last of a panel; first of the second; mid second)
   at m = 200 and 4200 with n = 130; c in 0, 63, 64 at m = 16384 (the fold
   takes exactly 256 partials), 16385 and 32769 (128 and 192 rows per
   workgroup, waves of two and three passes) with n = 70.

C. The tall regime otherwise, at (16385, 70) and (32769, 5): test_qr.py's
   signed scaled permutations and its invariants (runs and layouts, phases,
   column nesting), and the bounds of its ``test_bounds_factor`` (backward
   error and orthogonality <= max(m n, 16) u, Q rebuilt in extended precision)
   at (16385, 70). Measured there in u, backward error / orthogonality,
   Gaussian (``test_tall_bounds_factor`` prints them):  GPU 4.14 / 4.56,  CPU
   reference 6.81 / 68.90 (it sums the 16384 products of a column one after
   the other; mu = 1146950 u).

D. ``qr_solve_r_`` alone: R upper triangular with diagonal +-2^k, k in -2 .. 2,
   and integers in [-2, 2] above it, NaN below the diagonal and in the rows
   below row n of the ``qr`` buffer (never to be read into the result); X
   integers in [-8, 8], B = R X. Every partial sum of the back substitution is
   a multiple of 1/4 of at most n * 2 * 8 * 4 (asserted), so any order is exact
   and X comes back. n in 1, 63, 64, 65 (one block and its edges), 129, 200
   (``dense_update_kernel<kRows>`` with M = 64 and 128 and a ragged K of 1 and
   8); 1, 3, 65, 130 columns and the 1-D form.

E. The operand classes give the same bits on Gaussian data: the
   factorisation, both applications and the solve with R, for every ``qr``
   class x B class at (300, 193) and (130, 63) with 17 and 64 columns, equal
   the result with both operands contiguous. The two staging kernels load the
   same values into the same LDS layout and nothing else depends on the class,
   so capi.h's "pitch alignment class" is pinned as equal bits across classes,
   the mixed cases (one operand aligned, the other not) included.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops

from .test_qr import (DEVICES, LAYOUTS, LD, SENT, _backward_ratio, _chunk_shape, _factor, _gauss, _householder, _ld_ok,
                      _np, _orth_ratio, _place, _plan, _q_ld, _signed_permutation, dev)  # noqa: F401 (dev: a fixture)

QR_CLASSES = ["contig", "p2", "p3", "base8"]
B_CLASSES = ["contig", "even", "odd", "base8", "col1d", "rows2"]
B_CLASSES_2D = [c for c in B_CLASSES if c != "col1d"]
GUARD = 2  # rows of the backing buffer below the operand
NB = 64
MAX_RHS = 130


# ---------------------------------------------------------------- operand classes
def _lay(shape, cls):
    """(shape of the backing buffer, the operand's place in it) for an (r,) or (r, c) operand."""
    r = shape[0]
    if len(shape) == 1:
        if cls == "contig":
            return (r + GUARD,), lambda x: x[:r]
        if cls == "rows2":
            return (2 * r + GUARD,), lambda x: x[:2 * r:2]
        width, k = {"even": (4, 0), "odd": (3, 0), "base8": (4, 1), "col1d": (5, 2)}[cls]
        return (r + GUARD, width), lambda x: x[:r, k]
    c = shape[1]
    if cls == "rows2":
        return (2 * r + GUARD, c), lambda x: x[:2 * r:2]
    even, odd = c + 1 + (c + 1) % 2, c + 1 + c % 2
    pitch, off = {"contig": (c, 0), "p2": (c + 2, 0), "p3": (c + 3, 0), "even": (even, 0), "odd": (odd, 0),
                  "base8": (even, 1)}[cls]
    return (r + GUARD, pitch), lambda x: x[:r, off:off + c]


def _put(arr: np.ndarray, cls: str, device):
    """``arr`` as an operand of class ``cls`` in a sentinel-filled buffer: (view,
    check), check() true while everything in the buffer outside the operand
    (padding, rows below, unused rows) is as it was."""
    arr = np.asarray(arr, dtype=np.float64)
    shape, place = _lay(arr.shape, cls)
    host = np.full(shape, SENT)
    place(host)[...] = arr
    outside = np.ones(shape, dtype=bool)
    place(outside)[...] = False
    assert outside.any() or cls == "contig"
    back = torch.from_numpy(host).to(device)
    view = place(back)
    assert view.shape == arr.shape and (arr.ndim == 1 or arr.shape[1] == 0 or view.stride(1) == 1)
    if arr.ndim == 2 and arr.shape[0] > 1:
        aligned = view.data_ptr() % 16 == 0 and view.stride(0) % 2 == 0
        if cls in ("even", "rows2"):
            assert aligned
        if cls in ("odd", "base8"):
            assert not aligned
        if cls == "base8":
            assert view.data_ptr() % 16 == 8 and view.stride(0) % 2 == 0

    def check() -> bool:
        return bool((_np(back)[outside] == SENT).all())

    return view, check


def _t(x: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.array(x, dtype=np.float64)).to(device)


# ---------------------------------------------------------------- what a sum needs to be exact
def _frac_bits(x, axis=None):
    """The number of fraction bits of the entries of ``x`` (0 for integers and
    for zero), their maximum along ``axis``."""
    x = np.asarray(x, dtype=np.float64)
    mant, exp = np.frexp(x)
    low = np.abs(mant * 2.0 ** 53).astype(np.int64)
    low = low & -low  # the lowest set bit of the 53-bit mantissa
    tz = np.log2(np.maximum(low, 1).astype(np.float64)).astype(np.int64)
    bits = np.where(x == 0.0, 0, np.maximum(53 - exp.astype(np.int64) - tz, 0))
    return bits.max(axis=axis, initial=0)


class _Bits:
    """The most bits any sum seen so far needs: log2 of the sum of the absolute
    values of its terms plus the terms' fraction bits. Up to 53 every partial
    sum in every order is a representable fp64 number; 50 is what is asked."""

    def __init__(self):
        self.worst, self.where = 0.0, ""

    def note(self, where: str, top: float, frac: int):
        need = (math.log2(top) if top > 0 else 0.0) + frac
        if need > self.worst:
            self.worst, self.where = need, where

    def product(self, where: str, a: np.ndarray, b: np.ndarray, plus=None) -> np.ndarray:
        """a @ b, noting what the sums over k (with ``plus`` as one more term) need."""
        top = np.abs(a) @ np.abs(b)
        frac = int((_frac_bits(a, axis=0) + _frac_bits(b, axis=1)).max(initial=0))
        if plus is not None:
            top = top + np.abs(plus)
            frac = max(frac, int(_frac_bits(plus)))
        self.note(where, float(top.max(initial=0.0)), frac)
        return a @ b


def _unit_lower(block: np.ndarray) -> np.ndarray:
    """A panel (rows x jb, its diagonal block on top) as V: unit lower."""
    v = np.tril(block, -1)
    v[np.arange(block.shape[1]), np.arange(block.shape[1])] = 1.0
    return v


def _block_step(v: np.ndarray, tau: np.ndarray, c: np.ndarray, transpose: bool, bits: _Bits) -> np.ndarray:
    """qr.hip's block reflector on the host: (I - V T^T V^T) C or (I - V T V^T) C."""
    jb = v.shape[1]
    g = bits.product("V^T V", v.T, v)
    w = bits.product("W", v.T, c)
    t = np.zeros((jb, jb))
    for j in range(jb):
        t[j, j] = tau[j]
        if j:
            s = bits.product("T", t[:j, :j], g[:j, j:j + 1])[:, 0]
            bits.note("T", float(abs(tau[j]) * np.abs(s).max()), int(_frac_bits(s)) + int(_frac_bits(tau[j])))
            t[:j, j] = -tau[j] * s
    z = bits.product("Z", t.T if transpose else t, w)
    return c - bits.product("C - V Z", v, z, plus=c)


def _blocked(qr: np.ndarray, tau: np.ndarray, b: np.ndarray, transpose: bool, bits: _Bits) -> np.ndarray:
    """``mpx_qr_apply_f64``'s algorithm in numpy fp64 (exact while ``bits`` stays within 53)."""
    n = qr.shape[1]
    c = np.array(b, dtype=np.float64)
    last = (n - 1) // NB * NB
    for q in range(0, last + 1, NB):
        j0 = q if transpose else last - q
        jb = min(NB, n - j0)
        c[j0:] = _block_step(_unit_lower(qr[j0:, j0:j0 + jb]), tau[j0:j0 + jb], c[j0:], transpose, bits)
    return c


def _sequential(qr: np.ndarray, tau: np.ndarray, b: np.ndarray, transpose: bool, bits: _Bits) -> np.ndarray:
    """H_j = I - tau_j v_j v_j^T one after the other in extended precision,
    ascending j for Q^T and descending for Q; only the nonzero rows of v_j are
    visited. The result as fp64, which it must fit."""
    n = qr.shape[1]
    x = np.array(b, dtype=LD)
    for j in (range(n) if transpose else range(n - 1, -1, -1)):
        if tau[j] == 0.0:
            continue
        idx = j + 1 + np.flatnonzero(qr[j + 1:, j])
        v = qr[idx, j]
        xi, xj = x[idx].astype(np.float64), x[j].astype(np.float64)
        fv, fx = int(_frac_bits(v)), max(int(_frac_bits(xi)), int(_frac_bits(xj)))
        tops = np.abs(xj) + np.abs(v) @ np.abs(xi)
        bits.note("v^T b", float(tops.max()), fv + fx)
        s = LD(tau[j]) * (x[j] + v.astype(LD) @ x[idx])
        fs = int(_frac_bits(s.astype(np.float64)))
        bits.note("tau s", float(abs(tau[j]) * tops.max()), fv + fx + int(_frac_bits(tau[j])))
        bits.note("b - v s", float((np.abs(xi) + np.outer(np.abs(v), np.abs(s.astype(np.float64)))).max(initial=0.0)),
                  max(fx, fv + fs))
        bits.note("b - v s", float((np.abs(xj) + np.abs(s.astype(np.float64))).max()), max(fx, fs))
        x[j] -= s
        x[idx] -= np.outer(v.astype(LD), s)
    out = x.astype(np.float64)
    assert np.array_equal(out.astype(LD), x)
    return out


# ---------------------------------------------------------------- A. exact block reflectors
A_SHAPES = [(5, 3), (65, 64), (130, 63), (300, 193), (200, 200), _chunk_shape(), (16385, 70)]
A_NRHS = [1, 3, 64, 65, 130, None]  # None: the 1-D form


@functools.lru_cache(maxsize=None)
def _family(m: int, n: int):
    # a seed at which the 50-bit condition holds: at (200, 200) the family needs 41 to 57 bits depending on the draw
    rng = np.random.RandomState(1001 + 3 * m + n)
    qr = np.zeros((m, n))
    upper = np.triu_indices(m, 0, n)
    qr[upper] = rng.randint(-9, 10, size=len(upper[0])) + 0.5
    for j in range(n):
        below = m - j - 1
        if below <= 0:
            continue
        if j % NB == 7:
            qr[j + 1:, j] = rng.choice([-1.0, 1.0], size=below)
        else:
            rows = j + 1 + rng.choice(below, size=min(2, below), replace=False)
            qr[rows, j] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=len(rows))
    tau = rng.choice([0.0, 0.5, 1.0, 2.0, -1.0], size=n)
    tau[7::NB] = 0.5
    qr.setflags(write=False)
    tau.setflags(write=False)
    return qr, tau


@functools.lru_cache(maxsize=None)
def _family_rhs(m: int) -> np.ndarray:
    b = np.random.RandomState(2000 + m).randint(-4, 5, size=(m, MAX_RHS)).astype(np.float64)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _family_expect(m: int, n: int, transpose: bool):
    """(Q^T B or Q B for the family's 130 columns, the bits its sums need): the
    sequential application, proved exact and equal to the blocked one."""
    qr, tau = _family(m, n)
    bits = _Bits()
    want = _sequential(qr, tau, _family_rhs(m), transpose, bits)
    assert np.array_equal(_blocked(qr, tau, _family_rhs(m), transpose, bits), want)
    assert bits.worst <= 50, (bits.worst, bits.where)
    want.setflags(write=False)
    return want, bits.worst


@pytest.mark.parametrize("transpose", [True, False])
@pytest.mark.parametrize("m,n", A_SHAPES)
def test_exact_family_is_exact(m, n, transpose):
    qr, tau = _family(m, n)
    assert set(np.unique(tau)) <= {0.0, 0.5, 1.0, 2.0, -1.0}
    assert not (np.triu(qr[:n]) == np.rint(np.triu(qr[:n])))[np.triu_indices(n)].any()  # the sentinels are no integers
    want, need = _family_expect(m, n, transpose)
    print(f"qr exact family ({m}, {n}) transpose={transpose}: {need:.1f} bits needed")
    assert need <= 50 and np.abs(want).max() > 4  # and something happened


def _rotation(si: int, ni: int, nrhs):
    qcls = QR_CLASSES[(si + ni) % len(QR_CLASSES)]
    pool = B_CLASSES if nrhs is None else B_CLASSES_2D
    return qcls, pool[(2 * si + ni) % len(pool)]


def _apply_and_check(qr, tau, cols, want, qcls, bcls, transpose, device):
    """``qr_mul_q_`` on operands of the given classes: the result, the guards, ``qr`` and ``tau`` as they were."""
    qv, qcheck = _put(qr, qcls, device)
    bv, bcheck = _put(cols, bcls, device)
    tv = _t(tau, device)
    out = ops.qr_mul_q_(qv, tv, bv, transpose=transpose)
    assert out.data_ptr() == bv.data_ptr() and out.shape == cols.shape
    assert np.array_equal(_np(bv), want), (qcls, bcls)
    assert qcheck() and bcheck(), (qcls, bcls)
    assert np.array_equal(_np(qv), qr) and np.array_equal(_np(tv), tau)
    return qv, tv


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("ni", range(len(A_NRHS)), ids=[str(k) for k in A_NRHS])
@pytest.mark.parametrize("transpose", [True, False])
@pytest.mark.parametrize("si", range(len(A_SHAPES)), ids=[f"{m}x{n}" for m, n in A_SHAPES])
def test_exact_block_reflectors(si, transpose, ni, dev):
    (m, n), nrhs = A_SHAPES[si], A_NRHS[ni]
    qr, tau = _family(m, n)
    want, _ = _family_expect(m, n, transpose)
    qcls, bcls = _rotation(si, ni + (0 if transpose else 1), nrhs)
    if bcls == "rows2" and 2 * m * (nrhs or 1) * 8 > 20e6:
        bcls = "odd"  # no buffer beyond the size of the tallest matrix
    cols, want = (_family_rhs(m)[:, 0], want[:, 0]) if nrhs is None else (_family_rhs(m)[:, :nrhs], want[:, :nrhs])
    qv, tv = _apply_and_check(qr, tau, cols, want, qcls, bcls, transpose, dev)
    assert np.array_equal(_np(ops.qr_mul_q(qv, tv, _t(cols, dev), transpose=transpose)), want)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("nrhs", [17, 64])
def test_exact_class_cross_product(nrhs, dev):
    m, n = 300, 193
    qr, tau = _family(m, n)
    for transpose in (True, False):
        b, want = _family_rhs(m), _family_expect(m, n, transpose)[0]
        for qcls in QR_CLASSES:
            for bcls in B_CLASSES:
                if bcls == "col1d":
                    _apply_and_check(qr, tau, b[:, nrhs - 1], want[:, nrhs - 1], qcls, bcls, transpose, dev)
                else:
                    _apply_and_check(qr, tau, b[:, :nrhs], want[:, :nrhs], qcls, bcls, transpose, dev)


def _phase(view, tau, info, j0, phase, ws, device):
    L = _native.lib()
    m, n = view.shape
    _native.check(L.mpx_qr_phase_f64(view.data_ptr(), m, n, view.stride(0), tau.data_ptr(), info.data_ptr(), j0, phase,
                                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream(device).cuda_stream))


@pytest.mark.gpu
@pytest.mark.parametrize("qcls", ["contig", "p3", "base8"])
@pytest.mark.parametrize("m,n,j0", [(300, 193, 0), (300, 193, 64), _chunk_shape() + (0,)])
def test_gpu_exact_block_step_of_the_factorisation(m, n, j0, qcls, gpu):
    """Phases 1 to 3 (W and V^T V; T and Z; the apply) with a made-up panel."""
    jb = min(NB, n - j0)
    rows, right = m - j0, n - j0 - jb
    assert right > 0
    rng = np.random.RandomState(m + n + j0)
    a = rng.randint(-9, 10, size=(m, n)) + 0.25  # above and left of the panel step: never read, never written
    pqr, ptau = _family(rows, jb)
    a[j0:, j0:j0 + jb] = pqr
    c = rng.randint(-4, 5, size=(rows, right)).astype(np.float64)
    a[j0:, j0 + jb:] = c
    bits = _Bits()
    want = _sequential(pqr, ptau, c, True, bits)
    assert np.array_equal(_block_step(_unit_lower(pqr), ptau, c, True, bits), want)
    assert bits.worst <= 50, (bits.worst, bits.where)
    tau_in = np.full(n, SENT)
    tau_in[j0:j0 + jb] = ptau
    view, check = _put(a, qcls, gpu)
    tau = _t(tau_in, gpu)
    info = torch.full((1,), -5, dtype=torch.int32, device=gpu)
    ws = torch.empty(int(_native.lib().mpx_qr_workspace_bytes(m, n, 0)), dtype=torch.uint8, device=gpu)
    for phase in (1, 2, 3):
        _phase(view, tau, info, j0, phase, ws, gpu)
    torch.cuda.synchronize(gpu)
    got = _np(view)
    assert np.array_equal(got[j0:, j0 + jb:], want)
    assert np.array_equal(got[:, :j0 + jb], a[:, :j0 + jb]) and np.array_equal(got[:j0], a[:j0])
    assert np.array_equal(_np(tau), tau_in) and int(info.item()) == -5 and check()


# ---------------------------------------------------------------- B. exact first reflector
def _power_of_four_rows(m: int, c: int) -> int:
    q = 0
    while q < 7 and 4 ** (q + 1) <= m - c - 1:
        q += 1
    return q


@functools.lru_cache(maxsize=None)
def _first_reflector(m: int, n: int, c: int):
    """(A, q, column c of the result, tau[:c + 1], row c of R right of c)."""
    rng = np.random.RandomState(7 * m + 3 * n + c)
    q = _power_of_four_rows(m, c)
    a = rng.randint(-3, 4, size=(m, n)).astype(np.float64)
    a[:, :c] = np.triu(a[:, :c])
    a[np.arange(c), np.arange(c)] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=c)
    groups = [(max(c + 1, lo), min(m, lo + 16)) for lo in range(c, m, 16)]
    groups = [g for g in groups if g[0] < g[1]]
    assert 4 ** q >= len(groups) and 4 ** q <= m - c - 1
    rows = np.array([rng.randint(lo, hi) for lo, hi in groups])  # one in every pass of 16 rows from row c on
    rest = np.setdiff1d(np.arange(c + 1, m), rows)
    rows = np.concatenate([rows, rng.choice(rest, size=4 ** q - len(rows), replace=False)])
    a[c:, c] = 0.0
    a[rows, c] = rng.choice([-1.0, 1.0], size=len(rows))
    assert np.count_nonzero(a[c + 1:, c]) == 4 ** q
    gram = a[c + 1:, c].astype(np.int64) @ a[c + 1:, c + 1:].astype(np.int64)
    assert np.abs(gram).max(initial=0) <= 3 * 4 ** q
    row = -gram.astype(np.float64) / 2.0 ** q
    hqr, htau, hinfo = _householder(a[:, :c + 1])
    assert hinfo == 0 and np.array_equal(htau, np.r_[np.zeros(c), 1.0]) and hqr[c, c] == -(2.0 ** q)
    assert set(np.unique(np.abs(hqr[c + 1:, c]))) == {0.0, 2.0 ** -q} or 4 ** q == m - c - 1
    a.setflags(write=False)
    return a, q, hqr[:, c], htau, row


B_CASES = ([(m, 130, c) for m in (200, 4200) for c in (0, 5, 63, 64, 70)]
           + [(m, 70, c) for m in (16384, 16385, 32769) for c in (0, 63, 64)])


def test_first_reflector_cases_reach_the_regimes():
    assert [_plan(m, 70)[0] for m in (200, 4200, 16384, 16385, 32769)] == [64, 64, 64, 128, 192]
    assert (16384 + 63) // 64 == 256 and (16385 + 127) // 128 == 129  # the partials the last workgroup folds at c = 0
    assert [_first_reflector(m, n, c)[1] for m, n, c in B_CASES] == [3] * 5 + [6] * 5 + [6, 6, 6, 7, 6, 6, 7, 7, 7]


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("m,n,c", B_CASES)
def test_exact_first_reflector(m, n, c, dev):
    a, q, col, etau, row = _first_reflector(m, n, c)
    layout = list(LAYOUTS)[(m + c) % 3]
    qr, tau, info = _factor(a, layout, dev)
    assert np.array_equal(tau[:c + 1], etau)
    assert np.array_equal(qr[:, c], col)
    assert np.array_equal(qr[c, c + 1:], row)
    assert np.array_equal(qr[:, :c], a[:, :c])
    assert info == 0 or info > c + 1


# ---------------------------------------------------------------- C. the tall regime
TALL = [(16385, 70), (32769, 5)]


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m,n", TALL)
def test_tall_signed_scaled_permutations(m, n, layout, dev):
    a, (eqr, etau, einfo) = _signed_permutation(m, n)
    assert einfo == 0 and set(np.unique(etau)) <= {0.0, 1.0}
    qr, tau, info = _factor(a, layout, dev)
    assert info == 0 and np.array_equal(tau, etau) and np.array_equal(qr, eqr)
    x = np.random.RandomState(m).randint(-8, 9, size=(n, 3)).astype(np.float64)
    b = a @ x
    assert np.array_equal(_np(ops.lstsq(_t(a, dev), _t(b, dev))), x)
    assert np.array_equal(_np(ops.lstsq(_t(a, dev), _t(b[:, 1], dev))), x[:, 1])


@functools.lru_cache(maxsize=None)
def _tall_factored(m: int, n: int, devname: str):
    out = _factor(_gauss(m, n), "contig", torch.device(devname))
    for x in out[:2]:
        x.setflags(write=False)
    return out


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("m,n", TALL)
def test_tall_runs_and_layouts_give_the_same_bits(m, n, dev):
    first = _tall_factored(m, n, str(dev))
    for layout in ("contig", "even", "odd"):
        again = _factor(_gauss(m, n), layout, dev)
        assert again[2] == first[2] == 0
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]), layout


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_tall_column_nesting(dev):
    m, n = 16385, 70
    qr, tau, _ = _tall_factored(m, n, str(dev))
    for k in (1, 63, 64, 65):
        kqr, ktau, _ = _factor(_gauss(m, n)[:, :k], "odd", dev)
        assert np.array_equal(kqr, qr[:, :k]) and np.array_equal(ktau, tau[:k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m,n", TALL)
def test_gpu_tall_phases_give_the_factorisation(m, n, layout, gpu):
    qr, tau, info = _tall_factored(m, n, str(gpu))
    view, back = _place(_gauss(m, n), layout, gpu)
    ptau = torch.full((n,), SENT, dtype=torch.float64, device=gpu)
    pinfo = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    ws = torch.empty(int(_native.lib().mpx_qr_workspace_bytes(m, n, 0)), dtype=torch.uint8, device=gpu)
    for j0 in range(0, n, _plan(m, n)[3]):
        for phase in range(4):
            _phase(view, ptau, pinfo, j0, phase, ws, gpu)
    torch.cuda.synchronize(gpu)
    assert int(pinfo.item()) == info and np.array_equal(_np(ptau), tau) and np.array_equal(_np(view), qr)
    assert bool((back[:, n:] == SENT).all())


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_tall_bounds_factor(dev):
    """``test_bounds_factor`` of test_qr.py at (16385, 70): the same bounds, no new tolerance."""
    _ld_ok()
    m, n = 16385, 70
    a = _gauss(m, n)
    qr, tau, info = _tall_factored(m, n, str(dev))
    assert info == 0 and np.isfinite(qr).all() and np.isfinite(tau).all()
    q = _q_ld(qr, tau)
    back, orth = _backward_ratio(a, q, np.triu(qr[:n]).astype(LD)), _orth_ratio(q)
    print(f"qr bounds {dev.type} ({m}, {n}): backward {back:.2f} u, orthogonality {orth:.2f} u, mu = {m * n} u")
    assert back <= max(m * n, 16) and orth <= max(m * n, 16)


# ---------------------------------------------------------------- D. the solve with R alone
D_SIZES = [1, 63, 64, 65, 129, 200]
D_NRHS = [1, 3, 65, 130, None]


@functools.lru_cache(maxsize=None)
def _triangular(n: int):
    """(the qr buffer's contents, X, B = R X): R in the top n rows, NaN wherever the solve must not look."""
    rng = np.random.RandomState(300 + n)
    r = np.triu(rng.randint(-2, 3, size=(n, n)), 1).astype(np.float64)
    r[np.arange(n), np.arange(n)] = rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.randint(-2, 3, size=n)
    x = rng.randint(-8, 9, size=(n, MAX_RHS)).astype(np.float64)
    bound = n * 2 * 8 * 4
    assert (np.abs(r) @ np.abs(x)).max() <= bound and _frac_bits(r) <= 2 and math.log2(bound) + 2 <= 50
    b = r @ x  # exact: see the bound
    assert _frac_bits(b) <= 2 and np.abs(b).max() <= bound
    qr = np.full((n + 3, n), np.nan)
    qr[:n][np.triu_indices(n)] = r[np.triu_indices(n)]
    for arr in (qr, x, b):
        arr.setflags(write=False)
    return qr, x, b


def _solve_and_check(n, cols, want, qcls, bcls, device):
    qr = _triangular(n)[0]
    qv, qcheck = _put(qr, qcls, device)
    bv, bcheck = _put(cols, bcls, device)
    out = ops.qr_solve_r_(qv, bv)
    assert out.data_ptr() == bv.data_ptr() and out.shape == cols.shape
    assert np.array_equal(_np(bv), want, equal_nan=True), (qcls, bcls)
    assert qcheck() and bcheck(), (qcls, bcls)
    assert np.array_equal(_np(qv), qr, equal_nan=True)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("ni", range(len(D_NRHS)), ids=[str(k) for k in D_NRHS])
@pytest.mark.parametrize("si", range(len(D_SIZES)), ids=[str(n) for n in D_SIZES])
def test_exact_solve_with_r(si, ni, dev):
    n, nrhs = D_SIZES[si], D_NRHS[ni]
    _, x, b = _triangular(n)
    qcls, bcls = _rotation(si, ni, nrhs)
    if nrhs is None:
        _solve_and_check(n, b[:, 0], x[:, 0], qcls, bcls, dev)
    else:
        _solve_and_check(n, b[:, :nrhs], x[:, :nrhs], qcls, bcls, dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("nrhs", [3, 65])
def test_exact_solve_with_r_class_cross_product(nrhs, dev):
    n = 200
    _, x, b = _triangular(n)
    for qcls in QR_CLASSES:
        for bcls in B_CLASSES:
            if bcls == "col1d":
                _solve_and_check(n, b[:, nrhs - 1], x[:, nrhs - 1], qcls, bcls, dev)
            else:
                _solve_and_check(n, b[:, :nrhs], x[:, :nrhs], qcls, bcls, dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("n,nrhs,j", [(65, 3, 1), (129, 65, 64), (200, 130, 63), (200, 130, 129)])
def test_solve_with_r_keeps_a_nan_in_its_column(n, nrhs, j, dev):
    qr, x, b = _triangular(n)
    cols = np.array(b[:, :nrhs])
    i = n // 2
    cols[i, j] = np.nan
    view, check = _put(cols, "odd", dev)
    ops.qr_solve_r_(_put(qr, "p2", dev)[0], view)
    got = _np(view)
    keep = np.arange(nrhs) != j
    assert check() and np.array_equal(got[:, keep], x[:, :nrhs][:, keep])
    # in column j: the rows below row i are solved before it; row i and every row above it that R couples to it are NaN
    assert np.array_equal(got[i + 1:, j], x[i + 1:, j]) and np.isnan(got[i, j])
    assert np.isnan(got[:i, j][qr[:i, i] != 0.0]).all()


# ---------------------------------------------------------------- E. operand classes on random data
@functools.lru_cache(maxsize=None)
def _class_baseline(m: int, n: int, nrhs: int, devname: str):
    """Factorisation, Q^T B, Q B and R^-1 B[:n] with both operands contiguous."""
    return _class_results(m, n, nrhs, "contig", "contig", torch.device(devname))


def _class_results(m, n, nrhs, qcls, bcls, device):
    b = np.random.RandomState(m + n + nrhs).standard_normal((m, nrhs))
    if bcls == "col1d":
        b = b[:, nrhs - 1]
    qv, qcheck = _put(_gauss(m, n), qcls, device)
    out, tau, info = ops.qr_factor_(qv)
    assert out.data_ptr() == qv.data_ptr() and int(info.item()) == 0 and qcheck()
    res = [_np(qv), _np(tau)]
    for transpose in (True, False):
        bv, bcheck = _put(b, bcls, device)
        ops.qr_mul_q_(qv, tau, bv, transpose=transpose)
        assert bcheck() and qcheck()
        res.append(_np(bv))
    bv, bcheck = _put(b[:n], bcls, device)
    ops.qr_solve_r_(qv, bv)
    assert bcheck() and qcheck() and np.array_equal(_np(qv), res[0])
    res.append(_np(bv))
    return res


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("nrhs", [17, 64])
@pytest.mark.parametrize("m,n", [(300, 193), (130, 63)])
def test_operand_classes_give_the_same_bits(m, n, nrhs, dev):
    base = _class_baseline(m, n, nrhs, str(dev))
    assert all(np.isfinite(x).all() for x in base)
    for qcls in QR_CLASSES:
        for bcls in B_CLASSES:
            got = _class_results(m, n, nrhs, qcls, bcls, dev)
            for k, (g, w) in enumerate(zip(got, base)):
                if bcls == "col1d" and k >= 2:
                    w = w[:, nrhs - 1]
                assert np.array_equal(g, w), (qcls, bcls, k)
