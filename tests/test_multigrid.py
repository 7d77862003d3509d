"""Geometric multigrid for the 2-D Poisson solver: the damped Jacobi sweep, the
residual, full-weighting restriction and bilinear prolongation, from the
kernels to ``models.PoissonMultigrid``.

Every operator has one rounding order, so GPU fp32, GPU fp64, the CPU library
and the dtype-preserving torch expressions of ``ops.reference`` agree bit for
bit; no kernel comparison here carries a tolerance. Sentinels follow
test_jacobi_accel.py: inputs carry NaN in every element the contract says is
never read (pitch padding, b's boundary, r's boundary for the restriction),
outputs are pre-filled with NaN and must keep those bits wherever the contract
says "not written" (compared on the whole backing buffer, padding included).

Layouts: "contig" (row pitch = width: odd widths take the per-element
kernels), "vec" (pitch rounded up to 16 bytes: the vector kernels) and "shift"
(that pitch with the base moved by one element: unaligned, per-element).
"""

from __future__ import annotations

import ctypes
import functools
import math

import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops, parallel
from cuda_mpi_openmp_amd.models import PoissonMultigrid, SlabJacobi
from cuda_mpi_openmp_amd.ops import reference as ref

DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector
NAN = float("nan")
MODES = ("contig", "vec", "shift")
# fine shapes of the transfer kernels: no coarse interior; the smallest with one;
# the smallest non-square; a row-block remainder across one wave; coarse width
# 258 across a 256-thread block; several blocks; and a tall strip, the smallest
# launch that keeps the full walks (16 rows per lane in the residual, 8 coarse
# rows in the transfers, each with a remainder block): smaller launches shorten
# their walks to fill the device
FINE_SHAPES = [(3, 3), (5, 5), (7, 11), (35, 131), (67, 515), (131, 1031), (32799, 131)]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _place(t: torch.Tensor, mode: str, device):
    """(view, backing): t's values in a pitched view of a NaN-filled backing
    buffer on ``device``."""
    h, w = t.shape
    nv = NV[t.dtype]
    if mode == "contig":
        backing = t.clone().to(device)
        return backing, backing
    pitch = (w + nv - 1) // nv * nv
    if mode == "vec":
        backing = torch.full((h, pitch), NAN, dtype=t.dtype, device=device)
        view = backing[:, :w]
    else:
        backing = torch.full((h * pitch + nv,), NAN, dtype=t.dtype, device=device)
        view = backing[1:1 + h * pitch].view(h, pitch)[:, :w]
        assert view.data_ptr() % 16 != 0
    view.copy_(t)
    return view, backing


def _rand(shape, seed, dtype, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(dtype)


def _nan_boundary(t: torch.Tensor) -> torch.Tensor:
    t = t.clone()
    t[0] = t[-1] = NAN
    t[:, 0] = t[:, -1] = NAN
    return t


# ---------------------------------------------------------------------------
# the transfer operators and the residual, on any device
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _transfer_case(dtype, h, w):
    """Inputs and torch-expression results, computed once and never modified."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    u = _rand((h, w), 100 * h + w, dtype)
    b = _nan_boundary(_rand((h, w), 100 * h + w + 1, dtype, -1.0, 1.0))
    r = _nan_boundary(_rand((h, w), 100 * h + w + 2, dtype, -1.0, 1.0))
    e = _rand((hc, wc), 100 * h + w + 3, dtype, -1.0, 1.0)  # boundary random: it is read
    uf = _nan_boundary(_rand((h, w), 100 * h + w + 4, dtype))
    nan_f = torch.full((h, w), NAN, dtype=dtype)
    nan_c = torch.full((hc, wc), NAN, dtype=dtype)
    want = {
        "res": ref.mg_residual(u, out=nan_f),
        "res_rhs": ref.mg_residual(u, rhs=b, out=nan_f),
        "restrict": ref.mg_restrict(r, out=nan_c),
        "prolong": ref.mg_prolong_add(e, uf),
    }
    for k in ("res", "res_rhs"):
        assert not bool(torch.isnan(want[k][1:-1, 1:-1]).any())
        assert bool(torch.isnan(want[k][0]).all()) and bool(torch.isnan(want[k][:, -1]).all())
    assert not bool(torch.isnan(want["restrict"][1:-1, 1:-1]).any()) and bool(torch.isnan(want["restrict"][0]).all())
    assert not bool(torch.isnan(want["prolong"][1:-1, 1:-1]).any()) and bool(torch.isnan(want["prolong"][0]).all())
    assert all(v.dtype == dtype for v in want.values())
    return u, b, r, e, uf, nan_f, nan_c, want


def _run_transfers(device, dtype, h, w, mode):
    """Backing buffers of the four results (padding included) and the two
    residual words, as CPU tensors."""
    u, b, r, e, uf, nan_f, nan_c, _ = _transfer_case(dtype, h, w)
    out = {}
    uv, _ = _place(u, mode, device)
    bv, _ = _place(b, mode, device)
    for key, rhs in (("res", None), ("res_rhs", bv)):
        rv, rb = _place(nan_f, mode, device)
        word = torch.zeros(1, dtype=dtype, device=device)
        ret = ops.mg_residual(uv, rv, rhs=rhs, resid=word)
        out[key] = rb.cpu()
        out[key + "_max"] = float(word.item())
        if device == "cpu":
            assert ret == out[key + "_max"]
        # without the residual word: the same r
        rv2, rb2 = _place(nan_f, mode, device)
        ops.mg_residual(uv, rv2, rhs=rhs)
        assert _same_bits(rb2, rb), ("residual without the word differs", h, w, mode)
    rv, _ = _place(r, mode, device)
    cv, cb = _place(nan_c, mode, device)
    ops.mg_restrict(rv, cv)
    out["restrict"] = cb.cpu()
    ev, _ = _place(e, mode, device)
    fv, fb = _place(uf, mode, device)
    ops.mg_prolong_add_(ev, fv)
    out["prolong"] = fb.cpu()
    return out


def _check_transfers(device, dtype, h, w):
    want = _transfer_case(dtype, h, w)[-1]
    for mode in MODES:
        got = _run_transfers(device, dtype, h, w, mode)
        for key in ("res", "res_rhs", "restrict", "prolong"):
            exp = _place(want[key], mode, "cpu")[1]
            assert _same_bits(got[key], exp), (key, h, w, mode, str(dtype))
        for key in ("res", "res_rhs"):
            inner = want[key][1:-1, 1:-1]
            assert got[key + "_max"] == float(inner.abs().max()), (key, h, w, mode)
        if device != "cpu" and dtype == torch.float64:
            lib = _run_transfers("cpu", dtype, h, w, mode)
            for key, val in lib.items():
                same = _same_bits(got[key], val) if isinstance(val, torch.Tensor) else got[key] == val
                assert same, ("GPU differs from the CPU library", key, h, w, mode)


@pytest.mark.parametrize("h,w", FINE_SHAPES[:5])
def test_cpu_transfers_equal_the_torch_expressions(h, w):
    _check_transfers("cpu", torch.float64, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", FINE_SHAPES)
def test_gpu_transfers_bit_exact(gpu, dtype, h, w):
    _check_transfers(gpu, dtype, h, w)


def test_restrict_writes_nothing_without_a_coarse_interior():
    want = _transfer_case(torch.float64, 3, 3)[-1]["restrict"]
    assert want.shape == (2, 2) and bool(torch.isnan(want).all())


# ---------------------------------------------------------------------------
# jacobi_relax
# ---------------------------------------------------------------------------
OMEGAS = (0.8, 1.0, 1.7)
PER_LANE_WIDTHS = [3, 5, 129, 131, 257]
STRIP_WIDTHS = [128, 250, 504]  # 250 crosses a strip boundary in fp64, 504 in fp32
HEIGHTS = (18, 37)


@functools.lru_cache(maxsize=None)
def _relax_case(dtype, h, w):
    u = _rand((h, w), 7000 * w + h, dtype)
    b = _nan_boundary(_rand((h, w), 7000 * w + h + 1, dtype, -1.0, 1.0))
    rowres = []
    for rhs in (None, b):
        plain = ref.jacobi(u, 1, h - 1, keep_dtype=True, rhs=rhs)
        rowres.append((plain[1:-1, 1:-1] - u[1:-1, 1:-1]).abs().amax(dim=1))
    return u, b, rowres[0], rowres[1]


@functools.lru_cache(maxsize=None)
def _relax_want(dtype, h, w, with_rhs, omega):
    u, b, _, _ = _relax_case(dtype, h, w)
    want = ref.jacobi(u, 1, h - 1, keep_dtype=True, rhs=b if with_rhs else None, omega=omega, prev=u)
    assert want.dtype == dtype and not bool(torch.isnan(want).any())
    return want


def _ranges(h):
    return ((1, h - 1), (1, 2), (4, 11), (h - 2, h - 1), (6, 6), (2, h - 2), (1, 17))


def _check_relax(device, dtype, w, modes=MODES):
    n = 0
    for h in HEIGHTS:
        u, b, rr_lap, rr_rhs = _relax_case(dtype, h, w)
        nan_f = torch.full((h, w), NAN, dtype=dtype)
        for mode in modes:
            uv, _ = _place(u, mode, device)
            bv, _ = _place(b, mode, device)
            for with_rhs in (False, True):
                rowres = rr_rhs if with_rhs else rr_lap
                for r0, r1 in _ranges(h):
                    omega, with_res = OMEGAS[n % 3], (n // 3) % 2 == 0
                    n += 1
                    tag = (str(dtype), h, w, mode, with_rhs, r0, r1, omega, with_res)
                    want = _relax_want(dtype, h, w, with_rhs, omega)
                    exp = nan_f.clone()
                    exp[r0:r1] = want[r0:r1]
                    ov, ob = _place(nan_f, mode, device)
                    word = torch.zeros(1, dtype=dtype, device=device) if with_res else None
                    ret = ops.jacobi_relax(uv, ov, r0, r1, omega, resid=word, rhs=bv if with_rhs else None)
                    assert _same_bits(ob, _place(exp, mode, "cpu")[1]), tag
                    exp_res = float(rowres[r0 - 1:r1 - 1].max()) if r1 > r0 else 0.0
                    if with_res:
                        assert float(word.item()) == exp_res, tag
                    if device == "cpu":
                        assert ret == exp_res, tag


@pytest.mark.parametrize("w", [3, 5, 64, 131])
def test_cpu_relax_equals_the_torch_expression(w):
    _check_relax("cpu", torch.float64, w)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w", PER_LANE_WIDTHS + STRIP_WIDTHS)
def test_gpu_relax_bit_exact(gpu, dtype, w):
    _check_relax(gpu, dtype, w)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [131, 250])
def test_gpu_relax_equals_the_cpu_library(gpu, w):
    h = 37
    u, b, _, _ = _relax_case(torch.float64, h, w)
    for mode in MODES:
        outs = []
        for device in ("cpu", gpu):
            uv, _ = _place(u, mode, device)
            bv, _ = _place(b, mode, device)
            ov, ob = _place(torch.full((h, w), NAN, dtype=torch.float64), mode, device)
            word = torch.zeros(1, dtype=torch.float64, device=device)
            ops.jacobi_relax(uv, ov, 1, h - 1, 0.8, resid=word, rhs=bv)
            outs.append((ob.cpu(), float(word.item())))
        assert _same_bits(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], (w, mode)


# ---------------------------------------------------------------------------
# argument refusals
# ---------------------------------------------------------------------------
def test_argument_refusals():
    f = torch.zeros((9, 13), dtype=torch.float64)
    c = torch.zeros((5, 7), dtype=torch.float64)
    out = torch.full((9, 13), -7.0, dtype=torch.float64)
    for w in (0.0, -1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.jacobi_relax(f, out, 1, 8, w)
        assert math.isnan(_native.lib().mpx_cpu_jacobi_relax_f64(f.data_ptr(), None, out.data_ptr(), 13, 13, 1, 8, w))
        assert _native.lib().mpx_jacobi_relax_f64(f.data_ptr(), None, out.data_ptr(), 13, 13, 1, 8, w, None, None) != 0
        assert _native.lib().mpx_jacobi_relax_f32(f.data_ptr(), None, out.data_ptr(), 13, 13, 1, 8, w, None, None) != 0
        with pytest.raises(ValueError):
            PoissonMultigrid(7, 9, omega=w)
    assert bool((out == -7.0).all())
    # shape mismatch
    with pytest.raises(ValueError):
        ops.jacobi_relax(f, torch.zeros((9, 12), dtype=torch.float64), 1, 8, 0.8)
    with pytest.raises(ValueError):
        ops.jacobi_relax(f, out, 1, 8, 0.8, rhs=torch.zeros((8, 13), dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.jacobi_relax(f, out, 0, 8, 0.8)
    with pytest.raises(ValueError):
        ops.mg_residual(f, torch.zeros((9, 11), dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.mg_residual(f, out, rhs=c)
    for bad in (torch.zeros((5, 6), dtype=torch.float64), torch.zeros((4, 7), dtype=torch.float64), f):
        with pytest.raises(ValueError):
            ops.mg_restrict(f, bad)
        with pytest.raises(ValueError):
            ops.mg_prolong_add_(bad, f)
    with pytest.raises(ValueError):
        ops.mg_restrict(torch.zeros((8, 13), dtype=torch.float64), torch.zeros((4, 7), dtype=torch.float64))
    # dtype and device mismatch
    f32, c32 = f.to(torch.float32), c.to(torch.float32)
    meta_f, meta_c = torch.zeros((9, 13), dtype=torch.float64, device="meta"), torch.zeros((5, 7), device="meta")
    for other_f, other_c in ((f32, c32), (meta_f, meta_c.to(torch.float64))):
        with pytest.raises(ValueError):
            ops.jacobi_relax(f, other_f, 1, 8, 0.8)
        with pytest.raises(ValueError):
            ops.jacobi_relax(f, out, 1, 8, 0.8, rhs=other_f)
        with pytest.raises(ValueError):
            ops.mg_residual(f, other_f)
        with pytest.raises(ValueError):
            ops.mg_residual(f, out, rhs=other_f)
        with pytest.raises(ValueError):
            ops.mg_restrict(f, other_c)
        with pytest.raises(ValueError):
            ops.mg_prolong_add_(other_c, f)
    with pytest.raises(ValueError):
        ops.mg_residual(f, out, resid=torch.zeros(1, dtype=torch.float32))
    with pytest.raises(ValueError):  # the CPU references are float64
        ops.mg_restrict(f32, c32)
    # stride(1) != 1
    ft = torch.zeros((13, 9), dtype=torch.float64).t()
    ct = torch.zeros((7, 5), dtype=torch.float64).t()
    assert ft.shape == f.shape and ft.stride(1) != 1
    with pytest.raises(ValueError):
        ops.jacobi_relax(ft, out, 1, 8, 0.8)
    with pytest.raises(ValueError):
        ops.jacobi_relax(f, ft, 1, 8, 0.8)
    with pytest.raises(ValueError):
        ops.mg_residual(ft, out)
    with pytest.raises(ValueError):
        ops.mg_residual(f, ft)
    with pytest.raises(ValueError):
        ops.mg_restrict(ft, c)
    with pytest.raises(ValueError):
        ops.mg_restrict(f, ct)
    with pytest.raises(ValueError):
        ops.mg_prolong_add_(ct, f)
    with pytest.raises(ValueError):
        ops.mg_prolong_add_(c, ft)
    # the native entry points refuse null pointers and bad geometry
    L = _native.lib()
    assert L.mpx_mg_residual_f64(None, None, out.data_ptr(), 9, 13, 13, 0, 13, None, None) != 0
    assert L.mpx_mg_residual_f64(f.data_ptr(), None, out.data_ptr(), 9, 13, 12, 0, 13, None, None) != 0
    assert L.mpx_mg_restrict_f32(None, c.data_ptr(), 5, 7, 13, 7, None) != 0
    assert L.mpx_mg_restrict_f64(f.data_ptr(), c.data_ptr(), 5, 7, 12, 7, None) != 0
    assert L.mpx_mg_prolong_add_f64(c.data_ptr(), f.data_ptr(), 5, 7, 6, 13, None) != 0
    assert math.isnan(L.mpx_cpu_mg_residual_f64(f.data_ptr(), None, out.data_ptr(), 9, 13, 12, 0, 13))
    assert L.mpx_cpu_mg_restrict_f64(f.data_ptr(), c.data_ptr(), 5, 7, 12, 7) != 0
    assert L.mpx_cpu_mg_prolong_add_f64(c.data_ptr(), f.data_ptr(), 5, 7, 7, 12) != 0
    assert bool((out == -7.0).all()) and bool((f == 0).all()) and bool((c == 0).all())
    # the model
    with pytest.raises(ValueError):
        PoissonMultigrid(7, 9, nu2=0)
    with pytest.raises(ValueError):
        PoissonMultigrid(7, 9, dtype=torch.float32)  # the CPU model is float64
    with pytest.raises(ValueError):
        PoissonMultigrid(7, 9).set_rhs()
    with pytest.raises(ValueError):
        PoissonMultigrid(7, 9).set_rhs(tensor=torch.zeros((9, 9)))
    # jacobi_sweep keeps refusing what it refused
    with pytest.raises(ValueError):
        ops.jacobi_sweep(_place(f, "vec", "cpu")[0][:, :12], out[:, :12], 1, 8)


def test_symbols():
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    for name in ("mpx_jacobi_relax_f64", "mpx_jacobi_relax_f32", "mpx_cpu_jacobi_relax_f64", "mpx_mg_residual_f64",
                 "mpx_mg_residual_f32", "mpx_cpu_mg_residual_f64", "mpx_mg_restrict_f64", "mpx_mg_restrict_f32",
                 "mpx_cpu_mg_restrict_f64", "mpx_mg_prolong_add_f64", "mpx_mg_prolong_add_f32",
                 "mpx_cpu_mg_prolong_add_f64"):
        assert hasattr(raw, name), name
    import subprocess

    names = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True,
                           check=True).stdout.split()
    assert any(n.startswith("mpx_mg_") for n in names)
    assert not [n for n in names if n.startswith("mpx_mg_") and "variant" in n]


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def test_levels():
    assert PoissonMultigrid(127, 129).levels == [(129, 129), (65, 65), (33, 33), (17, 17), (9, 9), (5, 5), (3, 3)]
    assert PoissonMultigrid(47, 81).levels == [(49, 81), (25, 41), (13, 21), (7, 11), (4, 6)]
    assert PoissonMultigrid(6, 9).levels == [(8, 9)]  # H - 1 = 7 is odd
    assert PoissonMultigrid(63, 129).levels[-1] == (3, 5)
    assert PoissonMultigrid(127, 129, max_levels=3).levels == [(129, 129), (65, 65), (33, 33)]
    m = PoissonMultigrid(47, 81)
    assert m.u.shape == (49, 81) and m.u.stride(1) == 1 and (m.u.stride(0) * 8) % 16 == 0 and m.u.stride(0) >= 81
    assert m.cycles == 0 and m.last_residual is None


def _problem(device, dtype, rows, cols, **kw):
    """Random interior in [0, 1), top boundary 1, rhs uniform in +-0.01, seeded."""
    m = PoissonMultigrid(rows, cols, dtype=dtype, device=device, **kw)
    m.set_boundary(top=1.0)
    m.fill(seed=3)
    m.set_rhs(tensor=_rand((rows, cols), 11, torch.float64, -0.01, 0.01))
    return m


def _defect(m) -> float:
    """max|4u - (sum of the neighbours) - b| over the interior, by a plain torch expression."""
    u, b = m.u, m.rhs
    nb = u[:-2, 1:-1] + u[2:, 1:-1] + u[1:-1, :-2] + u[1:-1, 2:]
    return float((4.0 * u[1:-1, 1:-1] - nb - b[1:-1, 1:-1]).abs().max())


def test_cpu_convergence():
    m = _problem("cpu", torch.float64, 63, 129)
    assert m.levels[-1] == (3, 5)
    res = [m.cycle() for _ in range(7)]
    ratios = [res[k] / res[k - 1] for k in range(1, 7)]
    print("last_residual per cycle:", res, "ratios:", ratios)
    assert all(r <= 0.2 for r in ratios), ratios  # the numpy prototype gave 0.11-0.155
    assert m.cycles == 7 and m.last_residual == res[-1]
    s = _problem("cpu", torch.float64, 63, 129)
    n = s.solve(1e-8)
    print("cycles to 1e-8:", n, "defect:", _defect(s))
    assert n <= 12 and s.cycles == n and s.last_residual <= 1e-8  # the prototype gave 9-10
    assert _defect(s) <= 1e-7
    # a single level is plain damped Jacobi: it still runs and reduces the residual
    one = _problem("cpu", torch.float64, 6, 9)
    first = one.cycle()
    for _ in range(20):
        last = one.cycle()
    assert last < first


def test_cpu_same_answer_as_chebyshev_jacobi():
    rows, cols = 31, 33
    m = _problem("cpu", torch.float64, rows, cols)
    m.solve(1e-13, max_cycles=40)
    j = SlabJacobi(parallel.DistContext(), rows, cols, check_every=5, accel="chebyshev")
    j.set_boundary(top=1.0)
    j.fill(seed=3)
    j.set_rhs(tensor=_rand((rows, cols), 11, torch.float64, -0.01, 0.01))
    j.run(20000, tol=1e-12)
    assert j.last_residual is not None and j.last_residual < 1e-12
    diff = float((m.u - j.u).abs().max())
    print("multigrid vs Chebyshev Jacobi, max-abs:", diff, "cycles:", m.cycles, "iterations:", j.iteration)
    assert diff <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(63, 129), (47, 81)])
def test_gpu_cycle_fp64_equals_the_cpu_model(gpu, rows, cols):
    g = _problem(gpu, torch.float64, rows, cols)
    c = _problem("cpu", torch.float64, rows, cols)
    for k in range(3):
        rg, rc = g.cycle(), c.cycle()
        assert rg == rc, (k, rg, rc)
    assert _same_bits(g.u, c.u)
    assert g.last_residual == c.last_residual and g.cycles == 3


class _TorchCycle:
    """The V-cycle composed from the torch expressions, in the model's order."""

    def __init__(self, m: PoissonMultigrid):
        self.m = m
        self.u = [torch.zeros(s, dtype=m.dtype) for s in m.levels]
        self.b = [torch.zeros(s, dtype=m.dtype) for s in m.levels]
        self.u[0] = m.u.cpu().clone()
        self.b[0] = m.rhs.cpu().clone()
        self.last = None

    def relax(self, k, omega, track=False):
        u, h = self.u[k], self.m.levels[k][0]
        if track:
            s = ref.jacobi(u, 1, h - 1, keep_dtype=True, rhs=self.b[k])
            self.last = float((s[1:-1, 1:-1] - u[1:-1, 1:-1]).abs().max())
        self.u[k] = ref.jacobi(u, 1, h - 1, keep_dtype=True, rhs=self.b[k], omega=omega, prev=u)

    def vcycle(self, k=0):
        m, n = self.m, len(self.m.levels)
        if k + 1 == n and k > 0:
            if m.levels[k] == (3, 3):
                self.relax(k, 1.0)
            else:
                for _ in range(m.coarse_sweeps):
                    self.relax(k, m.omega)
            return
        for _ in range(m.nu1):
            self.relax(k, m.omega)
        if k + 1 < n:
            r = ref.mg_residual(self.u[k], rhs=self.b[k])
            self.b[k + 1] = ref.mg_restrict(r)
            self.u[k + 1] = torch.zeros(m.levels[k + 1], dtype=m.dtype)
            self.vcycle(k + 1)
            self.u[k] = ref.mg_prolong_add(self.u[k + 1], self.u[k])
        for s in range(m.nu2):
            self.relax(k, m.omega, track=(k == 0 and s == m.nu2 - 1))


@pytest.mark.gpu
def test_gpu_cycle_fp32_equals_the_torch_cycle_and_converges(gpu):
    g = _problem(gpu, torch.float32, 63, 129)
    t = _TorchCycle(g)
    for k in range(3):
        rg = g.cycle()
        t.vcycle()
        assert rg == t.last, (k, rg, t.last)
        assert _same_bits(g.u, t.u[0]), k
    for _ in range(7):
        g.cycle()
    print("fp32 last_residual after 10 cycles:", g.last_residual)
    assert g.cycles == 10 and g.last_residual <= 2.0 ** -21  # the prototype reaches 2^-23 by cycle 8


def test_cpu_cycle_equals_the_torch_cycle():
    for rows, cols in ((15, 17), (47, 81)):  # down to 3 x 3 (one undamped sweep); a 4 x 6 coarsest level
        c = _problem("cpu", torch.float64, rows, cols)
        t = _TorchCycle(c)
        for k in range(2):
            rc = c.cycle()
            t.vcycle()
            assert rc == t.last and _same_bits(c.u, t.u[0]), (rows, cols, k)


@pytest.mark.gpu
def test_gpu_cycle_allocates_nothing(gpu):
    g = _problem(gpu, torch.float64, 63, 129)
    g.cycle()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    g.cycle()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before


@pytest.mark.gpu
def test_gpu_headline_1023x1025(gpu):
    g = _problem(gpu, torch.float64, 1023, 1025)
    n = g.solve(1e-8)
    d = _defect(g)
    print("1023x1025 fp64: cycles", n, "last_residual", g.last_residual, "defect", d)
    assert n <= 12 and g.last_residual <= 1e-8
    assert d <= 1e-7
