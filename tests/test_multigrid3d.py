"""Geometric multigrid for the 3-D Poisson solver: the damped 7-point sweep, the
residual, 27-point full weighting and trilinear prolongation, from the kernels
to ``models.PoissonMultigrid3D``.

Conventions are test_multigrid.py's: every operator has one rounding order, so
GPU fp32, GPU fp64, the CPU library and the dtype-preserving torch expressions
of ``ops.reference`` agree bit for bit and no kernel comparison carries a
tolerance. Inputs carry NaN in every element the contract says is never read
(padding, b's boundary, r's boundary for the restriction); outputs are
pre-filled with NaN and must keep those bits wherever the contract says "not
written" (compared on the whole backing buffer, padding included).

Layouts: "contig" (odd widths take the per-element kernels), "vec" (row pitch
rounded up to 16 bytes and one spare row per plane, so the plane stride exceeds
H * pitch: the vector kernels) and "shift" (the rounded pitch with the base
moved by one element: unaligned, per-element).
"""

from __future__ import annotations

import ctypes
import functools
import math

import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops, parallel
from cuda_mpi_openmp_amd.models import PoissonMultigrid3D, SlabJacobi3D
from cuda_mpi_openmp_amd.ops import reference as ref

DTYPES = [torch.float64, torch.float32]
NV = {torch.float64: 2, torch.float32: 4}  # elements per 16-byte vector
NAN = float("nan")
MODES = ("contig", "vec", "shift")
OMEGA = 6.0 / 7.0
# fine shapes (D, H, W): no coarse interior; the smallest with one; the smallest
# with three different edges; a width across one wave with a row remainder; a
# coarse width of 258
CPU_SHAPES = [(3, 3, 3), (5, 5, 5), (5, 7, 11), (7, 35, 131), (5, 11, 515)]


def _full_walk_shape():
    """The smallest narrow launch that keeps the full walks: launches with fewer
    than ``min_waves`` waves shorten theirs. With one wave across x, the
    restriction has (Hc - 2) * ceil((Dc - 2) / restrict_planes) waves and the
    prolongation (Hc - 1) * ceil((Dc - 1) / prolong_planes). Dc - 2 is a
    multiple of both walks plus one, so each walk down z ends in a remainder
    block (walks of 1 or 2 planes have none to leave); H - 2 is odd, a
    remainder for an even row walk of the stencil kernels, which have far more
    waves than they need here."""
    wk = ops.mg3_walk()
    pr, pp, need = wk["restrict_planes"], wk["prolong_planes"], wk["min_waves"]
    both = pr * pp // math.gcd(pr, pp)
    dc = both * max(1, 120 // both) + 3
    blocks = min(-(-(dc - 2) // pr), -(-(dc - 1) // pp))
    hc = -(-need // blocks) + 2
    shape = (2 * dc - 1, 2 * hc - 1, 9)
    assert (hc - 2) * -(-(dc - 2) // pr) >= need and (hc - 1) * -(-(dc - 1) // pp) >= need
    assert -(-(shape[1] - 2) // wk["rows"]) * (shape[0] - 2) >= need
    assert pr == 1 or (dc - 2) % pr != 0
    assert pp <= 2 or (dc - 1) % pp != 0
    assert shape[0] * shape[1] * shape[2] <= 10 ** 7
    return shape


def _gpu_shapes():
    return CPU_SHAPES + [(9, 67, 1031), _full_walk_shape()]  # several workgroups across x; the full walks


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _place(t: torch.Tensor, mode: str, device):
    """(view, backing): t's values in a pitched view of a NaN-filled backing
    buffer on ``device``."""
    d, h, w = t.shape
    nv = NV[t.dtype]
    if mode == "contig":
        backing = t.clone().to(device)
        return backing, backing
    pitch = (w + nv - 1) // nv * nv
    if mode == "vec":
        backing = torch.full((d, h + 1, pitch), NAN, dtype=t.dtype, device=device)
        view = backing[:, :h, :w]
        assert view.stride(0) > h * pitch
    else:
        backing = torch.full((d * h * pitch + nv,), NAN, dtype=t.dtype, device=device)
        view = backing[1:1 + d * h * pitch].view(d, h, pitch)[:, :, :w]
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
    t[:, :, 0] = t[:, :, -1] = NAN
    return t


def _inner(t: torch.Tensor) -> torch.Tensor:
    return t[1:-1, 1:-1, 1:-1]


# ---------------------------------------------------------------------------
# the four operators on any device
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(dtype, shape):
    """Inputs and torch-expression results, computed once and never modified."""
    d, h, w = shape
    cs = tuple((s + 1) // 2 for s in shape)
    seed = 10000 * d + 100 * h + w
    u = _rand(shape, seed, dtype)
    b = _nan_boundary(_rand(shape, seed + 1, dtype, -1.0, 1.0))
    r = _nan_boundary(_rand(shape, seed + 2, dtype, -1.0, 1.0))
    e = _rand(cs, seed + 3, dtype, -1.0, 1.0)  # boundary random: it is read
    uf = _nan_boundary(_rand(shape, seed + 4, dtype))
    nan_f = torch.full(shape, NAN, dtype=dtype)
    nan_c = torch.full(cs, NAN, dtype=dtype)
    relax = nan_f.clone()
    relax[1:-1] = ref.jacobi3d(u, 1, d - 1, keep_dtype=True, rhs=b, omega=OMEGA, prev=u)[1:-1]
    plain = ref.jacobi3d(u, 1, d - 1, keep_dtype=True, rhs=b)
    want = {
        "res": ref.mg3_residual(u, out=nan_f),
        "res_rhs": ref.mg3_residual(u, rhs=b, out=nan_f),
        "restrict": ref.mg3_restrict(r, out=nan_c),
        "prolong": ref.mg3_prolong_add(e, uf),
        "relax": relax,
    }
    maxes = {"res_max": float(_inner(want["res"]).abs().max()), "res_rhs_max": float(_inner(want["res_rhs"]).abs().max()),
             "relax_max": float((_inner(plain) - _inner(u)).abs().max())}
    for k in ("res", "res_rhs", "prolong"):
        assert not bool(torch.isnan(_inner(want[k])).any()), k
        assert bool(torch.isnan(want[k][0]).all()) and bool(torch.isnan(want[k][:, :, -1]).all()), k
    assert not bool(torch.isnan(want["relax"][1:-1]).any()) and bool(torch.isnan(want["relax"][0]).all())
    assert bool(torch.isnan(want["restrict"][0]).all()) and bool(torch.isnan(want["restrict"][:, -1]).all())
    if min(cs) >= 3:
        assert not bool(torch.isnan(_inner(want["restrict"])).any())
    else:
        assert bool(torch.isnan(want["restrict"]).all())  # no coarse interior: nothing is written
    assert all(v.dtype == dtype for v in want.values())
    return u, b, r, e, uf, nan_f, nan_c, want, maxes


def _run_ops(device, dtype, shape, mode):
    """Backing buffers of the five results (padding included) and the three
    residual words, as CPU tensors."""
    u, b, r, e, uf, nan_f, nan_c, _, _ = _case(dtype, shape)
    out = {}
    uv, _ = _place(u, mode, device)
    bv, _ = _place(b, mode, device)
    for key, rhs in (("res", None), ("res_rhs", bv)):
        rv, rb = _place(nan_f, mode, device)
        word = torch.zeros(1, dtype=dtype, device=device)
        ret = ops.mg3_residual(uv, rv, rhs=rhs, resid=word)
        out[key] = rb.cpu()
        out[key + "_max"] = float(word.item())
        if device == "cpu":
            assert ret == out[key + "_max"]
    rv2, rb2 = _place(nan_f, mode, device)  # without the residual word: the same r
    ops.mg3_residual(uv, rv2, rhs=bv)
    assert _same_bits(rb2, out["res_rhs"]), ("residual without the word differs", shape, mode)
    rv, _ = _place(r, mode, device)
    cv, cb = _place(nan_c, mode, device)
    ops.mg3_restrict(rv, cv)
    out["restrict"] = cb.cpu()
    ev, _ = _place(e, mode, device)
    fv, fb = _place(uf, mode, device)
    ops.mg3_prolong_add_(ev, fv)
    out["prolong"] = fb.cpu()
    ov, ob = _place(nan_f, mode, device)
    word = torch.zeros(1, dtype=dtype, device=device)
    ops.jacobi3d_relax(uv, ov, 1, shape[0] - 1, OMEGA, resid=word, rhs=bv)
    out["relax"] = ob.cpu()
    out["relax_max"] = float(word.item())
    return out


def _check_ops(device, dtype, shape):
    want, maxes = _case(dtype, shape)[-2:]
    for mode in MODES:
        got = _run_ops(device, dtype, shape, mode)
        for key, val in want.items():
            assert _same_bits(got[key], _place(val, mode, "cpu")[1]), (key, shape, mode, str(dtype))
        for key, val in maxes.items():
            assert got[key] == val, (key, shape, mode, str(dtype), got[key], val)
        if device != "cpu" and dtype == torch.float64:
            lib = _run_ops("cpu", dtype, shape, mode)
            for key, val in lib.items():
                same = _same_bits(got[key], val) if isinstance(val, torch.Tensor) else got[key] == val
                assert same, ("GPU differs from the CPU library", key, shape, mode)


@pytest.mark.parametrize("shape", CPU_SHAPES)
def test_cpu_operators_equal_the_torch_expressions(shape):
    _check_ops("cpu", torch.float64, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(len(CPU_SHAPES) + 2))
def test_gpu_operators_bit_exact(gpu, dtype, index):
    _check_ops(gpu, dtype, _gpu_shapes()[index])


def test_restrict_writes_nothing_without_a_coarse_interior():
    want = _case(torch.float64, (3, 3, 3))[-2]["restrict"]
    assert want.shape == (2, 2, 2) and bool(torch.isnan(want).all())
    # one thin direction is enough
    f = _rand((9, 9, 3), 5, torch.float64)
    c = torch.full((5, 5, 2), NAN, dtype=torch.float64)
    ops.mg3_restrict(f, c)
    assert bool(torch.isnan(c).all())


def test_transfers_equal_the_direct_27_weight_and_trilinear_forms():
    """The separable definitions against the textbook forms (rounding differs:
    a tolerance of a few ulp of the values, which are at most 1 in size)."""
    shape = (7, 9, 11)
    r = torch.zeros(shape, dtype=torch.float64)
    r[1:-1, 1:-1, 1:-1] = _rand((5, 7, 9), 1, torch.float64, -1.0, 1.0)
    w1 = torch.tensor([0.5, 1.0, 0.5], dtype=torch.float64)
    w3 = 0.5 * w1.view(3, 1, 1) * w1.view(1, 3, 1) * w1.view(1, 1, 3)
    assert float(w3[1, 1, 1]) == 0.5 and float(w3[0, 1, 1]) == 0.25 and float(w3[0, 0, 1]) == 0.125 \
        and float(w3[0, 0, 0]) == 0.0625
    direct = torch.nn.functional.conv3d(r[None, None, 1:, 1:, 1:], w3[None, None], stride=2)[0, 0]  # centres 2, 4, ...
    got = ref.mg3_restrict(r)
    assert got.shape == (4, 5, 6) and float((_inner(got) - direct).abs().max()) <= 1e-14
    e = _rand((4, 5, 6), 2, torch.float64, -1.0, 1.0)
    tri = torch.nn.functional.interpolate(e[None, None], size=shape, mode="trilinear", align_corners=True)[0, 0]
    got = ref.mg3_prolong_add(e, torch.zeros(shape, dtype=torch.float64))
    assert float((_inner(got) - _inner(tri)).abs().max()) <= 1e-14


# ---------------------------------------------------------------------------
# jacobi3d_relax
# ---------------------------------------------------------------------------
OMEGAS = (OMEGA, 1.0, 1.7)
CPU_WIDTHS = [3, 5, 64, 131]
GPU_WIDTHS = [3, 5, 129, 131, 257, 128, 250, 504]
HEIGHTS = (3, 10, 37)
DEPTHS = (3, 6)


def _ranges(d):
    return ((1, 2), (1, 1)) if d == 3 else ((1, d - 1), (1, 2), (2, 4), (d - 2, d - 1), (3, 3))


@functools.lru_cache(maxsize=None)
def _relax_case(dtype, d, h, w):
    u = _rand((d, h, w), 7000 * w + 10 * h + d, dtype)
    b = _nan_boundary(_rand((d, h, w), 7000 * w + 10 * h + d + 1, dtype, -1.0, 1.0))
    planeres = []
    for rhs in (None, b):
        plain = ref.jacobi3d(u, 1, d - 1, keep_dtype=True, rhs=rhs)
        planeres.append((_inner(plain) - _inner(u)).abs().amax(dim=(1, 2)))
    return u, b, planeres[0], planeres[1]


@functools.lru_cache(maxsize=None)
def _relax_want(dtype, d, h, w, with_rhs, omega):
    u, b, _, _ = _relax_case(dtype, d, h, w)
    want = ref.jacobi3d(u, 1, d - 1, keep_dtype=True, rhs=b if with_rhs else None, omega=omega, prev=u)
    assert want.dtype == dtype and not bool(torch.isnan(want).any())
    return want


def _check_relax(device, dtype, w):
    n = 0
    for d in DEPTHS:
        for h in HEIGHTS:
            u, b, pr_lap, pr_rhs = _relax_case(dtype, d, h, w)
            nan_f = torch.full((d, h, w), NAN, dtype=dtype)
            for mode in MODES:
                uv, _ = _place(u, mode, device)
                bv, _ = _place(b, mode, device)
                for with_rhs in (False, True):
                    planeres = pr_rhs if with_rhs else pr_lap
                    for k0, k1 in _ranges(d):
                        omega, with_res = OMEGAS[n % 3], (n // 3) % 2 == 0
                        n += 1
                        tag = (str(dtype), d, h, w, mode, with_rhs, k0, k1, omega, with_res)
                        want = _relax_want(dtype, d, h, w, with_rhs, omega)
                        exp = nan_f.clone()
                        exp[k0:k1] = want[k0:k1]  # boundary rows and columns of a swept plane copy through
                        ov, ob = _place(nan_f, mode, device)
                        word = torch.zeros(1, dtype=dtype, device=device) if with_res else None
                        ret = ops.jacobi3d_relax(uv, ov, k0, k1, omega, resid=word, rhs=bv if with_rhs else None)
                        assert _same_bits(ob, _place(exp, mode, "cpu")[1]), tag
                        exp_res = float(planeres[k0 - 1:k1 - 1].max()) if k1 > k0 else 0.0
                        if with_res:
                            assert float(word.item()) == exp_res, tag
                        if device == "cpu":
                            assert ret == exp_res, tag


@pytest.mark.parametrize("w", CPU_WIDTHS)
def test_cpu_relax_equals_the_torch_expression(w):
    _check_relax("cpu", torch.float64, w)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w", GPU_WIDTHS)
def test_gpu_relax_bit_exact(gpu, dtype, w):
    _check_relax(gpu, dtype, w)


# ---------------------------------------------------------------------------
# argument refusals
# ---------------------------------------------------------------------------
def test_argument_refusals():
    f64 = torch.float64
    f = torch.zeros((5, 9, 13), dtype=f64)
    c = torch.zeros((3, 5, 7), dtype=f64)
    out = torch.full((5, 9, 13), -7.0, dtype=f64)
    L = _native.lib()
    fp, cp, op = f.data_ptr(), c.data_ptr(), out.data_ptr()
    for w in (0.0, -1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.jacobi3d_relax(f, out, 1, 4, w)
        assert math.isnan(L.mpx_cpu_jacobi3d_relax_f64(fp, None, op, 5, 9, 13, 13, 117, 1, 4, w))
        assert L.mpx_jacobi3d_relax_f64(fp, None, op, 5, 9, 13, 13, 117, 1, 4, w, None, None) != 0
        assert L.mpx_jacobi3d_relax_f32(fp, None, op, 5, 9, 13, 13, 117, 1, 4, w, None, None) != 0
        with pytest.raises(ValueError):
            PoissonMultigrid3D(7, 9, 9, omega=w)
    assert L.mpx_jacobi3d_relax_f32(fp, None, op, 5, 9, 13, 13, 117, 1, 4, 1e-60, None, None) != 0  # rounds to 0
    assert bool((out == -7.0).all())
    # shape mismatch and ranges
    with pytest.raises(ValueError):
        ops.jacobi3d_relax(f, torch.zeros((5, 9, 12), dtype=f64), 1, 4, 0.8)
    with pytest.raises(ValueError):
        ops.jacobi3d_relax(f, out, 1, 4, 0.8, rhs=torch.zeros((5, 8, 13), dtype=f64))
    with pytest.raises(ValueError):  # same shape, another pitch
        ops.jacobi3d_relax(f, torch.zeros((5, 9, 14), dtype=f64)[:, :, :13], 1, 4, 0.8)
    for k0, k1 in ((0, 4), (1, 5), (3, 2)):
        with pytest.raises(ValueError):
            ops.jacobi3d_relax(f, out, k0, k1, 0.8)
    with pytest.raises(ValueError):
        ops.jacobi3d_relax(f[0], out[0], 1, 4, 0.8)  # 2-D
    with pytest.raises(ValueError):
        ops.mg3_residual(f, torch.zeros((5, 9, 11), dtype=f64))
    with pytest.raises(ValueError):
        ops.mg3_residual(f, out, rhs=c)
    with pytest.raises(ValueError):
        ops.mg3_residual(f[:2], out[:2])  # fewer than 3 planes
    for bad in (torch.zeros((3, 5, 6), dtype=f64), torch.zeros((3, 4, 7), dtype=f64), torch.zeros((2, 5, 7), dtype=f64), f):
        with pytest.raises(ValueError):
            ops.mg3_restrict(f, bad)
        with pytest.raises(ValueError):
            ops.mg3_prolong_add_(bad, f)
    with pytest.raises(ValueError):
        ops.mg3_restrict(torch.zeros((5, 8, 13), dtype=f64), torch.zeros((3, 4, 7), dtype=f64))
    # dtype and device mismatch
    f32, c32 = f.to(torch.float32), c.to(torch.float32)
    meta_f, meta_c = torch.zeros((5, 9, 13), dtype=f64, device="meta"), torch.zeros((3, 5, 7), dtype=f64, device="meta")
    for other_f, other_c in ((f32, c32), (meta_f, meta_c)):
        with pytest.raises(ValueError):
            ops.jacobi3d_relax(f, other_f, 1, 4, 0.8)
        with pytest.raises(ValueError):
            ops.jacobi3d_relax(f, out, 1, 4, 0.8, rhs=other_f)
        with pytest.raises(ValueError):
            ops.mg3_residual(f, other_f)
        with pytest.raises(ValueError):
            ops.mg3_residual(f, out, rhs=other_f)
        with pytest.raises(ValueError):
            ops.mg3_restrict(f, other_c)
        with pytest.raises(ValueError):
            ops.mg3_prolong_add_(other_c, f)
    with pytest.raises(ValueError):
        ops.mg3_residual(f, out, resid=torch.zeros(1, dtype=torch.float32))
    with pytest.raises(ValueError):  # the CPU references are float64
        ops.mg3_restrict(f32, c32)
    # strides: x not the fastest; planes that overlap
    ft = torch.zeros((5, 13, 9), dtype=f64).transpose(1, 2)
    ct = torch.zeros((3, 7, 5), dtype=f64).transpose(1, 2)
    fo = torch.zeros(5 * 9 * 13, dtype=f64).as_strided((5, 9, 13), (13 * 8, 13, 1))
    assert ft.shape == f.shape and ft.stride(2) != 1 and fo.stride(0) < 9 * 13
    for bad_f in (ft, fo):
        with pytest.raises(ValueError):
            ops.jacobi3d_relax(bad_f, out, 1, 4, 0.8)
        with pytest.raises(ValueError):
            ops.jacobi3d_relax(f, bad_f, 1, 4, 0.8)
        with pytest.raises(ValueError):
            ops.mg3_residual(bad_f, out)
        with pytest.raises(ValueError):
            ops.mg3_residual(f, bad_f)
        with pytest.raises(ValueError):
            ops.mg3_restrict(bad_f, c)
        with pytest.raises(ValueError):
            ops.mg3_prolong_add_(c, bad_f)
    with pytest.raises(ValueError):
        ops.mg3_restrict(f, ct)
    with pytest.raises(ValueError):
        ops.mg3_prolong_add_(ct, f)
    # the native entry points: null pointers, pitch < W, plane stride < H * pitch, bad ranges
    ok_f, ok_c = (13, 117), (7, 35)
    assert L.mpx_jacobi3d_relax_f64(None, None, op, 5, 9, 13, 13, 117, 1, 4, 0.8, None, None) != 0
    assert L.mpx_jacobi3d_relax_f64(fp, None, None, 5, 9, 13, 13, 117, 1, 4, 0.8, None, None) != 0
    assert L.mpx_jacobi3d_relax_f64(fp, None, op, 5, 9, 13, 12, 117, 1, 4, 0.8, None, None) != 0
    assert L.mpx_jacobi3d_relax_f32(fp, None, op, 5, 9, 13, 13, 116, 1, 4, 0.8, None, None) != 0
    assert L.mpx_jacobi3d_relax_f64(fp, None, op, 5, 9, 13, 13, 117, 1, 5, 0.8, None, None) != 0
    assert L.mpx_jacobi3d_relax_f64(fp, None, op, 5, 9, 13, 13, 117, 0, 4, 0.8, None, None) != 0
    assert math.isnan(L.mpx_cpu_jacobi3d_relax_f64(fp, None, op, 5, 9, 13, 12, 117, 1, 4, 0.8))
    assert math.isnan(L.mpx_cpu_jacobi3d_relax_f64(fp, None, op, 5, 9, 13, 13, 116, 1, 4, 0.8))
    assert math.isnan(L.mpx_cpu_jacobi3d_relax_f64(fp, None, None, 5, 9, 13, 13, 117, 1, 4, 0.8))
    assert L.mpx_mg3_residual_f64(None, None, op, 5, 9, 13, *ok_f, 0, 0, *ok_f, None, None) != 0
    assert L.mpx_mg3_residual_f64(fp, None, op, 5, 9, 13, 12, 117, 0, 0, *ok_f, None, None) != 0
    assert L.mpx_mg3_residual_f32(fp, None, op, 5, 9, 13, *ok_f, 0, 0, 13, 116, None, None) != 0
    assert L.mpx_mg3_residual_f64(fp, fp, op, 5, 9, 13, *ok_f, 12, 117, *ok_f, None, None) != 0
    assert L.mpx_mg3_residual_f64(fp, None, op, 2, 9, 13, *ok_f, 0, 0, *ok_f, None, None) != 0
    assert math.isnan(L.mpx_cpu_mg3_residual_f64(fp, None, op, 5, 9, 13, 12, 117, 0, 0, *ok_f))
    assert math.isnan(L.mpx_cpu_mg3_residual_f64(fp, None, op, 5, 9, 13, *ok_f, 0, 0, 13, 116))
    assert math.isnan(L.mpx_cpu_mg3_residual_f64(fp, None, None, 5, 9, 13, *ok_f, 0, 0, *ok_f))
    assert L.mpx_mg3_restrict_f32(None, cp, 3, 5, 7, *ok_f, *ok_c, None) != 0
    assert L.mpx_mg3_restrict_f64(op, cp, 3, 5, 7, 12, 117, *ok_c, None) != 0
    assert L.mpx_mg3_restrict_f64(op, cp, 3, 5, 7, 13, 116, *ok_c, None) != 0
    assert L.mpx_mg3_restrict_f64(op, cp, 3, 5, 7, *ok_f, 6, 35, None) != 0
    assert L.mpx_mg3_restrict_f64(op, cp, 3, 5, 7, *ok_f, 7, 34, None) != 0
    assert L.mpx_mg3_restrict_f64(op, cp, 3, 1, 7, *ok_f, *ok_c, None) != 0
    assert L.mpx_mg3_prolong_add_f64(None, op, 3, 5, 7, *ok_c, *ok_f, None) != 0
    assert L.mpx_mg3_prolong_add_f64(cp, op, 3, 5, 7, 6, 35, *ok_f, None) != 0
    assert L.mpx_mg3_prolong_add_f32(cp, op, 3, 5, 7, *ok_c, 13, 116, None) != 0
    assert L.mpx_cpu_mg3_restrict_f64(op, cp, 3, 5, 7, 12, 117, *ok_c) != 0
    assert L.mpx_cpu_mg3_restrict_f64(op, cp, 3, 5, 7, *ok_f, 7, 34) != 0
    assert L.mpx_cpu_mg3_restrict_f64(None, cp, 3, 5, 7, *ok_f, *ok_c) != 0
    assert L.mpx_cpu_mg3_prolong_add_f64(cp, op, 3, 5, 7, *ok_c, 12, 117) != 0
    assert L.mpx_cpu_mg3_prolong_add_f64(cp, op, 3, 5, 7, 7, 34, *ok_f) != 0
    assert L.mpx_cpu_mg3_prolong_add_f64(cp, None, 3, 5, 7, *ok_c, *ok_f) != 0
    assert bool((out == -7.0).all()) and bool((f == 0).all()) and bool((c == 0).all())
    # the model
    with pytest.raises(ValueError):
        PoissonMultigrid3D(7, 9, 9, nu2=0)
    with pytest.raises(ValueError):
        PoissonMultigrid3D(7, 9, 9, dtype=torch.float32)  # the CPU model is float64
    with pytest.raises(ValueError):
        PoissonMultigrid3D(0, 9, 9)
    with pytest.raises(ValueError):
        PoissonMultigrid3D(7, 9, 9, max_levels=0)
    with pytest.raises(ValueError):
        PoissonMultigrid3D(7, 9, 9).set_rhs()
    with pytest.raises(ValueError):
        PoissonMultigrid3D(7, 9, 9).set_rhs(tensor=torch.zeros((9, 9, 9)))


def test_symbols():
    raw = ctypes.CDLL(str(_native.LIB_PATH))
    for stem in ("jacobi3d_relax", "mg3_residual", "mg3_restrict", "mg3_prolong_add"):
        for name in (f"mpx_{stem}_f64", f"mpx_{stem}_f32", f"mpx_cpu_{stem}_f64"):
            assert hasattr(raw, name), name
    wk = ops.mg3_walk()
    assert all(wk[k] >= 1 for k in ("rows", "restrict_planes", "prolong_planes", "min_waves", "waves"))


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def test_levels():
    M = PoissonMultigrid3D
    assert M(15, 17, 17).levels == [(17, 17, 17), (9, 9, 9), (5, 5, 5), (3, 3, 3)]
    assert M(23, 41, 21).levels == [(25, 41, 21), (13, 21, 11), (7, 11, 6)]  # W - 1 = 5 is odd
    # one dimension stops the coarsening, whichever it is
    assert M(6, 17, 17).levels == [(8, 17, 17)]
    assert M(15, 18, 17).levels == [(17, 18, 17)]
    assert M(15, 17, 18).levels == [(17, 17, 18)]
    assert M(3, 65, 65).levels == [(5, 65, 65), (3, 33, 33)]  # the coarse grid must keep an interior
    assert M(31, 33, 5).levels == [(33, 33, 5), (17, 17, 3)]
    assert M(31, 33, 33, max_levels=2).levels == [(33, 33, 33), (17, 17, 17)]
    assert M(31, 33, 33, max_levels=1).levels == [(33, 33, 33)]
    assert M.level_shapes(15, 17, 17) == M(15, 17, 17).levels
    m = M(23, 41, 21)
    assert m.u.shape == (25, 41, 21) and m.u.stride(2) == 1 and (m.u.stride(1) * 8) % 16 == 0
    assert m.u.stride(1) >= 21 and m.u.stride(0) == 41 * m.u.stride(1)
    assert m.rhs.shape == m.u.shape and m.cycles == 0 and m.last_residual is None


def _problem(device, dtype, planes, ny, nx, **kw):
    """Random interior in [0, 1), z0 face 1, rhs uniform in +-0.01, seeded."""
    m = PoissonMultigrid3D(planes, ny, nx, dtype=dtype, device=device, **kw)
    m.set_boundary(z0=1.0)
    m.fill(seed=3)
    m.set_rhs(tensor=_rand((planes, ny, nx), 11, torch.float64, -0.01, 0.01))
    return m


def _defect(m) -> float:
    """max|6u - (sum of the neighbours) - b| over the interior, by a plain torch expression."""
    u, b = m.u, m.rhs
    c = slice(1, -1)
    nb = u[:-2, c, c] + u[2:, c, c] + u[c, :-2, c] + u[c, 2:, c] + u[c, c, :-2] + u[c, c, 2:]
    return float((6.0 * u[c, c, c] - nb - b[c, c, c]).abs().max())


def test_set_boundary_matches_slab_jacobi3d():
    m = PoissonMultigrid3D(5, 6, 7)
    j = SlabJacobi3D(parallel.DistContext(), 5, 6, 7)
    faces = dict(z0=1.0, z1=2.0, y0=3.0, y1=4.0, x0=5.0, x1=6.0)
    m.set_boundary(**faces)
    j.set_boundary(**faces)
    m.fill(seed=3)
    j.fill(seed=3)
    assert _same_bits(m.u, j.u)


@pytest.mark.parametrize("planes,ny,nx", [(31, 33, 33), (15, 33, 65)])
def test_cpu_convergence(planes, ny, nx):
    m = _problem("cpu", torch.float64, planes, ny, nx)
    res = [m.cycle() for _ in range(8)]
    ratios = [res[k] / res[k - 1] for k in range(1, 8)]  # cycles 2 - 8
    print("last_residual per cycle:", res, "ratios:", ratios)
    # the smoothing bound of V(2,2) with omega = 6/7 is (5/7)^4 = 0.26; the numpy prototype's worst was 0.264
    assert all(r <= 0.32 for r in ratios), ratios
    assert m.cycles == 8 and m.last_residual == res[-1]
    s = _problem("cpu", torch.float64, planes, ny, nx)
    n = s.solve(1e-8)
    print("cycles to 1e-8:", n, "defect:", _defect(s))
    assert n <= 16 and s.cycles == n and s.last_residual <= 1e-8  # the prototype needed 13


def test_cpu_same_answer_as_chebyshev_jacobi():
    planes, ny, nx = 15, 17, 17
    m = _problem("cpu", torch.float64, planes, ny, nx)
    m.solve(1e-13, max_cycles=60)
    j = SlabJacobi3D(parallel.DistContext(), planes, ny, nx, check_every=5, accel="chebyshev")
    j.set_boundary(z0=1.0)
    j.fill(seed=3)
    j.set_rhs(tensor=_rand((planes, ny, nx), 11, torch.float64, -0.01, 0.01))
    j.run(20000, tol=1e-12)
    assert j.last_residual is not None and j.last_residual < 1e-12
    diff = float((m.u - j.u).abs().max())
    print("multigrid vs Chebyshev Jacobi, max-abs:", diff, "cycles:", m.cycles, "iterations:", j.iteration)
    assert diff <= 1e-9


class _TorchCycle:
    """The V-cycle composed from the torch expressions, in the model's order."""

    def __init__(self, m: PoissonMultigrid3D):
        self.m = m
        self.u = [torch.zeros(s, dtype=m.dtype) for s in m.levels]
        self.b = [torch.zeros(s, dtype=m.dtype) for s in m.levels]
        self.u[0] = m.u.cpu().clone()
        self.b[0] = m.rhs.cpu().clone()
        self.last = None

    def relax(self, k, omega, track=False):
        u, d = self.u[k], self.m.levels[k][0]
        if track:
            s = ref.jacobi3d(u, 1, d - 1, keep_dtype=True, rhs=self.b[k])
            self.last = float((_inner(s) - _inner(u)).abs().max())
        self.u[k] = ref.jacobi3d(u, 1, d - 1, keep_dtype=True, rhs=self.b[k], omega=omega, prev=u)

    def vcycle(self, k=0):
        m, n = self.m, len(self.m.levels)
        if k + 1 == n and k > 0:
            if m.levels[k] == (3, 3, 3):
                self.relax(k, 1.0)
            else:
                for _ in range(m.coarse_sweeps):
                    self.relax(k, m.omega)
            return
        for _ in range(m.nu1):
            self.relax(k, m.omega)
        if k + 1 < n:
            r = ref.mg3_residual(self.u[k], rhs=self.b[k])
            self.b[k + 1] = ref.mg3_restrict(r)
            self.u[k + 1] = torch.zeros(m.levels[k + 1], dtype=m.dtype)
            self.vcycle(k + 1)
            self.u[k] = ref.mg3_prolong_add(self.u[k + 1], self.u[k])
        for s in range(m.nu2):
            self.relax(k, m.omega, track=(k == 0 and s == m.nu2 - 1))


CYCLE_SHAPES = [(15, 17, 17), (23, 41, 21)]  # down to (3, 3, 3): one undamped sweep; a (7, 11, 6) coarsest level


@pytest.mark.parametrize("planes,ny,nx", CYCLE_SHAPES)
def test_cpu_cycle_equals_the_torch_cycle(planes, ny, nx):
    c = _problem("cpu", torch.float64, planes, ny, nx)
    assert c.levels[-1] == ((3, 3, 3) if planes == 15 else (7, 11, 6))
    t = _TorchCycle(c)
    for k in range(2):
        rc = c.cycle()
        t.vcycle()
        assert rc == t.last and _same_bits(c.u, t.u[0]), (planes, ny, nx, k)
    assert c.last_residual == t.last


@pytest.mark.gpu
@pytest.mark.parametrize("planes,ny,nx", CYCLE_SHAPES)
def test_gpu_cycle_fp64_equals_the_cpu_model(gpu, planes, ny, nx):
    g = _problem(gpu, torch.float64, planes, ny, nx)
    c = _problem("cpu", torch.float64, planes, ny, nx)
    for k in range(3):
        rg, rc = g.cycle(), c.cycle()
        assert rg == rc, (k, rg, rc)
    assert _same_bits(g.u, c.u)
    assert g.last_residual == c.last_residual and g.cycles == 3


@pytest.mark.gpu
@pytest.mark.parametrize("planes,ny,nx", CYCLE_SHAPES)
def test_gpu_cycle_fp32_equals_the_torch_cycle_and_converges(gpu, planes, ny, nx):
    g = _problem(gpu, torch.float32, planes, ny, nx)
    t = _TorchCycle(g)
    for k in range(3):
        rg = g.cycle()
        t.vcycle()
        assert rg == t.last, (k, rg, t.last)
        assert _same_bits(g.u, t.u[0]), k
    for _ in range(9):
        g.cycle()
        t.vcycle()
    print("fp32 last_residual after 12 cycles:", g.last_residual, "torch composed cycle:", t.last)
    assert g.cycles == 12 and g.last_residual <= 2.0 * t.last


@pytest.mark.gpu
def test_gpu_cycle_allocates_nothing(gpu):
    g = _problem(gpu, torch.float64, 23, 41, 21)
    g.cycle()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    g.cycle()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before


@pytest.mark.gpu
def test_gpu_headline_127x129x129(gpu):
    g = _problem(gpu, torch.float64, 127, 129, 129)
    n = g.solve(1e-8)
    d = _defect(g)
    print("127x129x129 fp64: cycles", n, "last_residual", g.last_residual, "defect", d)
    assert n <= 16 and g.last_residual <= 1e-8
