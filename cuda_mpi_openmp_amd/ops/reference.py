"""Plain-PyTorch reference implementations (no native code) of every operator.

They are the independent oracles of the numerics tests: fp32 for the image
operators (luminance, Roberts, KxK conv via ``torch.nn.functional.conv2d``),
fp64 for lab1/lab3/Jacobi. Summation order can differ from the native
kernels', so image results agree to +-1 gray level except where stated.
The conv's exact oracle is ``tests/conv_oracle.py``: numpy only, every fp32
operation in the native order (one fma chain per filter), equal to the CPU
reference and the GPU kernels byte for byte (``tests/test_conv_exact.py``).
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .filters import MODE_ABS1, MODE_MAG2, Filter


def luma(img: torch.Tensor) -> torch.Tensor:
    """fp32 luminance with the reference's evaluation order and no FMA."""
    f = img[..., :3].to(torch.float32)
    t0 = torch.tensor(0.299, dtype=torch.float32) * f[..., 0]
    t1 = torch.tensor(0.587, dtype=torch.float32) * f[..., 1]
    t2 = torch.tensor(0.114, dtype=torch.float32) * f[..., 2]
    return (t0 + t1) + t2


def _gray(g: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    v = torch.clamp(g, 0.0, 255.0).to(torch.uint8)  # truncating cast, like the reference
    return torch.stack([v, v, v, alpha], dim=-1)


def roberts(img: torch.Tensor) -> torch.Tensor:
    y = luma(img.cpu())
    yd = torch.cat([y[1:], y[-1:]], dim=0)  # clamp-to-edge neighbours
    yr = torch.cat([y[:, 1:], y[:, -1:]], dim=1)
    ydr = torch.cat([yd[:, 1:], yd[:, -1:]], dim=1)
    gx = ydr - y
    gy = yr - yd
    g = torch.sqrt(gx * gx + gy * gy)
    return _gray(g, img.cpu()[..., 3])


def roberts_rgb(img: torch.Tensor) -> torch.Tensor:
    """Per-channel Roberts cross, L1 magnitude, saturated; alpha kept."""
    x = img.cpu().to(torch.int32)
    xd = torch.cat([x[1:], x[-1:]], dim=0)
    xr = torch.cat([x[:, 1:], x[:, -1:]], dim=1)
    xdr = torch.cat([xd[:, 1:], xd[:, -1:]], dim=1)
    g = ((x - xdr).abs() + (xr - xd).abs()).clamp(max=255)
    g[..., 3] = x[..., 3]
    return g.to(torch.uint8)


def conv(img: torch.Tensor, filt: Filter) -> torch.Tensor:
    y = luma(img.cpu())
    up, down = filt.anchor, filt.k - 1 - filt.anchor
    yp = F.pad(y[None, None], (up, down, up, down), mode="replicate")
    dwx, dwy = filt.dense()  # separable filters: their K x K outer products, one direct sum
    wx = torch.tensor(dwx, dtype=torch.float32).reshape(1, 1, filt.k, filt.k)
    gx = F.conv2d(yp, wx)[0, 0]
    if filt.base_mode == MODE_MAG2:
        wy = torch.tensor(dwy, dtype=torch.float32).reshape(1, 1, filt.k, filt.k)
        gy = F.conv2d(yp, wy)[0, 0]
        g = torch.sqrt(gx * gx + gy * gy)
    elif filt.base_mode == MODE_ABS1:
        g = gx.abs()
    else:
        g = gx
    return _gray(g, img.cpu()[..., 3])


def vsub(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return a.cpu() - b.cpu()


def classify_dist(img: torch.Tensor, mu: np.ndarray, inv: np.ndarray, device=None,
                  chunk: int = 1 << 21) -> torch.Tensor:
    """fp64 quadratic forms (p - mu_c)^T A_c (p - mu_c) of every pixel and class,
    (N, C), computed in pixel chunks (an 8192^2 image x 32 classes would need
    51 GB at once) on ``device`` (default: the CPU) with plain torch ops."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    p_all = img.reshape(-1, 4)[:, :3]
    m = torch.as_tensor(mu, dtype=torch.float64, device=dev)
    A = torch.as_tensor(inv, dtype=torch.float64, device=dev)
    out = torch.empty((p_all.shape[0], m.shape[0]), dtype=torch.float64)
    for s0 in range(0, p_all.shape[0], chunk):
        p = p_all[s0:s0 + chunk].to(dev).to(torch.float64)
        d = p[:, None, :] - m[None, :, :]  # (n, C, 3)
        t = torch.einsum("ncj,cji->nci", d, A)
        out[s0:s0 + chunk] = (t * d).sum(-1).cpu()
    return out


def classify(img: torch.Tensor, mu: np.ndarray, inv: np.ndarray, device=None) -> torch.Tensor:
    """fp64 direct quadratic forms, strict-< argmin (lowest class on ties), NaN -> 255."""
    dist = classify_dist(img, mu, inv, device)
    # a class is a candidate only if dist < DBL_MAX (NaN and +inf never win)
    cand = dist < torch.finfo(torch.float64).max
    d2 = torch.where(cand, dist, torch.full_like(dist, float("inf")))
    cls = torch.argmin(d2, dim=1)  # first minimum = lowest class index
    a = torch.where(cand.any(dim=1), cls, torch.full_like(cls, 255)).to(torch.uint8)
    out = img.cpu().clone().reshape(-1, 4)
    out[:, 3] = a
    return out.reshape(img.shape)


def jacobi(u: torch.Tensor, r0: int, r1: int, keep_dtype: bool = False,
           rhs: torch.Tensor | None = None, omega: float | None = None,
           prev: torch.Tensor | None = None) -> torch.Tensor:
    """One sweep over rows [r0, r1) (1-based, halo rows at 0 and rows+1), in
    fp64, or with ``keep_dtype`` in u's own dtype: three correctly rounded adds
    in the kernels' association and an exact scale, so the native result must
    equal it bit for bit. ``rhs`` (u's shape; b = h^2 f of -Laplace(u) = f) is
    a fourth correctly rounded add after the neighbours:
    (((up + down) + (left + right)) + b) * 0.25.

    ``omega`` with ``prev`` (u's shape: the iterate before u): the Chebyshev
    step prev + omega * (s - prev) at the interior points of rows [r0, r1),
    with s the value above and omega rounded once to the working dtype: a
    subtract, a multiply and an add, each rounded. Every other element of the
    result is u's, as without omega."""
    u = u.cpu() if keep_dtype else u.cpu().to(torch.float64)
    un = u.clone()
    c = u[r0:r1, 1:-1]
    s = (u[r0 - 1:r1 - 1, 1:-1] + u[r0 + 1:r1 + 1, 1:-1]) + (u[r0:r1, :-2] + u[r0:r1, 2:])
    if rhs is not None:
        b = rhs.cpu().to(u.dtype)
        if b.shape != u.shape:
            raise ValueError("rhs must have u's shape")
        s = s + b[r0:r1, 1:-1]
    s = s * 0.25
    if (omega is None) != (prev is None):
        raise ValueError("omega and prev come together")
    if omega is not None:
        p = prev.cpu().to(u.dtype)
        if p.shape != u.shape:
            raise ValueError("prev must have u's shape")
        p = p[r0:r1, 1:-1]
        s = p + torch.tensor(omega, dtype=u.dtype) * (s - p)
    un[r0:r1, 1:-1] = s
    del c
    return un


def jacobi3d(u: torch.Tensor, k0: int, k1: int, keep_dtype: bool = False,
             rhs: torch.Tensor | None = None, omega: float | None = None,
             prev: torch.Tensor | None = None) -> torch.Tensor:
    """One 3-D sweep over planes [k0, k1) of a (planes + 2, ny, nx) slab (halo
    planes at 0 and planes + 1), in fp64, or with ``keep_dtype`` in u's own
    dtype, in the kernels' association:
    s = ((((zm + zp) + (ym + yp)) + (xm + xp)) [+ rhs]) * c with c = 1/6 rounded
    once to the working dtype and every operation rounded, so the native result
    must equal it bit for bit. ``omega`` with ``prev`` (u's shape: the iterate
    before u): prev + omega * (s - prev) at the interior points of the swept
    planes. Every other element of the result is u's."""
    u = u.cpu() if keep_dtype else u.cpu().to(torch.float64)
    if u.dim() != 3:
        raise ValueError("u must be a (planes + 2, ny, nx) tensor")
    un = u.clone()
    z, y, x = slice(k0, k1), slice(1, -1), slice(1, -1)
    s = ((u[k0 - 1:k1 - 1, y, x] + u[k0 + 1:k1 + 1, y, x]) + (u[z, :-2, x] + u[z, 2:, x])) + (u[z, y, :-2] + u[z, y, 2:])
    if rhs is not None:
        b = rhs.cpu().to(u.dtype)
        if b.shape != u.shape:
            raise ValueError("rhs must have u's shape")
        s = s + b[z, y, x]
    s = s * torch.tensor(1.0 / 6.0, dtype=u.dtype)
    if (omega is None) != (prev is None):
        raise ValueError("omega and prev come together")
    if omega is not None:
        p = prev.cpu().to(u.dtype)
        if p.shape != u.shape:
            raise ValueError("prev must have u's shape")
        p = p[z, y, x]
        s = p + torch.tensor(omega, dtype=u.dtype) * (s - p)
    un[z, y, x] = s
    return un


def mg_residual(u: torch.Tensor, rhs: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Multigrid residual in u's own dtype, in the kernels' association:
    r = ((((up + dn) + (l + rt)) [+ b]) - 4 c) at the interior points of an
    (H, W) grid. Every other element of the result is ``out``'s (zeros without
    ``out``): the kernels leave r's boundary alone."""
    u = u.cpu()
    r = torch.zeros_like(u) if out is None else out.cpu().to(u.dtype).clone()
    n = (u[:-2, 1:-1] + u[2:, 1:-1]) + (u[1:-1, :-2] + u[1:-1, 2:])
    if rhs is not None:
        b = rhs.cpu().to(u.dtype)
        if b.shape != u.shape:
            raise ValueError("rhs must have u's shape")
        n = n + b[1:-1, 1:-1]
    r[1:-1, 1:-1] = n - u[1:-1, 1:-1] * 4.0
    return r


def mg_restrict(r: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Full weighting of a fine (2 Hc - 1, 2 Wc - 1) residual into the coarse
    interior, scaled for the h^2-scaled coarse right-hand side, in r's dtype:
    bc = (r[i,j] + e*0.5) + d*0.25 with e = (n + s) + (w + e) and
    d = (nw + ne) + (sw + se), every operation rounded. Every other element of
    the (Hc, Wc) result is ``out``'s (zeros without ``out``)."""
    r = r.cpu()
    h, w = r.shape
    if h % 2 == 0 or w % 2 == 0 or h < 3 or w < 3:
        raise ValueError("fine grid must be (2 Hc - 1, 2 Wc - 1)")
    hc, wc = (h + 1) // 2, (w + 1) // 2
    bc = torch.zeros((hc, wc), dtype=r.dtype) if out is None else out.cpu().to(r.dtype).clone()
    if bc.shape != (hc, wc):
        raise ValueError("out must be the coarse grid")
    if hc < 3 or wc < 3:
        return bc
    c, up, dn = slice(2, -2, 2), slice(1, -3, 2), slice(3, -1, 2)
    e = (r[up, c] + r[dn, c]) + (r[c, up] + r[c, dn])
    d = (r[up, up] + r[up, dn]) + (r[dn, up] + r[dn, dn])
    bc[1:-1, 1:-1] = (r[c, c] + e * 0.5) + d * 0.25
    return bc


def mg_prolong_add(e: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """u plus the bilinear interpolation of the coarse e at u's interior, in u's
    dtype and the kernels' association (the vertical pair sums come first at
    the odd rows); u's boundary is returned unchanged."""
    u = u.cpu()
    e = e.cpu().to(u.dtype)
    hc, wc = e.shape
    if u.shape != (2 * hc - 1, 2 * wc - 1):
        raise ValueError("u must be (2 Hc - 1, 2 Wc - 1)")
    add = torch.zeros_like(u)
    v = e[:-1] + e[1:]  # (Hc - 1, Wc): e[I,J] + e[I+1,J]
    add[0::2, 0::2] = e
    add[0::2, 1::2] = (e[:, :-1] + e[:, 1:]) * 0.5
    add[1::2, 0::2] = v * 0.5
    add[1::2, 1::2] = (v[:, :-1] + v[:, 1:]) * 0.25
    out = u.clone()
    out[1:-1, 1:-1] = u[1:-1, 1:-1] + add[1:-1, 1:-1]
    return out


def _cubic_rows(c: torch.Tensor) -> torch.Tensor:
    """``mg_prolong_cubic``'s 1-D rule along the last dimension: (..., n) to
    (..., 2n - 1), every operation rounded in c's dtype."""
    n = c.shape[-1]
    if n >= 4:
        gl = ((c[..., 0] + c[..., 2]) * 4 - c[..., 3]) - c[..., 1] * 6
        gr = ((c[..., -1] + c[..., -3]) * 4 - c[..., -4]) - c[..., -2] * 6
    else:
        gl = (c[..., 0] - c[..., 1]) * 3 + c[..., 2]
        gr = (c[..., 2] - c[..., 1]) * 3 + c[..., 0]
    x = torch.cat([gl.unsqueeze(-1), c, gr.unsqueeze(-1)], dim=-1)
    a = x[..., 1:-2] + x[..., 2:-1]
    o = x[..., :-3] + x[..., 3:]
    out = torch.empty(c.shape[:-1] + (2 * n - 1,), dtype=c.dtype)
    out[..., 0::2] = c
    out[..., 1::2] = (a + (a - o) * 0.125) * 0.5
    return out


def mg_prolong_cubic(c: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """u with its interior replaced by the cubic interpolation of the coarse c,
    in u's dtype and the kernels' order: the 1-D rule of ``ops.mg_prolong_cubic``
    along every coarse row, then down the columns of the interpolated rows;
    u's boundary is returned unchanged."""
    u = u.cpu()
    c = c.cpu().to(u.dtype)
    hc, wc = c.shape
    if hc < 3 or wc < 3 or u.shape != (2 * hc - 1, 2 * wc - 1):
        raise ValueError("u must be (2 Hc - 1, 2 Wc - 1) with Hc, Wc >= 3")
    full = _cubic_rows(_cubic_rows(c).t()).t()
    out = u.clone()
    out[1:-1, 1:-1] = full[1:-1, 1:-1]
    return out


def mg3_residual(u: torch.Tensor, rhs: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """3-D multigrid residual in u's own dtype, in the kernels' association:
    r = ((((zm + zp) + (ym + yp)) + (xm + xp)) [+ b]) - 6 c at the interior
    points of a (D, H, W) grid. Every other element of the result is ``out``'s
    (zeros without ``out``): the kernels leave r's boundary alone."""
    u = u.cpu()
    if u.dim() != 3:
        raise ValueError("u must be a (D, H, W) tensor")
    r = torch.zeros_like(u) if out is None else out.cpu().to(u.dtype).clone()
    c = slice(1, -1)
    n = ((u[:-2, c, c] + u[2:, c, c]) + (u[c, :-2, c] + u[c, 2:, c])) + (u[c, c, :-2] + u[c, c, 2:])
    if rhs is not None:
        b = rhs.cpu().to(u.dtype)
        if b.shape != u.shape:
            raise ValueError("rhs must have u's shape")
        n = n + b[c, c, c]
    r[c, c, c] = n - u[c, c, c] * 6.0
    return r


def mg3_restrict(r: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """27-point full weighting of a fine (2 Dc - 1, 2 Hc - 1, 2 Wc - 1) residual
    into the coarse interior, scaled for the h^2-scaled coarse right-hand side,
    in r's dtype and the kernels' separable association: P_k is ``mg_restrict``'s
    2-D rule in fine plane k, bc[K] = (P_2K + (P_2K-1 + P_2K+1) * 0.5) * 0.5,
    every operation rounded. Every other element of the (Dc, Hc, Wc) result is
    ``out``'s (zeros without ``out``)."""
    r = r.cpu()
    if r.dim() != 3 or any(s % 2 == 0 or s < 3 for s in r.shape):
        raise ValueError("fine grid must be (2 Dc - 1, 2 Hc - 1, 2 Wc - 1)")
    dc, hc, wc = ((s + 1) // 2 for s in r.shape)
    bc = torch.zeros((dc, hc, wc), dtype=r.dtype) if out is None else out.cpu().to(r.dtype).clone()
    if bc.shape != (dc, hc, wc):
        raise ValueError("out must be the coarse grid")
    if dc < 3 or hc < 3 or wc < 3:
        return bc
    c, up, dn = slice(2, -2, 2), slice(1, -3, 2), slice(3, -1, 2)
    q = r[1:-1]  # fine planes 1 .. D - 2: P[k - 1] is P_k
    e = (q[:, up, c] + q[:, dn, c]) + (q[:, c, up] + q[:, c, dn])
    d = (q[:, up, up] + q[:, up, dn]) + (q[:, dn, up] + q[:, dn, dn])
    P = (q[:, c, c] + e * 0.5) + d * 0.25
    bc[1:-1, 1:-1, 1:-1] = (P[1:-1:2] + (P[0:-2:2] + P[2::2]) * 0.5) * 0.5
    return bc


def mg3_prolong_add(e: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """u plus the trilinear interpolation of the coarse e at u's interior, in u's
    dtype and the kernels' association: unscaled pair sums in z, then y, then x,
    and one exact scale 0.5^(number of odd coordinates), with no multiply where
    it is 1; u's boundary is returned unchanged."""
    u = u.cpu()
    e = e.cpu().to(u.dtype)
    dc, hc, wc = e.shape
    if u.shape != (2 * dc - 1, 2 * hc - 1, 2 * wc - 1):
        raise ValueError("u must be (2 Dc - 1, 2 Hc - 1, 2 Wc - 1)")
    Z = torch.zeros((u.shape[0], hc, wc), dtype=u.dtype)
    Z[0::2] = e
    Z[1::2] = e[:-1] + e[1:]
    Y = torch.zeros((u.shape[0], u.shape[1], wc), dtype=u.dtype)
    Y[:, 0::2] = Z
    Y[:, 1::2] = Z[:, :-1] + Z[:, 1:]
    X = torch.zeros_like(u)
    X[:, :, 0::2] = Y
    X[:, :, 1::2] = Y[:, :, :-1] + Y[:, :, 1:]
    for oz in (0, 1):
        for oy in (0, 1):
            for ox in (0, 1):
                if oz + oy + ox:
                    X[oz::2, oy::2, ox::2] *= 0.5 ** (oz + oy + ox)
    out = u.clone()
    out[1:-1, 1:-1, 1:-1] = u[1:-1, 1:-1, 1:-1] + X[1:-1, 1:-1, 1:-1]
    return out


def mg3_prolong_cubic(c: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """u with its interior replaced by the tricubic interpolation of the coarse
    c, in u's dtype and the kernels' order: the 1-D rule of
    ``ops.mg_prolong_cubic`` along x in every coarse row, then along y down the
    columns of the interpolated rows, then along z through the interpolated
    planes; u's boundary is returned unchanged."""
    u = u.cpu()
    c = c.cpu().to(u.dtype)
    if c.dim() != 3 or min(c.shape) < 3 or u.shape != tuple(2 * n - 1 for n in c.shape):
        raise ValueError("u must be (2 Dc - 1, 2 Hc - 1, 2 Wc - 1) with Dc, Hc, Wc >= 3")
    full = _cubic_rows(c)
    full = _cubic_rows(full.transpose(1, 2)).transpose(1, 2)
    full = _cubic_rows(full.transpose(0, 2)).transpose(0, 2)
    out = u.clone()
    out[1:-1, 1:-1, 1:-1] = full[1:-1, 1:-1, 1:-1]
    return out
