"""Order-exact oracle of the image convolution (``ops.conv`` / ``mpx_conv``),
in numpy alone: no project code computes anything here.

It restates the numeric contract of ``native/src/cpu/cpu_kernels.c`` and the
header of ``native/src/kernels/edge.hip`` operation by operation, every one
rounded to fp32 on its own:

* luminance ``(0.299f * r + 0.587f * g) + 0.114f * b``: three products and two
  sums, no FMA;
* dense taps: one sequential ``fmaf`` chain from 0 in ``(dy, dx)`` row-major
  order (``gx`` and, for ``mag2``, ``gy``);
* separable taps (``mode | 16``, ``wx = hx + vx + (scale,)``): per input row a
  horizontal chain over ``dx``, per output a vertical chain over ``dy`` of
  those sums, then one multiply by the scale;
* finish: ``sqrtf(gx*gx + gy*gy)`` (two products, one sum, one correctly
  rounded root) for ``mag2``, ``fabsf(gx)`` for ``abs1``, ``gx`` for ``lin1``;
  clamp to [0, 255]; truncate;
* the gray byte goes to R, G and B; alpha is the pixel's own.

Column reads clamp to ``[0, w - 1]``, row reads to logical rows
``[y_lo, y_hi]``. Inputs, taps and sums are finite and far from overflow.
"""

import numpy as np

F32 = np.float32
MODE_MAG2, MODE_ABS1, MODE_LIN1, MODE_SEP = 0, 1, 2, 16


def fma32(a, b, c):
    """Correctly rounded fp32 ``a * b + c`` on arrays (round-to-odd in fp64).

    The product of two fp32 values is exact in fp64. TwoSum gives the exact
    error of adding ``c``; where it is nonzero and the fp64 sum is even, the
    sum moves one ulp toward the error, so it is the exact value rounded to
    odd. Rounding that to fp32 equals rounding the exact value, because fp64
    carries 53 >= 2 * 24 + 2 bits (also when the fp32 result is subnormal:
    its rounding point is then higher still above the fp64 sticky bit)."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(F32)


def luma(img):
    """fp32 luminance of (..., 4) uint8 pixels: three products, two sums."""
    r, g, b = (img[..., c].astype(F32) for c in range(3))
    return (F32(0.299) * r + F32(0.587) * g) + F32(0.114) * b


def _finish(base, gx, gy):
    if base == MODE_MAG2:
        g = np.sqrt(gx * gx + gy * gy)
    elif base == MODE_ABS1:
        g = np.abs(gx)
    else:
        g = gx
    assert np.isfinite(g).all()
    return np.clip(g, F32(0), F32(255)).astype(np.uint8)  # truncates


def conv_exact(img, k, anchor, mode, wx, wy=(), *, oy0, oy1, y_lo, y_hi, src_row0=0):
    """The ``(oy1 - oy0, w, 4)`` uint8 output rows of logical rows
    ``[oy0, oy1)``. ``img`` is a ``(rows, w, 4)`` uint8 buffer whose logical
    row 0 is buffer row ``src_row0``; ``mode`` is the library's encoding."""
    img = np.ascontiguousarray(np.asarray(img))
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4
    w = img.shape[1]
    base, sep = mode & 3, bool(mode & MODE_SEP)
    two = base == MODE_MAG2
    assert 1 <= k <= 7 and 0 <= anchor < k and base <= 2 and w > 0
    assert y_lo <= y_hi and y_lo <= oy0 < oy1 <= y_hi + 1
    assert 0 <= src_row0 + y_lo and src_row0 + y_hi < img.shape[0]
    n = 2 * k + 1 if sep else k * k
    wx = np.asarray(wx, np.float64).astype(F32)
    wy = np.asarray(wy, np.float64).astype(F32) if two else None
    assert wx.size == n and (not two or wy.size == n)

    lum = luma(img)
    ys = np.arange(oy0, oy1)
    xs = np.arange(w)
    # buffer row of window row dy, column of window column dx
    rows = [np.clip(ys + dy - anchor, y_lo, y_hi) + src_row0 for dy in range(k)]
    cols = [np.clip(xs + dx - anchor, 0, w - 1) for dx in range(k)]
    zero = np.zeros((oy1 - oy0, w), F32)
    filters = [wx, wy] if two else [wx]
    sums = []
    if sep:
        for t in filters:
            hs = np.zeros_like(lum)  # horizontal sums of every buffer row
            for dx in range(k):
                hs = fma32(t[dx], lum[:, cols[dx]], hs)
            acc = zero
            for dy in range(k):
                acc = fma32(t[k + dy], hs[rows[dy]], acc)
            sums.append(acc * t[2 * k])
    else:
        for t in filters:
            acc = zero
            for dy in range(k):
                for dx in range(k):
                    acc = fma32(t[dy * k + dx], lum[rows[dy]][:, cols[dx]], acc)
            sums.append(acc)
    gray = _finish(base, sums[0], sums[1] if two else None)
    out = np.empty((oy1 - oy0, w, 4), np.uint8)
    out[..., :3] = gray[..., None]
    out[..., 3] = img[src_row0 + oy0:src_row0 + oy1, :, 3]
    return out


def conv_image(img, k, anchor, mode, wx, wy=()):
    """``conv_exact`` of a whole image with clamp-to-edge borders."""
    h = np.asarray(img).shape[0]
    return conv_exact(img, k, anchor, mode, wx, wy, oy0=0, oy1=h, y_lo=0, y_hi=h - 1)


def clip_share(ref):
    """Share of the gray bytes of ``ref`` that sit at 0 or 255."""
    g = np.asarray(ref)[..., 0]
    return float(((g == 0) | (g == 255)).mean()) if g.size else 0.0
