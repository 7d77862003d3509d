"""The image convolution against an order-exact oracle (tests/conv_oracle.py:
numpy only, no project code): every byte, alpha included, of

* the CPU reference (``ops.conv`` on CPU tensors, ``mpx_cpu_conv`` through
  ctypes for pitches and row ranges the Python layer never passes), and
* the wave and direct GPU kernels (``conv_wave_kernel``,
  ``conv_direct_kernel``) at the wave kernel's strip edges (W1), segment
  counts (W2), buffer layouts (W3), row ranges and row sources (W4), every
  (k, anchor) pair of the direct kernel (D1) and extreme images (X1).

The GPU comparisons never involve the CPU library. The band kernel is left to
tests/test_conv_band.py, whose CPU reference this module pins to the oracle.

Input rule (as in test_conv_band.py): a clipped output byte hides a wrong tap
or a wrong pixel, so on every smooth image of at least 256 pixels at most 10 %
of the ORACLE's gray bytes may sit at 0 or 255; ``ref_of`` asserts it before
anything is compared. Random custom taps are scaled by a power of two chosen
with the oracle alone. The uniformly random images are there for the clipped
and saturated pixels and stand outside the rule.
"""

import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops

from .conv_oracle import clip_share, conv_exact, conv_image, fma32
from .helpers import rand_img, smooth_img

CLIP_MAX = 0.10
RULE_MIN_PIXELS = 256
MODES = ("mag2", "abs1", "lin1")


def gray_img(h, w, seed=0):
    """A smooth image with r = g = b: the luminance is then within an ulp of an
    integer, and the sums of taps on a coarse grid within a few ulps of a
    multiple of the grid step, where the truncation to a byte tells one fp32
    rounding from another (another tap order, a product rounded before the
    sum) that on other pixels changes a byte once in 10^5."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    v = 128 + 100 * torch.sin(xx / 17.0) * torch.cos(yy / 23.0) + torch.randn((h, w), generator=g) * 2
    v = torch.clamp(v, 0, 255).to(torch.uint8)
    a = torch.randint(0, 256, (h, w), dtype=torch.uint8, generator=g)
    return torch.stack([v, v, v, a], -1).contiguous()


MAKERS = {"smooth": smooth_img, "rand": rand_img, "gray": gray_img}
RULED = ("smooth", "gray")  # the makers under the input rule
# output columns per wave strip (edge::WaveGeom: 128 - even left pad - even right pad)
OW = {(2, 0): 126, (3, 1): 124, (5, 2): 124, (7, 3): 120}
WINDOWS = tuple(OW)
NAMED_OF = {(2, 0): ["roberts"], (3, 1): ["sobel3", "prewitt3", "scharr3", "laplace3", "box3", "sharpen3"],
            (5, 2): ["sobel5", "gauss5", "log5", "sobel5_dense", "gauss5_dense"], (7, 3): []}
# the largest share the input rule met in this process: [share, what]
worst_clip = [0.0, ""]


def _lib():
    return _native.lib()


# ---------------------------------------------------------------------------
# inputs, filters and oracle results, each computed once per process
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def image(maker, h, w, seed=None):
    return MAKERS[maker](h, w, seed=1000 * h + w if seed is None else seed)


def _note_clip(ref, what):
    share = clip_share(ref)
    if share > worst_clip[0]:
        worst_clip[:] = [share, what]
    assert share <= CLIP_MAX, f"input rule: {what}: {share:.1%} of the oracle's gray bytes are clipped"


@functools.lru_cache(maxsize=None)
def ref_of(f, maker, h, w, seed=None):
    """(image, oracle output) of a whole image, both torch uint8 (h, w, 4)."""
    img = image(maker, h, w, seed)
    ref = conv_image(img.numpy(), f.k, f.anchor, f.mode, f.wx, f.wy)
    if maker in RULED and h * w >= RULE_MIN_PIXELS:
        _note_clip(ref, f"{f.name} {maker} {h}x{w}")
    return img, torch.from_numpy(ref)


def _taps(rng, n, positive, grid):
    if grid:  # small integers, not all zero
        t = rng.integers(-1 if positive else -4, 5, n).astype(np.float64)
        t[0] += float(not t.any() or (positive and t.sum() <= 0))
        return t
    t = rng.standard_normal(n)
    if positive:  # lin1: a negative response would clip at 0; the sum becomes half the L1 norm
        t = t + (0.5 * np.abs(t).sum() - t.sum()) / n
    return t


def _custom(k, anchor, mode, sep, grid, attempt):
    base = MODES.index(mode)
    rng = np.random.default_rng([k, anchor, base, int(sep), int(grid), attempt])
    two, lin = mode == "mag2", mode == "lin1"
    name = f"{'sep' if sep else 'dense'}{k}a{anchor}_{mode}{'_grid' if grid else ''}"
    if sep:
        hx, vx = _taps(rng, k, lin, grid), _taps(rng, k, lin, grid)
        hy, vy = _taps(rng, k, False, grid), _taps(rng, k, False, grid)

        def build(s):
            return ops.Filter.separable_custom(hx.tolist(), vx.tolist(), s, hy.tolist() if two else (),
                                               vy.tolist() if two else (), s, anchor=anchor, mode=mode, name=name)
    else:
        tx, ty = _taps(rng, k * k, lin, grid), _taps(rng, k * k, False, grid)

        def build(s):
            return ops.Filter.custom(k, (tx * s).tolist(), (ty * s).tolist() if two else (), anchor=anchor, mode=mode,
                                     name=name)
    probe = image("gray" if grid else "smooth", 21, 65, 7).numpy()
    best = None
    for e in range(-6, 11):
        f = build(2.0 ** -e)
        share = clip_share(conv_image(probe, f.k, f.anchor, f.mode, f.wx, f.wy))
        if best is None or share < best[0]:
            best = (share, f)
    return best


@functools.lru_cache(maxsize=None)
def custom(k, anchor, mode, sep, grid=False):
    """Runtime taps of one (window, mode, layout): random normal ones, or
    (grid) small integers for the gray images. Either way scaled by the power
    of two that leaves the fewest clipped bytes in the oracle's output of a
    probe image: the first draw that stays under half the cap."""
    for attempt in range(8):
        share, f = _custom(k, anchor, mode, sep, grid, attempt)
        if share <= CLIP_MAX / 2:
            return f
    pytest.fail(f"no taps for {f.name} under half the clip cap")


def makers_for(f):
    """Named filters run on every maker; grid taps are made for the gray
    images, random taps for the others."""
    if f.name.endswith("_grid"):
        return ("gray",)
    return tuple(MAKERS) if f.name in ops.list_filters() else ("smooth", "rand")


def get(name):
    return ops.get_filter(name)


def tap_class_names(window):
    """The wave kernel's tap classes of a window: the compile-time taps of
    every named filter, runtime dense taps per mode, runtime separable taps."""
    runtime = ["dense_mag2", "dense_abs1", "dense_lin1", "dense_lin1_grid"]
    if window[0] != 2:  # (separable 2 x 2 taps take the direct kernel)
        runtime += ["sep_mag2", "sep_lin1", "sep_lin1_grid"]
    return NAMED_OF[window] + runtime


def tap_class(window, name):
    if name in NAMED_OF[window]:
        return get(name)
    layout, mode, *grid = name.split("_")
    return custom(*window, mode, layout == "sep", bool(grid))


TAP_CLASSES = [(w, n) for w in WINDOWS for n in tap_class_names(w)]


def pattern(shape, mul, add):
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.int64) * mul + add) % 251).to(torch.uint8).reshape(shape)


def assert_same(got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want).any(-1).nonzero()
    ys, xs = bad[:, -2], bad[:, -1]
    y, x = int(bad[0][-2]), int(bad[0][-1])
    pytest.fail(f"{what}: {len(bad)} pixels differ, rows {int(ys.min())}..{int(ys.max())}, "
                f"columns {int(xs.min())}..{int(xs.max())}, first at ({y}, {x}): got {got[y, x].tolist()} "
                f"want {want[y, x].tolist()}")


# ---------------------------------------------------------------------------
# C1: fma32 against exact rational arithmetic
# ---------------------------------------------------------------------------
def rn32(q):
    """(v, tie): the fp32 value nearest to the Fraction q, ties to even,
    subnormals included, by integer arithmetic on the Fraction; tie tells
    whether q lay exactly between two fp32 values."""
    if q == 0:
        return 0.0, False
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    e = max(e, -126)
    t = q / Fraction(2) ** (e - 23)
    n = t.numerator // t.denominator
    r = t - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    assert n <= 1 << 24 and e < 120
    return sign * math.ldexp(n, e - 23), r == Fraction(1, 2)


def _fma_triples():
    rng = np.random.default_rng(2024)
    f32 = np.float32

    def rnd(n, emin, emax):
        m = rng.integers(1 << 23, 1 << 24, n).astype(np.float64) * rng.choice([-1.0, 1.0], n)
        return np.ldexp(m, rng.integers(emin, emax, n) - 23).astype(f32)

    parts = []
    # random mantissas, exponents up to 2^60 apart (sticky bits far below fp64's last)
    parts.append((rnd(9000, -30, 30), rnd(9000, -30, 30), rnd(9000, -60, 60)))
    # massive cancellation: c is minus the rounded product, or a neighbour of it
    a, b = rnd(3000, -20, 20), rnd(3000, -20, 20)
    c = -(a.astype(np.float64) * b.astype(np.float64)).astype(f32)
    step = rng.integers(-1, 2, 3000)
    c = np.where(step > 0, np.nextafter(c, f32(np.inf)), np.where(step < 0, np.nextafter(c, f32(-np.inf)), c))
    parts.append((a, b, c.astype(f32)))
    # a*b + c exactly between two fp32 values: c plus an odd multiple of half its ulp
    c = rnd(3000, -20, 20)
    e = np.frexp(c)[1] - 1  # c = 1.x * 2^e, ulp 2^(e-23)
    m = (2 * rng.integers(0, 1 << 11, 3000) + 1).astype(np.float64) * rng.choice([-1.0, 1.0], 3000)
    parts.append((m.astype(f32), np.ldexp(1.0, e - 24).astype(f32), c))
    # ... and a hair to either side of such a midpoint: half an ulp times
    # (1 +- 2^-28) (one fp64 ulp of the sum) or (1 +- 2^-46) (far below it)
    assert 17 * 15790321 == 2**28 + 1 and 16383 * 16385 == 2**28 - 1
    assert 8392705 * 8384513 == 2**46 + 1 and (2**23 + 1) * (2**23 - 1) == 2**46 - 1
    for fa, fb, bits in ((17, 15790321, 28), (16383, 16385, 28), (8392705, 8384513, 46), (2**23 + 1, 2**23 - 1, 46)):
        c = rnd(1200, -20, 20)
        e = np.frexp(c)[1] - 1
        sgn = rng.choice([-1.0, 1.0], 1200)
        parts.append(((fa * sgn).astype(f32), np.ldexp(float(fb), e - 24 - bits).astype(f32), c))
    # results in the fp32 subnormal range: random, exact midpoints, a hair off them
    parts.append((rnd(1500, -80, -60), rnd(1500, -80, -60), rnd(1500, -150, -126)))
    csub = (rng.integers(-(1 << 22), 1 << 22, 1500).astype(np.float64) * 2.0 ** -149).astype(f32)
    parts.append((np.full(500, 2.0 ** -75, f32) * rng.choice([-1, 1], 500).astype(f32), np.full(500, 2.0 ** -75, f32),
                  csub[:500]))
    parts.append((np.full(500, 17 * 2.0 ** -90, f32), np.full(500, 15790321 * 2.0 ** -88, f32), csub[500:1000]))
    parts.append((np.full(500, -16383 * 2.0 ** -90, f32), np.full(500, 16385 * 2.0 ** -88, f32), csub[1000:]))
    a, b, c = (np.concatenate([p[i] for p in parts]) for i in range(3))
    assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()
    return a, b, c


def test_fma32_is_correctly_rounded():
    a, b, c = _fma_triples()
    assert a.size >= 20000
    got = fma32(a, b, c)
    assert got.dtype == np.float32
    seen = {"tie": 0, "subnormal": 0, "cancel": 0, "inexact": 0}
    bad = []
    for i in range(a.size):
        fa, fb, fc = Fraction(float(a[i])), Fraction(float(b[i])), Fraction(float(c[i]))
        q = fa * fb + fc
        want, tie = rn32(q)
        if float(got[i]) != want:
            bad.append((float(a[i]).hex(), float(b[i]).hex(), float(c[i]).hex(), float(got[i]).hex(), want.hex()))
        seen["tie"] += tie
        seen["subnormal"] += 0 < abs(q) < Fraction(2) ** -126
        seen["cancel"] += q != 0 and abs(q) * 2 ** 20 < abs(fc)
        seen["inexact"] += Fraction(want) != q
    assert not bad, (len(bad), bad[:5])
    # the constructed families are what they claim to be
    assert seen["tie"] >= 3000 and seen["subnormal"] >= 2500 and seen["cancel"] >= 1500, seen
    assert seen["inexact"] >= 15000, seen


def test_fma32_differs_from_two_roundings():
    """The oracle's chain is a real FMA: on the midpoint family a separate
    fp32 multiply and add gives other bits."""
    a, b, c = _fma_triples()
    two_step = (a * b + c).astype(np.float32)
    assert (two_step != fma32(a, b, c)).sum() > 1000


# ---------------------------------------------------------------------------
# C2: ops.conv on CPU tensors
# ---------------------------------------------------------------------------
def _cpu_shapes(k):
    return [s for s in ((1, 1), (2, 3), (k - 1, k + 1), (21, 19)) if s[0] > 0]  # (k = 1: no 0-row image)


@pytest.mark.parametrize("name", sum(NAMED_OF.values(), []))
def test_cpu_named_filters(name):
    assert set(sum(NAMED_OF.values(), [])) == set(ops.list_filters())
    f = get(name)
    assert (f.k, f.anchor) in NAMED_OF and name in NAMED_OF[(f.k, f.anchor)]
    for h, w in _cpu_shapes(f.k) + [(33, 130)]:
        for maker in makers_for(f):
            img, ref = ref_of(f, maker, h, w)
            assert_same(ops.conv(img, f), ref, f"{name} {maker} {h}x{w}")


@pytest.mark.parametrize("grid", [False, True], ids=["normal", "grid"])
@pytest.mark.parametrize("sep", [False, True], ids=["dense", "sep"])
@pytest.mark.parametrize("k", range(1, 8))
def test_cpu_every_window_and_mode(k, sep, grid):
    for anchor in range(k):
        for mode in MODES:
            f = custom(k, anchor, mode, sep, grid)
            for h, w in _cpu_shapes(k):
                for maker in makers_for(f):
                    img, ref = ref_of(f, maker, h, w)
                    assert_same(ops.conv(img, f), ref, f"{f.name} {maker} {h}x{w}")


# ---------------------------------------------------------------------------
# layouts and row ranges through the C entries (CPU part C3, GPU parts W3 / W4)
# ---------------------------------------------------------------------------
def _c_conv(f, in_ptr, out_ptr, w, pitch, oy0, oy1, y_lo, y_hi, stream=None, direct=False):
    wx, wy = f.c_taps()
    args = (in_ptr, out_ptr, w, pitch, oy0, oy1, y_lo, y_hi, f.k, f.anchor, f.mode, wx, wy)
    L = _lib()
    if stream is None:
        L.mpx_cpu_conv(*args)
    else:
        _native.check((L.mpx_conv_direct if direct else L.mpx_conv)(*args, stream))


def range_cases(rows):
    """name -> (src_row0, oy0, oy1, y_lo, y_hi) over a buffer of `rows` rows."""
    return {
        "whole": (0, 0, rows, 0, rows - 1),
        "subrange": (0, 3, rows - 4, 0, rows - 1),                  # oy0 > 0, oy1 < h
        "resident_halo": (2, 0, rows - 4, -2, rows - 4 + 1),        # halo rows above row 0 and past the last
        "all_clamped": (0, 3, rows - 4, 3, rows - 5),               # every halo read clamps
    }


@functools.lru_cache(maxsize=None)
def layout_case(f, maker, rows, w, pitch, case, shift_in=0, shift_out=0):
    """Backing buffers of one C-entry launch: ``(src, fill, want, in_off,
    out_off, args)``. ``src`` and ``fill`` are flat byte buffers of
    `shift_in` / `shift_out` pixels, then `rows` rows of `pitch` pixels,
    patterned everywhere the image is not; ``want`` is ``fill`` with the
    oracle's rows stored, so comparing the whole buffer checks padding, rows
    outside [oy0, oy1) and the bytes in front of a shifted base as well. The
    offsets are those of logical row 0, in bytes."""
    src_row0, oy0, oy1, y_lo, y_hi = range_cases(rows)[case]
    img = image(maker, rows, w, 31 * rows + w)
    ref = conv_exact(img.numpy(), f.k, f.anchor, f.mode, f.wx, f.wy, oy0=oy0, oy1=oy1, y_lo=y_lo, y_hi=y_hi,
                     src_row0=src_row0)
    if maker in RULED and ref.shape[0] * w >= RULE_MIN_PIXELS:
        _note_clip(ref, f"{f.name} {maker} {rows}x{w} {case}")
    src = pattern(((shift_in + rows * pitch) * 4,), 41, 3)
    src[shift_in * 4:].view(rows, pitch, 4)[:, :w] = img
    fill = pattern(((shift_out + rows * pitch) * 4,), 37, 11)
    want = fill.clone()
    want[shift_out * 4:].view(rows, pitch, 4)[src_row0 + oy0:src_row0 + oy1, :w] = torch.from_numpy(ref)
    return (src, fill, want, (shift_in + src_row0 * pitch) * 4, (shift_out + src_row0 * pitch) * 4,
            (w, pitch, oy0, oy1, y_lo, y_hi))


def assert_layout(got, want, shift, rows, pitch, what):
    if torch.equal(got, want):
        return
    assert torch.equal(got[:shift * 4], want[:shift * 4]), f"{what}: bytes in front of the base pointer changed"
    assert_same(got[shift * 4:].view(rows, pitch, 4), want[shift * 4:].view(rows, pitch, 4), what)


def layout_filters():
    return [get("sobel3"), get("sobel5"), get("laplace3"), custom(7, 3, "mag2", False), custom(7, 3, "lin1", True),
            custom(4, 1, "abs1", False), custom(2, 1, "mag2", True), custom(6, 5, "lin1", False),
            custom(5, 2, "lin1", False, True), custom(3, 1, "abs1", True, True)]


@pytest.mark.parametrize("case", list(range_cases(21)))
def test_cpu_c_entry_pitch_and_row_ranges(case):
    """mpx_cpu_conv with pitch = w + 3 inside patterned backing buffers."""
    rows, w = 21, 19
    for f in layout_filters():
        for maker in makers_for(f):
            src, fill, want, in_off, out_off, args = layout_case(f, maker, rows, w, w + 3, case)
            got = fill.clone()
            _c_conv(f, src.data_ptr() + in_off, got.data_ptr() + out_off, *args)
            assert_layout(got, want, 0, rows, w + 3, f"{f.name} {maker} {case}")


# ---------------------------------------------------------------------------
# extreme images (CPU part C4, GPU part X1)
# ---------------------------------------------------------------------------
def extreme_images(h, w):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    checker = (((yy + xx) % 2) * 255).to(torch.uint8)[..., None].expand(h, w, 4).contiguous()
    corners = torch.full((h, w, 4), 16, dtype=torch.uint8)
    for y in (0, h - 1):
        for x in (0, w - 1):
            corners[y, x] = torch.tensor([255, 250, 245, 9 + y + x], dtype=torch.uint8)
    ramp = smooth_img(h, w, seed=5)
    ramp[..., 3] = ((3 * xx + 7 * yy) % 256).to(torch.uint8)  # alpha differs between any two pixels of a window
    return {"zeros": torch.zeros((h, w, 4), dtype=torch.uint8), "ones": torch.full((h, w, 4), 255, dtype=torch.uint8),
            "checker": checker, "corners": corners, "alpha_ramp": ramp}


def extreme_filters():
    return [get("gauss5"), get("box3"), custom(7, 3, "mag2", False), get("sobel5"), custom(4, 1, "lin1", False),
            custom(6, 0, "mag2", True)]


@functools.lru_cache(maxsize=None)
def extreme_ref(f, kind, h, w):
    img = extreme_images(h, w)[kind]
    return img, torch.from_numpy(conv_image(img.numpy(), f.k, f.anchor, f.mode, f.wx, f.wy))


EXTREME_KINDS = ("zeros", "ones", "checker", "corners", "alpha_ramp")


@pytest.mark.parametrize("kind", EXTREME_KINDS)
def test_cpu_extreme_images(kind):
    for f in extreme_filters():
        for h, w in ((9, 21), (1, 1), (2, 3)):
            img, ref = extreme_ref(f, kind, h, w)
            assert_same(ops.conv(img, f), ref, f"{f.name} {kind} {h}x{w}")
    if kind == "alpha_ramp":  # the alpha is the pixel's own, whatever the anchor
        img, ref = extreme_ref(custom(6, 0, "mag2", True), kind, 9, 21)
        assert torch.equal(ref[..., 3], img[..., 3])


# ---------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------
def plan(w, rows, k, anchor, resident=False, remote=False):
    """Kernel of mpx_conv_band_plan under the current band state (0 = wave)."""
    seg, opt = ctypes.c_int(-1), ctypes.c_int(-1)
    return _lib().mpx_conv_band_plan(w, rows, k, anchor, int(resident), int(remote), ctypes.byref(seg),
                                     ctypes.byref(opt))


def on_wave(f):
    return (f.k, f.anchor) in OW and not (f.separable and (f.base_mode == 1 or f.k == 2))


def gpu_conv(gpu, img, f, direct=False):
    """ops.conv on the GPU into a patterned output, so a pixel never written shows."""
    h, w = img.shape[:2]
    if not direct and on_wave(f):
        assert plan(w, h, f.k, f.anchor) == 0, "meant for the wave kernel"
    out = pattern((h, w, 4), 37, 11).to(gpu)
    ops.conv(img.to(gpu), f, out=out, direct=direct)
    return out.cpu()


def strip_widths(window):
    ow = OW[window]
    return [1, 2, 3, ow - 1, ow, ow + 1, ow + 2, 2 * ow - 1, 2 * ow, 2 * ow + 1, 2 * ow + 2]


def segment_heights(k):
    # one partial 8-row segment .. exactly one .. one and a row .. two .. three
    # (boundary segments first, one walking up) .. four
    return sorted({1, 2, k - 1, k, 7, 8, 9, 16, 17, 25} - {0})


def w1_cases(window, name):
    """(filter, [(maker, h, w)]) of one W1 test."""
    f = tap_class(window, name)
    ow = OW[window]
    shapes = [(m, 9, w) for w in strip_widths(window) for m in makers_for(f)]
    shapes += [(makers_for(f)[0], h, w) for h in segment_heights(window[0]) if h != 9 for w in (ow + 1, 2 * ow + 2)]
    return f, shapes


@pytest.mark.gpu
@pytest.mark.parametrize("window,name", TAP_CLASSES, ids=[f"k{w[0]}-{n}" for w, n in TAP_CLASSES])
def test_wave_strip_edges(gpu, window, name):
    """W1: one column, one pair, below / at / past one strip and two strips,
    even widths on the 8-byte pair loads and odd ones on the per-pixel loads,
    for every tap class of the window."""
    f, shapes = w1_cases(window, name)
    assert on_wave(f)
    for maker, h, w in shapes:
        img, ref = ref_of(f, maker, h, w)
        assert_same(gpu_conv(gpu, img, f), ref, f"{f.name} {maker} {h}x{w}")


def w2_cases(window):
    k, a = window
    named = {(2, 0): "roberts", (3, 1): "sobel3", (5, 2): "log5", (7, 3): None}[window]
    fs = [get(named) if named else custom(k, a, "abs1", False)]
    if k != 2:
        fs.append(get("sobel5") if k == 5 else custom(k, a, "mag2", True))
    ow = OW[window]
    return fs, [(h, w) for h in segment_heights(k) for w in (ow + 1, 2 * ow + 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("window", WINDOWS, ids=[f"k{w[0]}" for w in WINDOWS])
def test_wave_segments(gpu, window):
    """W2: 1 .. 4 segments of 8 rows with short tails, on images of their own
    (seeded apart from W1's), one dense and one separable filter."""
    fs, shapes = w2_cases(window)
    for f in fs:
        assert on_wave(f)
        for h, w in shapes:
            for maker in makers_for(f):
                img, ref = ref_of(f, maker, h, w, 77 * h + w)
                assert_same(gpu_conv(gpu, img, f), ref, f"{f.name} {maker} {h}x{w}")


def w3_filters(window):
    k, a = window
    return [custom(k, a, "mag2", False), custom(k, a, "lin1", True), custom(k, a, "lin1", False, True)] + \
        ([get("sobel3")] if k == 3 else [])


# (pitch - w, shift of `in`, shift of `out`) in pixels -> the loads the launcher must pick
W3_LAYOUTS = {"pitch_even": (2, 0, 0), "pitch_odd": (3, 0, 0), "in_shifted": (2, 1, 0), "out_shifted": (2, 0, 1),
              "both_shifted": (0, 1, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(W3_LAYOUTS))
@pytest.mark.parametrize("window", [(3, 1), (7, 3)], ids=["k3", "k7"])
def test_wave_layouts_through_c_entry(gpu, window, layout):
    """W3: even w with pitch = w + 2 (pair loads), an odd pitch, and `in` or
    `out` starting 4 bytes into its buffer (per-pixel loads); nothing but the
    output rows' own pixels may change."""
    rows, w = 17, OW[window] + 2
    pad, shift_in, shift_out = W3_LAYOUTS[layout]
    pitch = w + pad
    for f in w3_filters(window):
        assert plan(w, rows, f.k, f.anchor) == 0
        for maker in makers_for(f):
            src, fill, want, in_off, out_off, args = layout_case(f, maker, rows, w, pitch, "whole", shift_in, shift_out)
            src_g, got_g = src.to(gpu), fill.to(gpu)
            assert src_g.data_ptr() % 16 == 0 and got_g.data_ptr() % 16 == 0
            _c_conv(f, src_g.data_ptr() + in_off, got_g.data_ptr() + out_off, *args, stream=_native.stream_of(src_g))
            assert_layout(got_g.cpu(), want, shift_out, rows, pitch, f"{f.name} {maker} {layout}")


def w4_filters(window):
    k, a = window
    named = {(3, 1): ["sobel3"], (5, 2): ["sobel5", "gauss5_dense"], (7, 3): []}[window]
    return [get(n) for n in named] + [custom(k, a, "mag2", False), custom(k, a, "lin1", True),
                                      custom(k, a, "abs1", False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["subrange", "resident_halo", "all_clamped"])
@pytest.mark.parametrize("window", [(3, 1), (5, 2), (7, 3)], ids=["k3", "k5", "k7"])
def test_wave_row_ranges(gpu, window, case):
    """W4: a sub-range, resident halo rows and an all-clamping range over a
    27-row buffer (three segments), at an odd width, which never plans onto
    the band kernel, and an even one. The whole output buffer is compared."""
    rows = 27
    for w in (OW[window] + 1, OW[window] + 2):
        for f in w4_filters(window):
            for maker in makers_for(f):
                src, fill, want, in_off, out_off, args = layout_case(f, maker, rows, w, w, case)
                assert plan(w, args[3] - args[2], f.k, f.anchor) == 0
                src_g, got_g = src.to(gpu), fill.to(gpu)
                _c_conv(f, src_g.data_ptr() + in_off, got_g.data_ptr() + out_off, *args,
                        stream=_native.stream_of(src_g))
                assert_layout(got_g.cpu(), want, 0, rows, w, f"{f.name} {maker} w {w} {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("window", [(5, 2), (7, 3)], ids=["k5", "k7"])
def test_wave_row_sources(gpu, window):
    """W4: mpx_conv_peer with the upper and lower halo rows in buffers of
    their own (biased pointers); the rows next to `own` in its allocation are
    patterned, so a halo row read through `in` shows."""
    L = _lib()
    w, own_rows, pad = OW[window] + 1, 19, 3
    for f in w4_filters(window):
        nu, nd = f.halo_up, f.halo_down
        assert plan(w, own_rows, f.k, f.anchor, remote=True) == 0
        for maker in makers_for(f):
            img = image(maker, nu + own_rows + nd, w, 5 * w + f.k)
            ref = conv_exact(img.numpy(), f.k, f.anchor, f.mode, f.wx, f.wy, oy0=0, oy1=own_rows, y_lo=-nu,
                             y_hi=own_rows - 1 + nd, src_row0=nu)
            if maker in RULED:
                _note_clip(ref, f"{f.name} peer {own_rows}x{w}")
            big = pattern((pad + own_rows + pad, w, 4), 29, 5)
            big[pad:pad + own_rows] = img[nu:nu + own_rows]
            big_g = big.to(gpu)
            up_rows, dn_rows = img[:nu].contiguous().to(gpu), img[nu + own_rows:].contiguous().to(gpu)
            fill = pattern((pad + own_rows + pad, w, 4), 37, 11)
            want = fill.clone()
            want[pad:pad + own_rows] = torch.from_numpy(ref)
            out_g = fill.to(gpu)
            wx, wy = f.c_taps()
            _native.check(L.mpx_conv_peer(big_g[pad:].data_ptr(), up_rows.data_ptr() + nu * w * 4,
                                          dn_rows.data_ptr() - own_rows * w * 4, own_rows, out_g[pad:].data_ptr(), w, w,
                                          0, own_rows, -nu, own_rows - 1 + nd, f.k, f.anchor, f.mode, wx, wy,
                                          _native.stream_of(big_g)))
            assert_same(out_g.cpu(), want, f"{f.name} {maker} peer")


def d1_shapes(k):
    small = [s for s in ((1, 1), (2, 3), (k - 1, k + 1)) if s[0] > 0]
    return small + [(h, w) for h in (3, 4, 5) for w in (63, 64, 65)]  # around the 64 x 4 launch block


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [False, True], ids=["normal", "grid"])
@pytest.mark.parametrize("sep", [False, True], ids=["dense", "sep"])
@pytest.mark.parametrize("k", range(1, 8))
def test_direct_every_window_and_mode(gpu, k, sep, grid):
    """D1: every (k, anchor) pair and mode through ops.conv (the direct kernel
    for all but the four centred windows, and for separable abs1); the centred
    windows once more with direct=True."""
    for anchor in range(k):
        for mode in MODES:
            f = custom(k, anchor, mode, sep, grid)
            for h, w in d1_shapes(k):
                for maker in makers_for(f):
                    img, ref = ref_of(f, maker, h, w)
                    what = f"{f.name} {maker} {h}x{w}"
                    assert_same(gpu_conv(gpu, img, f), ref, what)
                    if (k, anchor) in OW:
                        assert_same(gpu_conv(gpu, img, f, direct=True), ref, what + " direct")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", EXTREME_KINDS)
def test_gpu_extreme_images(gpu, kind):
    """X1: all 0, all 255, the period-1 checkerboard (the largest |gx|), bright
    corners and an alpha ramp, on the wave kernel (one strip and a column) and
    on the direct kernel."""
    for f in extreme_filters():
        w = OW.get((f.k, f.anchor), 124) + 1
        img, ref = extreme_ref(f, kind, 9, w)
        if on_wave(f):
            assert_same(gpu_conv(gpu, img, f), ref, f"{f.name} {kind} wave")
        assert_same(gpu_conv(gpu, img, f, direct=True), ref, f"{f.name} {kind} direct")
