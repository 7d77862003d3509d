"""The band conv kernels (conv_band4_kernel / band4_walk, conv_band16v_kernel)
across band modes, walk lengths, tap classes, guard rows, pitches and row
sources — every byte (alpha included) against the native CPU reference, which
tests/test_cpu_reference.py pins to the torch fp32 expression.

Shapes aimed at a launcher limit (the 32-row walk of the batched aprons) come
from ``mpx_conv_band_plan``, the query the launcher itself decides by, so they
keep aiming at the limit when the segment rule changes.

Input rule: a clipped output byte hides a wrong tap or apron value, so every
(filter, input) pair used here must leave at most 10 % of the reference's gray
bytes at 0 or 255 (``_ref_of`` asserts it on the reference output alone).
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.ops.filters import MODE_SEP

from .helpers import rand_img, smooth_img

CLIP_MAX = 0.10
BPA = 2048  # OPT bit 11: batched aprons (walks of at most 32 rows)
NAMED = ["roberts", "sobel3", "prewitt3", "scharr3", "laplace3", "box3", "sharpen3", "sobel5", "gauss5", "log5",
         "sobel5_dense", "gauss5_dense"]
# the named filters whose output does not clip on uniformly random pixels
RAND_OK = {"roberts", "sobel5", "gauss5", "box3", "sobel5_dense", "gauss5_dense"}


def _lib():
    return _native.lib()


@pytest.fixture
def band():
    """``band(mode, band_min=0)`` sets the band mode and minimum for this test;
    both are restored afterwards, also when the test fails."""
    L = _lib()
    saved_min, saved_mode = L.mpx_conv_set_band_min(-1), L.mpx_conv_set_band_mode(-1)

    def set_state(mode, band_min=0):
        if band_min is not None:
            L.mpx_conv_set_band_min(band_min)
        L.mpx_conv_set_band_mode(mode)

    try:
        yield set_state
    finally:
        L.mpx_conv_set_band_min(saved_min)
        L.mpx_conv_set_band_mode(saved_mode)


def plan(w, rows, k, anchor, resident=False, remote=False):
    """(kernel, seg, opt) of mpx_conv_band_plan under the current band state."""
    seg, opt = ctypes.c_int(-1), ctypes.c_int(-1)
    kern = _lib().mpx_conv_band_plan(w, rows, k, anchor, int(resident), int(remote), ctypes.byref(seg),
                                     ctypes.byref(opt))
    return kern, seg.value, opt.value


def expected_opt(mode, resident, walk):
    if mode == 1:
        return 0
    return (2 if mode == 2 or resident else 34) | (BPA if walk <= 32 else 0)


def largest_rows(pred, hi=1 << 22):
    """Largest rows in [1, hi) with pred(rows), for a pred that holds up to some row count."""
    assert pred(1) and not pred(hi)
    lo = 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


def clip_share(ref):
    g = ref[..., 0]
    return float(((g == 0) | (g == 255)).float().mean()) if g.numel() else 0.0


def assert_same(got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want).any(-1).nonzero()
    ys, xs = bad[:, -2], bad[:, -1]
    pytest.fail(f"{what}: {len(bad)} pixels differ, rows {int(ys.min())}..{int(ys.max())}, "
                f"columns {int(xs.min())}..{int(xs.max())}, first at {tuple(int(v) for v in bad[0])}")


_inputs = {}


def _ref_of(f, h, w, maker=smooth_img):
    """(image, CPU reference) of one (filter, shape), computed once and shared
    by every mode. The input of a (filter, width) is one 70-row image, the
    first seed whose reference meets the input rule; shorter images are its
    leading rows, each with a reference of its own. (The rule cannot hold on
    the few-pixel images themselves: where clamp-to-edge collapses the whole
    window the output is 0 whatever the pixels are, e.g. the last column of a
    one-row Roberts image, a quarter of a 1 x 4 image.)"""
    top = HEIGHTS[-1]
    key = (f.name, w, maker.__name__)
    if key not in _inputs:
        for seed in range(16):
            img = maker(top, w, seed=1000 * seed + w)
            ref = ops.conv(img, f)
            if clip_share(ref) <= CLIP_MAX:
                _inputs[key] = {top: (img, ref)}
                break
        else:
            pytest.fail(f"{f.name} {top}x{w}: no input with at most {CLIP_MAX:.0%} clipped gray bytes")
    per_h = _inputs[key]
    if h not in per_h:
        img = per_h[top][0][:h]
        per_h[h] = (img, ops.conv(img, f))
    return per_h[h]


def _scaled(build, lin):
    """A runtime-tap filter, its taps scaled on the CPU until a smooth probe
    image leaves at most half the clip budget (LIN1 taps sum to a positive value:
    a negative response would clip at 0)."""
    probe = smooth_img(70, 516, seed=3)
    best = None
    for e in range(-10, 4):
        f = build(2.0 ** -e)
        share = clip_share(ops.conv(probe, f))
        if best is None or share < best[0]:
            best = (share, f)
    assert best[0] <= CLIP_MAX / 2, (best[1].name, best[0])
    return best[1]


@functools.lru_cache(maxsize=None)
def runtime_filters():
    """Runtime tap classes on the band kernel: RuntimeTaps (dense) and
    RuntimeSepTaps, name -> Filter."""
    out = {}

    def taps(rng, n, positive):
        t = rng.standard_normal(n)
        return t * (1.0 if not positive or t.sum() > 0 else -1.0)

    for i, (k, anchor, mode) in enumerate([(2, 0, "mag2"), (3, 1, "mag2"), (3, 1, "abs1"), (3, 1, "lin1"),
                                           (5, 2, "mag2"), (5, 2, "abs1")]):
        rng = np.random.default_rng(100 + i)
        tx, ty = taps(rng, k * k, mode == "lin1"), taps(rng, k * k, False)
        name = f"rt_dense{k}_{mode}"
        out[name] = _scaled(lambda s, k=k, anchor=anchor, mode=mode, tx=tx, ty=ty, name=name: ops.Filter.custom(
            k, (tx * s).tolist(), (ty * s).tolist() if mode == "mag2" else (), anchor=anchor, mode=mode, name=name),
            mode == "lin1")
    # separable abs1 has no band instantiation (the direct kernel serves it): it
    # rides along so every band mode is shown to leave it alone
    for i, (k, mode) in enumerate([(3, "mag2"), (3, "lin1"), (5, "mag2"), (5, "lin1"), (3, "abs1")]):
        rng = np.random.default_rng(200 + i)
        hx, vx = taps(rng, k, mode == "lin1"), taps(rng, k, mode == "lin1")
        hy, vy = taps(rng, k, False), taps(rng, k, False)
        name = f"rt_sep{k}_{mode}"
        out[name] = _scaled(lambda s, hx=hx, vx=vx, hy=hy, vy=vy, mode=mode, name=name: ops.Filter.separable_custom(
            hx.tolist(), vx.tolist(), s, hy.tolist() if mode == "mag2" else (), vy.tolist() if mode == "mag2" else (),
            s, mode=mode, name=name), mode == "lin1")
    return out


RUNTIME = ["rt_dense2_mag2", "rt_dense3_mag2", "rt_dense3_abs1", "rt_dense3_lin1", "rt_dense5_mag2", "rt_dense5_abs1",
           "rt_sep3_mag2", "rt_sep3_lin1", "rt_sep5_mag2", "rt_sep5_lin1", "rt_sep3_abs1"]


def get(name):
    return runtime_filters()[name] if name.startswith("rt_") else ops.get_filter(name)


def on_band(f):
    """The filter's tap class has a band instantiation (separable abs1 has none)."""
    return not (f.mode & MODE_SEP and f.base_mode == 1)


# ---------------------------------------------------------------------------
# B1: the plan query (host arithmetic only: runs without a GPU)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("k,anchor", [(2, 0), (3, 1), (5, 2)])
def test_plan_batched_apron_limit(band, k, anchor, mode):
    """The largest image whose walks still take the batched aprons walks
    exactly 32 rows (lane 63's batch slot live); one row more leaves them."""
    band(mode)
    w = 260
    has = lambda rows: bool(plan(w, rows, k, anchor)[2] & BPA)  # noqa: E731
    rows = largest_rows(has)
    kern, seg, opt = plan(w, rows, k, anchor)
    assert kern == 1 and opt == expected_opt(mode, False, 32), (rows, seg, opt)
    assert seg + k - 1 == 32, (rows, seg)
    kern1, seg1, opt1 = plan(w, rows + 1, k, anchor)
    assert kern1 == 1
    assert not (opt1 & BPA) or seg1 + k - 1 == 33, (rows + 1, seg1, opt1)
    # the limit once more through the resident hint (mode 3 keeps plain loads then)
    assert plan(w, rows, k, anchor, resident=True)[2] == (2 | BPA)
    # and no walk anywhere below it is longer than 32 rows or without the bit
    for r in (1, 7, 8, 9, 2048, rows // 2, rows - 1):
        _, s, o = plan(w, r, k, anchor)
        assert s + k - 1 <= 32 and o & BPA, (r, s, o)


def test_plan_modes_and_thresholds(band):
    # the default minimum keeps images below 4 Mpx on the wave kernel
    band(3, band_min=None)
    assert plan(2048, 2047, 5, 2)[0] == 0
    assert plan(2048, 2048, 5, 2) == (1, 8, 34 | BPA)
    assert plan(4096, 4096, 5, 2) == (1, 16, 34 | BPA)
    band(1)
    for rows in (1, 70, 4096, 60000, 70000, 200000):
        for k, a in ((2, 0), (3, 1), (5, 2)):
            kern, seg, opt = plan(260, rows, k, a)
            assert (kern, opt) == (1, 0) and seg >= 8, (rows, k, seg, opt)
    band(0)
    assert plan(260, 70, 5, 2) == (0, 0, 0)
    assert plan(4096, 4096, 5, 2) == (0, 0, 0)
    for mode in (1, 2, 3, 4):
        band(mode)
        for w in (258, 261, 262, 263, 4095):
            assert plan(w, 4096, 5, 2)[0] == 0, (mode, w)
        # windows reaching more than two columns to a side have no band kernel
        assert plan(260, 70, 7, 3)[0] == 0 and plan(260, 70, 4, 0)[0] == 0
    band(4)
    assert plan(260, 70, 5, 2) == (2, 16, 2 | 64)
    assert plan(260, 70, 5, 2, resident=True)[0] == 2
    assert plan(260, 70, 5, 2, remote=True) == (1, 8, 34 | BPA)
    assert plan(260, 70, 3, 1) == (1, 8, 34 | BPA) and plan(260, 70, 2, 0) == (1, 8, 34 | BPA)


# ---------------------------------------------------------------------------
# B2: mode x tap class x strip shape
# ---------------------------------------------------------------------------
MODES = [(1, False), (2, False), (3, False), (3, True), (4, False)]
MODE_IDS = ["m1", "m2", "m3", "m3res", "m4"]
WIDTHS = (4, 8, 252, 256, 260, 512, 516)  # one lane, partial strip, one strip, +4 columns, two strips, two + partial
HEIGHTS = (1, 2, 5, 17, 33, 70)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMED + RUNTIME)
@pytest.mark.parametrize("mode,resident", MODES, ids=MODE_IDS)
def test_band_mode_tap_class_matrix(gpu, band, mode, resident, name):
    f = get(name)
    band(mode)
    for w in WIDTHS:
        for h in HEIGHTS:
            kern, seg, opt = plan(w, h, f.k, f.anchor, resident)
            if not on_band(f):
                pass  # the query speaks of windows, not tap classes: nothing to assert
            elif mode == 4 and (f.k, f.anchor) == (5, 2):
                assert (kern, opt) == (2, 2 | 64), (h, w)
            else:
                assert (kern, seg, opt) == (1, 8, expected_opt(mode, resident, 8 + f.k - 1)), (h, w)
            makers = (smooth_img, rand_img) if name in RAND_OK else (smooth_img,)
            for maker in makers:
                img, ref = _ref_of(f, h, w, maker)
                out = ops.conv(img.to(gpu), f, resident=resident).cpu()
                assert_same(out, ref, f"{name} mode {mode} resident {resident} {h}x{w} {maker.__name__}")


# ---------------------------------------------------------------------------
# B3: walk-length ladder
# ---------------------------------------------------------------------------
WALKS = (21, 27, 31, 32, 33, 36)
LADDER = {2: ["roberts"], 3: ["sobel3", "laplace3"], 5: ["sobel5", "gauss5", "sobel5_dense", "rt_sep5_mag2"]}
ANCHOR = {2: 0, 3: 1, 5: 2}
LADDER_CASES = [(k, walk, 260) for k in LADDER for walk in WALKS] + \
               [(k, walk, w) for k in LADDER for walk in (32, 33) for w in (8, 512)]


def rows_for_walk(w, k, walk):
    """A row count (from the query, band mode 2 or 3 set) whose segments walk
    `walk` rows and whose last segment is short."""
    a, s = ANCHOR[k], walk - k + 1
    rows = largest_rows(lambda r: plan(w, r, k, a)[1] <= s) - 3
    kern, seg, _ = plan(w, rows, k, a)
    assert kern == 1 and seg == s and rows % seg != 0, (w, k, walk, rows, seg)
    return rows


@functools.lru_cache(maxsize=None)
def _tall(w, rows):
    return smooth_img(rows, w, seed=w)


@pytest.mark.gpu
@pytest.mark.parametrize("k,walk,w", LADDER_CASES)
def test_band_walk_ladder(gpu, band, k, walk, w):
    """Walks of 21 .. 32 rows (batched aprons, up to lane 63's slot) and of 33
    and 36 rows (per-row aprons) in modes 1, 2, 3 and 3 + resident; w = 8 (one
    partial strip) and w = 512 (inside strips only, the right image edge at a
    strip's end) at the limit itself."""
    band(3)
    need = max(rows_for_walk(w, kk, ww) for kk, ww, w2 in LADDER_CASES if w2 == w)
    rows = rows_for_walk(w, k, walk)
    img = _tall(w, need)[:rows]
    img_g = img.to(gpu)
    for name in LADDER[k]:
        f = get(name)
        ref = ops.conv(img, f)
        assert clip_share(ref) <= CLIP_MAX, name
        ref_g = ref.to(gpu)
        for mode, resident in MODES[:4]:
            band(mode)
            kern, seg, opt = plan(w, rows, k, ANCHOR[k], resident)
            assert kern == 1 and seg + k - 1 == walk and opt == expected_opt(mode, resident, walk), (rows, seg, opt)
            out = torch.full_like(img_g, 0x5A)
            ops.conv(img_g, f, out=out, resident=resident)
            assert_same(out, ref_g, f"{name} mode {mode} resident {resident} {rows}x{w} seg {seg} opt {opt}")


# ---------------------------------------------------------------------------
# B4: guard rows, sub-ranges, pitch
# ---------------------------------------------------------------------------
def pattern(shape, mul, add):
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.int64) * mul + add) % 251).to(torch.uint8).reshape(shape)


GUARD_FILTERS = ["roberts", "sobel3", "sobel5", "sobel5_dense"]
SRC_ROWS = 64
# (rows, oy0): 1, 2, 3 and 5 segments of 8 rows, each with a short tail
RANGES = ((5, 7), (11, 3), (19, 2), (35, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("w", [260, 516])
@pytest.mark.parametrize("name", GUARD_FILTERS)
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_band_guard_rows_and_subranges(gpu, band, mode, name, w):
    """conv_rows sub-ranges of a 64-row buffer: the launch writes rows
    [out_row0 + oy0, out_row0 + oy1) and nothing else, and reads no row outside
    [y_lo, y_hi]."""
    f = get(name)
    band(mode)
    src = smooth_img(SRC_ROWS, w, seed=w + 1)
    src_g = src.to(gpu)
    fill = pattern((SRC_ROWS, w, 4), 37, 11)
    for src_row0 in (0, 2, 3):
        out_row0 = src_row0 + 5
        for nrows, oy0 in RANGES:
            oy1 = oy0 + nrows
            assert oy0 > 0 and src_row0 + oy1 + f.halo_down < SRC_ROWS
            assert plan(w, nrows, f.k, f.anchor)[0] == (2 if mode == 4 and f.k == 5 else 1)
            for clamp in ("tight", "mid", "loose"):
                y_lo, y_hi = {"tight": (oy0, oy1 - 1), "mid": (oy0 - 1, oy1),
                              "loose": (-src_row0, SRC_ROWS - 1 - src_row0)}[clamp]
                kw = dict(src_row0=src_row0, out_row0=out_row0, oy0=oy0, oy1=oy1, y_lo=y_lo, y_hi=y_hi)
                what = f"{name} mode {mode} w {w} {kw}"
                want = fill.clone()
                ops.conv_rows(src, want, f, **kw)
                lo, hi = out_row0 + oy0, out_row0 + oy1
                assert clip_share(want[lo:hi]) <= CLIP_MAX, what
                assert torch.equal(want[:lo], fill[:lo]) and torch.equal(want[hi:], fill[hi:])
                got = fill.to(gpu)
                ops.conv_rows(src_g, got, f, **kw)
                got = got.cpu()
                assert torch.equal(got[:lo], fill[:lo]) and torch.equal(got[hi:], fill[hi:]), what + ": guard rows"
                assert_same(got, want, what)
                # rows outside the clamp range hold other bytes: nothing may change
                other = src.clone()
                other[:src_row0 + y_lo] = pattern(other[:src_row0 + y_lo].shape, 29, 5)
                other[src_row0 + y_hi + 1:] = pattern(other[src_row0 + y_hi + 1:].shape, 31, 7)
                got2 = fill.to(gpu)
                ops.conv_rows(other.to(gpu), got2, f, **kw)
                assert_same(got2.cpu(), want, what + ": rows outside [y_lo, y_hi] re-poisoned")


def _conv_pitch(L, src, out, w, pitch, oy0, oy1, y_lo, y_hi, f):
    wx, wy = f.c_taps()
    args = (src.data_ptr(), out.data_ptr(), w, pitch, oy0, oy1, y_lo, y_hi, f.k, f.anchor, f.mode, wx, wy)
    if src.is_cuda:
        _native.check(L.mpx_conv(*args, _native.stream_of(src)))
    else:
        L.mpx_cpu_conv(*args)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [260, 516])
@pytest.mark.parametrize("name", GUARD_FILTERS)
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_band_pitch_wider_than_image(gpu, band, mode, name, w):
    """pitch > w through the C ABI: the padding columns of the output stay
    untouched and those of the source are never read."""
    L = _lib()
    f = get(name)
    band(mode)
    rows = 37
    img = smooth_img(rows, w, seed=w + 2)
    for pad in (4, 64):
        pitch = w + pad
        for oy0, oy1 in ((0, rows), (3, 30)):
            what = f"{name} mode {mode} w {w} pitch {pitch} rows [{oy0}, {oy1})"
            assert plan(w, oy1 - oy0, f.k, f.anchor)[0] == (2 if mode == 4 and f.k == 5 else 1)
            src = pattern((rows, pitch, 4), 41, 3)
            src[:, :w] = img
            fill = pattern((rows, pitch, 4), 37, 11)
            want = fill.clone()
            _conv_pitch(L, src, want, w, pitch, oy0, oy1, 0, rows - 1, f)
            assert clip_share(want[oy0:oy1, :w]) <= CLIP_MAX, what
            assert torch.equal(want[:, w:], fill[:, w:])
            got = fill.to(gpu)
            _conv_pitch(L, src.to(gpu), got, w, pitch, oy0, oy1, 0, rows - 1, f)
            got = got.cpu()
            assert torch.equal(got[:, w:], fill[:, w:]), what + ": output padding columns"
            assert torch.equal(got[:oy0], fill[:oy0]) and torch.equal(got[oy1:], fill[oy1:]), what + ": guard rows"
            assert_same(got, want, what)
            src2 = src.clone()
            src2[:, w:] = pattern((rows, pad, 4), 43, 9)
            got2 = fill.to(gpu)
            _conv_pitch(L, src2.to(gpu), got2, w, pitch, oy0, oy1, 0, rows - 1, f)
            assert_same(got2.cpu(), want, what + ": source padding re-poisoned")


# ---------------------------------------------------------------------------
# B5: row sources (mpx_conv_peer) in one process
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", [260, 512])
@pytest.mark.parametrize("name", GUARD_FILTERS)
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_band_row_sources_one_process(gpu, band, mode, name, w):
    """mpx_conv_peer with the upper / lower halo rows in buffers of their own
    (biased pointers, as parallel/peer.py passes its mailbox rows). The rows
    next to `own` in its allocation hold other bytes, so a halo row read
    through `in` shows. 1, 2, 3, 4 and 7 segments: from 3 on the boundary
    segments run first."""
    L = _lib()
    f = get(name)
    band(mode)
    wx, wy = f.c_taps()
    row_bytes = w * 4
    pad = 2
    for own_rows in (5, 13, 21, 29, 53):
        for sides in ("up", "dn", "both"):
            nu = f.halo_up if sides in ("up", "both") else 0
            nd = f.halo_down if sides in ("dn", "both") else 0
            if nu + nd == 0 or (sides == "both" and 0 in (nu, nd)):
                continue  # (roberts reads no row above: only its lower side exists)
            what = f"{name} mode {mode} w {w} own_rows {own_rows} {sides}"
            kern, seg, opt = plan(w, own_rows, f.k, f.anchor, remote=True)
            assert (kern, seg, opt) == (1, 8, expected_opt(3 if mode == 4 else mode, False, 8 + f.k - 1)), what
            img = smooth_img(nu + own_rows + nd, w, seed=own_rows + w)
            want = torch.empty((own_rows, w, 4), dtype=torch.uint8)
            ops.conv_rows(img, want, f, src_row0=nu, out_row0=0, oy0=0, oy1=own_rows, y_lo=-nu,
                          y_hi=own_rows - 1 + nd)
            assert clip_share(want) <= CLIP_MAX, what
            # own rows inside an allocation whose neighbouring rows are poison
            big = pattern((pad + own_rows + pad, w, 4), 29, 5)
            big[pad:pad + own_rows] = img[nu:nu + own_rows]
            big_g = big.to(gpu)
            own = big_g[pad:pad + own_rows]
            up_rows = img[:nu].contiguous().to(gpu) if nu else None
            dn_rows = img[nu + own_rows:].contiguous().to(gpu) if nd else None
            up = up_rows.data_ptr() + nu * row_bytes if nu else None
            dn = dn_rows.data_ptr() - own_rows * row_bytes if nd else None
            fill = pattern((pad + own_rows + pad, w, 4), 37, 11)
            out_g = fill.to(gpu)
            _native.check(L.mpx_conv_peer(own.data_ptr(), up, dn, own_rows, out_g[pad:].data_ptr(), w, w, 0, own_rows,
                                          -nu, own_rows - 1 + nd, f.k, f.anchor, f.mode, wx, wy,
                                          _native.stream_of(big_g)))
            out = out_g.cpu()
            assert torch.equal(out[:pad], fill[:pad]) and torch.equal(out[pad + own_rows:], fill[pad + own_rows:]), \
                what + ": guard rows"
            assert_same(out[pad:pad + own_rows], want, what)
