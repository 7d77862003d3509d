"""lab3 classifier against an exact integer oracle, on adversarial statistics.

Every other classifier test takes its statistics from ops.class_stats on an
image and compares the GPU with mpx_cpu_classify (the same FMA chain). Here the
statistics are hand-made and exactly representable: means on a 2^-6 grid,
inverse covariances at integer x 2^-s. Every operation of the reference fp64
chain is then exact (helpers.exact_dist asserts the bit budget), so the true
class, the exact top-2 margin and the exact ties of every pixel come from
int64 numpy alone, independently of any project code.

The families drive the branches of the host bound builders that generated
statistics never reach (asymmetric A, Cholesky refusal, means outside the
colour cube, one common f16 scale / int8 unit over classes 2^14 apart, tiny
weights next to a large pivot, an int8 unit that has to double); the images
hold every value a product feature can take (pair_cube) and decided, undecided
and exactly tied pixels interleaved lane by lane (clouds)."""

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import ops

from .helpers import G, exact_dist
from .test_classify_f16 import emulate as emulate_f16
from .test_classify_f16 import f16_params
from .test_classify_i8 import emulate as emulate_i8
from .test_classify_i8 import i8_params

PATHS = ("direct", "fast", "mfma", "mfma64", "mfma8", "mfma16", "auto")


# ---------------------------------------------------------------------------
# statistic families: (mu_grid (nc, 3) int64, A_int (nc, 3, 3) int64, s)
# ---------------------------------------------------------------------------
def _pd(rng):
    """L L^T of an integer lower-triangular L: diagonal in [4, 16), the rest in [-15, 15]."""
    L = np.tril(rng.integers(-15, 16, (3, 3)), -1) + np.diag(rng.integers(4, 16, 3))
    return L @ L.T


def _cube_means(rng, nc):
    return rng.integers(0, 255 * G + 1, (nc, 3))


def fam_generic(nc):
    rng = np.random.default_rng(1000 + nc)
    return _cube_means(rng, nc), np.stack([_pd(rng) for _ in range(nc)]), 10


def fam_mixed_scale():
    """Class k's A is PD x 4^k: 2^14 between classes under one f16 scale and one int8 unit."""
    rng = np.random.default_rng(2)
    return _cube_means(rng, 8), np.stack([_pd(rng) * 4**k for k in range(8)]), 20


def fam_outside():
    rng = np.random.default_rng(3)
    mu = rng.integers(-64 * G, 320 * G, (6, 3))
    mu[0] = 0
    mu[1] = 255 * G
    return mu, np.stack([_pd(rng) for _ in range(6)]), 10


def fam_far():
    """Means 1500 to 2000 from the cube centre in every channel: the constant
    term and the slots together outgrow the int8 key budget at the smallest
    unit, so build_i8 has to double its unit u (with means in [-64, 320) they
    can never fill 2^26, whatever the matrices)."""
    rng = np.random.default_rng(15)
    mu = 128 * G + rng.choice([-1, 1], (4, 3)) * rng.integers(1500 * G, 2000 * G, (4, 3))
    return mu, np.stack([_pd(rng) for _ in range(4)]), 10


def fam_skew():
    """PD plus a skew-symmetric part: the chain uses A as given, the fast paths (A + A^T) / 2."""
    rng = np.random.default_rng(4)
    A = []
    for _ in range(5):
        K = np.triu(rng.integers(-300, 301, (3, 3)), 1)
        A.append(_pd(rng) + K - K.T)
    return _cube_means(rng, 5), np.stack(A), 10


def fam_illcond():
    """L D L^T, L unit lower-triangular, D = one pivot of 1024 among ones."""
    rng = np.random.default_rng(5)
    A = []
    for c in range(4):
        L = np.tril(rng.integers(-15, 16, (3, 3)), -1) + np.eye(3, dtype=np.int64)
        D = np.ones(3, np.int64)
        D[c % 3] = 1024
        A.append(L @ np.diag(D) @ L.T)
    return _cube_means(rng, 4), np.stack(A), 20


def fam_indefinite():
    rng = np.random.default_rng(6)
    A = np.stack([_pd(rng) for _ in range(4)])
    A[2] = np.diag([5, -3, 7])
    return _cube_means(rng, 4), A, 10


def fam_twins():
    """Three twin pairs (one A, means 1, 2 and 8 grid steps apart in one
    channel), a mirror pair (diag A, means 10 apart in r: exact ties on the
    plane of integer r half-way) and two unrelated classes."""
    rng = np.random.default_rng(11)
    mu, A = [], []
    for ch, steps in enumerate((1, 2, 8)):
        a = _pd(rng)
        m = rng.integers(40 * G, 215 * G, 3)
        m2 = m.copy()
        m2[ch] += steps
        mu += [m, m2]
        A += [a, a]
    m = rng.integers(40, 205, 3) * G
    mu += [m, m + np.array([10 * G, 0, 0])]
    A += [np.diag([300, 200, 250])] * 2
    for _ in range(2):
        mu.append(rng.integers(0, 255 * G + 1, 3))
        A.append(_pd(rng))
    return np.stack(mu), np.stack(A), 10


# ---------------------------------------------------------------------------
# images: (N, 4) uint8, N odd and above several 4096-pixel one-shot blocks
# ---------------------------------------------------------------------------
THIRD = (0, 1, 127, 128, 129, 254, 255)


def img_pair_cube():
    """Per channel pair all 65536 value pairs x the third channel in THIRD
    (every value of every product feature, all eight cube corners), plus seven
    repeated pixels so that N is no multiple of 4."""
    rng = np.random.default_rng(11)
    a, b, t = np.meshgrid(np.arange(256), np.arange(256), np.array(THIRD), indexing="ij")
    blocks = []
    for i, j, k in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
        blk = np.empty(a.shape + (3,), np.uint8)
        blk[..., i], blk[..., j], blk[..., k] = a, b, t
        blocks.append(blk.reshape(-1, 3))
    rgb = np.concatenate(blocks)
    rgb = np.concatenate([rgb, rgb[rng.integers(0, rgb.shape[0], 7)]])
    assert rgb.shape[0] == 3 * 7 * 65536 + 7
    return np.concatenate([rgb, rng.integers(0, 256, (rgb.shape[0], 1), dtype=np.uint8)], 1)


def img_uniform():
    return np.random.default_rng(12).integers(0, 256, ((1 << 18) + 5, 4), dtype=np.uint8)


def img_clouds(mu_grid):
    """70 % round(mean + N(0, 10)) around one of the first eight means, the
    rest uniform; shuffled, so that decided, undecided and tied pixels alternate
    lane by lane."""
    rng = np.random.default_rng(13)
    n = (1 << 18) + 5
    px = rng.integers(0, 256, (n, 4))
    near = rng.random(n) < 0.7
    centre = mu_grid[rng.integers(0, 8, n)] / G
    cloud = np.rint(centre + rng.normal(0.0, 10.0, (n, 3)))
    px[near, :3] = np.clip(cloud, 0, 255)[near]
    return rng.permutation(px.astype(np.uint8))


# (family, nc, image); generic at 4 and 32 classes takes pair_cube, its other counts uniform
CASES = [("generic", 4, "pair_cube"), ("generic", 32, "pair_cube"), ("mixed_scale", 8, "pair_cube"),
         ("outside", 6, "pair_cube"), ("skew", 5, "pair_cube")]
CASES += [("generic", nc, "uniform") for nc in (1, 2, 5, 16, 17)]
CASES += [("illcond", 4, "uniform"), ("indefinite", 4, "uniform"), ("far", 4, "uniform"), ("twins", 10, "clouds")]
CASE_IDS = [f"{f}{nc}-{im}" if f == "generic" else f"{f}-{im}" for f, nc, im in CASES]
TWINS = ("twins", 10, "clouds")
GENERIC4_UNIFORM = ("generic", 4, "uniform")  # the small interlude of the state-reuse test

# (family, requested path) pairs that no bound can be proven for: planned direct
EXPECTED_DIRECT = {("indefinite", p) for p in PATHS}  # expand_classes: a Cholesky pivot of diag(5, -3, 7) is <= 0

_FAMILIES = {"mixed_scale": fam_mixed_scale, "outside": fam_outside, "far": fam_far, "skew": fam_skew,
             "illcond": fam_illcond, "indefinite": fam_indefinite, "twins": fam_twins}
_IMAGES = {}
_ORACLE = {}


class Oracle:
    """One (family, image): statistics, image, and per pixel the exact class,
    best / second distance and margin (int64, in units of 2^-s / G^2)."""

    def __init__(self, family, nc, image):
        self.family, self.nc = family, nc
        self.mu_grid, self.A_int, self.s = fam_generic(nc) if family == "generic" else _FAMILIES[family]()
        assert self.mu_grid.shape == (nc, 3) and self.A_int.shape == (nc, 3, 3)
        self.mu = self.mu_grid / float(G)
        self.inv = self.A_int / float(2**self.s)
        assert np.array_equal(self.mu * G, self.mu_grid) and np.array_equal(self.inv * 2**self.s, self.A_int)
        self.unit = float(G * G * 2**self.s)
        if image == "clouds":
            px = img_clouds(self.mu_grid)
        else:
            if image not in _IMAGES:
                _IMAGES[image] = img_pair_cube() if image == "pair_cube" else img_uniform()
            px = _IMAGES[image]
        self.n = n = px.shape[0]
        assert n % 4 != 0 and n > 8 * 4096
        # kept for the whole session: the input (shared by the cases of one image; never written, the tests
        # clone or upload it), the expected output, and the margin and runner-up distance
        self.img = torch.from_numpy(px).reshape(1, n, 4)
        want = px.copy()
        self.cls = want[:, 3]  # the class, as a view of the expected alpha
        # one class has no runner-up: nothing ties, everything is decided
        self.margin = np.full(n, np.iinfo(np.int64).max)
        self.q2 = np.zeros(n, np.int64)
        self.any_negative = False
        for a in range(0, n, 1 << 17):
            dist = exact_dist(px[a:a + (1 << 17), :3], self.mu_grid, self.A_int)
            b = a + dist.shape[0]
            self.cls[a:b] = dist.argmin(1)  # first minimum = the reference's strict '<'
            self.any_negative |= bool((dist < 0).any())
            if nc > 1:
                two = np.partition(dist, 1, axis=1)
                self.q2[a:b] = two[:, 1]
                self.margin[a:b] = two[:, 1] - two[:, 0]
        self.want = torch.from_numpy(want).reshape(1, n, 4)

    @property
    def tie(self):
        return self.margin == 0

    def near(self, t2):
        """Pixels a fast / mfma margin test may leave undecided: exact margin
        <= 2 T2 + 2^-15 (Q2 + 3 T2). Each fp32 value is within T2 / 2 of the
        exact distance plus a common bias <= 2 T2; the class tag costs a key at
        most 2^-18 of its value and decided() asks 1.125 2^-17 of it on top of
        T2: a larger exact margin is always decided."""
        if self.nc == 1:
            return np.zeros(self.n, bool)
        m, q2 = self.margin / self.unit, self.q2 / self.unit  # exact: below 2^52, the unit a power of two
        return m <= 2.0 * t2 + 2.0**-15 * (q2 + 3.0 * t2)


def oracle(case):
    if case not in _ORACLE:
        _ORACLE[case] = Oracle(*case)
    return _ORACLE[case]


def planned(case, path):
    family, nc, _ = case
    if (family, path) in EXPECTED_DIRECT:
        return "direct"
    if path == "auto":
        return "mfma16" if nc >= 4 else "fast"
    return path


def margin_tested(case, path):
    """Pixels of the image that `path` puts through a margin test: the rest (a
    tail shorter than one work unit of the path) goes to the direct kernel,
    which counts nothing. The units are those of the launcher (classify_impl
    in native/src/kernels/classify.hip: `done = ...` of each path's branch:
    fast 4 * kFastNQ pixels, mfma 128-pixel and mfma64 64-pixel chunks, mfma8
    one 16-B vector up to kMfma8sMaxClasses = 13 classes and 128-pixel chunks
    above, mfma16 one vector) and must follow it. For twins / clouds the tail
    holds no tie (asserted with the image's statistics), so there the bound is
    the number of ALL exact ties."""
    o = oracle(case)
    p = planned(case, path)
    unit = {"direct": o.n, "fast": 8, "mfma": 128, "mfma64": 64, "mfma8": 4 if o.nc <= 13 else 128, "mfma16": 4}[p]
    return o.n - o.n % unit


# ---------------------------------------------------------------------------
# CPU: oracle = library chain, the plan table, the emulations
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + [GENERIC4_UNIFORM], ids=CASE_IDS + ["generic4-uniform"])
def test_cpu_chain_equals_oracle(case):
    o = oracle(case)
    got = o.img.clone()
    ops.classify_(got, o.mu, o.inv)
    bad = (got[0, :, 3].numpy() != o.want[0, :, 3].numpy())
    assert not bad.any(), f"{bad.sum()} pixels, first {np.flatnonzero(bad)[:5]}"
    assert torch.equal(got, o.want)
    if case[0] == "indefinite":
        assert o.any_negative and (o.cls == 2).any()  # negative distances do occur and win


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_plan_table(case):
    o = oracle(case)
    for path in PATHS:
        got, margin = ops.classify_plan(o.mu, o.inv, path)
        assert got == planned(case, path), (path, got)
        assert (margin > 0) == (got != "direct"), (path, margin)


def test_clouds_statistics_from_the_oracle_alone():
    """The twins / clouds image really holds the interleaved mixture the GPU
    tests rely on; no kernel runs here."""
    o = oracle(TWINS)
    t2 = ops.classify_plan(o.mu, o.inv, "fast")[1]
    ties = o.tie.mean()
    near = (o.margin / o.unit <= t2 / 4).mean()
    decided = 1.0 - o.near(t2).mean()
    wins = np.bincount(o.cls, minlength=o.nc) / o.n
    print(f"clouds: ties {ties:.4%} near {near:.2%} decided {decided:.2%} min class share {wins.min():.2%} T2 {t2:.4g}")
    assert ties >= 0.002
    assert near >= 0.10
    assert decided >= 0.25
    assert wins.min() >= 0.01
    # shuffled: the ties are spread over the whole image, not gathered in one run
    assert np.diff(np.flatnonzero(o.tie)).max() < 8192
    # the scalar tail every path hands to the (uncounted) direct kernel holds no tie,
    # so each path's ambiguity counter is bounded below by ALL exact ties
    assert not o.tie[o.n - o.n % 128:].any()


EMULATED = [c for c in CASES if c[0] in ("mixed_scale", "outside", "skew", "illcond", "far", "twins")]
EMULATED_IDS = [CASE_IDS[CASES.index(c)] for c in EMULATED]


@pytest.mark.parametrize("case", EMULATED, ids=EMULATED_IDS)
def test_f16_emulation_decides_only_oracle_classes(case):
    o = oracle(case)
    rc, w, c, t2 = f16_params(o.mu, o.inv)
    assert rc == 0
    assert np.all(w[o.nc:] == 0) and np.all(c[o.nc:] == np.float32(3e38))
    tie, ndec = o.tie, 0
    for a in range(0, o.n, 1 << 16):  # every pixel of the family's image
        sel = slice(a, min(a + (1 << 16), o.n))
        cls, decided = emulate_f16(o.img[0, sel], w, c, t2, o.nc)  # asserts every accumulator > 0
        bad = decided & (cls != o.cls[sel])
        assert not bad.any(), f"{bad.sum()} decided pixels differ from the oracle, first {a + np.flatnonzero(bad)[:5]}"
        assert not (decided & tie[sel]).any(), "an exact tie passed the margin test"
        ndec += int(decided.sum())
    print(f"{case[0]}: f16 emulation decides {ndec / o.n:.2%}")


@pytest.mark.parametrize("case", EMULATED, ids=EMULATED_IDS)
def test_i8_emulation_decides_only_oracle_classes(case):
    o = oracle(case)
    rc, a8, b8, c, t2 = i8_params(o.mu, o.inv)
    assert rc == 0
    assert np.all(a8[o.nc:] == 0) and np.all(b8[o.nc:] == 0) and np.all(c[o.nc:] == (1 << 26) - 64)
    tie, ndec = o.tie, 0
    for a in range(0, o.n, 1 << 16):  # every pixel of the family's image
        sel = slice(a, min(a + (1 << 16), o.n))
        cls, decided = emulate_i8(o.img[0, sel], a8, b8, c, t2, o.nc)  # asserts no int32 key overflow
        bad = decided & (cls != o.cls[sel])
        assert not bad.any(), f"{bad.sum()} decided pixels differ from the oracle, first {a + np.flatnonzero(bad)[:5]}"
        assert not (decided & tie[sel]).any(), "an exact tie passed the margin test"
        ndec += int(decided.sum())
    print(f"{case[0]}: int8 emulation decides {ndec / o.n:.2%}")


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_equals_oracle(gpu, case, path):
    """The whole output equals the oracle image (RGB unchanged, alpha = class)
    and the ambiguity counter lies within its derived bounds."""
    o = oracle(case)
    d = o.img.to(gpu)
    amb = torch.zeros(1, dtype=torch.int32, device=gpu)
    ops.classify_(d, o.mu, o.inv, path=path, ambiguous=amb)
    got = d.cpu()
    count = int(amb.item())
    n = margin_tested(case, path)
    ties = int((o.margin[:n] == 0).sum())
    upper = None
    if planned(case, path) in ("fast", "mfma"):  # auto below 4 classes is fast, with fast's T2
        upper = int(o.near(ops.classify_plan(o.mu, o.inv, path)[1])[:n].sum())
    print(f"{CASE_IDS[CASES.index(case)]} {path}: ambiguous {count}, exact ties {ties}, upper bound {upper}, of {o.n}")
    bad = got[0, :, 3].numpy() != o.want[0, :, 3].numpy()
    assert not bad.any(), f"{bad.sum()} pixels, first {np.flatnonzero(bad)[:5]}"
    assert torch.equal(got, o.want)
    if planned(case, path) == "direct":
        assert count == 0
    else:
        assert count >= ties, "a tied pixel was decided by rounding"
    if upper is not None:
        assert count <= upper
    if o.nc == 1:
        # the runner-up of a single class is a padded class's sentinel (3e38, 1e300, or the int8 keys'
        # 2^26 - 64), farther from any real value than every margin: nothing can be undecided
        assert count == 0


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["mfma16", "auto"])
def test_gpu_state_reuse_on_one_stream(gpu, path):
    """twins / clouds (a large deferral list), generic nc = 4 on uniform (a
    nearly empty one), twins again, all on one stream: the deferral list's
    alternating counter sets and the cached parameters carry nothing over."""
    stream = torch.cuda.Stream(device=gpu)
    outs = []
    with torch.cuda.stream(stream):
        for case in (TWINS, GENERIC4_UNIFORM, TWINS):
            o = oracle(case)
            d = o.img.to(gpu)
            ops.classify_(d, o.mu, o.inv, path=path)
            outs.append((d, o))
    stream.synchronize()
    for i, (d, o) in enumerate(outs):
        assert torch.equal(d.cpu(), o.want), i
