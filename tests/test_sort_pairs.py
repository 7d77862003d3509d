"""Stable key-value sort and argsort (ops.sort_pairs_, ops.argsort, ops.sort;
mpx_sort_pairs_ws / mpx_cpu_sort_pairs).

The oracle is independent of the library: numpy's stable argsort of the
order-preserving uint32 key (int32: sign flip; float32: the IEEE total order
of the bit patterns), complemented for descending order. Indices and key
bytes must be exactly equal. A full-range random array almost never has
duplicates, so the `ties` family (at most 7 distinct values; floats include
0.0, -0.0 and a NaN) is the one that exercises stability, and `range1000`
(one digit holds every key in three passes) the hot-digit ranking.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from cuda_mpi_openmp_amd import _native, ops
from cuda_mpi_openmp_amd.ops.sort import read_fixture

from .helpers import ROOT
from .test_lab5_sort import random_array

LAB5_DATA = os.path.join(ROOT, "labs", "lab5", "data")
TORCH_DT = {"int": torch.int32, "float": torch.float32}
MPX_DT = {"int": 0, "float": 1}
IOTA, DESCENDING = 1, 2

INT_TIES = np.array([-2**31, -5, -1, 0, 7, 0x12345678, 2**31 - 1], dtype=np.int32)
FLOAT_TIES = np.array([0.0, -0.0, np.nan, 1.5, -1.5, np.inf, -np.inf], dtype=np.float32)


def make_keys(kind, family, n, seed):
    rng = np.random.default_rng(seed)
    if family == "uniform":
        return random_array(kind, n, seed)
    if family == "ties":
        return rng.choice(INT_TIES if kind == "int" else FLOAT_TIES, n)
    assert family == "range1000" and kind == "int"
    return rng.integers(0, 1000, n, dtype=np.int64).astype(np.int32)


def oracle_perm(a: np.ndarray, descending: bool) -> np.ndarray:
    """numpy's stable argsort of the order-preserving key (complemented for
    descending: equal keys keep their input order in both directions)."""
    u = a.view(np.uint32)
    if a.dtype == np.float32:
        key = np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))
    else:
        key = u ^ np.uint32(0x80000000)
    if descending:
        key = ~key
    return np.argsort(key, kind="stable").astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(kind, family, n, descending):
    """(keys, oracle permutation) of one case; computed once, never modified."""
    a = make_keys(kind, family, n, seed=n + 17)
    perm = oracle_perm(a, descending)
    a.setflags(write=False)
    perm.setflags(write=False)
    return a, perm


def check_sort_and_argsort(a, perm, descending, device):
    x = torch.from_numpy(a.copy()).to(device)
    idx = ops.argsort(x, descending=descending)
    assert idx.dtype == torch.int32 and idx.shape == x.shape
    assert x.cpu().numpy().tobytes() == a.tobytes()  # argsort leaves x untouched
    assert np.array_equal(idx.cpu().numpy(), perm)
    vals, idx2 = ops.sort(x, descending=descending)
    assert x.cpu().numpy().tobytes() == a.tobytes()
    assert np.array_equal(idx2.cpu().numpy(), perm)
    assert vals.dtype == x.dtype and vals.cpu().numpy().tobytes() == a[perm].tobytes()


# ---------------------------------------------------------------- CPU ----

@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("family", ["uniform", "ties"])
@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 10, 1000, 4097, 200_003])
def test_cpu_sort_pairs_matches_stable_oracle(n, kind, family, descending):
    """mpx_cpu_sort_pairs (n >= 2^16: the OpenMP run-sort + merge path on the
    64-bit composites) through ops.argsort / ops.sort and ops.sort_pairs_."""
    a, perm = case(kind, family, n, descending)
    check_sort_and_argsort(a, perm, descending, "cpu")
    payload = np.random.default_rng(n).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    k, v = torch.from_numpy(a.copy()), torch.from_numpy(payload.copy())
    rk, rv = ops.sort_pairs_(k, v, descending=descending)
    assert rk is k and rv is v
    assert k.numpy().tobytes() == a[perm].tobytes()
    assert v.numpy().tobytes() == payload[perm].tobytes()


@pytest.mark.parametrize("kind,asc,desc", [
    ("int", [0, 9, 8, 7, 6, 5, 4, 3, 2, 1], [1, 2, 3, 4, 5, 6, 7, 8, 9, 0]),
    ("float", [0, 9, 8, 7, 6, 5, 4, 3, 2, 1], [1, 2, 3, 4, 5, 6, 7, 8, 9, 0]),
    ("uchar", [0, 3, 6, 1, 4, 7, 2, 5, 8, 9], [9, 2, 5, 8, 1, 4, 7, 0, 3, 6]),
])
def test_cpu_argsort_of_the_lab5_fixtures(kind, asc, desc):
    """Stability pinned by hand: uchar10 is [1,2,3,1,2,3,1,2,3,4], so equal
    keys must come out in input order, ascending and descending."""
    x = torch.from_numpy(read_fixture(os.path.join(LAB5_DATA, kind + "10"), kind))
    assert ops.argsort(x).tolist() == asc
    assert ops.argsort(x, descending=True).tolist() == desc
    vals, idx = ops.sort(x, descending=True)
    assert vals.dtype == x.dtype and idx.tolist() == desc
    assert vals.tolist() == x[torch.tensor(desc)].tolist()


def test_sort_pairs_argument_errors():
    i32 = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.argsort(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.sort(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.sort_pairs_(torch.zeros(8, dtype=torch.float64), i32.clone())
    with pytest.raises(ValueError):  # non-contiguous keys / values
        ops.argsort(torch.zeros(16, dtype=torch.int32)[::2])
    with pytest.raises(ValueError):
        ops.sort_pairs_(torch.zeros(16, dtype=torch.int32)[::2], i32.clone())
    with pytest.raises(ValueError):
        ops.sort_pairs_(i32.clone(), torch.zeros(16, dtype=torch.int32)[::2])
    with pytest.raises(ValueError):  # size mismatch
        ops.sort_pairs_(i32.clone(), torch.zeros(7, dtype=torch.int32))
    with pytest.raises(ValueError):  # uint8 keys: argsort / sort only
        ops.sort_pairs_(torch.zeros(8, dtype=torch.uint8), i32.clone())
    with pytest.raises(ValueError):  # payload words are 4 bytes
        ops.sort_pairs_(i32.clone(), torch.zeros(8, dtype=torch.int64))


def test_sort_pairs_c_abi_refusals():
    """Refused before any pointer is touched (NULL arrays, no device needed)."""
    L = _native.lib()
    assert L.mpx_sort_pairs_ws(None, None, 1 << 30, 0, 0, None, 0, None) == 3  # MPX_ERR_UNSUPPORTED
    assert b"2^30" in L.mpx_last_error()
    assert L.mpx_sort_pairs_ws(None, None, 1000, 0, 4, None, 0, None) == 3  # unknown flag bit
    assert b"flag" in L.mpx_last_error()
    assert L.mpx_sort_pairs_ws(None, None, 1000, 2, 0, None, 0, None) == 3  # MPX_SORT_U8
    assert L.mpx_last_error()
    assert L.mpx_sort_pairs_ws(None, None, 0, 0, 0, None, 0, None) == 0  # nothing to do
    assert int(L.mpx_sort_pairs_workspace_bytes(1, 0)) == 0
    n = 100_000  # a second n x 4 byte array beside the keys-only layout
    assert int(L.mpx_sort_pairs_workspace_bytes(n, 1)) >= int(L.mpx_sort_workspace_bytes(n, 1)) + 4 * n
    assert _native.tune_lib().mpx_sort_pairs_variant(None, None, 1000, 0, 0, None, 0, 9, None) != 0
    assert b"variant" in L.mpx_last_error()


def test_pairs_variant_entry_lives_in_the_tuning_library():
    raw = ctypes.CDLL(_native.lib()._name)  # a fresh handle: no attributes bound by _native
    assert hasattr(_native.tune_lib(), "mpx_sort_pairs_variant")
    assert not hasattr(raw, "mpx_sort_pairs_variant")
    for name in ("mpx_sort_pairs_ws", "mpx_sort_pairs_workspace_bytes", "mpx_cpu_sort_pairs"):
        assert hasattr(raw, name)


# ---------------------------------------------------------------- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("family", ["ties", "uniform"])
@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 10, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 100_003, (1 << 20) + 7])
def test_gpu_sort_and_argsort_auto(gpu, n, kind, family, descending):
    """AUTO. Every n >= 2 takes the radix path (there is no separate small-n
    kernel), on 4096-key tiles at these sizes: a single partial tile, exactly
    one and just over one tile, fewer tiles than XCDs."""
    a, perm = case(kind, family, n, descending)
    check_sort_and_argsort(a, perm, descending, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("descending", [False, True])
def test_gpu_sort_pairs_moves_opaque_payload(gpu, descending):
    """The payload's bits are never interpreted: random float32 bit patterns,
    NaN patterns included, come out as payload[perm] byte for byte."""
    n = 100_003
    a, perm = case("float", "ties", n, descending)
    bits = np.random.default_rng(3).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    bits[:4] = [0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000]
    k = torch.from_numpy(a.copy()).to(gpu)
    v = torch.from_numpy(bits.view(np.float32).copy()).to(gpu)
    ops.sort_pairs_(k, v, descending=descending)
    assert k.cpu().numpy().tobytes() == a[perm].tobytes()
    assert v.cpu().numpy().tobytes() == bits[perm].tobytes()


def run_variant(keys, vals, dt, flags, variant):
    L = _native.lib()
    n = keys.numel()
    nb = int(L.mpx_sort_pairs_workspace_bytes(n, dt))
    ws = torch.empty(nb, dtype=torch.uint8, device=keys.device)
    _native.check(_native.tune_lib().mpx_sort_pairs_variant(keys.data_ptr(), vals.data_ptr(), n, dt, flags,
                                                            ws.data_ptr(), nb, variant, _native.stream_of(keys)))


@pytest.mark.gpu
@pytest.mark.parametrize("keys", ["float-ties", "int-range1000"])
@pytest.mark.parametrize("n", [4097, 8193, 100_003])
@pytest.mark.parametrize("variant", [7, 8, 20, 21, 22])
def test_gpu_pairs_every_production_form(gpu, variant, n, keys):
    """Each ranking form and tile size at small n: the peer-mask fallback
    (7 / 8, which AUTO never takes on gfx950) and the returning-add ranking
    with hot digits on 8192 / 4096 / 16384-key tiles (20 / 21 / 22), iota
    payload. 100_003 keys are 7 tiles of 16384: some XCDs own no tile."""
    kind, family = keys.split("-")
    a, perm = case(kind, family, n, False)
    k = torch.from_numpy(a.copy()).to(gpu)
    idx = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    run_variant(k, idx, MPX_DT[kind], IOTA, variant)
    assert np.array_equal(idx.cpu().numpy(), perm)
    assert k.cpu().numpy().tobytes() == a[perm].tobytes()


def big_range1000(n, descending):
    """range1000 keys on the GPU and torch's stable sort of them (no NaN or
    signed zero: torch's order and the total order agree)."""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(n)
    x = torch.randint(0, 1000, (n,), dtype=torch.int32, device="cuda:0", generator=g)
    vals, idx = torch.sort(x, stable=True, descending=descending)
    return x, vals, idx.to(torch.int32)


@functools.lru_cache(maxsize=None)
def walk_case():
    return big_range1000((1 << 23) + 5, False)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [20, 21, 22])
def test_gpu_pairs_forms_walk_several_tiles(gpu, variant):
    """(1 << 23) + 5 keys: every block walks two or three tiles, so the key
    prefetch and a payload that arrives later than its keys are exercised;
    a loaded payload (not iota), hot digits in three passes."""
    x, vals, idx = walk_case()
    n = x.numel()
    k = x.clone()
    payload = torch.arange(n, dtype=torch.int32, device=gpu) * 3 + 1
    v = payload.clone()
    run_variant(k, v, 0, 0, variant)
    assert torch.equal(k, vals)
    assert torch.equal(v, payload[idx.long()])


@pytest.mark.gpu
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("n", [(1 << 23) + 1, 1 << 25])
def test_gpu_pairs_auto_tile_thresholds(gpu, n, descending):
    """AUTO picks the tile size by n: 8192-key tiles above 2^23 keys (the
    keys-only threshold, inherited), 16384-key tiles from 2^25 (measured for
    pairs). The smallest n on the far side of each."""
    x, vals, idx = big_range1000(n, descending)
    got_vals, got_idx = ops.sort(x, descending=descending)
    assert torch.equal(got_vals, vals)
    assert torch.equal(got_idx, idx)


@pytest.mark.gpu
def test_gpu_sort_pairs_three_times_in_place(gpu):
    """Re-sorting sorted pairs is the identity permutation: three calls on the
    same buffers leave the first call's result."""
    n = 50_000
    a, perm = case("int", "ties", n, False)
    payload = np.arange(n, dtype=np.int32)[::-1].copy()
    k, v = torch.from_numpy(a.copy()).to(gpu), torch.from_numpy(payload.copy()).to(gpu)
    for _ in range(3):
        ops.sort_pairs_(k, v)
        assert k.cpu().numpy().tobytes() == a[perm].tobytes()
        assert v.cpu().numpy().tobytes() == payload[perm].tobytes()


@pytest.mark.gpu
def test_gpu_pairs_on_two_streams_stay_independent(gpu):
    cases = [case("int", "ties", 300_001, False), case("float", "ties", 200_003, True)]
    xs = [torch.from_numpy(a.copy()).to(gpu) for a, _ in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(gpu) for _ in xs]
    outs = []
    for x, st, desc in zip(xs, streams, (False, True)):
        with torch.cuda.stream(st):
            for _ in range(3):
                out = ops.argsort(x, descending=desc)
            outs.append(out)
    torch.cuda.synchronize()
    for out, (_, perm) in zip(outs, cases):
        assert np.array_equal(out.cpu().numpy(), perm)


@pytest.mark.gpu
def test_gpu_sort_pairs_workspace_and_device_contract(gpu):
    L = _native.lib()
    n = 100_000
    need = int(L.mpx_sort_pairs_workspace_bytes(n, 0))
    k = torch.zeros(n, dtype=torch.int32, device=gpu)
    v = torch.zeros(n, dtype=torch.int32, device=gpu)
    ws = torch.empty(need - 16, dtype=torch.uint8, device=gpu)
    rc = L.mpx_sort_pairs_ws(k.data_ptr(), v.data_ptr(), n, 0, 0, ws.data_ptr(), need - 16, _native.stream_of(k))
    assert rc != 0 and b"workspace" in L.mpx_last_error()
    with pytest.raises(ValueError):  # keys and values on different devices
        ops.sort_pairs_(k, torch.zeros(n, dtype=torch.int32))
    one = torch.tensor([5], dtype=torch.int32, device=gpu)
    assert ops.argsort(one).tolist() == [0]  # n = 1 with iota writes index 0
