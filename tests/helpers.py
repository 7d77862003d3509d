"""Shared test helpers: fixture locations and the .data / hex GT codecs."""

import binascii
import os
import struct

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB2_DATA = os.path.join(ROOT, "labs", "lab2", "data")
LAB2_GT = os.path.join(ROOT, "labs", "lab2", "data_out_gt")
LAB3_DATA = os.path.join(ROOT, "labs", "lab3", "data")
LAB3_GT = os.path.join(ROOT, "labs", "lab3", "data_out_gt")

# the reference's hard-coded lab3 classes (lab3/lab3_processor.py:42-51)
LAB3_CLASSES = [np.array([[1, 2], [1, 0], [2, 2], [2, 1]]), np.array([[0, 0], [0, 1], [1, 1], [2, 0]])]


# exactly representable lab3 statistics: means on a 2^-6 grid (mu = mu_grid / G)
# and inverse covariances at integer x 2^-s (inv = A_int / 2**s)
G = 64


def exact_dist(px, mu_grid, A_int, chunk=1 << 15):
    """int64 (N, nc): sum_ij d_i A_ij d_j with d = G * p - mu_grid, for pixels
    px (N, 3), means mu_grid (nc, 3) and matrices A_int (nc, 3, 3), all integer.

    These are the reference's Mahalanobis distances times G^2 2^s, computed
    without any project code. The bit budget asserted here (the sum of the
    absolute values of ALL terms of a class stays below 2^52) makes every
    partial result of the reference's fp64 FMA chain on mu_grid / G and
    A_int / 2^s an integer times a power of two below 2^53, hence exact: the
    chain must reproduce argmin (first minimum = strict '<') on every pixel."""
    px = np.asarray(px, np.int64).reshape(-1, 3)
    mu_grid = np.asarray(mu_grid, np.int64).reshape(-1, 3)
    A_int = np.asarray(A_int, np.int64).reshape(-1, 3, 3)
    nc = mu_grid.shape[0]
    assert A_int.shape[0] == nc and px.shape[0] > 0
    lo, hi = G * px.min(0), G * px.max(0)
    for c in range(nc):
        dmax = [max(abs(int(lo[i]) - int(mu_grid[c, i])), abs(int(hi[i]) - int(mu_grid[c, i]))) for i in range(3)]
        total = sum(abs(int(A_int[c, i, j])) * dmax[i] * dmax[j] for i in range(3) for j in range(3))
        assert total < 2**52, f"class {c}: {total.bit_length()} bits: the fp64 chain would round"
    out = np.empty((px.shape[0], nc), np.int64)
    for a in range(0, px.shape[0], chunk):
        d = G * px[a:a + chunk, None, :] - mu_grid[None, :, :]           # (n, nc, 3)
        d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
        acc = (d0 * A_int[None, :, 0, 0] + d1 * A_int[None, :, 1, 0] + d2 * A_int[None, :, 2, 0]) * d0
        acc += (d0 * A_int[None, :, 0, 1] + d1 * A_int[None, :, 1, 1] + d2 * A_int[None, :, 2, 1]) * d1
        acc += (d0 * A_int[None, :, 0, 2] + d1 * A_int[None, :, 1, 2] + d2 * A_int[None, :, 2, 2]) * d2
        out[a:a + chunk] = acc
    return out


def hex_bytes(path):
    return binascii.unhexlify(open(path).read().replace("\n", "").replace(" ", ""))


def bytes_to_img(b: bytes) -> torch.Tensor:
    w, h = struct.unpack("<ii", b[:8])
    return torch.frombuffer(bytearray(b[8:8 + 4 * w * h]), dtype=torch.uint8).reshape(h, w, 4).clone()


def img_to_bytes(img: torch.Tensor) -> bytes:
    h, w = img.shape[:2]
    return struct.pack("<ii", w, h) + img.cpu().contiguous().numpy().tobytes()


def rand_img(h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, generator=g)


def smooth_img(h, w, seed=0):
    """Natural-image-like data: smooth gradients + noise (exercises non-saturated outputs)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    base = torch.stack([128 + 100 * torch.sin(xx / 17.0 + c) * torch.cos(yy / 23.0 - c) for c in range(3)], -1)
    noise = torch.randn((h, w, 3), generator=g) * 6
    rgb = torch.clamp(base + noise, 0, 255).to(torch.uint8)
    a = torch.randint(0, 256, (h, w, 1), dtype=torch.uint8, generator=g)
    return torch.cat([rgb, a], -1).contiguous()
