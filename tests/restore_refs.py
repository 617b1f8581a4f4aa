"""float64 closed forms of the group-sum measurement operators (average-pooling super-resolution, colorization), the cases the
GPU tests run and the first-order error bounds they assert.  No GPU, no reference import: tests/test_restore_refs_cpu.py holds
these forms to the reference's own arrays (tests/golden/restore_ops.npz), tests/test_restore_ops_gpu.py holds the kernels to them.

With the weights w of one group (n entries) and p_i = w_i / sum_j w_j^2:
    A(x)[g]        = sum_i w_i x_i
    A^+(y)[i of g] = p_i y[g]
    project(x0, y) = x0_i + p_i (y[g] - sum_j w_j x0_j)                       x0 - A^+(A x0 - y)
BLOCK: a group is an r x r block of one channel, i row-major in the block, y[b][c][by][bx].  CHANNEL: the 3 channels of a pixel,
y[b][p].  The tables are the ones the kernels are handed - computed in float64, rounded to float32 once - taken back to float64:
they define the operator (the reference's own weights are float32 tensors as well).
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch

BLOCK, CHANNEL = "block", "channel"
U32 = 2.0 ** -24
B = 2
COLOR_WEIGHTS = (0.3333, 0.3334, 0.3333)             # functions/svd_operators.py:632, literal

# (mode, C, img_dim, r): with a fixture in restore_ops.npz
FIXTURE_CASES = [
    (BLOCK, 1, 2, 2), (BLOCK, 3, 4, 4), (BLOCK, 3, 8, 8),        # one block per channel
    (BLOCK, 3, 6, 2), (BLOCK, 3, 12, 4),                         # odd number of blocks per row
    (BLOCK, 3, 12, 3), (BLOCK, 1, 9, 3),                         # r = 3: scalar path, unaligned rows
    (BLOCK, 3, 16, 1),                                           # r = 1: the identity
    (CHANNEL, 3, 1, 1), (CHANNEL, 3, 8, 1),                      # single pixel; plane-strided reads
]
# float64 closed form only.  More groups per sample than one grid of 1024 x 256 threads, so the grid-stride loop wraps: 270 000
# blocks, 270 400 pixels; 300 x 300 pixels fill 352 workgroups without wrapping
LARGE_CASES = [(BLOCK, 3, 600, 2), (CHANNEL, 3, 300, 1), (CHANNEL, 3, 520, 1)]
# float64 closed form only.  r = 5, 6, 7, the block sizes no fixture has: 2 x 2 blocks per channel, the smallest shape at which the
# row and bx indexing of those instantiations can go wrong
CLOSED_FORM_CASES = [(BLOCK, 3, 10, 5), (BLOCK, 3, 12, 6), (BLOCK, 3, 14, 7)]


def case_name(mode, C, dim, r):
    return f"{mode}_c{C}_d{dim}_r{r}"


def tables(mode, r):
    """(w, p) as float64 tensors holding the float32-rounded tables."""
    w = np.full(r * r, 1.0 / (r * r)) if mode == BLOCK else np.asarray(COLOR_WEIGHTS, dtype=np.float64)
    p = np.ones_like(w) if mode == BLOCK else w / np.sum(w * w)
    return (torch.from_numpy(w.astype(np.float32).astype(np.float64)), torch.from_numpy(p.astype(np.float32).astype(np.float64)))


def gen(key):
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:7], "little"))


def inputs(mode, C, dim, r):
    """Seeded x, x0 ~ U(-1, 1), float32 (B, C, dim, dim)."""
    g = gen(("restore", mode, C, dim, r))
    return (torch.rand(B, C, dim, dim, generator=g) * 2 - 1, torch.rand(B, C, dim, dim, generator=g) * 2 - 1)


def to_groups(x, mode, r):
    """(B, C, H, W) -> (B, groups, n) in the order of the measurement vector and of the sum."""
    Bn, C, H, W = x.shape
    if mode == CHANNEL:
        return x.reshape(Bn, C, H * W).permute(0, 2, 1)
    return x.reshape(Bn, C, H // r, r, W // r, r).permute(0, 1, 2, 4, 3, 5).reshape(Bn, C * (H // r) * (W // r), r * r)


def from_groups(g, mode, C, dim, r):
    Bn = g.shape[0]
    if mode == CHANNEL:
        return g.permute(0, 2, 1).reshape(Bn, C, dim, dim)
    return g.reshape(Bn, C, dim // r, dim // r, r, r).permute(0, 1, 2, 4, 3, 5).reshape(Bn, C, dim, dim)


def A64(x, mode, r):
    """(B, C, H, W) -> float64 (B, groups)."""
    w, _ = tables(mode, r)
    return (to_groups(x.double(), mode, r) * w).sum(-1)


def Apinv64(y, mode, C, dim, r):
    """(B, groups) -> float64 (B, C, dim, dim)."""
    _, p = tables(mode, r)
    return from_groups(y.double().unsqueeze(-1) * p, mode, C, dim, r)


def project64(x0, y, mode, r):
    _, C, dim, _ = x0.shape
    _, p = tables(mode, r)
    g = to_groups(x0.double(), mode, r)
    return from_groups(g + p * (y.double() - A64(x0, mode, r)).unsqueeze(-1), mode, C, dim, r)


# ---- bounds: n products, n-1 additions and one final rounding with u = 2^-24, doubled for the higher-order terms ------------
def bound_A(x, mode, r):
    """(n + 2) 2^-23 sum_i |w_i x_i| per group, (B, groups)."""
    w, _ = tables(mode, r)
    return (w.numel() + 2) * 2 * U32 * (to_groups(x.double(), mode, r) * w).abs().sum(-1)


def p_is_one(mode, r):
    return bool((tables(mode, r)[1] == 1.0).all())


def bound_Apinv(y, mode, C, dim, r):
    """One rounding of p_i y: 2^-23 |p_i y|; nothing where p_i = 1 (the product is exact)."""
    if p_is_one(mode, r):
        return torch.zeros(y.shape[0], C, dim, dim, dtype=torch.float64)
    return 2 * U32 * Apinv64(y, mode, C, dim, r).abs()


def bound_project(x0, y, mode, r):
    """bound_A |p_i| + 2^-23 (|x0_i| + |p_i (y - A x0)|), (B, C, dim, dim)."""
    _, C, dim, _ = x0.shape
    _, p = tables(mode, r)
    corr = (p * (y.double() - A64(x0, mode, r)).unsqueeze(-1)).abs()
    ba = bound_A(x0, mode, r).unsqueeze(-1) * p.abs()
    return from_groups(ba + 2 * U32 * (to_groups(x0.double(), mode, r).abs() + corr), mode, C, dim, r)
