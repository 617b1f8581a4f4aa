"""Yardsticks of the 3-D SSIM metric (diffusion_nlc_amd.metrics.ssim3d / nlc_ssim3d), on the CPU, without the reference tree.

The operator, restated from ssim_fn (reference image_sample.py:571-582) and _ssim_3d (basicsr/metrics/psnr_ssim.py:157-208,251-337):
per pair of (C, H, W) f32 images in [0, 1], a = round(sample * 255), b = round(orig * 255) (f32 product, ties to even, uint8);
max_value = 1 if max(a) <= 1 else 255 (sample only), C1 = (0.01 max_value)^2, C2 = (0.03 max_value)^2; the five fields a, b, a^2,
b^2, ab are filtered over the volume (H, W, C) with the table w[d][h][w] = f32(g_d * (g_h * g_w)), g the normalised 11-tap
Gaussian of sigma 1.5 in float64, replicate padding of 5 on all three axes; the SSIM map is averaged over H * W * C.

``ssim64`` is that in float64 (the f32-rounded table taken back to float64): it DEFINES the operator.  ``ssim32`` is the same
arithmetic in f32 with torch on the CPU (replicate F.pad + F.conv3d with the product table) and stands for the reference's own
rounding.  The GPU gate is GATE = 4 * E32_MEASURED, E32 = max |ssim32 - ssim64| over CASES: the kernel's three separable passes
and its different summation order each carry first-order error of the size of the reference's single 1331-tap sum, neither is
"the exact one", and the cancellation in E[a^2] - mu^2 at values up to 65025 dominates both.  The gate is measured against the
reference arithmetic, never against the kernel; tests/test_ssim_refs_cpu.py re-measures E32 and fails if the constant is below it.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

TAPS, RAD, SIGMA = 11, 5, 1.5

# printed by tests/test_ssim_refs_cpu.py::test_e32_constants_cover_the_measurement (pytest -s), rounded up in the third digit:
#   E32 = max |ssim32 - ssim64| over 19 cases = 5.6591e-04 (at constant_40x70); without the FLAT cases 2.8244e-06 (at noisy_3x5)
# Flat images are where the cancellation is everything: sigma^2 = E[a^2] - mu^2 is 0 in exact arithmetic and 23409 * 2^-24 * k in
# f32, against C2 = 58.5.  That one case sets E32 two hundred times above all others, so the cases with texture are held to the
# tighter gate that their own measurement gives, by the same rule; no case is held to more than GATE.
E32_MEASURED = 5.66e-4
E32_TEXTURED_MEASURED = 2.83e-6
GATE = 4 * E32_MEASURED
GATE_TEXTURED = 4 * E32_TEXTURED_MEASURED
FLAT = ("constant_40x70",)


def gate_of(name):
    return GATE if name in FLAT else GATE_TEXTURED


@functools.lru_cache(maxsize=None)
def gauss():
    """cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 sigma^2)) in float64, normalised to sum 1."""
    i = np.arange(TAPS, dtype=np.float64) - RAD
    g = np.exp(-(i * i) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


@functools.lru_cache(maxsize=None)
def weight_table():
    """(11, 11, 11) f32: g_d * (g_h * g_w) in float64 (the reference's np.outer, then * k), rounded once on assignment."""
    g = gauss()
    return torch.from_numpy(np.stack([np.outer(g, g) * k for k in g], axis=0)).to(torch.float32)


def channel_matrix(C, taps=None):
    """M[c][c'] = sum_j taps[j] [clamp(c + j - 5, 0, C - 1) == c'] in float64: what replicate padding makes of the channel axis."""
    taps = gauss() if taps is None else np.asarray(taps, dtype=np.float64)
    M = np.zeros((C, C), dtype=np.float64)
    for c in range(C):
        for j in range(TAPS):
            M[c, min(max(c + j - RAD, 0), C - 1)] += taps[j]
    return M


def quantise(x):
    return torch.round(x * 255).to(torch.uint8)


def _constants(a):
    mv = 1.0 if float(a.max()) <= 1 else 255.0
    return (0.01 * mv) ** 2, (0.03 * mv) ** 2


def _ssim64_pair(sample, orig):
    a = quantise(sample).permute(1, 2, 0).numpy().astype(np.float64)          # (H, W, C)
    b = quantise(orig).permute(1, 2, 0).numpy().astype(np.float64)
    H, W, C = a.shape
    C1, C2 = _constants(a)
    table = weight_table().numpy().astype(np.float64)
    fields = np.stack([a, b, a * a, b * b, a * b])
    padded = np.pad(fields, ((0, 0), (RAD, RAD), (RAD, RAD), (0, 0)), mode="edge")
    out = np.zeros_like(fields)
    for d in range(TAPS):
        for h in range(TAPS):
            out += np.einsum("fyxk,ck->fyxc", padded[:, d:d + H, h:h + W, :], channel_matrix(C, table[d, h]))
    mu1, mu2, e11, e22, e12 = out
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    ssim_map = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return float(ssim_map.mean())


def _ssim32_pair(sample, orig):
    a = quantise(sample).permute(1, 2, 0).to(torch.float32)
    b = quantise(orig).permute(1, 2, 0).to(torch.float32)
    C1, C2 = _constants(a)
    w = weight_table()[None, None]

    def filt(v):
        return F.conv3d(F.pad(v[None, None], (RAD,) * 6, mode="replicate"), w)[0, 0]
    mu1, mu2 = filt(a), filt(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1, s2, s12 = filt(a ** 2) - mu1_sq, filt(b ** 2) - mu2_sq, filt(a * b) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return float(ssim_map.mean())


def _pairs(fn, sample, orig):
    N, P = sample.shape[0], orig.shape[0]
    assert 1 <= P <= N and N % P == 0 and sample.shape[1:] == orig.shape[1:]
    return torch.tensor([fn(sample[n], orig[n % P]) for n in range(N)], dtype=torch.float64)


def ssim64(sample, orig):
    """float64 closed form: (N, C, H, W) against (P, C, H, W), pair n uses orig[n % P].  Returns float64 (N,)."""
    return _pairs(_ssim64_pair, sample.cpu(), orig.cpu())


def ssim32(sample, orig):
    """The reference's f32 arithmetic (dense 1331-tap Conv3d per field) on the CPU.  Returns float64 (N,)."""
    return _pairs(_ssim32_pair, sample.cpu(), orig.cpu())


# ---- seeded cases ----------------------------------------------------------------------------------------------------------
def half_way_grid(n):
    """n values around every x = f32((k + 0.5) / 255): the value and its two f32 neighbours, where x * 255 lands on, just below or
    just above a tie."""
    k = torch.arange(255, dtype=torch.float64)
    mid = ((k + 0.5) / 255).to(torch.float32)
    up = torch.nextafter(mid, torch.tensor(2.0))
    down = torch.nextafter(mid, torch.tensor(-1.0))
    grid = torch.stack([mid, up, down], dim=1).reshape(-1)
    return grid.repeat((n + grid.numel() - 1) // grid.numel())[:n]


def make(content, N, P, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    shape_s, shape_o = (N, C, H, W), (P, C, H, W)
    if content == "noisy":
        orig = torch.rand(shape_o, generator=g)
        reps = orig.repeat(N // P, 1, 1, 1)
        sample = (reps + 0.05 * torch.randn(shape_s, generator=g)).clamp(0, 1)
    elif content == "unrelated":
        orig, sample = torch.rand(shape_o, generator=g), torch.rand(shape_s, generator=g)
    elif content == "same":
        orig = torch.rand(shape_o, generator=g)
        sample = orig.repeat(N // P, 1, 1, 1).clone()
    elif content == "constant":
        orig, sample = torch.full(shape_o, 0.3), torch.full(shape_s, 0.6)
    elif content in ("dim", "dim_one_bright"):
        # quantised sample in {0, 1}: max_value = 1; one pixel at 2 / 255 switches the whole image to max_value = 255
        orig = torch.rand(shape_o, generator=g)
        sample = torch.randint(0, 2, shape_s, generator=g).to(torch.float32) / 255
        if content == "dim_one_bright":
            sample[:, C - 1, H // 2, W // 3] = 2.0 / 255
    elif content == "half_way":
        sample = half_way_grid(N * C * H * W).view(shape_s).clone()
        orig = half_way_grid(P * C * H * W + 7)[7:].view(shape_o).clone()
    else:
        raise ValueError(content)
    return sample.contiguous(), orig.contiguous()


# name -> (content, N, P, C, H, W); the seed is the position in the list (SAME_SEED_AS: another case's position)
CASES = {
    "noisy_1x1": ("noisy", 1, 1, 3, 1, 1),                   # smaller than the halo: everything is replicate
    "noisy_3x5": ("noisy", 1, 1, 3, 3, 5),
    "noisy_5x11": ("noisy", 1, 1, 3, 5, 11),
    "noisy_11x11": ("noisy", 1, 1, 3, 11, 11),
    "noisy_16x16": ("noisy", 2, 2, 3, 16, 16),
    "noisy_33x17": ("noisy", 5, 5, 3, 33, 17),               # no multiple of a tile: tile boundaries inside, N = 5
    "noisy_40x70": ("noisy", 1, 1, 3, 40, 70),
    "noisy_64x64": ("noisy", 1, 1, 3, 64, 64),
    "noisy_256x256": ("noisy", 1, 1, 3, 256, 256),           # the workload's size, once
    "noisy_c1_8x8": ("noisy", 1, 1, 1, 8, 8),
    "noisy_c4_8x8": ("noisy", 1, 1, 4, 8, 8),
    "noisy_p2_n6": ("noisy", 6, 2, 3, 20, 36),               # P < N
    "unrelated_40x70": ("unrelated", 1, 1, 3, 40, 70),
    "same_40x70": ("same", 1, 1, 3, 40, 70),
    "constant_40x70": ("constant", 1, 1, 3, 40, 70),
    "dim_40x70": ("dim", 1, 1, 3, 40, 70),
    "dim_one_bright_40x70": ("dim_one_bright", 1, 1, 3, 40, 70),
    "half_way_16x17": ("half_way", 1, 1, 3, 16, 17),
    "half_way_c2_40x33": ("half_way", 2, 1, 2, 40, 33),
}
SAME_SEED_AS = {"dim_one_bright_40x70": "dim_40x70"}         # the same images but for the one pixel


@functools.lru_cache(maxsize=None)
def case(name):
    """(sample, orig, ssim64) of a case; computed once and shared: do not modify."""
    content, N, P, C, H, W = CASES[name]
    sample, orig = make(content, N, P, C, H, W, seed=list(CASES).index(SAME_SEED_AS.get(name, name)))
    return sample, orig, ssim64(sample, orig)
