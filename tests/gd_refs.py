"""The yardstick of the gradient-descent projection (``--constraint_proj svd_gd``; affine_proj_GD, image_sample.py:344-357 and its
set-up at :384-399): the ITERATED float64 form - one gradient step per iteration, nothing collapsed -, the first-order rounding bound
the GPU tests assert and the guard that leaves out ill-posed signs.  No GPU, no reference import; built on tests/restore_refs.py.

One iteration, with r = A x - y (per group g) and the tables w of restore_refs:
    l1:  x_i <- x_i - lr w_i sign(r_g)                     sign(0) = 0                       grad of sum_b ||r_b||_1
    l2:  x_i <- x_i - lr w_i r_g / rho ,  rho = ||r_b||_2  per sample b, no step where rho = 0    grad of sum_b ||r_b||_2
(what torch.autograd gives through the reference's operators; tests/test_gd_refs_cpu.py holds this form to autograd).  Inpainting is
the same with groups of one entry, w = 1, over the known entries only: a missing entry has no residual and never moves.

bound_gd - derived like restore_refs.bound_project: the roundings of ONE float32 iteration with u = 2^-24, doubled for the
higher-order terms, summed over the iterations, all evaluated on the float64 iterates.
    l1: the sign is exact outside the guard, so an iteration rounds the step lr w_i sign (once) and the subtraction (once):
            2u (|lr w_i sign(r_g)| + |x_i'|)                                               x' = the next iterate
    l2: the residual carries A's summation error and the subtraction's rounding,  e_g = bound_A(x)_g + 2u |r_g|  (bound_A is
        doubled already).  rho = sqrt(sum r_g^2): squares (u each), a pairwise sum over G groups (log2 G / 1 u), the root (u) - half
        of the first two survives the root - and the residual's error moves the norm by at most ||e||_2:
            d_rho / rho = 2u (2 + log2(G) / 2) + ||e||_2 / rho
        The step lr w_i r_g / rho rounds three times (division, w_i, lr), the subtraction once:
            |lr w_i| (e_g + |r_g| d_rho / rho) / rho  +  2u (3 |lr w_i r_g / rho| + |x_i'|)
A kernel that collapses the iterations rounds less often than this, one that iterates literally rounds exactly so.

guard - sign() is discontinuous: where the float64 |r_g| (l1) or rho (l2) of ANY iterate falls below 8 x the error the residual can
carry there - bound_A of that iterate; its 2-norm over the groups for rho, since an error vector e moves ||r|| by at most ||e||_2 - a
float32 evaluation may take the other sign and land a whole step away.  Such a group (l1) or sample (l2) is ill-posed, not wrong,
and is left out of the comparison; the tests cap the share that may be left out (CAP_SMALL, CAP_L2, CAP_WRAP).
"""
from __future__ import annotations

import functools
import math

import torch

from tests import restore_refs as R
from tests.restore_refs import A64, CLOSED_FORM_CASES, FIXTURE_CASES, LARGE_CASES, U32, bound_A, from_groups, inputs, tables  # noqa: F401

INPAINT = "inpaint"
N_ITER = 10
LRS = (10.0, 0.5)
LOSSES = ("l1", "l2")
# (mode, C, dim, r) with reference arrays in tests/golden/restore_gd.npz, and the inpainting case there: C = 3, dim = 8, seeded 50 % mask
GOLDEN_GROUP_CASES = [(R.BLOCK, 3, 8, 8), (R.BLOCK, 3, 12, 3), (R.CHANNEL, 3, 8, 1)]
INPAINT_CASE = (3, 8)
UNALIGNED_CASES = [(R.BLOCK, 3, 6, 2), (R.BLOCK, 3, 12, 4), (R.BLOCK, 3, 8, 8)]
CAP_SMALL, CAP_L2, CAP_WRAP = 0.0, 0.0, 1e-3          # share of groups (samples for l2) the guard may leave out


def loss_id(loss):
    return {"l1": 1, "l2": 2, 1: 1, 2: 2}[loss]


def measurement(mode, C, dim, r):
    """(x0, y): the seeded state and the float32 measurement y = A(x) of the other seeded image."""
    x, x0 = inputs(mode, C, dim, r)
    return x0, A64(x, mode, r).float()


def inpaint_inputs(C=INPAINT_CASE[0], dim=INPAINT_CASE[1], share=0.5):
    """(x0, missing, mask_chw, known): seeded U(-1, 1) state and image, ``missing`` = the indices of a seeded mask over pixels
    (all C channels of a pixel go together) in the pixel-interleaved flattening idx = p*C + c, the [C][HW] f32 mask of KNOWN
    entries and known = the image on the known entries, 0 elsewhere (A^+ A x)."""
    g = R.gen(("gd-inpaint", C, dim, share))
    x = torch.rand(R.B, C, dim, dim, generator=g) * 2 - 1
    x0 = torch.rand(R.B, C, dim, dim, generator=g) * 2 - 1
    pix = torch.randperm(dim * dim, generator=g)[: int(round(dim * dim * share))]
    missing = torch.cat([pix * C + c for c in range(C)])
    mask = torch.ones(C, dim * dim)
    mask[:, pix] = 0.0
    known = x * mask.view(1, C, dim, dim)
    return x0, missing, mask, known


def _iterate(xg, y, w, active, lr, n_iter, loss, rhos=None):
    """xg: (B, G, n) float64 entries by group; y: (B, G); w: (n,); active: (G,) bool or None (inpainting: the known entries).
    Returns (x^n by group, bound by group entry, kept groups (B, G) bool).  ``rhos``: a list that receives every l2 iterate's rho (B,)."""
    Bn, G, n = xg.shape
    act = torch.ones(G, dtype=torch.bool) if active is None else active
    actf = act.double()
    logG = math.log2(max(int(act.sum()), 2))
    x = xg.clone()
    bound = torch.zeros_like(x)
    keep = torch.ones(Bn, G, dtype=torch.bool)
    lw = (lr * w).abs()
    for _ in range(n_iter):
        wx = x * w
        r = (wx.sum(-1) - y) * actf
        bA = (n + 2) * 2 * U32 * wx.abs().sum(-1) * actf                      # restore_refs.bound_A of this iterate
        if loss_id(loss) == 1:
            keep &= ~(act & (r.abs() < 8 * bA))
            step = lr * w * torch.sign(r).unsqueeze(-1)
            nxt = x - step
            bound += 2 * U32 * (step.abs() + nxt.abs()) * actf.unsqueeze(-1)
        else:
            rho = r.pow(2).sum(-1).sqrt()                                       # (B,)
            if rhos is not None:
                rhos.append(rho)
            keep &= ~(rho < 8 * bA.pow(2).sum(-1).sqrt()).unsqueeze(-1)
            safe = (rho > 0).double().unsqueeze(-1)
            rs = torch.where(rho > 0, rho, torch.ones_like(rho)).unsqueeze(-1)
            step = lr * w * (safe * r / rs).unsqueeze(-1)
            nxt = x - step
            e = bA + 2 * U32 * r.abs()
            d_rho = 2 * U32 * (2 + logG / 2) + e.pow(2).sum(-1).sqrt().unsqueeze(-1) / rs
            dirn = safe * (e + r.abs() * d_rho) / rs
            bound += (lw * dirn.unsqueeze(-1) + 2 * U32 * (3 * step.abs() + nxt.abs())) * actf.unsqueeze(-1)
        x = nxt
    return x, bound, keep


@functools.lru_cache(maxsize=None)
def _group_case(mode, C, dim, r, lr, n_iter, loss):
    x0, y = measurement(mode, C, dim, r)
    return _group(x0, y, mode, r, lr, n_iter, loss)


def _group(x0, y, mode, r, lr, n_iter, loss):
    _, C, dim, _ = x0.shape
    w, _ = tables(mode, r)
    xg, bg, keep = _iterate(R.to_groups(x0.double(), mode, r), y.double(), w, None, lr, n_iter, loss)
    n = w.numel()
    return (from_groups(xg, mode, C, dim, r), from_groups(bg, mode, C, dim, r),
            from_groups(keep.unsqueeze(-1).expand(-1, -1, n), mode, C, dim, r), keep)


def gd64(x0, y, mode, r, lr, n_iter, loss):
    """The iterated float64 form, (B, C, dim, dim)."""
    return _group(x0, y, mode, r, lr, n_iter, loss)[0]


def bound_gd(x0, y, mode, r, lr, n_iter, loss):
    """Per entry, (B, C, dim, dim): the derivation is in the module docstring."""
    return _group(x0, y, mode, r, lr, n_iter, loss)[1]


def guard(x0, y, mode, r, lr, n_iter, loss):
    """(entries to compare (B, C, dim, dim) bool, share of groups left out)."""
    _, _, kx, keep = _group(x0, y, mode, r, lr, n_iter, loss)
    return kx, 1.0 - keep.double().mean().item()


def case64(mode, C, dim, r, lr, n_iter, loss):
    """(x^n, bound, entries to compare, share left out) of a seeded case (``measurement``), computed once per process."""
    xn, b, kx, keep = _group_case(mode, C, dim, r, lr, n_iter, loss)
    return xn, b, kx, 1.0 - keep.double().mean().item()


def _inpaint(x0, mask, known, lr, n_iter, loss):
    Bn = x0.shape[0]
    act = mask.reshape(-1) != 0
    xg, bg, keep = _iterate(x0.double().reshape(Bn, -1, 1), known.double().reshape(Bn, -1), torch.ones(1, dtype=torch.float64), act,
                            lr, n_iter, loss)
    left = 1.0 - keep[:, act].double().mean().item() if bool(act.any()) else 0.0
    return xg.reshape(x0.shape), bg.reshape(x0.shape), keep.reshape(x0.shape), left


def gd64_inpaint(x0, mask, known, lr, n_iter, loss):
    """The iterated float64 form over the known entries (``mask``: [C][HW], non-zero = known; ``known``: (B, C, H, W))."""
    return _inpaint(x0, mask, known, lr, n_iter, loss)[0]


def inpaint64(x0, mask, known, lr, n_iter, loss):
    """(x^n, bound, entries to compare, share of known entries left out)."""
    return _inpaint(x0, mask, known, lr, n_iter, loss)


def min_rho_over_c(x0, y, mode, r, lr, n_iter, mask=None):
    """min over the l2 iterates and the samples of rho_k / c, c = lr sum w^2: how far the run stays from the sign change of the
    collapsed recurrence rho_{k+1} = rho_k - c sign(rho_k), in units of its step.  ``mode`` INPAINT: y = known, ``mask`` [C][HW]."""
    rhos, Bn = [], x0.shape[0]
    if mode == INPAINT:
        w = torch.ones(1, dtype=torch.float64)
        _iterate(x0.double().reshape(Bn, -1, 1), y.double().reshape(Bn, -1), w, mask.reshape(-1) != 0, lr, n_iter, "l2", rhos)
    else:
        w = tables(mode, r)[0]
        _iterate(R.to_groups(x0.double(), mode, r), y.double().reshape(Bn, -1), w, None, lr, n_iter, "l2", rhos)
    return torch.stack(rhos).min().item() / (lr * float(w.pow(2).sum()))


def cap_of(mode, C, dim, r, loss):
    if loss_id(loss) == 2:
        return CAP_L2
    return CAP_WRAP if (mode, C, dim, r) in LARGE_CASES else CAP_SMALL


def gd_name(mode, C, dim, r, lr, loss):
    return f"{R.case_name(mode, C, dim, r)}_lr{lr:g}_{loss}"


# every (case, lr, loss) the GPU op tests run
OP_RUNS = [(c, lr, loss) for c in FIXTURE_CASES + LARGE_CASES + CLOSED_FORM_CASES for lr in LRS for loss in LOSSES]
