"""Measurement operators for restoration sampling: inpainting (BASELINE config 4), average-pooling
super-resolution and colorization.

Mirrors the parts of the reference that these paths touch: ``functions/svd_operators.py:324-359`` (``Inpainting``),
``:479-533`` (``SuperResolution``), ``:627-667`` (``Colorization``), ``src/constraint_functions.py:216-251`` (the
``svd_constraint`` branches) and ``image_sample.py:282-343,371-383`` (``Constraint_Function`` with the ``affine_svd``
projection  x0 <- x0 - A^+(A x0 - y)).

* Inpainting: the projection is "copy the known pixels"; the per-step work is fused into ``nlc_sched_step`` (mask /
  known), A and A^+ themselves are the two gather kernels of ``csrc/constraint.hip``.
* Super-resolution and colorization are "one weighted sum per group of n entries" (an r x r block, or the 3 channels of
  a pixel).  With the weights w and p_i = w_i / sum w^2:  A(x)[g] = sum_i w_i x_i,  A^+(y)[i of g] = p_i y[g],  and the
  projection is  x0_i + p_i (y[g] - sum_j w_j x0_j):  three operations of the one group kernel of ``csrc/restore.hip``
  (layout x operation; the ``svd_gd`` phases below are the other three).  Per step the loop
  runs clip / ``nlc_group_project`` / x_prev (three launches; the projection needs a per-group reduction that the
  element-wise scheduler kernel does not have).

* ``svd_gd`` (``affine_proj_GD``, ``image_sample.py:344-357,384-399``) runs n_iter gradient steps on ||A x0 - y||_1 or _2 for
  the same three operators.  Their A A^T is a multiple of the identity, so the gradient and the whole iteration have a closed
  form: ``nlc_group_gd`` / ``nlc_inpaint_gd`` (``GradientProjection``), one launch for l1 and two for l2 whatever n_iter is.

The other degradations of the reference (bicubic SR, deblurring, compressed sensing, denoising), the ``simple`` / ``simple_gd``
projections and ``ddrm`` with the group-sum operators raise NotImplementedError.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from . import _ext, ops
from ._ext import NlcError, check


def _in_place(what, x0, partner, n_x0, n_partner):
    """The state a kernel updates in place and the tensor it is held to: contiguous float32, x0 on a GPU, both on one device, with
    ``n_x0`` / ``n_partner`` elements."""
    for t in (x0, partner):
        if not (t.is_contiguous() and t.dtype == torch.float32):
            raise NlcError(f"{what}: x0 and its measurement must be contiguous float32 tensors")
    if not (x0.is_cuda and x0.device == partner.device):
        raise NlcError(f"{what}: x0 and its measurement must be on the operator's device")
    if x0.numel() != n_x0 or partner.numel() != n_partner:
        raise NlcError(f"{what}: shape mismatch")


class Inpainting:
    """functions/svd_operators.py:324-359.  ``missing_indices`` index the pixel-interleaved (H*W, C) flattening."""

    def __init__(self, channels, img_dim, missing_indices, device):
        self.channels, self.img_dim = channels, img_dim
        self.device = torch.device(device)
        n = channels * img_dim ** 2
        missing = torch.as_tensor(missing_indices).long().cpu()
        keep = torch.ones(n, dtype=torch.bool)
        keep[missing] = False
        self.missing_indices = missing.to(self.device)
        kept = torch.nonzero(keep).reshape(-1)
        inv = torch.full((n,), -1, dtype=torch.int32)
        inv[kept] = torch.arange(kept.numel(), dtype=torch.int32)
        self.kept_indices = kept.to(self.device).contiguous()
        self._inv = inv.to(self.device).contiguous()
        self._singulars = torch.ones(kept.numel(), device=self.device)
        # [C][HW] f32 mask of KNOWN entries, the layout nlc_sched_step wants
        self.mask_chw = keep.view(img_dim * img_dim, channels).t().contiguous().float().to(self.device)

    def singulars(self):
        return self._singulars

    @ops.on_device
    def A(self, vec):
        x = vec.reshape(vec.shape[0], self.channels, -1).to(self.device, torch.float32).contiguous()
        B, C, HW = x.shape
        nk = self.kept_indices.numel()
        out = torch.empty(B, nk, device=self.device, dtype=torch.float32)
        check(_ext.load().nlc_inpaint_A(x.data_ptr(), self.kept_indices.data_ptr(), out.data_ptr(), B, C, HW, nk, ops._stream()),
              "nlc_inpaint_A")
        return out

    @ops.on_device
    def A_pinv(self, vec):
        y = vec.reshape(vec.shape[0], -1).to(self.device, torch.float32).contiguous()
        B, nk = y.shape
        if nk != self.kept_indices.numel():
            raise ValueError("A_pinv: measurement length mismatch")
        C, HW = self.channels, self.img_dim ** 2
        out = torch.empty(B, C * HW, device=self.device, dtype=torch.float32)
        check(_ext.load().nlc_inpaint_Apinv(y.data_ptr(), self._inv.data_ptr(), out.data_ptr(), B, C, HW, nk, ops._stream()),
              "nlc_inpaint_Apinv")
        return out

    At = A_pinv          # singular values are all 1: A^T = A^+

    @ops.on_device
    def gd_(self, x0, known, lr, n_iter, loss, workspace=None):
        """``n_iter`` steps of x0 <- x0 - lr grad ||A x0 - y||_p in place (``nlc_inpaint_gd``).  ``x0``: contiguous f32 (B, C, H, W)
        on this device; ``known``: A^+ y in the same shape.  Only known entries move."""
        B, C, HW = x0.shape[0], self.channels, self.img_dim ** 2
        _in_place("gd_", x0, known, B * C * HW, B * C * HW)
        loss = gd_loss_id(loss)
        ws = workspace if workspace is not None else gd_workspace(B, C * HW, loss, x0.device)
        check(_ext.load().nlc_inpaint_gd(x0.data_ptr(), self.mask_chw.data_ptr(), known.data_ptr(), B, C, HW, float(lr), int(n_iter),
                                         loss, None if ws is None else ws.data_ptr(), ops._stream()), "nlc_inpaint_gd")
        return x0


GD_LOSSES = {"l1": 1, "l2": 2}


def gd_loss_id(loss):
    """'l1' / 'l2' (or 1 / 2) -> the ``loss`` argument of nlc_group_gd / nlc_inpaint_gd."""
    if loss in GD_LOSSES:
        return GD_LOSSES[loss]
    if loss in (1, 2):
        return int(loss)
    raise NlcError(f"constraint loss {loss!r}: expected 'l1' or 'l2'")


def gd_workspace(B, entries_per_sample, loss, device):
    """The l2 partial sums of one gradient-descent projection (``nlc_gd_workspace_bytes``); None for l1."""
    if gd_loss_id(loss) != 2:
        return None
    n = _ext.load().nlc_gd_workspace_bytes(int(B), int(entries_per_sample))
    return torch.empty(max(n, 8) // 8, dtype=torch.float64, device=device)


def group_tables(weights):
    """(w, p) of a group-sum operator as the kernels take them: p_i = w_i / sum_j w_j^2 in float64, each table rounded to
    float32 once.  The mean (w_i = 1/n) has p_i = 1: passed as 1.0f exactly, whatever 1/n rounds to."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size < 1 or w.size > 64:
        raise NlcError(f"group of {w.size} entries: 1..64 are supported")
    is_mean = bool(np.all(w == w[0])) and abs(w[0] * w.size - 1.0) < 1e-12
    p = np.ones_like(w) if is_mean else w / np.sum(w * w)
    return w.astype(np.float32), p.astype(np.float32)


def group_desc(mode, B, C, H, W, r, w, p):
    d = _ext.GroupDesc(mode=mode, B=B, C=C, H=H, W=W, r=r)
    for i, (wi, pi) in enumerate(zip(w, p)):
        d.w[i], d.p[i] = float(wi), float(pi)
    return d


def group_A(x, desc):
    """y = A x.  ``x``: contiguous f32 [B][C][H][W] on the current device; returns (B, groups per sample)."""
    B = desc.B
    n = (desc.C * (desc.H // max(desc.r, 1)) * (desc.W // max(desc.r, 1))) if desc.mode == _ext.GROUP_BLOCK else desc.H * desc.W
    out = torch.empty(B, n, device=x.device, dtype=torch.float32)
    check(_ext.load().nlc_group_A(x.data_ptr(), desc, out.data_ptr(), ops._stream()), "nlc_group_A")
    return out


def group_Apinv(y, desc):
    """x = A^+ y (or A^T y with w in the place of p).  Returns (B, C*H*W)."""
    out = torch.empty(desc.B, desc.C * desc.H * desc.W, device=y.device, dtype=torch.float32)
    check(_ext.load().nlc_group_Apinv(y.data_ptr(), desc, out.data_ptr(), ops._stream()), "nlc_group_Apinv")
    return out


def group_project_(x0, y, desc):
    """x0 <- x0 + p (y - A x0), in place, one launch."""
    check(_ext.load().nlc_group_project(x0.data_ptr(), y.data_ptr(), desc, ops._stream()), "nlc_group_project")
    return x0


class _GroupSum:
    """An operator with one weighted sum per group (csrc/restore.hip).  Subclasses set mode / channels / img_dim / ratio and
    the weights of one group."""

    def _setup(self, mode, channels, img_dim, ratio, weights, device):
        self.mode, self.channels, self.img_dim, self.ratio = mode, channels, img_dim, ratio
        self.device = torch.device(device)
        self.w, self.p = group_tables(weights)
        self.groups = channels * (img_dim // ratio) ** 2 if mode == _ext.GROUP_BLOCK else img_dim ** 2
        self._singular = float(np.float32(np.sqrt(np.sum(self.w.astype(np.float64) ** 2))))

    def desc(self, B, transpose=False):
        return group_desc(self.mode, B, self.channels, self.img_dim, self.img_dim, self.ratio, self.w, self.w if transpose else self.p)

    def singulars(self):
        return torch.full((self.groups,), self._singular, device=self.device)

    @ops.on_device
    def A(self, vec):
        x = vec.reshape(vec.shape[0], -1).to(self.device, torch.float32).contiguous()
        if x.shape[1] != self.channels * self.img_dim ** 2:
            raise ValueError("A: vector length mismatch")
        return group_A(x, self.desc(x.shape[0]))

    def _back(self, vec, transpose):
        y = vec.reshape(vec.shape[0], -1).to(self.device, torch.float32).contiguous()
        if y.shape[1] != self.groups:
            raise ValueError("A_pinv: measurement length mismatch")
        return group_Apinv(y, self.desc(y.shape[0], transpose))

    @ops.on_device
    def A_pinv(self, vec):
        return self._back(vec, False)

    @ops.on_device
    def At(self, vec):
        return self._back(vec, True)

    @ops.on_device
    def project_(self, x0, y):
        """x0 <- x0 - A^+(A x0 - y) in place.  ``x0``: contiguous f32 (B, C, H, W) on this device; ``y``: contiguous f32 (B, groups)."""
        _in_place("project_", x0, y, x0.shape[0] * self.channels * self.img_dim ** 2, x0.shape[0] * self.groups)
        return group_project_(x0, y, self.desc(x0.shape[0]))

    @ops.on_device
    def gd_(self, x0, y, lr, n_iter, loss, workspace=None):
        """``n_iter`` steps of x0 <- x0 - lr grad ||A x0 - y||_p in place (``nlc_group_gd``: one launch for l1, two for l2).
        ``x0`` and ``y`` as for ``project_``."""
        _in_place("gd_", x0, y, x0.shape[0] * self.channels * self.img_dim ** 2, x0.shape[0] * self.groups)
        loss = gd_loss_id(loss)
        ws = workspace if workspace is not None else gd_workspace(x0.shape[0], self.groups, loss, x0.device)
        check(_ext.load().nlc_group_gd(x0.data_ptr(), y.data_ptr(), self.desc(x0.shape[0]), float(lr), int(n_iter), loss,
                                       None if ws is None else ws.data_ptr(), ops._stream()), "nlc_group_gd")
        return x0


class SuperResolution(_GroupSum):
    """functions/svd_operators.py:479-533: the mean of every ratio x ratio block; y is (B, C * (img_dim/ratio)^2), channel-major."""

    def __init__(self, channels, img_dim, ratio, device):
        ratio = int(ratio)
        if not 1 <= ratio <= 8:
            raise NlcError(f"SuperResolution: ratio {ratio} outside 1..8")
        if img_dim % ratio != 0:
            raise NlcError(f"SuperResolution: img_dim {img_dim} is not a multiple of ratio {ratio}")
        self.y_dim = img_dim // ratio
        self._setup(_ext.GROUP_BLOCK, channels, img_dim, ratio, [1.0 / ratio ** 2] * ratio ** 2, device)


class Colorization(_GroupSum):
    """functions/svd_operators.py:627-667: grey = 0.3333 R + 0.3334 G + 0.3333 B (the reference's literal weights); y is (B, H*W)."""

    WEIGHTS = (0.3333, 0.3334, 0.3333)

    def __init__(self, img_dim, device):
        self._setup(_ext.GROUP_CHANNEL, 3, img_dim, 1, self.WEIGHTS, device)


GROUP_SUM_CONSTRAINTS = ("sr_averagepooling", "colorization")


def svd_constraint(fn, fn_scale=4, device="cuda:0", base_mask_dir="store/inp_masks", image_size=256, channels=3):
    """src/constraint_functions.py:206-251: the inpainting, ``sr_averagepooling`` and ``colorization`` branches."""
    if fn == "sr_averagepooling":
        return SuperResolution(channels, image_size, int(fn_scale), device)
    if fn == "colorization":
        return Colorization(image_size, device)
    if "inpainting" not in fn:
        raise NotImplementedError(f"constraint '{fn}': only the inpainting, sr_averagepooling and colorization operators are on the "
                                  f"HIP path (SURVEY.md §8 f-1)")
    if fn == "inpainting_random":
        missing_r = torch.randperm(image_size ** 2)[: image_size ** 2 // 2].long() * 3
    elif fn in ("inpainting_ddnm", "inpainting_half"):
        name = "mask.npy" if fn == "inpainting_ddnm" else "mask_half.npy"
        mask = torch.from_numpy(np.load(os.path.join(base_mask_dir, name))).reshape(-1)
        missing_r = torch.nonzero(mask == 0).long().reshape(-1) * 3
    else:
        missing_r = torch.load(os.path.join(base_mask_dir, "mask_random.pt")).long().cpu()
    missing = torch.cat([missing_r, missing_r + 1, missing_r + 2], dim=0)
    return Inpainting(channels, image_size, missing, device)


class AffineInpaint:
    """``partial(affine_svd, A=A, Ap=Ap, y=y)`` (image_sample.py:376-381) as an object the sampling loop can fuse:
    x0 - A^+(A x0 - y) == where(known, A^+ y, x0)."""

    def __init__(self, op: Inpainting, y: torch.Tensor, shape):
        self.op = op
        self.y = y
        self.mask_chw = op.mask_chw
        self.known = op.A_pinv(y).view(*shape).contiguous()

    def __call__(self, x0_t):
        A, Ap = self.op.A, self.op.A_pinv
        flat = x0_t.reshape(x0_t.size(0), -1)
        return x0_t - Ap(A(flat) - self.y.reshape(self.y.size(0), -1)).reshape(*x0_t.size())


class AffineGroup:
    """``partial(affine_svd, A=A, Ap=Ap, y=y)`` (image_sample.py:376-381) for a group-sum operator.  ``project_`` is what the
    sampling loop calls: one ``nlc_group_project`` launch, in place.  Calling the object gives the reference-shaped composition."""

    def __init__(self, op: _GroupSum, y: torch.Tensor, shape):
        self.op = op
        self.shape = tuple(shape)
        self.y = y.reshape(y.shape[0], -1).to(op.device, torch.float32).contiguous()

    def project_(self, x0):
        return self.op.project_(x0, self.y)

    def __call__(self, x0_t):
        A, Ap = self.op.A, self.op.A_pinv
        return x0_t - Ap(A(x0_t.reshape(x0_t.size(0), -1)) - self.y).reshape(*x0_t.size())


class GradientProjection:
    """``partial(affine_proj_GD, infer_fn=Constraint.transform, loss_fn=..., n_iter=...)`` bound to y and lambda_t = lr
    (image_sample.py:344-357,384-399): n_iter steps of x0 <- x0 - lr grad ||A x0 - y||_p, p = 1 ('l1') or 2 ('l2', per sample).
    For these operators A A^T = s^2 I, so the steps collapse to a closed form (csrc/gd.h) and no autograd runs.  ``project_`` is
    what the sampling loop calls, in place; calling the object runs the same kernels on a clone.  Holds no ``mask_chw`` / ``known``
    attribute: the loop must not take it for the fused copy-the-known-pixels projection."""

    def __init__(self, op, y, shape, lr, n_iter, loss):
        self.op, self.shape = op, tuple(shape)
        self.lr, self.n_iter, self.loss = float(lr), int(n_iter), gd_loss_id(loss)
        if isinstance(op, _GroupSum):
            self._target = y.reshape(y.shape[0], -1).to(op.device, torch.float32).contiguous()
            entries = op.groups
        else:
            self._target = op.A_pinv(y).view(*shape).contiguous()           # A^+ y: y on the known entries
            entries = op.channels * op.img_dim ** 2
        self._ws = gd_workspace(self.shape[0], entries, self.loss, self._target.device) if self._target.is_cuda else None

    def project_(self, x0):
        ws = self._ws if x0.shape[0] == self.shape[0] else None
        return self.op.gd_(x0, self._target, self.lr, self.n_iter, self.loss, workspace=ws)

    def __call__(self, x0_t):
        x = x0_t.to(self._target.device, torch.float32).contiguous().clone()
        return self.project_(x).view(*x0_t.size())


PROJECTIONS = ("svd", "svd_gd")


class Constraint_Function:
    """image_sample.py:282-343 for deg='inpainting*' / 'sr_averagepooling' / 'colorization' and proj='svd' / 'svd_gd'."""

    def __init__(self, deg, A_funcs, channels=3, image_size=256, lr=1.0, proj="svd", n_iter=10, loss="l1"):
        if "inp" not in deg and deg not in GROUP_SUM_CONSTRAINTS:
            raise NotImplementedError(deg)
        if proj not in PROJECTIONS:
            raise NotImplementedError(f"projection '{proj}': only {PROJECTIONS} are on the HIP path")
        self.deg, self.op = deg, A_funcs
        self.A, self.Ap = A_funcs.A, A_funcs.A_pinv
        self.proj, self.channels, self.image_size, self.lr = proj, channels, image_size, lr
        self.n_iter, self.gd_loss = int(n_iter), loss
        gd_loss_id(loss)

    def transform(self, x):
        return self.A(x)

    def inv_transform(self, y):
        if self.deg == "colorization":               # image_sample.py:319-320: the grey image on all three channels, not A^+ y
            return y.view(y.shape[0], 1, self.image_size, self.image_size).repeat(1, 3, 1, 1)
        Apy = self.Ap(y).view(y.shape[0], self.channels, self.image_size, self.image_size)
        if self.deg == "inpainting":                 # image_sample.py:321-322
            Apy = Apy + self.Ap(self.A(torch.ones_like(Apy))).reshape(*Apy.shape) - 1
        return Apy

    def constraint_fn(self, x0_t, y, lambda_t=None):
        return self.bind(y, x0_t.shape, lambda_t)(x0_t)

    def bind(self, y, shape, lr=None):
        """The per-batch projection (what evaluate_constraint builds with functools.partial, image_sample.py:648).  ``lr``: the
        step size of svd_gd in the place of ``self.lr`` (affine_proj_GD(x0_t, y, lambda_t, ...): lambda_t is the step size)."""
        if self.proj == "svd_gd":
            return GradientProjection(self.op, y, shape, self.lr if lr is None else lr, self.n_iter, self.gd_loss)
        if isinstance(self.op, _GroupSum):
            return AffineGroup(self.op, y, shape)
        return AffineInpaint(self.op, y, shape)

    def loss(self, x, y):
        y_hat = self.transform(x)
        x_hat = self.inv_transform(y)
        f = torch.linalg.vector_norm(y_hat - y, ord=1, dim=tuple(range(1, y.dim()))).cpu()
        b = torch.linalg.vector_norm(x_hat - x, ord=1, dim=tuple(range(1, x.dim()))).cpu()
        return f, b
