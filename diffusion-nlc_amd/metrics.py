"""Image-quality metrics of restoration runs on the HIP path.

``ssim3d`` is the reference's SSIM: ``ssim_fn`` (``image_sample.py:571-582``) -> ``calculate_ssim(crop_border=0,
test_y_channel=False)`` with its default ``ssim3d=True`` -> ``_ssim_3d`` (``basicsr/metrics/psnr_ssim.py:157-208,251-337``).  The
reference needs cv2 and the vendored BasicSR tree and rebuilds an 11 x 11 x 11 Conv3d per image; ``nlc_ssim3d`` (csrc/ssim.hip)
computes the whole batch in one fused launch plus one small reduction, with nothing but the inputs read from global memory.
"""
from __future__ import annotations

import torch

from . import _ext
from ._ext import NlcError, check

_workspaces = {}        # (device, N, C, H, W) -> float64 tensor of nlc_ssim3d_workspace_bytes


def _workspace(device, N, C, H, W):
    key = (device, N, C, H, W)
    ws = _workspaces.get(key)
    if ws is None:
        n = _ext.load().nlc_ssim3d_workspace_bytes(N, C, H, W)
        if n <= 0:
            raise NlcError(f"ssim3d: unsupported shape N={N} C={C} H={H} W={W} (C is 1..4, H and W 1..65536)")
        ws = _workspaces[key] = torch.empty(n // 8, dtype=torch.float64, device=device)
    return ws


def ssim3d(sample, orig):
    """3-D SSIM of ``sample[n]`` against ``orig[n % P]``: contiguous float32 CUDA tensors (N, C, H, W) and (P, C, H, W) in [0, 1] on
    one device, P dividing N.  Returns a float64 tensor (N,) on that device; the same input gives the same bits on every call.
    Nothing is moved or converted for the caller: anything else raises NlcError."""
    for name, t in (("sample", sample), ("orig", orig)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
            raise NlcError(f"ssim3d: {name} must be a contiguous float32 CUDA tensor (N, C, H, W)")
    if sample.device != orig.device or sample.shape[1:] != orig.shape[1:]:
        raise NlcError(f"ssim3d: sample {tuple(sample.shape)} on {sample.device} and orig {tuple(orig.shape)} on {orig.device} do not match")
    N, C, H, W = sample.shape
    P = orig.shape[0]
    if N < 1 or P < 1 or P > N or N % P:
        raise NlcError(f"ssim3d: {P} originals do not divide {N} samples")
    with torch.cuda.device(sample.device):
        ws = _workspace(sample.device, N, C, H, W)
        out = torch.empty(N, dtype=torch.float64, device=sample.device)
        check(_ext.load().nlc_ssim3d(sample.data_ptr(), orig.data_ptr(), N, P, C, H, W, out.data_ptr(), ws.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "nlc_ssim3d")
    return out
