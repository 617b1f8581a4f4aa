#!/usr/bin/env python3
"""Time per call of the fused 3-D SSIM (metrics.ssim3d = nlc_ssim3d: map launch + finalise launch) on one GPU.

    python tools/ssim_bench.py [--calls 500] [--windows 5]

Shapes: the restoration workload's batch (N = 16, 3 x 256 x 256), one image of it, and the analyze_log call (50 steps x 3 keys x B = 2
states against P = 2 originals at 32 x 32).  Per shape: 20 warm-up calls, then `windows` windows of `calls` back-to-back calls, each
between two device events and closed by one synchronise; the host clock runs around the same window.  One JSON line per shape.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diffusion_nlc_amd import metrics  # noqa: E402

SHAPES = [(16, 16, 3, 256, 256), (1, 1, 3, 256, 256), (50 * 3 * 2, 2, 3, 32, 32)]


def bench(N, P, C, H, W, calls, windows):
    g = torch.Generator().manual_seed(0)
    orig = torch.rand((P, C, H, W), generator=g).cuda()
    sample = (orig.repeat(N // P, 1, 1, 1) + 0.05 * torch.randn((N, C, H, W), generator=g).cuda()).clamp(0, 1).contiguous()
    for _ in range(20):
        metrics.ssim3d(sample, orig)
    torch.cuda.synchronize()
    event_us, host_us = [], []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(calls):
            out = metrics.ssim3d(sample, orig)
        b.record()
        torch.cuda.synchronize()
        host_us.append((time.perf_counter() - t0) / calls * 1e6)
        event_us.append(a.elapsed_time(b) / calls * 1e3)
    return dict(N=N, P=P, C=C, H=H, W=W, calls_per_window=calls, event_us_per_call=event_us, host_us_per_call=host_us,
                input_bytes=4 * (N + P) * C * H * W, mean_ssim=float(out.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench: no GPU - a timing needs one")
    for shape in SHAPES:
        print(json.dumps(bench(*shape, args.calls, args.windows)), flush=True)


if __name__ == "__main__":
    main()
