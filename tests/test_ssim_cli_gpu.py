"""Restoration runs report SSIM: image_sample.py's results.json carries a finite ``ssim`` and the per-image list, and
evaluate_constraint(return_log=True) adds analyze_log's per-step table (reference image_sample.py:584-606,675,687,698,706-707)."""
import math
from functools import partial

import numpy as np
import pytest
import torch

from tests.test_cli_gpu import _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flags", [("--constraint", "inpainting", "--clip_fn", "clamp"),
                                   ("--constraint", "sr_averagepooling", "--constraint_scale", "4", "--clip_fn", "clamp")],
                         ids=["inpainting", "sr4"])
def test_results_json_carries_ssim(tmp_path, flags):
    args, out, saved = _run(tmp_path, "--method", "pred_denoise_base", "--eta", "0", *flags)
    assert math.isfinite(saved["ssim"]) and -1.0 < saved["ssim"] <= 1.0
    full = saved["full_log"]
    assert len(full["ssim"]) == len(full["psnr"]) >= 4
    assert all(math.isfinite(v) and -1.0 < v <= 1.0 for v in full["ssim"])
    assert saved["ssim"] == float(np.mean(full["ssim"])) == out["ssim"]
    assert list(full)[:3] == ["psnr", "mse", "ssim"]                   # the reference's key order
    assert saved["full_results"] == []                                 # the CLI keeps return_log off for constrained runs
    print(f"{flags[1]}: ssim {saved['ssim']:.6f}, psnr {saved['psner']:.3f}")


def test_evaluate_constraint_return_log_fills_full_results(tmp_path):
    """simple_tiny, 32 x 32, B = 2, 4 DDIM steps, x4 super-resolution: full_results[0] has the three keys with one entry per step,
    and its SSIM entries are what ssim_fn gives on the same logged tensors."""
    import image_sample
    from diffusion_nlc_amd.constraint_functions import Constraint_Function, SuperResolution
    from diffusion_nlc_amd.experiments import ImageExperiment
    from diffusion_nlc_amd.schedulers import get_sampler
    from tests.test_nets_gpu import _models
    res, B, steps = 32, 2, 4
    eps, sig = _models("simple_tiny", torch.float32)
    s = get_sampler("ddim", 1000, steps, sigma_style="DDIM", start_sigma=100, end_sigma=0, sampler_var="fixedsmall", eta=0.0)
    s.to("cuda:0")
    exp = ImageExperiment(eps, s, batch_size=B, data_shape=(3, res, res), seed=3, device="cuda:0")
    exp.set_model(eps, sig, learn_epsvar=False)
    exp.set_norm_maxmin(0.0, 54.63)
    exp.set_clip_fn("clamp")
    cf = Constraint_Function("sr_averagepooling", SuperResolution(3, res, 4, "cuda:0"), channels=3, image_size=res)
    x_orig = torch.rand((B, 3, res, res), generator=torch.Generator().manual_seed(11))
    loader = [(x_orig, torch.zeros(B, dtype=torch.long))]
    log, return_list = image_sample.evaluate_constraint(exp, loader, cf, str(tmp_path), norm_init_noise=False, style="pred", sampling="denoise",
                                                        norm_eps=True, refine_prior_sigma=True, return_log=True, save_images=False)
    assert len(log["full_results"]) == 1 and len(log["full_log"]["ssim"]) == B and math.isfinite(log["ssim"])
    table = log["full_results"][0]
    assert list(table) == ["zt", "z0_prec", "z0_postc"]
    z_list, eps_list, x0_prec_list, x0_postc_list = return_list[:4]
    assert len(eps_list) == steps
    y = cf.transform(2 * x_orig.to("cuda:0") - 1.0)
    for key, states in zip(table, (z_list, x0_prec_list, x0_postc_list)):
        assert list(table[key]) == ["psnr", "ssim", "const"] and all(len(table[key][k]) == steps for k in table[key])
        for kk in range(steps):
            sample = states[kk].add(1).div(2).clamp(0, 1)
            assert table[key]["ssim"][kk] == float(np.mean(image_sample.ssim_fn(sample, x_orig))), (key, kk)
            psnr = (10 * torch.log10(1 / torch.mean((sample - x_orig) ** 2))).item()
            assert table[key]["psnr"][kk] == pytest.approx(psnr, rel=1e-6)
            const = torch.mean(partial(cf.loss, y=y)(2 * sample.to("cuda:0") - 1.0)[0]).item()
            assert table[key]["const"][kk] == pytest.approx(const, rel=1e-5, abs=1e-7)
        assert all(math.isfinite(v) and -1.0 < v <= 1.0 for v in table[key]["ssim"])
    print("zt ssim", table["zt"]["ssim"], "z0_postc ssim", table["z0_postc"]["ssim"])
