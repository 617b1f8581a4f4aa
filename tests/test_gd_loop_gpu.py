"""Constrained DDIM + NLC sampling with the gradient-descent projection (svd_gd) against the reference's own ``denoise_loop`` running
its ``affine_proj_GD`` (tests/golden/restore_gd.npz, "loop/...": simple_tiny, 32 x 32, B = 2, 10 steps, the set-up of
tests/test_restore_loop_gpu.py, whose 1e-3 bound is used; l2, n_iter = 10, lr recorded in the fixture; the fixture also records that no
step of the run comes within 1e-2 steps of a sign change of the l2 recurrence), and the fused in-place path against the logged
composition, bit for bit, for both losses.
"""
from functools import partial

import pytest
import torch

from tests.test_nets_gpu import _models
from tests.util import load_npz, max_err

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("conv_policy")]
DEV = "cuda:0"


def _experiment(c):
    from diffusion_nlc_amd.experiments import ImageExperiment
    from diffusion_nlc_amd.schedulers import get_sampler
    eps, sig = _models("simple_tiny", torch.float32)
    s = get_sampler("ddim", 1000, c["steps"], sigma_style="DDIM", start_sigma=100, end_sigma=0, sampler_var="fixedsmall", eta=0.0)
    s.to(DEV)
    exp = ImageExperiment(eps, s, batch_size=c["B"], data_shape=(3, c["res"], c["res"]), seed=c["seed"], device=DEV)
    exp.set_model(eps, sig, learn_epsvar=False)
    exp.set_norm_maxmin(0.0, 54.63)
    exp.set_clip_fn("clamp")
    return exp


def _operator(tag, g, res):
    from diffusion_nlc_amd.constraint_functions import Colorization, Inpainting, SuperResolution
    if tag == "sr4":
        return "sr_averagepooling", SuperResolution(3, res, 4, DEV)
    if tag == "color":
        return "colorization", Colorization(res, DEV)
    return "inpainting_random", Inpainting(3, res, g["loop/inpaint/missing"], DEV)


def _loops(exp, cf, y, shape, logged):
    kw = dict(shape=shape, gen=exp.new_gen(), style="pred", norm_eps=True, refine_prior_sigma=True, chunk_size=1,
              constrain_loss=partial(cf.loss, y=y), sigma_pred_threshold=960)
    if logged:
        return exp.denoise_loop(constrain_fn=partial(cf.constraint_fn, y=y, lambda_t=cf.lr), return_log=True, **kw)
    return exp.denoise_loop(constrain_fn=cf.bind(y, shape), return_log=False, **kw)


@pytest.mark.parametrize("tag", ["sr4", "color", "inpaint"])
def test_gd_loop_matches_the_reference(tag):
    from diffusion_nlc_amd.constraint_functions import Constraint_Function, GradientProjection
    g = load_npz("restore_gd")
    c = g["cfg"]
    res, B = c["res"], c["B"]
    shape = (B, 3, res, res)
    deg, op = _operator(tag, g, res)
    lr = g[f"loop/{tag}/lr"].item()
    assert g[f"loop/{tag}/min_rho_over_c"].item() >= 1e-2
    cf = Constraint_Function(deg, op, channels=3, image_size=res, lr=lr, proj="svd_gd", n_iter=c["n_iter"], loss=c["loss"])
    y = cf.transform(g[f"loop/{tag}/x_gt"])
    assert y.shape == g[f"loop/{tag}/y"].shape and max_err(y.cpu(), g[f"loop/{tag}/y"]) <= 1e-6
    assert isinstance(cf.bind(y, shape), GradientProjection)
    exp = _experiment(c)
    x1, logs = _loops(exp, cf, y, shape, logged=True)
    x2, _ = _loops(exp, cf, y, shape, logged=False)
    e1, e2 = max_err(x1, g[f"loop/{tag}/x"]), max_err(x2.cpu(), g[f"loop/{tag}/x"])
    el = (torch.stack(logs[4]).double() - g[f"loop/{tag}/const_loss"].double()).abs().max().item()
    print(f"gd loop {tag} (lr {lr:g}, l2): L-inf logged {e1:.2e}, fused {e2:.2e}, const-loss abs {el:.2e}")
    assert e1 < 1e-3 and e2 < 1e-3
    assert torch.equal(x1.cpu(), x2.cpu())


@pytest.mark.parametrize("loss", ["l1", "l2"])
@pytest.mark.parametrize("tag", ["sr4", "color", "inpaint"])
def test_fused_and_logged_paths_agree_bit_for_bit(tag, loss):
    """return_log=False (project_ in place between the clip and the x_prev phases) and return_log=True (the callable, on a clone) run
    the same kernels: identical final samples.  The three --constraint_* values change the result."""
    from diffusion_nlc_amd.constraint_functions import Constraint_Function
    g = load_npz("restore_gd")
    c = g["cfg"]
    res, B = c["res"], c["B"]
    shape = (B, 3, res, res)
    deg, op = _operator(tag, g, res)
    exp = _experiment(c)
    finals = {}
    for lr, n_iter, ls in ((10.0, 10, loss), (0.5, 10, loss), (10.0, 3, loss)):
        cf = Constraint_Function(deg, op, channels=3, image_size=res, lr=lr, proj="svd_gd", n_iter=n_iter, loss=ls)
        y = cf.transform(g[f"loop/{tag}/x_gt"])
        if (lr, n_iter) == (10.0, 10):
            x1, _ = _loops(exp, cf, y, shape, logged=True)
        x2, _ = _loops(exp, cf, y, shape, logged=False)
        if (lr, n_iter) == (10.0, 10):
            assert torch.equal(x1.cpu(), x2.cpu())
        assert bool(torch.isfinite(x2).all())
        finals[(lr, n_iter)] = x2.cpu()
    assert not torch.equal(finals[(10.0, 10)], finals[(0.5, 10)]) and not torch.equal(finals[(10.0, 10)], finals[(10.0, 3)])
