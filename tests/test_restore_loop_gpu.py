"""Constrained DDIM + NLC sampling with the super-resolution (x4) and colorization operators against the reference's own
``denoise_loop`` (tests/golden/restore_loop.npz: simple_tiny, 32 x 32, B = 2, 10 steps, style 'pred', norm_eps, refine_prior_sigma,
clip 'clamp', sigma_pred_threshold 960 - the set-up of test_inpainting_operator_and_constrained_loop, whose 1e-3 bound is used).

Measured on an MI355X (f32): L-inf to the reference's x  sr4 1.83e-4 (reference-shaped) / 1.83e-4 (bound), the two runs bit-equal;
color 1.48e-4 / 1.37e-4, 1.11e-4 between the two; logged loss within 2.96e-5 / 2.34e-4 absolute; |A x - y| of the returned sample
5.1e-8 / 6.6e-8 against bounds of 1.5e-6 / 5.9e-7.
"""
from functools import partial

import pytest
import torch

from tests import restore_refs as R
from tests.test_nets_gpu import _models
from tests.util import load_npz, max_err

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("conv_policy")]


@pytest.mark.parametrize("tag,deg,mode,r", [("sr4", "sr_averagepooling", R.BLOCK, 4), ("color", "colorization", R.CHANNEL, 1)])
def test_constrained_loop_matches_the_reference(tag, deg, mode, r):
    from diffusion_nlc_amd.constraint_functions import AffineGroup, Colorization, Constraint_Function, SuperResolution
    from diffusion_nlc_amd.experiments import ImageExperiment
    from diffusion_nlc_amd.schedulers import get_sampler
    g = load_npz("restore_loop")
    c = g["cfg"]
    res, B = c["res"], c["B"]
    shape = (B, 3, res, res)
    op = SuperResolution(3, res, r, "cuda:0") if mode == R.BLOCK else Colorization(res, "cuda:0")
    cf = Constraint_Function(deg, op, channels=3, image_size=res)
    y = cf.transform(g[f"{tag}/x_gt"])
    assert y.shape == g[f"{tag}/y"].shape and max_err(y.cpu(), g[f"{tag}/y"]) <= float(R.bound_A(g[f"{tag}/x_gt"], mode, r).max()) + 1e-7
    eps, sig = _models("simple_tiny", torch.float32)
    s = get_sampler("ddim", 1000, c["steps"], sigma_style="DDIM", start_sigma=100, end_sigma=0, sampler_var="fixedsmall", eta=0.0)
    s.to("cuda:0")
    exp = ImageExperiment(eps, s, batch_size=B, data_shape=(3, res, res), seed=c["seed"], device="cuda:0")
    exp.set_model(eps, sig, learn_epsvar=False)
    exp.set_norm_maxmin(0.0, 54.63)
    exp.set_clip_fn("clamp")
    # (1) reference-shaped: generic callable x0 - A^+(A x0 - y), per-step constraint loss, logging on
    x1, logs = exp.denoise_loop(shape=shape, gen=exp.new_gen(), style="pred", constrain_fn=partial(cf.constraint_fn, y=y), norm_eps=True,
                                refine_prior_sigma=True, return_log=True, chunk_size=1, constrain_loss=partial(cf.loss, y=y),
                                sigma_pred_threshold=960)
    e1 = max_err(x1, g[f"{tag}/x"])
    el = (torch.stack(logs[4]).double() - g[f"{tag}/const_loss"].double()).abs().max().item()
    # (2) bound: one nlc_group_project launch per constrained step, between the clip and the x_prev phases of the scheduler kernel
    bound = cf.bind(y, shape)
    assert isinstance(bound, AffineGroup)
    calls, seen = [], []
    inner = bound.project_

    def counting(x0):
        calls.append(x0.data_ptr())
        out = inner(x0)
        assert out is x0                                        # in place: no copy, no temporary
        seen.append(x0)
        return out
    bound.project_ = counting
    x2, _ = exp.denoise_loop(shape=shape, gen=exp.new_gen(), style="pred", constrain_fn=bound, norm_eps=True, refine_prior_sigma=True,
                             return_log=False, chunk_size=1, constrain_loss=partial(cf.loss, y=y), sigma_pred_threshold=960,
                             return_on_device=True)
    assert len(calls) == c["steps"]
    e2 = max_err(x2.cpu(), g[f"{tag}/x"])
    e12 = max_err(x1, x2.cpu())
    print(f"restore loop {tag}: L-inf reference-shaped {e1:.2e}, bound {e2:.2e}, between the two {e12:.2e}, const-loss abs {el:.2e}")
    assert e1 < 1e-3 and e2 < 1e-3 and el < 1e-3
    assert e12 < 1e-3
    # the returned sample IS one of the projected x0 (the step with the best constraint loss), unclamped: it satisfies the
    # measurement within the op bound
    assert x2.data_ptr() in calls
    xf = x2.cpu()
    resid = (R.A64(xf, mode, r) - y.cpu().double()).abs()
    lim = R.bound_A(xf, mode, r)
    print(f"    |A x - y| max {resid.max().item():.2e}, bound max {lim.max().item():.2e}, max(resid - bound) {(resid - lim).max().item():.2e}")
    assert bool((resid <= lim).all())
