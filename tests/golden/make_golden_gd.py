"""Generate tests/golden/restore_gd.npz from the REFERENCE's gradient-descent projection: its own ``affine_proj_GD``
(image_sample.py:344-357) with ``Constraint_Function.transform`` and ``const_loss`` (:282-343), set up as :384-399 does, over its own
operators (functions/svd_operators.py).  Runs in the build container only, as make_golden_restore.py does (whose operators and model
set-up it reuses); the file it writes is committed and is the only thing the tests read.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gd.py

Op level, n_iter = 10, lr in {10, 0.5}, both losses (keys "<case>/x0", "<case>/y" and "<case>_lr<lr>_<loss>/out", "/err"):
    block_c3_d8_r8, block_c3_d12_r3, channel_c3_d8_r1      x0, y of tests/gd_refs.measurement
    inpaint                                                C = 3, dim = 8, seeded 50 % mask (gd_refs.inpaint_inputs): x0, known, missing
    out     the reference's affine_proj_GD(x0, y, lr)       (B, C, H, W)
    err     its own L-inf error against the iterated float64 form gd_refs.gd64 / gd64_inpaint, measured here: what a comparison
            against the reference arrays adds to the kernels' bound
Loop level ("loop/<tag>/..."; tags sr4, color, inpaint): the 10-step DDIM + NLC loop of make_golden_restore.gen_loop with svd_gd and the
l2 loss: x_gt, y, z, the final x, the logged constraint loss, lr, and min_rho_over_c = min over all steps, iterations and samples of
rho_k / c (asserted >= 1e-2: no step of the run comes near a sign change of the recurrence).  lr is the first of LOOP_LRS for which
that holds.
"""
from __future__ import annotations

import json
import sys
import types
from functools import partial
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(HERE))

import make_golden as MG  # noqa: E402  (puts the repository root and the reference on sys.path)
import make_golden_restore as MR  # noqa: E402

from tests import gd_refs as G  # noqa: E402
from tests import restore_refs as R  # noqa: E402

LOOP_LRS = (10.0, 5.0, 2.0, 1.0, 0.5)


def reference_image_sample():
    for name, attrs in (("basicsr", {}), ("basicsr.metrics", {}), ("basicsr.metrics.psnr_ssim", dict(calculate_ssim=None)),
                        ("datasets", dict(get_dataset=None))):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    import image_sample as RIS
    assert Path(RIS.__file__).resolve().parent == MG.REF, RIS.__file__
    return RIS


def reference_gd(RIS, deg, op, lr, loss, image_size):
    """image_sample.py:394-399 -> constraint_fn(x0_t, y, lambda_t)."""
    cf = RIS.Constraint_Function(deg, op.A, op.A_pinv, constraint_fn=None, proj="svd_gd", lr=lr, channels=3, image_size=image_size)
    loss_fn = partial(cf.const_loss, ord=1 if "l1" in loss else 2, reduce="sum")
    cf.constraint_fn = partial(RIS.affine_proj_GD, infer_fn=cf.transform, loss_fn=loss_fn, n_iter=G.N_ITER)
    return cf


def reference_inpainting(C, dim, missing):
    from functions.svd_operators import Inpainting
    return Inpainting(C, dim, missing, "cpu")


def gen_ops(RIS):
    arrays = {}
    for mode, C, dim, r in G.GOLDEN_GROUP_CASES:
        name = R.case_name(mode, C, dim, r)
        op = MR.reference_op(mode, C, dim, r)
        deg = "sr_averagepooling" if mode == R.BLOCK else "colorization"
        x0, y = G.measurement(mode, C, dim, r)
        arrays.update({f"{name}/x0": x0, f"{name}/y": y})
        for lr in G.LRS:
            for loss in G.LOSSES:
                out = reference_gd(RIS, deg, op, lr, loss, dim).constraint_fn(x0, y, lr)
                err = (out.double() - G.gd64(x0, y, mode, r, lr, G.N_ITER, loss)).abs().max()
                key = G.gd_name(mode, C, dim, r, lr, loss)
                print(key, "reference's own error:", err.item())
                arrays.update({f"{key}/out": out, f"{key}/err": err})
    C, dim = G.INPAINT_CASE
    x0, missing, mask, known = G.inpaint_inputs()
    op = reference_inpainting(C, dim, missing)
    y = op.A(known)
    assert torch.equal(op.A_pinv(y).view(known.shape), known)
    arrays.update({"inpaint/x0": x0, "inpaint/known": known, "inpaint/missing": missing})
    for lr in G.LRS:
        for loss in G.LOSSES:
            out = reference_gd(RIS, "inpainting", op, lr, loss, dim).constraint_fn(x0, y, lr)
            err = (out.double() - G.gd64_inpaint(x0, mask, known, lr, G.N_ITER, loss)).abs().max()
            print(f"inpaint_lr{lr:g}_{loss}", "reference's own error:", err.item())
            arrays.update({f"inpaint_lr{lr:g}_{loss}/out": out, f"inpaint_lr{lr:g}_{loss}/err": err})
    return arrays


def gen_loop(RIS):
    from diffusion_nlc_amd.filler import fill_state_dict
    from src import script_util
    from src.experiments import ImageExperiment
    from src.schedulers import get_sampler
    eps, sig, _ = script_util.create_simple_sigma_eps_model(MG.simple_namespace(MG.SIMPLE_TINY))
    eps.load_state_dict(fill_state_dict(eps.state_dict(), seed=0))
    sig.load_state_dict(fill_state_dict(sig.state_dict(), seed=1, overrides=MG.SIGMA_OVERRIDES))
    eps.eval(); sig.eval()
    res, C, B, steps, seed = 32, 3, 2, 10, 1234
    shape = (B, C, res, res)
    arrays = {}
    for tag, deg, mode, r in (("sr4", "sr_averagepooling", R.BLOCK, 4), ("color", "colorization", R.CHANNEL, 1), ("inpaint", "inpainting", G.INPAINT, 1)):
        g = torch.Generator().manual_seed(11)
        mask = missing = None
        if mode == G.INPAINT:
            missing_r = torch.randperm(res * res, generator=g)[: res * res // 2].long() * 3
            missing = torch.cat([missing_r, missing_r + 1, missing_r + 2], dim=0)
            op = reference_inpainting(C, res, missing)
            keep = torch.ones(res * res * C, dtype=torch.bool)
            keep[missing] = False
            mask = keep.view(res * res, C).t().float()
        else:
            op = MR.reference_op(mode, C, res, r)
        x_gt = torch.rand(shape, generator=g) * 2 - 1
        y = op.A(x_gt)
        target = op.A_pinv(y).view(shape) if mode == G.INPAINT else y
        for lr in LOOP_LRS:
            cf = reference_gd(RIS, deg, op, lr, "l2", res)
            margins = []

            def constrain(x0_t, cf=cf, lr=lr, margins=margins):
                margins.append(G.min_rho_over_c(x0_t.detach(), target, mode, r, lr, G.N_ITER, mask))
                return cf.constraint_fn(x0_t, y, lr)
            sch = get_sampler("ddim", 1000, steps, sigma_style="DDIM", start_sigma=100, end_sigma=0, sampler_var="fixedsmall", eta=0.0)
            exp = ImageExperiment(eps, sch, batch_size=B, data_shape=(C, res, res), seed=seed, device="cpu", save_folder="/tmp")
            exp.set_model(eps, sig, learn_epsvar=False)
            exp.set_norm_maxmin(0.0, 54.63)
            exp.set_clip_fn("clamp")
            z = torch.randn(shape, generator=exp.new_gen())
            with torch.no_grad():
                x, logs = exp.denoise_loop(shape=shape, gen=exp.new_gen(), style="pred", constrain_fn=constrain, norm_eps=True,
                                           refine_prior_sigma=True, return_log=True, chunk_size=1, constrain_loss=partial(cf.loss, y=y),
                                           sigma_pred_threshold=960)
            print(f"loop {tag} lr {lr:g}: {len(margins)} projections, min rho_k / c = {min(margins):.3e}")
            if min(margins) >= 1e-2:
                break
        assert min(margins) >= 1e-2 and len(margins) == steps, (tag, margins)
        arrays.update({f"loop/{tag}/x_gt": x_gt, f"loop/{tag}/y": y, f"loop/{tag}/z": z, f"loop/{tag}/x": x,
                       f"loop/{tag}/const_loss": torch.stack(logs[4]), f"loop/{tag}/lr": torch.tensor(lr, dtype=torch.float64),
                       f"loop/{tag}/min_rho_over_c": torch.tensor(min(margins), dtype=torch.float64)})
        if missing is not None:
            arrays[f"loop/{tag}/missing"] = missing
    arrays["cfg"] = json.dumps(dict(res=res, steps=steps, seed=seed, B=B, n_iter=G.N_ITER, loss="l2"))
    return arrays


if __name__ == "__main__":
    MG._stub_missing_modules()
    torch.manual_seed(0)
    RIS = reference_image_sample()
    arrays = gen_ops(RIS)
    arrays.update(gen_loop(RIS))
    MG.save("restore_gd", **arrays)
