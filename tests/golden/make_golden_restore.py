"""Generate tests/golden/restore_ops.npz and restore_loop.npz from the REFERENCE's SuperResolution / Colorization operators
(functions/svd_operators.py:479-533,627-667).  Runs in the build container only, as make_golden.py does (whose module stubs,
model configuration and ``save`` it reuses); the files it writes are committed and are the only thing the tests read.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_restore.py

restore_ops.npz, per case of tests/restore_refs.py FIXTURE_CASES (keys "<case>/<name>"):
    x, x0         seeded U(-1, 1) inputs (restore_refs.inputs)
    A             reference A(x)                          (B, groups)
    Apinv         reference A_pinv(A)                     (B, C*H*W)
    proj          reference affine_svd(x0, y = A)         (B, C, H, W)          image_sample.py:376-380
    err           the reference's own L-inf error of the three against the float64 closed form (restore_refs), measured here:
                  what a comparison against the reference arrays adds to the kernels' bound
restore_loop.npz, per operator ("sr4" = SuperResolution(3, 32, 4), "color" = Colorization(32)): x_gt, y, z, the final x and the
logged constraint loss of a constrained 10-step DDIM + NLC denoise_loop set up as make_golden.gen_inpaint's.
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

from tests import restore_refs as R  # noqa: E402


def affine_svd(x0_t, y, A, Ap):                                                          # image_sample.py:376-380
    return x0_t - Ap(A(x0_t.reshape(x0_t.size(0), -1)) - y.reshape(y.size(0), -1)).reshape(*x0_t.size())


def reference_op(mode, C, dim, r):
    from functions.svd_operators import Colorization, SuperResolution
    return SuperResolution(C, dim, r, "cpu") if mode == R.BLOCK else Colorization(dim, "cpu")


@torch.no_grad()
def gen_ops():
    arrays = {}
    for mode, C, dim, r in R.FIXTURE_CASES:
        name = R.case_name(mode, C, dim, r)
        op = reference_op(mode, C, dim, r)
        x, x0 = R.inputs(mode, C, dim, r)
        a = op.A(x)
        ap = op.A_pinv(a)
        pr = affine_svd(x0, a, op.A, op.A_pinv)
        err = torch.tensor([(a.double() - R.A64(x, mode, r)).abs().max(),
                            (ap.double().view(x.shape) - R.Apinv64(a, mode, C, dim, r)).abs().max(),
                            (pr.double() - R.project64(x0, a, mode, r)).abs().max()], dtype=torch.float64)
        print(name, "reference's own error (A, A_pinv, proj):", err.tolist())
        arrays.update({f"{name}/x": x, f"{name}/x0": x0, f"{name}/A": a, f"{name}/Apinv": ap, f"{name}/proj": pr, f"{name}/err": err})
    MG.save("restore_ops", **arrays)


@torch.no_grad()
def gen_loop():
    for name, attrs in (("basicsr", {}), ("basicsr.metrics", {}), ("basicsr.metrics.psnr_ssim", dict(calculate_ssim=None)),
                        ("datasets", dict(get_dataset=None))):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    import image_sample as RIS
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
    for tag, deg, mode, r in (("sr4", "sr_averagepooling", R.BLOCK, 4), ("color", "colorization", R.CHANNEL, 1)):
        op = reference_op(mode, C, res, r)
        g = torch.Generator().manual_seed(11)
        x_gt = torch.rand(shape, generator=g) * 2 - 1
        y = op.A(x_gt)
        cf = RIS.Constraint_Function(deg, op.A, op.A_pinv, None, proj="svd", channels=C, image_size=res)
        sch = get_sampler("ddim", 1000, steps, sigma_style="DDIM", start_sigma=100, end_sigma=0, sampler_var="fixedsmall", eta=0.0)
        exp = ImageExperiment(eps, sch, batch_size=B, data_shape=(C, res, res), seed=seed, device="cpu", save_folder="/tmp")
        exp.set_model(eps, sig, learn_epsvar=False)
        exp.set_norm_maxmin(0.0, 54.63)
        exp.set_clip_fn("clamp")
        z = torch.randn(shape, generator=exp.new_gen())
        x, logs = exp.denoise_loop(shape=shape, gen=exp.new_gen(), style="pred",
                                   constrain_fn=partial(affine_svd, y=y, A=op.A, Ap=op.A_pinv), norm_eps=True, refine_prior_sigma=True,
                                   return_log=True, chunk_size=1, constrain_loss=partial(cf.loss, y=y), sigma_pred_threshold=960)
        arrays.update({f"{tag}/x_gt": x_gt, f"{tag}/y": y, f"{tag}/z": z, f"{tag}/x": x, f"{tag}/const_loss": torch.stack(logs[4])})
    MG.save("restore_loop", cfg=json.dumps(dict(res=res, steps=steps, seed=seed, B=B)), **arrays)


if __name__ == "__main__":
    MG._stub_missing_modules()
    torch.manual_seed(0)
    gen_ops()
    gen_loop()
