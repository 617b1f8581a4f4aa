"""image_sample.py with --constraint_proj svd_gd for the three operators and both losses, in process, with the arguments
tests/test_cli_gpu.py uses."""
import math

import pytest

from tests.test_cli_gpu import _run

pytestmark = pytest.mark.gpu

OPERATORS = {"sr4": ("--constraint", "sr_averagepooling", "--constraint_scale", "4"), "colorization": ("--constraint", "colorization"),
             "inpainting": ("--constraint", "inpainting")}


@pytest.mark.parametrize("loss", ["l1", "l2"])
@pytest.mark.parametrize("name", list(OPERATORS))
def test_image_sample_gradient_projection(tmp_path, name, loss):
    flags = OPERATORS[name]
    args, out, saved = _run(tmp_path, "--method", "pred_denoise_base", "--eta", "0", "--clip_fn", "clamp", *flags,
                            "--constraint_proj", "svd_gd", "--constraint_loss", loss)
    assert args.constraint == flags[1] and args.constraint_proj == "svd_gd" and args.constraint_loss == loss
    assert (args.constraint_lr, args.constraint_iter) == (10, 10)                       # the reference's defaults
    for k in ("psner", "const_f_loss", "const_b_loss"):
        assert math.isfinite(saved[k]), k
    assert len(saved["full_log"]["psnr"]) >= 4
    print(f"{name} svd_gd {loss}: psnr {saved['psner']:.3f}, const_f_loss {saved['const_f_loss']:.3e}, const_b_loss {saved['const_b_loss']:.3e}")


def test_image_sample_simple_gd_still_raises(tmp_path):
    with pytest.raises(NotImplementedError):
        _run(tmp_path, "--method", "pred_denoise_base", "--eta", "0", "--clip_fn", "clamp", "--constraint", "sr_averagepooling",
             "--constraint_proj", "simple_gd")
