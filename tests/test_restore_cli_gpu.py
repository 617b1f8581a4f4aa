"""image_sample.py with the two group-sum degradations, in process, with the arguments tests/test_cli_gpu.py uses."""
import math

import pytest

from tests.test_cli_gpu import _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flags", [("--constraint", "sr_averagepooling", "--constraint_scale", "4", "--clip_fn", "clamp"),
                                   ("--constraint", "colorization", "--clip_fn", "clamp")], ids=["sr4", "colorization"])
def test_image_sample_restoration(tmp_path, flags):
    """No small const_f_loss is asserted: the saved sample is clamped to [0, 1] AFTER the projection, and unlike copying known
    pixels a block-mean (or grey-value) correction can leave the range."""
    args, out, saved = _run(tmp_path, "--method", "pred_denoise_base", "--eta", "0", *flags)
    assert args.constraint == flags[1] and args.constraint_proj == "svd"
    for k in ("psner", "const_f_loss", "const_b_loss"):
        assert math.isfinite(saved[k]), k
    assert len(saved["full_log"]["psnr"]) >= 4
    print(f"{flags[1]}: psnr {saved['psner']:.3f}, const_f_loss {saved['const_f_loss']:.3e}, const_b_loss {saved['const_b_loss']:.3e}")


@pytest.mark.parametrize("flags", [("--constraint", "sr_averagepooling", "--constraint_proj", "ddrm"), ("--constraint", "deblur_gauss")],
                         ids=["sr-ddrm", "deblur"])
def test_image_sample_out_of_scope_raises(tmp_path, flags):
    with pytest.raises(NotImplementedError):
        _run(tmp_path, "--method", "pred_denoise_base", "--eta", "0", "--clip_fn", "clamp", *flags)
