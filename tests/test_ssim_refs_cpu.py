"""The yardsticks of the 3-D SSIM metric on the CPU (tests/ssim_refs.py), and the host side of its entry points.

No fixture from the reference's own ssim_fn is checked here: that function imports cv2 and scikit-image, which a fixture maker
could not replace within its brief, so the metric rests on ssim64 (the float64 closed form), on a float64 dense Conv3d written
separately from it, and on ssim32 (the reference's f32 arithmetic)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ssim_refs as S


def test_channel_matrix():
    for C in (1, 2, 3, 4):
        M = S.channel_matrix(C)
        assert M.shape == (C, C) and np.allclose(M.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    one = S.channel_matrix(1)                                      # C = 1 gives [1]: the taps' float64 sum, 1.0f once rounded to f32
    assert one.shape == (1, 1) and abs(one[0, 0] - 1.0) <= 1e-15 and np.float32(one[0, 0]) == np.float32(1.0)
    # C = 3 against the brute-force padded form: filter the replicate-padded unit vectors
    g = S.gauss()
    brute = np.zeros((3, 3))
    for k in range(3):
        padded = np.pad(np.eye(3)[k], S.RAD, mode="edge")
        for c in range(3):
            brute[c, k] = sum(g[j] * padded[c + j] for j in range(S.TAPS))
    assert np.allclose(S.channel_matrix(3), brute, rtol=0, atol=1e-16)
    assert abs(g.sum() - 1.0) <= 1e-15 and np.array_equal(g, g[::-1]) and S.weight_table().shape == (11, 11, 11)


def test_quantiser_is_one_f32_product_rounded_half_to_even():
    """What the kernel does - rint of the f32 product, nothing clamped inside [0, 1] - is torch.round(x * 255).to(torch.uint8), on
    a grid that holds every x = f32((k + 0.5) / 255) and its two neighbours, the end points and a dense ramp."""
    x = torch.cat([S.half_way_grid(3 * 255), torch.linspace(0, 1, 100001), torch.tensor([0.0, 1.0, 0.5 / 255, 254.5 / 255])])
    want = S.quantise(x)
    prod = x.numpy().astype(np.float32) * np.float32(255)
    assert prod.dtype == np.float32
    got = np.rint(prod)
    assert got.min() >= 0 and got.max() <= 255
    assert np.array_equal(got.astype(np.uint8), want.numpy())
    ties = prod[np.abs(prod - np.floor(prod) - 0.5) == 0]
    assert ties.size >= 100 and np.array_equal(np.rint(ties) % 2, np.zeros_like(ties))      # the grid does hit exact ties: to even


def _dense64(sample, orig):
    """The operator once more, written apart from ssim64: a float64 dense Conv3d with the f32-rounded table."""
    a = S.quantise(sample).permute(1, 2, 0).double()
    b = S.quantise(orig).permute(1, 2, 0).double()
    mv = 1.0 if a.max().item() <= 1 else 255.0
    C1, C2 = (0.01 * mv) ** 2, (0.03 * mv) ** 2
    w = S.weight_table().double()[None, None]
    E = lambda v: F.conv3d(F.pad(v[None, None], (5,) * 6, mode="replicate"), w)[0, 0]                   # noqa: E731
    mu1, mu2 = E(a), E(b)
    s1, s2, s12 = E(a * a) - mu1 * mu1, E(b * b) - mu2 * mu2, E(a * b) - mu1 * mu2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean().item()


@pytest.mark.parametrize("name", [n for n in S.CASES if "256" not in n])
def test_ssim64_is_the_dense_form(name):
    sample, orig, want = S.case(name)
    P = orig.shape[0]
    for n in range(sample.shape[0]):
        assert abs(_dense64(sample[n], orig[n % P]) - want[n].item()) <= 1e-11, name


def test_ssim64_properties():
    assert torch.equal(S.case("same_40x70")[2], torch.ones(1, dtype=torch.float64))
    dim, bright = S.case("dim_40x70"), S.case("dim_one_bright_40x70")
    assert S.quantise(dim[0]).max().item() == 1 and S.quantise(bright[0]).max().item() == 2
    assert (S.quantise(dim[0]) != S.quantise(bright[0])).sum().item() == 1 and torch.equal(dim[1], bright[1])   # one pixel apart ...
    assert abs(dim[2].item() - bright[2].item()) > 4 * S.GATE_TEXTURED                   # ... and the constants switch, visibly at the gate
    sample, orig, want = S.case("noisy_p2_n6")
    assert torch.equal(want, S.ssim64(sample, orig.repeat(3, 1, 1, 1)))
    assert bool((want.abs() <= 1).all())


def test_e32_constants_cover_the_measurement():
    """E32 = max |ssim32 - ssim64| over all cases, re-measured: the constants in ssim_refs.py may not lie below it, and not far
    above it either (a constant ten per cent above its measurement would be a wider gate than the rule gives)."""
    worst = {True: (0.0, None), False: (0.0, None)}
    for name in S.CASES:
        sample, orig, want = S.case(name)
        e = (S.ssim32(sample, orig) - want).abs().max().item()
        print(f"{name:24s} ssim64 {want[0].item():+.9f}  |ssim32 - ssim64| {e:.4e}")
        if e > worst[name in S.FLAT][0]:
            worst[name in S.FLAT] = (e, name)
    e_all, at_all = max(worst.values())
    e_tex, at_tex = worst[False]
    print(f"E32 = max |ssim32 - ssim64| over {len(S.CASES)} cases = {e_all:.4e} (at {at_all}); without the FLAT cases {e_tex:.4e} (at {at_tex})")
    assert e_all <= S.E32_MEASURED <= 1.1 * e_all
    assert e_tex <= S.E32_TEXTURED_MEASURED <= 1.1 * e_tex
    assert S.GATE == 4 * S.E32_MEASURED and S.GATE_TEXTURED == 4 * S.E32_TEXTURED_MEASURED and S.GATE_TEXTURED < S.GATE


def test_ssim_entry_points_reject_bad_arguments_on_the_host():
    """NLC_REQUIRE, before anything is launched (no GPU needed)."""
    from diffusion_nlc_amd import _ext
    lib = _ext.load()
    assert lib.nlc_version() == _ext.ABI_VERSION == 10                  # additive: the ABI version does not move
    mem = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(mem)
    assert ptr % 8 == 0

    def call(s=ptr, o=ptr, N=4, P=2, C=3, H=8, W=8, out=ptr, ws=ptr):
        return lib.nlc_ssim3d(s, o, N, P, C, H, W, out, ws, None)
    bad = [(dict(s=None), b"null"), (dict(o=None), b"null"), (dict(out=None), b"null"), (dict(ws=None), b"null"),
           (dict(C=0), b"C = 0"), (dict(C=5), b"C = 5"), (dict(N=0), b"shape"), (dict(N=-1), b"shape"), (dict(H=0), b"shape"),
           (dict(W=-3), b"shape"), (dict(H=65537), b"above"), (dict(P=3), b"divide"), (dict(P=0), b"divide"), (dict(P=8), b"divide"),
           (dict(ws=ptr + 4), b"aligned"), (dict(out=ptr + 4), b"aligned"), (dict(s=ptr + 2), b"aligned")]
    for kw, word in bad:
        assert call(**kw) == _ext.NLC_EINVAL and word in lib.nlc_last_error(), (kw, lib.nlc_last_error())
    # three doubles per 16 x 32 tile and pair
    wb = lib.nlc_ssim3d_workspace_bytes
    assert wb(1, 3, 1, 1) == 24 and wb(2, 1, 16, 32) == 48 and wb(1, 4, 17, 33) == 4 * 24 and wb(16, 3, 256, 256) == 16 * 128 * 24
    assert wb(0, 3, 8, 8) == 0 and wb(1, 0, 8, 8) == 0 and wb(1, 5, 8, 8) == 0 and wb(1, 3, 0, 8) == 0 and wb(1, 3, 8, 65537) == 0


def test_metrics_module_rejects_host_tensors_without_a_gpu():
    from diffusion_nlc_amd import metrics
    from diffusion_nlc_amd._ext import NlcError
    x = torch.rand(2, 3, 8, 8)
    with pytest.raises(NlcError):
        metrics.ssim3d(x, x)


def test_image_sample_has_the_reference_signatures():
    import image_sample
    assert list(inspect.signature(image_sample.ssim_fn).parameters) == ["sample", "orig"]
    assert list(inspect.signature(image_sample.analyze_log).parameters) == ["return_list", "x_orig", "y", "constrain_loss"]
    assert "return_log" in inspect.signature(image_sample.evaluate_constraint).parameters
