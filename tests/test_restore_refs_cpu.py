"""The yardstick of the restoration tests on the CPU: the float64 closed forms of tests/restore_refs.py reproduce the reference's
SuperResolution / Colorization arrays (tests/golden/restore_ops.npz), and the host side of the feature - tables, argument checks,
the operators that stay out of scope - behaves without a GPU."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from tests import restore_refs as R
from tests.util import load_npz


@pytest.mark.parametrize("mode,C,dim,r", R.FIXTURE_CASES, ids=[R.case_name(*c) for c in R.FIXTURE_CASES])
def test_closed_forms_reproduce_the_reference(mode, C, dim, r):
    """Within the reference's recorded own error plus the kernels' bound; the recorded errors themselves stay at the few-ulp level
    (A <= 1e-7, A_pinv <= 3e-7 - exact for r = 4, 8 and 1 -, projection <= 5e-7)."""
    g = load_npz("restore_ops")
    name = R.case_name(mode, C, dim, r)
    x, x0, a, ap, pr, err = (g[f"{name}/{k}"] for k in ("x", "x0", "A", "Apinv", "proj", "err"))
    xs, x0s = R.inputs(mode, C, dim, r)
    assert torch.equal(x, xs) and torch.equal(x0, x0s)
    assert bool(((a.double() - R.A64(x, mode, r)).abs() <= R.bound_A(x, mode, r) + err[0]).all())
    assert bool(((ap.double().view(x.shape) - R.Apinv64(a, mode, C, dim, r)).abs() <= R.bound_Apinv(a, mode, C, dim, r) + err[1]).all())
    assert bool(((pr.double() - R.project64(x0, a, mode, r)).abs() <= R.bound_project(x0, a, mode, r) + err[2]).all())
    assert err[0] <= 1e-7 and err[1] <= 3e-7 and err[2] <= 5e-7
    if mode == R.BLOCK and r in (1, 4, 8):
        assert err[1] == 0.0
    # the layouts: block means channel-major, the grey image pixel-major
    if mode == R.BLOCK:
        want = torch.nn.functional.avg_pool2d(x.double(), r).reshape(x.shape[0], -1)
    else:
        want = (x.double() * R.tables(mode, r)[0].view(1, 3, 1, 1)).sum(1).reshape(x.shape[0], -1)
    assert (R.A64(x, mode, r) - want).abs().max() < 1e-15 + 1e-7 * (mode == R.BLOCK and r == 3)      # f32(1/9) is not 1/9
    # algebra of the closed forms themselves: A A^+ = 1 up to the rounding of the tables, the projection lands on y
    w, p = R.tables(mode, r)
    assert abs(float((w * p).sum()) - 1.0) < 2 * R.U32 * 2
    assert (R.A64(R.project64(x0, a, mode, r), mode, r) - a.double()).abs().max() < 1e-6


def test_host_tables_are_the_yardsticks():
    from diffusion_nlc_amd import constraint_functions as cf
    for r in range(1, 9):
        w, p = cf.group_tables([1.0 / r ** 2] * r ** 2)
        rw, rp = R.tables(R.BLOCK, r)
        assert w.dtype == np.float32 and np.array_equal(w.astype(np.float64), rw.numpy()) and np.array_equal(p, np.ones(r * r, np.float32))
        assert np.array_equal(p.astype(np.float64), rp.numpy())
    w, p = cf.group_tables(cf.Colorization.WEIGHTS)
    rw, rp = R.tables(R.CHANNEL, 1)
    assert np.array_equal(w.astype(np.float64), rw.numpy()) and np.array_equal(p.astype(np.float64), rp.numpy())
    assert cf.Colorization.WEIGHTS == R.COLOR_WEIGHTS
    assert float(np.float32(0.2)) != 0.2 and np.array_equal(cf.group_tables([0.2] * 4)[1], np.float32([1.25] * 4))     # uniform, not a mean


def test_group_entry_points_reject_bad_descriptors_on_the_host():
    """NLC_REQUIRE, before anything is launched (no GPU needed)."""
    from diffusion_nlc_amd import _ext
    from diffusion_nlc_amd import constraint_functions as cf
    lib = _ext.load()
    mem = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(mem)
    w, p = cf.group_tables([0.25] * 4)
    ok = cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 8, 8, 2, w, p)
    assert ctypes.sizeof(ok) == 6 * 4 + 2 * 64 * 4
    bad = [(cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 10, 8, 4, w, p), b"multiples"), (cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 8, 10, 4, w, p), b"multiples"),
           (cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 18, 18, 9, w, p), b"outside 1..8"), (cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 8, 8, 0, w, p), b"outside 1..8"),
           (cf.group_desc(_ext.GROUP_CHANNEL, 2, 1, 8, 8, 1, w, p), b"C = 3"), (cf.group_desc(_ext.GROUP_BLOCK, 0, 3, 8, 8, 2, w, p), b"B = 0"),
           (cf.group_desc(_ext.GROUP_BLOCK, 65536, 3, 8, 8, 2, w, p), b"B = 65536"), (cf.group_desc(2, 2, 3, 8, 8, 2, w, p), b"mode")]
    for d, word in bad:
        for rc in (lib.nlc_group_A(ptr, d, ptr, None), lib.nlc_group_Apinv(ptr, d, ptr, None), lib.nlc_group_project(ptr, ptr, d, None)):
            assert rc == _ext.NLC_EINVAL and word in lib.nlc_last_error(), (word, lib.nlc_last_error())
    for rc in (lib.nlc_group_A(None, ok, ptr, None), lib.nlc_group_A(ptr, ok, None, None), lib.nlc_group_Apinv(None, ok, ptr, None),
               lib.nlc_group_project(None, ptr, ok, None), lib.nlc_group_project(ptr, None, ok, None)):
        assert rc == _ext.NLC_EINVAL and b"null" in lib.nlc_last_error()


def test_scope_of_the_constraint_layer():
    """sr_averagepooling / colorization are built; everything else the reference's --constraint offers beyond inpainting, and
    ddrm with the new operators, still raises NotImplementedError."""
    import image_sample
    from diffusion_nlc_amd import constraint_functions as cf
    from diffusion_nlc_amd._ext import NlcError
    sr = cf.svd_constraint("sr_averagepooling", fn_scale=4.0, device="cpu", image_size=32, channels=3)
    assert isinstance(sr, cf.SuperResolution) and (sr.ratio, sr.y_dim, sr.channels, sr.img_dim) == (4, 8, 3, 32)
    assert sr.singulars().shape == (3 * 64,) and sr.singulars()[0].item() == 0.25
    co = cf.svd_constraint("colorization", device="cpu", image_size=32)
    assert isinstance(co, cf.Colorization) and co.singulars().shape == (1024,) and co.channels == 3
    for name in ("sr_bicubic", "deblur_gauss", "cs_walshhadamard", "denoising"):
        with pytest.raises(NotImplementedError):
            cf.svd_constraint(name, device="cpu", image_size=32)
        with pytest.raises(NotImplementedError):
            cf.Constraint_Function(name, sr)
    with pytest.raises(NlcError):
        cf.svd_constraint("sr_averagepooling", fn_scale=5, device="cpu", image_size=32)
    for deg, op in (("sr_averagepooling", sr), ("colorization", co)):
        c = cf.Constraint_Function(deg, op, channels=3, image_size=32)
        assert c.proj == "svd" and isinstance(c.bind(torch.zeros(2, op.groups), (2, 3, 32, 32)), cf.AffineGroup)
    y = torch.arange(2 * 1024, dtype=torch.float32).view(2, 1024)
    grey = cf.Constraint_Function("colorization", co, image_size=32).inv_transform(y)           # image_sample.py:319-320
    assert grey.shape == (2, 3, 32, 32) and all(torch.equal(grey[:, c].reshape(2, -1), y) for c in range(3))
    ns = argparse.Namespace(constraint_scale=4.0, device="cpu", synthetic="cifar_tiny", constraint_lr=1.0)
    for constraint, proj in (("sr_averagepooling", "ddrm"), ("colorization", "ddrm"), ("deblur_gauss", "svd"), ("sr_averagepooling", "simple")):
        ns.constraint, ns.constraint_proj = constraint, proj
        with pytest.raises(NotImplementedError):
            image_sample.get_constraint_function(ns, 32, 3)
    ns.constraint, ns.constraint_proj = "sr_averagepooling", "svd"
    assert isinstance(image_sample.get_constraint_function(ns, 32, 3).op, cf.SuperResolution)
