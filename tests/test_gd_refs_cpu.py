"""The yardstick of the gradient-descent projection on the CPU: the iterated float64 form of tests/gd_refs.py is what
torch.autograd gives through CPU operators, its bound holds for a literal float32 iteration and for the reference's own arrays
(tests/golden/restore_gd.npz), the guard leaves out no more than the caps, and the host side - argument checks of the two entry
points, the constraint layer's scope - behaves without a GPU."""
import argparse
import ctypes
import math

import pytest
import torch

from tests import gd_refs as G
from tests import restore_refs as R
from tests.util import load_npz

AUTOGRAD_CASES = [(R.BLOCK, 3, 8, 4), (R.BLOCK, 3, 12, 3), (R.BLOCK, 3, 600, 2), (R.CHANNEL, 3, 8, 1)]


def _autograd_gd(x0, y, A, lr, n_iter, ord_):
    """affine_proj_GD (image_sample.py:344-357) with loss_fn = const_loss(ord, reduce='sum') (:335-342,397), in x0's dtype."""
    x = x0
    for _ in range(n_iter):
        X = x.clone().detach().requires_grad_(True)
        loss = torch.linalg.vector_norm(A(X) - y, ord=ord_, dim=1).sum()
        x = (X - lr * torch.autograd.grad(loss, X)[0]).detach()
    return x


def _cpu_operator(mode, r, dtype):
    if mode == R.BLOCK:
        return lambda X: torch.nn.functional.avg_pool2d(X, r).reshape(X.shape[0], -1)
    w = R.tables(mode, r)[0].to(dtype).view(1, 3, 1, 1)
    return lambda X: (X * w).sum(1).reshape(X.shape[0], -1)


@pytest.mark.parametrize("loss", G.LOSSES)
@pytest.mark.parametrize("lr", G.LRS)
@pytest.mark.parametrize("mode,C,dim,r", AUTOGRAD_CASES, ids=[R.case_name(*c) for c in AUTOGRAD_CASES])
def test_iterated_form_is_what_autograd_gives(mode, C, dim, r, lr, loss):
    """In float64 the two agree to rounding (avg_pool2d divides by 9 where the table holds float32(1/9): 6e-8 relative on every step
    of r = 3).  In float32 the autograd loop IS a literal iteration: it must lie within bound_gd outside the guard, which tests the
    bound against something that is not the kernel."""
    x0, y = G.measurement(mode, C, dim, r)
    want, bound, keep, left = G.case64(mode, C, dim, r, lr, G.N_ITER, loss)
    got64 = _autograd_gd(x0.double(), y.double(), _cpu_operator(mode, r, torch.float64), lr, G.N_ITER, G.loss_id(loss))
    e64 = ((got64 - want).abs() * keep).max().item()
    got32 = _autograd_gd(x0, y, _cpu_operator(mode, r, torch.float32), lr, G.N_ITER, G.loss_id(loss))
    err = (got32.double() - want).abs()
    slack = 2e-6 if r == 3 else 0.0                                  # avg_pool2d's 1/9 against the table's float32(1/9), as above
    print(f"f64 autograd {e64:.2e}; f32 autograd max err {(err * keep).max().item():.2e}, max bound {bound.max().item():.2e}, left out {left:.2e}")
    assert e64 <= 1e-12 + slack
    assert bool((err <= bound + slack)[keep].all())
    assert left <= (G.CAP_WRAP if dim == 600 else 0.0)


def test_inpainting_form_is_what_autograd_gives():
    x0, missing, mask, known = G.inpaint_inputs()
    act = (mask.reshape(-1) != 0)
    for lr in G.LRS:
        for loss in G.LOSSES:
            want, bound, keep, left = G.inpaint64(x0, mask, known, lr, G.N_ITER, loss)
            A = lambda X: X.reshape(X.shape[0], -1)[:, act]             # noqa: E731
            got = _autograd_gd(x0.double(), A(known.double()), A, lr, G.N_ITER, G.loss_id(loss))
            assert (got - want).abs().max().item() <= 1e-12 and left == 0.0
            assert torch.equal(want[:, mask.view(3, 8, 8) == 0], x0.double()[:, mask.view(3, 8, 8) == 0])      # missing entries never move
            got32 = _autograd_gd(x0, A(known), A, lr, G.N_ITER, G.loss_id(loss))
            assert bool(((got32.double() - want).abs() <= bound)[keep].all())


def test_iteration_count_and_step_size_matter():
    """The yardstick itself honours n_iter, lr and the loss (the GPU tests compare runs that differ in one of them)."""
    mode, C, dim, r = R.BLOCK, 3, 12, 4
    x0, y = G.measurement(mode, C, dim, r)
    a = G.gd64(x0, y, mode, r, 0.5, 10, "l1")
    assert not torch.equal(a, G.gd64(x0, y, mode, r, 0.5, 1, "l1")) and not torch.equal(a, G.gd64(x0, y, mode, r, 10.0, 10, "l1"))
    assert not torch.equal(a, G.gd64(x0, y, mode, r, 0.5, 10, "l2")) and torch.equal(G.gd64(x0, y, mode, r, 0.5, 0, "l2"), x0.double())
    # per-sample norm: sample 0 alone gives what it gives inside the batch
    one = G.gd64(x0[:1], y[:1], mode, r, 0.5, 10, "l2")
    assert torch.equal(one, G.gd64(x0, y, mode, r, 0.5, 10, "l2")[:1])


@pytest.mark.parametrize("case,lr,loss", G.OP_RUNS, ids=[G.gd_name(*c, lr, loss) for c, lr, loss in G.OP_RUNS])
def test_guard_caps_hold_for_the_gpu_cases(case, lr, loss):
    """None left out in a small case and for l2; at most 0.1 % of the groups where the grid wraps."""
    _, bound, _, left = G.case64(*case, lr, G.N_ITER, loss)
    print(f"left out {left:.3e}, max bound {bound.max().item():.3e}")
    assert left <= G.cap_of(*case, loss)
    assert bool(torch.isfinite(bound).all())


def test_guard_caps_hold_for_inpainting_and_the_unaligned_trio():
    x0, _, mask, known = G.inpaint_inputs()
    for lr in G.LRS:
        for loss in G.LOSSES:
            assert G.inpaint64(x0, mask, known, lr, G.N_ITER, loss)[3] == 0.0
            for case in G.UNALIGNED_CASES:
                assert G.case64(*case, lr, G.N_ITER, loss)[3] == 0.0


def test_reference_arrays_lie_within_the_bound():
    """tests/golden/restore_gd.npz: the reference's affine_proj_GD (float32 autograd through its own operators) against gd64, within
    bound_gd plus the reference's recorded own error."""
    g = load_npz("restore_gd")
    for mode, C, dim, r in G.GOLDEN_GROUP_CASES:
        x0, y = G.measurement(mode, C, dim, r)
        name = R.case_name(mode, C, dim, r)
        assert torch.equal(g[f"{name}/x0"], x0) and torch.equal(g[f"{name}/y"], y)
        for lr in G.LRS:
            for loss in G.LOSSES:
                want, bound, keep, left = G.case64(mode, C, dim, r, lr, G.N_ITER, loss)
                key = G.gd_name(mode, C, dim, r, lr, loss)
                err = (g[f"{key}/out"].double() - want).abs()
                assert left == 0.0 and bool((err <= bound + g[f"{key}/err"].double()).all()), key
                assert abs(err.max().item() - g[f"{key}/err"].item()) <= 1e-12
    x0, missing, mask, known = G.inpaint_inputs()
    assert torch.equal(g["inpaint/x0"], x0) and torch.equal(g["inpaint/known"], known) and torch.equal(g["inpaint/missing"], missing)
    for lr in G.LRS:
        for loss in G.LOSSES:
            want, bound, keep, left = G.inpaint64(x0, mask, known, lr, G.N_ITER, loss)
            err = (g[f"inpaint_lr{lr:g}_{loss}/out"].double() - want).abs()
            assert left == 0.0 and bool((err <= bound + g[f"inpaint_lr{lr:g}_{loss}/err"].double()).all())
    for tag in ("sr4", "color", "inpaint"):
        assert g[f"loop/{tag}/min_rho_over_c"].item() >= 1e-2


def test_gd_entry_points_reject_bad_arguments_on_the_host():
    """NLC_REQUIRE, before anything is launched (no GPU needed); n_iter = 0 is the identity and launches nothing."""
    from diffusion_nlc_amd import _ext
    from diffusion_nlc_amd import constraint_functions as cf
    lib = _ext.load()
    assert lib.nlc_version() == _ext.ABI_VERSION == 10
    mem = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(mem)
    w, p = cf.group_tables([0.25] * 4)
    ok = cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 8, 8, 2, w, p)

    def group(x=ptr, y=ptr, d=ok, lr=10.0, n=10, loss=1, ws=ptr):
        return lib.nlc_group_gd(x, y, d, lr, n, loss, ws, None)

    def inpaint(x=ptr, m=ptr, k=ptr, B=2, C=3, HW=64, lr=10.0, n=10, loss=1, ws=ptr):
        return lib.nlc_inpaint_gd(x, m, k, B, C, HW, lr, n, loss, ws, None)
    bad = [(dict(x=None), b"null"), (dict(y=None), b"null"), (dict(loss=0), b"loss"), (dict(loss=3), b"loss"), (dict(n=-1), b"n_iter"),
           (dict(n=1025), b"n_iter"), (dict(lr=math.inf), b"finite"), (dict(lr=math.nan), b"finite"), (dict(loss=2, ws=None), b"workspace")]
    for kw, word in bad:
        assert group(**kw) == _ext.NLC_EINVAL and word in lib.nlc_last_error(), (kw, lib.nlc_last_error())
        if "y" in kw:
            kw = dict(m=None)
        assert inpaint(**kw) == _ext.NLC_EINVAL and word in lib.nlc_last_error(), (kw, lib.nlc_last_error())
    assert inpaint(k=None) == _ext.NLC_EINVAL and b"null" in lib.nlc_last_error()
    for kw in (dict(B=0), dict(B=65536), dict(C=0), dict(HW=0)):
        assert inpaint(**kw) == _ext.NLC_EINVAL and b"shape" in lib.nlc_last_error()
    # the descriptor is held to nlc_group_project's rules
    for d, word in [(cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 10, 8, 4, w, p), b"multiples"), (cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 18, 18, 9, w, p), b"outside 1..8"),
                    (cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 8, 8, 0, w, p), b"outside 1..8"), (cf.group_desc(_ext.GROUP_CHANNEL, 2, 1, 8, 8, 1, w, p), b"C = 3"),
                    (cf.group_desc(_ext.GROUP_BLOCK, 0, 3, 8, 8, 2, w, p), b"B = 0"), (cf.group_desc(_ext.GROUP_BLOCK, 65536, 3, 8, 8, 2, w, p), b"B = 65536"),
                    (cf.group_desc(2, 2, 3, 8, 8, 2, w, p), b"mode")]:
        assert group(d=d) == _ext.NLC_EINVAL and word in lib.nlc_last_error(), (word, lib.nlc_last_error())
        assert lib.nlc_group_project(ptr, ptr, d, None) == _ext.NLC_EINVAL and word in lib.nlc_last_error()
    # n_iter = 0: nothing to do, for either loss, with or without a workspace for l1
    assert group(n=0) == 0 and group(n=0, ws=None) == 0 and group(n=0, loss=2) == 0 and inpaint(n=0) == 0 and inpaint(n=0, loss=2) == 0
    # workspace: one double per workgroup of 256 entries and sample, 1024 workgroups per sample at most
    assert lib.nlc_gd_workspace_bytes(2, 1) == 16 and lib.nlc_gd_workspace_bytes(2, 257) == 32
    assert lib.nlc_gd_workspace_bytes(16, 3 * 256 * 256) == 16 * 768 * 8 and lib.nlc_gd_workspace_bytes(1, 10 ** 9) == 1024 * 8
    assert lib.nlc_gd_workspace_bytes(0, 5) == 0 and lib.nlc_gd_workspace_bytes(2, 0) == 0


def test_scope_of_the_gradient_projection():
    """svd_gd is built for the three operators and carries --constraint_lr / _iter / _loss; simple_gd and the other degradations
    still raise; the svd objects are what they were."""
    import image_sample
    from diffusion_nlc_amd import constraint_functions as cf
    from diffusion_nlc_amd._ext import NlcError
    ns = argparse.Namespace(constraint_scale=4.0, device="cpu", synthetic="cifar_tiny", constraint_lr=0.5, constraint_iter=7,
                            constraint_loss="l2", constraint_proj="svd_gd")
    for constraint, kind in (("sr_averagepooling", cf.SuperResolution), ("colorization", cf.Colorization), ("inpainting", cf.Inpainting)):
        ns.constraint = constraint
        c = image_sample.get_constraint_function(ns, 32, 3)
        assert isinstance(c.op, kind) and (c.proj, c.lr, c.n_iter, c.gd_loss) == ("svd_gd", 0.5, 7, "l2")
    for constraint, proj in (("deblur_gauss", "svd_gd"), ("sr_averagepooling", "simple_gd"), ("inpainting", "simple_gd"),
                             ("sr_averagepooling", "simple"), ("sr_averagepooling", "none"), ("colorization", "ddrm")):
        ns.constraint, ns.constraint_proj = constraint, proj
        with pytest.raises(NotImplementedError):
            image_sample.get_constraint_function(ns, 32, 3)
    sr = cf.svd_constraint("sr_averagepooling", fn_scale=4.0, device="cpu", image_size=32, channels=3)
    c = cf.Constraint_Function("sr_averagepooling", sr, channels=3, image_size=32)
    assert (c.proj, c.n_iter, c.gd_loss) == ("svd", 10, "l1") and isinstance(c.bind(torch.zeros(2, sr.groups), (2, 3, 32, 32)), cf.AffineGroup)
    with pytest.raises(NotImplementedError):
        cf.Constraint_Function("sr_averagepooling", sr, proj="simple_gd")
    with pytest.raises(NlcError):
        cf.Constraint_Function("sr_averagepooling", sr, proj="svd_gd", loss="l3")
    gd = cf.Constraint_Function("sr_averagepooling", sr, channels=3, image_size=32, lr=0.5, proj="svd_gd", n_iter=3, loss="l2")
    bound = gd.bind(torch.zeros(2, sr.groups), (2, 3, 32, 32))
    assert isinstance(bound, cf.GradientProjection) and (bound.lr, bound.n_iter, bound.loss) == (0.5, 3, 2)
    assert hasattr(bound, "project_") and not hasattr(bound, "mask_chw") and not hasattr(bound, "known")
    assert cf.gd_loss_id("l1") == 1 and cf.gd_loss_id(2) == 2
