"""The gradient-descent projection kernels (csrc/restore.hip: nlc_group_gd; csrc/constraint.hip: nlc_inpaint_gd) through the public
classes, at the shapes of tests/test_restore_ops_gpu.py - every row-load path, the r = 3, 5, 6, 7 scalar rows, the grid-stride wrap - with
n_iter = 10, lr in {10, 0.5}, both losses and B = 2 (a batch-wide norm in place of the per-sample one would show).

Every output is held to the ITERATED float64 form of tests/gd_refs.py within bound_gd, outside the guard (both derived there; the
share the guard leaves out is capped: none in a small case, none for l2, at most 0.1 % of the groups where the grid wraps), and - where
tests/golden/restore_gd.npz has the case - to the reference's own arrays within the same bound plus the reference's recorded own error.

Measured on an MI355X: L-inf to the float64 form <= 1.8e-7 over all cases (bounds from 2.5e-7 up to 6.5e-4, the largest where an l2 run
passes close to rho = 0); the guard leaves out at most 5.4e-5 of the groups (block 600 x 600, lr 0.5, l1) and none elsewhere but the
two other wrap cases.
"""
import pytest
import torch

from tests import gd_refs as G
from tests import restore_refs as R
from tests.util import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_FIX = {}


def golden():
    if not _FIX:
        _FIX.update(load_npz("restore_gd"))
    return _FIX


def make_op(mode, C, dim, r):
    from diffusion_nlc_amd.constraint_functions import Colorization, SuperResolution
    return SuperResolution(C, dim, r, DEV) if mode == R.BLOCK else Colorization(dim, DEV)


def make_inpaint(C, dim, missing):
    from diffusion_nlc_amd.constraint_functions import Inpainting
    return Inpainting(C, dim, missing, DEV)


def within(got, want, bound, keep, what):
    assert bool(torch.isfinite(got).all()), what
    err = (got.double() - want.double()).abs()
    worst = ((err - bound) * keep).max().item()
    print(f"    {what}: max err {(err * keep).max().item():.3e}, max bound {bound.max().item():.3e}, max(err - bound) {worst:.3e}")
    assert bool((err <= bound)[keep].all()), what


@pytest.mark.parametrize("case,lr,loss", G.OP_RUNS, ids=[G.gd_name(*c, lr, loss) for c, lr, loss in G.OP_RUNS])
def test_group_gd(case, lr, loss):
    mode, C, dim, r = case
    x0, y = G.measurement(mode, C, dim, r)
    want, bound, keep, left = G.case64(mode, C, dim, r, lr, G.N_ITER, loss)
    assert left <= G.cap_of(mode, C, dim, r, loss)
    if case in R.LARGE_CASES:
        assert y.shape[1] > (256 if dim == 300 else 1024 * 256)            # many workgroups / the grid-stride loop wraps
    op = make_op(mode, C, dim, r)
    x1 = x0.to(DEV).clone()
    assert op.gd_(x1, y.to(DEV), lr, G.N_ITER, loss) is x1
    got = x1.cpu()
    print(f"{G.gd_name(mode, C, dim, r, lr, loss)}: left out {left:.2e}")
    within(got, want, bound, keep, "gd vs f64")
    if case in G.GOLDEN_GROUP_CASES:
        g = golden()
        key = G.gd_name(mode, C, dim, r, lr, loss)
        assert torch.equal(g[f"{R.case_name(*case)}/x0"], x0) and torch.equal(g[f"{R.case_name(*case)}/y"], y)
        within(got, g[f"{key}/out"], bound + g[f"{key}/err"].double(), keep, "gd vs reference")


@pytest.mark.parametrize("loss", G.LOSSES)
@pytest.mark.parametrize("lr", G.LRS)
def test_inpaint_gd(lr, loss):
    C, dim = G.INPAINT_CASE
    x0, missing, mask, known = G.inpaint_inputs()
    op = make_inpaint(C, dim, missing)
    assert torch.equal(op.mask_chw.cpu(), mask)
    y = op.A(known.to(DEV))
    assert torch.equal(op.A_pinv(y).view(known.shape).cpu(), known)
    want, bound, keep, left = G.inpaint64(x0, mask, known, lr, G.N_ITER, loss)
    assert left == 0.0
    x1 = x0.to(DEV).clone()
    assert op.gd_(x1, known.to(DEV), lr, G.N_ITER, loss) is x1
    got = x1.cpu()
    within(got, want, bound, keep, f"inpaint gd lr {lr:g} {loss} vs f64")
    g = golden()
    within(got, g[f"inpaint_lr{lr:g}_{loss}/out"], bound + g[f"inpaint_lr{lr:g}_{loss}/err"].double(), keep, "inpaint gd vs reference")
    miss = mask.view(C, dim, dim) == 0
    assert torch.equal(got[:, miss], x0[:, miss])                          # only known entries move
    # an odd number of entries per sample (no float4 items) and a state 4 bytes into an allocation: the scalar kernel
    x0o, missing_o, mask_o, known_o = G.inpaint_inputs(3, 5)
    opo = make_inpaint(3, 5, missing_o)
    wo, bo, ko, lo = G.inpaint64(x0o, mask_o, known_o, lr, G.N_ITER, loss)
    assert lo == 0.0
    xo = x0o.to(DEV).clone()
    opo.gd_(xo, known_o.to(DEV), lr, G.N_ITER, loss)
    within(xo.cpu(), wo, bo, ko, "inpaint gd, 75 entries per sample")
    buf = torch.empty(x0.numel() + 1, device=DEV)
    xu = buf[1:].view(x0.shape)
    xu.copy_(x0)
    assert xu.data_ptr() % 8 == 4
    op.gd_(xu, known.to(DEV), lr, G.N_ITER, loss)
    assert torch.equal(xu.cpu(), got)                                       # the two kernels round alike


@pytest.mark.parametrize("loss", G.LOSSES)
def test_group_gd_unaligned_base_takes_the_scalar_rows(loss):
    """A state that starts 4 bytes into an allocation: the r = 2 / 4 / 8 launches must not use vector rows."""
    for mode, C, dim, r in G.UNALIGNED_CASES:
        for lr in G.LRS:
            x0, y = G.measurement(mode, C, dim, r)
            want, bound, keep, left = G.case64(mode, C, dim, r, lr, G.N_ITER, loss)
            assert left == 0.0
            op = make_op(mode, C, dim, r)
            buf = torch.empty(x0.numel() + 1, device=DEV)
            x1 = buf[1:].view(x0.shape)
            x1.copy_(x0)
            assert x1.data_ptr() % 8 == 4
            op.gd_(x1, y.to(DEV), lr, G.N_ITER, loss)
            within(x1.cpu(), want, bound, keep, f"gd r={r} lr {lr:g} {loss}, base + 4 bytes")


@pytest.mark.parametrize("loss", G.LOSSES)
def test_exact_cases_are_bit_identical(loss):
    """Where the residual is exactly 0 nothing moves, and nothing turns into a NaN (l2: rho_0 = 0)."""
    x, _ = R.inputs(R.BLOCK, 3, 16, 1)
    op = make_op(R.BLOCK, 3, 16, 1)
    x1 = x.to(DEV).clone()
    op.gd_(x1, x.reshape(R.B, -1).to(DEV), 10.0, G.N_ITER, loss)            # r = 1 and y = x0
    assert torch.equal(x1.cpu(), x)
    C, dim = G.INPAINT_CASE
    x0, missing, mask, known = G.inpaint_inputs()
    opi = make_inpaint(C, dim, missing)
    m = mask.view(1, C, dim, dim)
    start = known * m + x0 * (1 - m)                                        # x0 == known on the known pixels
    x1 = start.to(DEV).clone()
    opi.gd_(x1, known.to(DEV), 10.0, G.N_ITER, loss)
    assert torch.equal(x1.cpu(), start)
    nothing = make_inpaint(C, dim, torch.arange(C * dim * dim))              # every pixel missing
    assert float(nothing.mask_chw.abs().sum()) == 0.0
    x1 = x0.to(DEV).clone()
    nothing.gd_(x1, torch.zeros_like(x1), 10.0, G.N_ITER, loss)
    assert torch.equal(x1.cpu(), x0)
    # one sample of the batch already on the constraint, the other not: the first stays bit for bit (l2: its own rho_0 is 0,
    # whatever the other's is), the second moves as the yardstick says
    mixed = torch.stack([start[0], x0[1]])
    want, bound, keep, left = G.inpaint64(mixed, mask, known, 0.5, G.N_ITER, loss)
    x1 = mixed.to(DEV).clone()
    opi.gd_(x1, known.to(DEV), 0.5, G.N_ITER, loss)
    got = x1.cpu()
    assert torch.equal(got[0], mixed[0]) and not torch.equal(got[1], mixed[1])
    keep[0] = True                                                          # sample 0 sits exactly on the sign change and still has one right answer
    within(got, want, bound, keep, "one sample on the constraint")


@pytest.mark.parametrize("loss", G.LOSSES)
def test_iteration_count_is_honoured_and_runs_repeat(loss):
    mode, C, dim, r = R.BLOCK, 3, 12, 4
    x0, y = G.measurement(mode, C, dim, r)
    op = make_op(mode, C, dim, r)
    yd = y.to(DEV)

    def run(n_iter, lr=0.5, case=(x0, yd, op)):
        x1 = case[0].to(DEV).clone()
        case[2].gd_(x1, case[1], lr, n_iter, loss)
        return x1.cpu()
    assert torch.equal(run(0), x0)                                          # n_iter = 0 is the identity
    one, ten = run(1), run(10)
    for n_iter, got in ((1, one), (10, ten)):
        want, bound, keep, left = G.case64(mode, C, dim, r, 0.5, n_iter, loss)
        assert left == 0.0
        within(got, want, bound, keep, f"n_iter = {n_iter}")
    assert not torch.equal(one, ten) and not torch.equal(ten, run(10, lr=10.0))
    # the same input gives the same bits: no floating-point atomics, the partial sums are added in a fixed order
    big = (R.BLOCK, 3, 600, 2)
    xb, yb = G.measurement(*big)
    bigcase = (xb, yb.to(DEV), make_op(*big))
    assert torch.equal(run(10, 10.0, bigcase), run(10, 10.0, bigcase)) and torch.equal(ten, run(10))
    C2, d2 = G.INPAINT_CASE
    xi, missing, _, known = G.inpaint_inputs()
    opi = make_inpaint(C2, d2, missing)
    outs = []
    for _ in range(2):
        x1 = xi.to(DEV).clone()
        opi.gd_(x1, known.to(DEV), 10.0, 10, loss)
        outs.append(x1.cpu())
    assert torch.equal(*outs)


def test_rejections():
    from diffusion_nlc_amd import _ext
    from diffusion_nlc_amd import constraint_functions as cf
    from diffusion_nlc_amd._ext import NlcError
    op = cf.Colorization(8, DEV)
    with pytest.raises(NlcError):
        op.gd_(torch.zeros(2, 3, 8, 8), torch.zeros(2, 64), 10.0, 10, "l1")                 # a host tensor is not projected behind the caller's back
    x, y = torch.zeros(2, 3, 8, 8, device=DEV), torch.zeros(2, 64, device=DEV)
    with pytest.raises(NlcError):
        op.gd_(x, y[:, :63].contiguous(), 10.0, 10, "l1")
    with pytest.raises(NlcError):
        op.gd_(x, y, 10.0, 10, "l3")
    for kw in (dict(lr=float("inf")), dict(n_iter=1025), dict(n_iter=-1)):
        with pytest.raises(NlcError) as e:
            op.gd_(x, y, **{**dict(lr=10.0, n_iter=10, loss="l2"), **kw})
        assert e.value.rc == _ext.NLC_EINVAL
    inp = cf.Inpainting(3, 8, torch.arange(0, 96), DEV)
    with pytest.raises(NlcError):
        inp.gd_(torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), 10.0, 10, "l1")
    with pytest.raises(NlcError):
        inp.gd_(x, torch.zeros(2, 3, 8, 4, device=DEV), 10.0, 10, "l1")
