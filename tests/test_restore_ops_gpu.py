"""The group-sum measurement kernels (csrc/restore.hip: nlc_group_A / nlc_group_Apinv / nlc_group_project) through the public
classes ``SuperResolution`` and ``Colorization``, at the smallest shapes at which they can still go wrong:

    BLOCK    (1, 2, 2) (3, 4, 4) (3, 8, 8)     one block per channel; the float2 / float4 / 2 x float4 row loads
             (3, 6, 2) (3, 12, 4)              odd number of blocks per row
             (3, 12, 3) (1, 9, 3)              r = 3: scalar path, unaligned rows
             (3, 16, 1)                        r = 1: A is the identity, bit exact
             (3, 10, 5) (3, 12, 6) (3, 14, 7)  r = 5, 6, 7: 2 x 2 blocks per channel, float64 closed form only
             (3, 600, 2)                       270 000 groups > 1024 x 256 threads: the grid-stride loop wraps
    CHANNEL  img_dim 1, 8, 300, 520            single pixel; plane-strided reads; many workgroups; 270 400 pixels: the loop wraps

Every output is held to the float64 closed form of tests/restore_refs.py with the first-order bound derived there (n products,
n-1 additions, one final rounding, u = 2^-24, doubled), and - where tests/golden/restore_ops.npz has the case - to the reference's
own arrays with the same bound plus the reference's recorded own error against that closed form, nothing more.
"""
import pytest
import torch

from tests import restore_refs as R
from tests.util import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_op(mode, C, dim, r):
    from diffusion_nlc_amd.constraint_functions import Colorization, SuperResolution
    return SuperResolution(C, dim, r, DEV) if mode == R.BLOCK else Colorization(dim, DEV)


_FIX = {}


def fixture_of(mode, C, dim, r):
    if not _FIX:
        _FIX.update(load_npz("restore_ops"))
    name = R.case_name(mode, C, dim, r)
    return {k: _FIX[f"{name}/{k}"] for k in ("x", "x0", "A", "Apinv", "proj", "err")}


def within(got, want, bound, what):
    err = (got.double() - want.double()).abs()
    worst = (err - bound).max().item()
    print(f"    {what}: max err {err.max().item():.3e}, max bound {bound.max().item():.3e}, max(err - bound) {worst:.3e}")
    assert bool((err <= bound).all()), what


def check_case(op, mode, C, dim, r, x, x0, y, ref=None, issue_bound=True, to_dev=lambda t: t.to(DEV), to_host=lambda t: t.cpu()):
    """``y``: the float32 measurement given to A^+ and to the projection.  ``ref``: the reference's arrays and own errors, or None.
    ``issue_bound``: hold  A(project(x0)) = y  and  project(project(x0)) = project(x0)  to the bound of A evaluated on the
    projected x0' alone.  That bound is not rigorous: the residual carries A's summation error on x0 BEFORE the projection, so a
    group whose entries nearly cancel after it (sum |w x0'| << sum |w x0|) can exceed it without any defect - about one group in
    10^4 for U(-1, 1) inputs.  The small cases keep it (their seeded inputs have no such group, and the arithmetic is
    deterministic); the large cases, which the closed form alone judges, use the term-by-term bound written out below."""
    Bn = x.shape[0]
    print(f"{R.case_name(mode, C, dim, r)}:")
    # A
    a = to_host(op.A(to_dev(x)))
    assert a.shape == (Bn, R.A64(x, mode, r).shape[1]) and a.dtype == torch.float32
    within(a, R.A64(x, mode, r), R.bound_A(x, mode, r), "A vs f64")
    if mode == R.BLOCK and r == 1:
        assert torch.equal(a, x.reshape(Bn, -1))
    # A^+
    ap = to_host(op.A_pinv(to_dev(y)))
    assert ap.shape == (Bn, C * dim * dim)
    ap = ap.view(Bn, C, dim, dim)
    if R.p_is_one(mode, r):
        assert torch.equal(ap, R.Apinv64(y, mode, C, dim, r).float())                       # an exact broadcast
    within(ap, R.Apinv64(y, mode, C, dim, r), R.bound_Apinv(y, mode, C, dim, r), "A_pinv vs f64")
    # projection, in place
    yd = to_dev(y).contiguous()
    x1 = to_dev(x0).clone()
    assert op.project_(x1, yd) is x1
    x1h = to_host(x1)
    within(x1h, R.project64(x0, y, mode, r), R.bound_project(x0, y, mode, r), "project vs f64")
    if ref is not None:
        e = ref["err"].double()
        within(a, ref["A"], R.bound_A(x, mode, r) + e[0], "A vs reference")
        within(ap, ref["Apinv"].view(Bn, C, dim, dim), R.bound_Apinv(y, mode, C, dim, r) + e[1], "A_pinv vs reference")
        within(x1h, ref["proj"], R.bound_project(x0, y, mode, r) + e[2], "project vs reference")
    # properties
    w, p = R.tables(mode, r)
    n = w.numel()

    def spread(per_group):
        return R.from_groups(per_group.unsqueeze(-1).expand(-1, -1, n), mode, C, dim, r)
    b1 = R.bound_A(x1h, mode, r)
    if issue_bound:
        resid, twice = b1, spread(b1)
    else:
        # what the projection leaves, term by term: the summation error of A on x0 itself (bound_A(x0)), one rounding of
        # d = y - A x0, the tables' sum_i w_i p_i - 1 (times d), and the final rounding of every entry (<= bound_A(x0'));
        # a second projection moves an entry by that residual seen through A's own error once more, plus one rounding
        d = (y.double() - R.A64(x0, mode, r)).abs()
        resid = R.bound_A(x0, mode, r) + b1 + (2 * R.U32 + abs(float((w * p).sum()) - 1.0)) * d
        twice = R.from_groups((resid + b1).unsqueeze(-1) * p.abs(), mode, C, dim, r) + 2 * R.U32 * x1h.double().abs()
    within(R.A64(x1h, mode, r), y, resid, "A(project(x0)) = y")
    x2 = x1.clone()
    op.project_(x2, yd)
    within(to_host(x2), x1h, twice, "project twice")
    apf = ap.reshape(Bn, C, dim, dim)
    within(to_host(op.A(to_dev(apf))), y, R.bound_A(apf, mode, r), "A(A_pinv y) = y")


@pytest.mark.parametrize("mode,C,dim,r", R.FIXTURE_CASES, ids=[R.case_name(*c) for c in R.FIXTURE_CASES])
def test_group_ops_small(mode, C, dim, r):
    ref = fixture_of(mode, C, dim, r)
    x, x0 = R.inputs(mode, C, dim, r)
    assert torch.equal(x, ref["x"]) and torch.equal(x0, ref["x0"])              # the fixture's inputs are the seeded ones
    check_case(make_op(mode, C, dim, r), mode, C, dim, r, x, x0, ref["A"], ref)


@pytest.mark.parametrize("mode,C,dim,r", R.LARGE_CASES, ids=[R.case_name(*c) for c in R.LARGE_CASES])
def test_group_ops_grid_stride_wrap(mode, C, dim, r):
    x, x0 = R.inputs(mode, C, dim, r)
    assert R.A64(x, mode, r).shape[1] > (256 if dim == 300 else 1024 * 256)
    check_case(make_op(mode, C, dim, r), mode, C, dim, r, x, x0, R.A64(x, mode, r).float(), issue_bound=False)


@pytest.mark.parametrize("mode,C,dim,r", R.CLOSED_FORM_CASES, ids=[R.case_name(*c) for c in R.CLOSED_FORM_CASES])
def test_group_ops_block_sizes_without_a_fixture(mode, C, dim, r):
    x, x0 = R.inputs(mode, C, dim, r)
    check_case(make_op(mode, C, dim, r), mode, C, dim, r, x, x0, R.A64(x, mode, r).float(), issue_bound=False)


def test_group_ops_unaligned_base_takes_the_scalar_rows():
    """A state that starts 4 bytes into an allocation: the r = 2 / 4 / 8 launches must not use vector rows."""
    for C, dim, r in ((3, 6, 2), (3, 12, 4), (3, 8, 8)):
        x, x0 = R.inputs(R.BLOCK, C, dim, r)
        op = make_op(R.BLOCK, C, dim, r)
        y = R.A64(x, R.BLOCK, r).float()
        buf = torch.empty(x0.numel() + 1, device=DEV)
        x1 = buf[1:].view(x0.shape)
        x1.copy_(x0)
        assert x1.data_ptr() % 8 == 4
        op.project_(x1, y.to(DEV))
        within(x1.cpu(), R.project64(x0, y, R.BLOCK, r), R.bound_project(x0, y, R.BLOCK, r), f"project r={r}, base + 4 bytes")


def test_transpose_and_singulars():
    """At = A^T (w in the place of p) and singulars() = |w|_2 per measurement, as the reference's SVD gives them."""
    for mode, C, dim, r in ((R.BLOCK, 3, 12, 4), (R.CHANNEL, 3, 8, 1)):
        op = make_op(mode, C, dim, r)
        w, _ = R.tables(mode, r)
        y = R.A64(R.inputs(mode, C, dim, r)[0], mode, r).float()
        at = op.At(y.to(DEV)).cpu().view(R.B, C, dim, dim)
        want = R.from_groups(y.double().unsqueeze(-1) * w, mode, C, dim, r)
        within(at, want, 2 * R.U32 * want.abs(), "At")
        s = op.singulars()
        assert s.shape == (y.shape[1],) and abs(s[0].item() - float(w.pow(2).sum().sqrt())) < 1e-7


def test_rejections():
    from diffusion_nlc_amd import _ext
    from diffusion_nlc_amd import constraint_functions as cf
    from diffusion_nlc_amd._ext import NlcError
    with pytest.raises(NlcError):
        cf.SuperResolution(3, 10, 4, DEV)
    with pytest.raises(NlcError):
        cf.SuperResolution(3, 18, 9, DEV)
    w, p = cf.group_tables([0.25] * 4)
    x = torch.zeros(2, 3, 18, 18, device=DEV)
    y = torch.zeros(2, 3 * 18 * 18, device=DEV)
    for d in (cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 10, 10, 4, w, p),        # img_dim % r != 0
              cf.group_desc(_ext.GROUP_BLOCK, 2, 3, 18, 18, 9, w, p),        # r = 9
              cf.group_desc(_ext.GROUP_CHANNEL, 2, 1, 18, 18, 1, w, p)):     # CHANNEL with C = 1
        for call in (lambda: cf.group_A(x, d), lambda: cf.group_Apinv(y, d), lambda: cf.group_project_(x, y, d)):
            with pytest.raises(NlcError) as e:
                call()
            assert e.value.rc == _ext.NLC_EINVAL
    op = cf.Colorization(8, DEV)
    with pytest.raises(NlcError):
        op.project_(torch.zeros(2, 3, 8, 8), torch.zeros(2, 64))            # a host tensor is not projected behind the caller's back
