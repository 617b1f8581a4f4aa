"""Op-level parity of the kernels that run between two network evaluations (csrc/sampler.hip, csrc/edm.hip, the inpainting
gathers, the resample / layout helpers, the timestep embedding and conv_first) against plain PyTorch-CPU references, at the
shapes where each of them leaves its first workgroup, its first loop trip or its aligned path.

Tolerances (tests/sampler_refs.py has the restatements; tests/test_host_cpu.py holds them to the CPU oracle):
  * copies, gathers and chains of IEEE operations compiled without contraction: ``torch.equal`` with the f32 / f64 restatement;
  * short chains: the f64 evaluation on the same f32 inputs, half an ulp (U32 * |x|) per rounded operation plus one half;
  * positive-term reductions: (longest addition chain + 1) * unit roundoff, the chain read off the kernel;
  * logf / cosf / sinf / expf: twice the error measured on the MI355X, capped at the 1e-6 relative / 2e-6 absolute of
    tests/test_sched_gpu.py and test_timestep_embedding (the measured figures are in the docstrings);
  * sigma -> t: the CPU lookup applied to the sigma the kernel itself wrote, bit for bit; that sigma is held to its bound separately.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import sampler_refs as R
from tests.sampler_refs import F32, F64, U32, U64

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ["f32", "bf16", "f16"]
SENTINEL = -777.0


def _dev():
    return torch.device("cuda:0")


def _d(t):
    return None if t is None else t.to(_dev()).contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64)


@pytest.fixture(scope="module")
def tabs():
    return R.tables()


# ---- 1. row_sumsq ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D", [1, 3, 4, 5, 1023, 1024, 1025, 4099, 8193])
def test_row_sumsq(D, B):
    """Vector and scalar paths are chosen per row from the row pointer's alignment: strides of every residue mod 4 and a base
    pointer one float off put both into one launch.  |got - ref| <= (chain + 1) * 2^-24 * ref, ref the f64 sum of the squares."""
    from diffusion_nlc_amd import ops
    bound = (R.sumsq_chain_f32(D) + 1) * U32
    for res in (0, 1, 2, 3):
        stride = D + 1 + (res - (D + 1)) % 4              # the smallest stride > D with stride % 4 == res
        for off in (0, 1):
            buf = torch.randn(1 + B * stride, generator=R.gen(("sumsq", D, B, res, off)))
            x = buf.to(_dev())[off:off + B * stride].view(B, stride)
            got = ops.row_sumsq(x, d_used=D)
            again = ops.row_sumsq(x, d_used=D)
            ref = (buf[off:off + B * stride].view(B, stride)[:, :D].double() ** 2).sum(1)
            err = ((got.cpu().double() - ref).abs() / ref).max().item()
            print(f"row_sumsq D={D} B={B} stride%4={res} off={off}: rel err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (D, B, res, off, err, bound)
            assert torch.equal(got, again)
    x = torch.randn(B, D, generator=R.gen(("sumsq-full", D, B)))
    ref = (x.double() ** 2).sum(1)
    assert ((ops.row_sumsq(x.to(_dev())).cpu().double() - ref).abs() / ref).max().item() <= bound


# ---- 2. refine_sigma ------------------------------------------------------------------------------------------------------------
REFINE_B = [1, 3, 64, 65, 1024, 1025, 2500]
PAD = 7


def _outs(B):
    """Four over-allocated outputs; the kernel must leave the PAD elements past B alone."""
    full = [torch.full((B + PAD,), SENTINEL, device=_dev()) for _ in range(4)]
    return full, [f[:B] for f in full]


def _untouched(full, B):
    return all(bool((f[B:] == SENTINEL).all()) for f in full)


def _check_c_in(c_in, sigma_t):
    # sqrtf(1 / (sg*sg + 1)): mul, add, div, sqrt = 4 rounded operations, all on positive terms -> (4 + 1) half ulps
    ref = R.c_in_f64(sigma_t)
    assert bool(((c_in.double() - ref).abs() <= 5 * U32 * ref).all())


def _run_refine(tab, sumsq, raw, time_shift, prev_ratio):
    from diffusion_nlc_amd import ops
    sigmas, slopes = tab
    B = raw.numel()
    sqrt_dim, norm_max, norm_min = R.REFINE_SCALARS
    full, (st, sp, t, ci) = _outs(B)
    ops.refine_sigma(_d(sumsq), sqrt_dim, norm_max, norm_min, 0.0, 0.8, True, _d(sigmas), 0, time_shift, st, sp, t, ci,
                     sigma_in=_d(raw), prev_is_ratio=prev_ratio, t_slopes=_d(slopes))
    torch.cuda.synchronize()
    assert _untouched(full, B)
    return st.cpu(), sp.cpu(), t.cpu(), ci.cpu()


def _check_refine(tab, sumsq, raw, time_shift, got, prev_ratio):
    sigmas, slopes = tab
    st, sp, t, ci = got
    sqrt_dim, norm_max, norm_min = R.REFINE_SCALARS
    # sigma_t: sqrtf, /, then one of - / + (3 rounded operations) and a clamp.  norm_x - norm_max cancels, so the (3 + 1) half
    # ulps are taken of the largest intermediate, not of the result.
    ref, norm_x = R.refine_clamp_f64(sumsq, raw, sqrt_dim, norm_max, norm_min)
    mag = torch.maximum(norm_x.abs(), ref.abs()).clamp(min=norm_max)
    assert bool(((st.double() - ref).abs() <= 4 * U32 * mag).all())
    # t: the lookup, shift and clamp applied on the CPU to the sigma the kernel wrote
    t_ref = R.shift_clamp_f32(R.lookup_f32(sigmas, slopes, st), time_shift)
    assert torch.equal(t, t_ref), (t - t_ref).abs().max()
    assert torch.equal(sp, raw * R.f32s(0.8, raw) if prev_ratio else R.f32s(0.8, raw))
    _check_c_in(ci, st)
    return t_ref


@pytest.mark.parametrize("kind", R.TABLE_KINDS)
@pytest.mark.parametrize("B", REFINE_B)
def test_refine_sigma_clamps_and_lookup(tabs, kind, B):
    """refine = 1: each clamp binds for some samples; raw sigmas on, below and above the table; the stride loop (B > 1024) and the
    cross-wave minimum (B > 64).  With t51 a lookup result of 51 stays, with t1001 one of 1001 is cut to 1000."""
    tab = tabs[kind]
    for ratio in (False, True):
        sumsq, raw = R.refine_inputs(tab[0], B, kind)
        got = _run_refine(tab, sumsq, raw, 0, ratio)
        t_ref = _check_refine(tab, sumsq, raw, 0, got, ratio)
        if B >= 6:                   # the table's ends are reached: 51 stays, 1001 is cut to 1000
            assert t_ref.max().item() == min(float(tab[0].numel()), 1000.0) and t_ref.min().item() == 0.0


@pytest.mark.parametrize("kind", R.TABLE_KINDS)
@pytest.mark.parametrize("time_shift", [0, 3])
def test_refine_sigma_time_shift_needs_every_t_positive(tabs, kind, time_shift):
    """The shift is applied when every t > 0 and to nobody when one sample sits at t == 0 - at index 0, in another wave (70) or in
    the second trip of the loop (2499): a minimum that loses a wave or a trip shifts the batch."""
    tab = tabs[kind]
    B = 2500
    sumsq, raw = R.refine_inputs(tab[0], B, kind, every_t_positive=True)
    got = _run_refine(tab, sumsq, raw, time_shift, False)
    _check_refine(tab, sumsq, raw, time_shift, got, False)
    raw_t = R.lookup_f32(tab[0], tab[1], got[0])
    assert bool(raw_t.min() > 0)
    assert torch.equal(got[2], (raw_t - float(time_shift)).clamp(0.0, 1000.0))
    unshifted = raw_t.clamp(0.0, 1000.0)
    for z in (0, 70, 2499):
        sumsq, raw = R.refine_inputs(tab[0], B, kind, every_t_positive=True, zero_at=z)
        got = _run_refine(tab, sumsq, raw, time_shift, False)
        _check_refine(tab, sumsq, raw, time_shift, got, False)
        assert got[2][z].item() == 0.0
        keep = torch.arange(B) != z
        assert torch.equal(got[2][keep], unshifted[keep]), (kind, time_shift, z)


@pytest.mark.parametrize("B", REFINE_B)
def test_refine_sigma_pass_through(B):
    """refine = 0: the scheduled scalars, or the per-sample values aliasing the outputs, pass through; t is clamped;
    sigma_prev is the scalar or raw * ratio."""
    from diffusion_nlc_amd import ops
    for ratio in (False, True):
        for t_sched in (954.0, 1003.0):
            full, (st, sp, t, ci) = _outs(B)
            ops.refine_sigma(None, 1.0, 1.0, 0.0, 37.3, 0.83, False, None, t_sched, 3, st, sp, t, ci, prev_is_ratio=ratio)
            torch.cuda.synchronize()
            assert _untouched(full, B)
            s_in = R.f32s(37.3, st)
            assert torch.equal(st.cpu(), s_in) and torch.equal(t.cpu(), torch.full((B,), min(t_sched, 1000.0)))
            assert torch.equal(sp.cpu(), s_in * R.f32s(0.83, st) if ratio else R.f32s(0.83, st))
            _check_c_in(ci.cpu(), st.cpu())
        g = R.gen(("pass", B, ratio))
        sig = torch.rand(B, generator=g) * 90 + 0.01
        tin = torch.rand(B, generator=g) * 1200 - 100            # some below 0, some above 1000
        full, (st, sp, t, ci) = _outs(B)
        st.copy_(sig)
        t.copy_(tin)
        ops.refine_sigma(None, 1.0, 1.0, 0.0, 1.0, 0.83, False, None, 0, 3, st, sp, t, ci, sigma_in=st, t_in=t, prev_is_ratio=ratio)
        torch.cuda.synchronize()
        assert _untouched(full, B)
        assert torch.equal(st.cpu(), sig) and torch.equal(t.cpu(), tin.clamp(0.0, 1000.0))
        assert torch.equal(sp.cpu(), sig * R.f32s(0.83, sig) if ratio else R.f32s(0.83, sig))
        _check_c_in(ci.cpu(), sig)


# ---- 3. sigma_correct -----------------------------------------------------------------------------------------------------------
CORRECT_B = [1, 255, 256, 257, 1000]


def _correct_inputs(sigmas, B, kind):
    """sample b of kind b % 6: 0 random r; 1 dist_hat on a table entry (sigma_t an entry, r = 0); 2 below the table (r = -0.9999);
    3 above the table (r = 1e4); 4 r = -1 (dist_hat = 0); 5 r = -1.5 (dist_hat < 0)."""
    g = R.gen(("correct", kind, B))
    st = torch.rand(B, generator=g) * 40 + 0.05
    k = torch.arange(B) % 6
    st = torch.where(k == 1, sigmas[torch.randint(1, sigmas.numel(), (B,), generator=g)], st)
    r = torch.randn(B, generator=g) * 0.2
    for kk, v in ((1, 0.0), (2, -0.9999), (3, 1e4), (4, -1.0), (5, -1.5)):
        r = torch.where(k == kk, torch.tensor(v), r)
    return st.contiguous(), (st * 0.8).contiguous(), r.contiguous()


@pytest.mark.parametrize("partial", [False, True], ids=["pred", "pred_partial"])
@pytest.mark.parametrize("kind", R.TABLE_KINDS)
@pytest.mark.parametrize("B", CORRECT_B)
def test_sigma_correct(tabs, kind, B, partial):
    from diffusion_nlc_amd import ops
    sigmas, slopes = tabs[kind]
    st0, sp0, r = _correct_inputs(sigmas, B, kind)
    full, (st, sp, t, ci) = _outs(B)
    st.copy_(st0)
    sp.copy_(sp0)
    ops.sigma_correct(_d(r), partial, _d(sigmas), st, sp, t, ci, t_slopes=_d(slopes))
    torch.cuda.synchronize()
    assert _untouched(full, B)
    dist_hat, dist_prev = R.correct_f32(st0, sp0, r)
    assert torch.equal(st.cpu(), dist_hat)
    assert torch.equal(sp.cpu(), sp0 if partial else dist_prev)
    t_ref = R.lookup_f32(sigmas, slopes, st.cpu()).clamp(0.0, 1000.0)
    assert torch.equal(t.cpu(), t_ref)
    _check_c_in(ci.cpu(), st.cpu())
    if B >= 6:
        assert t_ref.min().item() == 0.0 and t_ref.max().item() == min(float(sigmas.numel()), 1000.0)


@pytest.mark.parametrize("kind", R.TABLE_KINDS)
def test_nan_sigma_looks_up_like_searchsorted(tabs, kind):
    """The decision documented in include/nlc_hip.h: a NaN sigma finds n_sigmas in a discrete table, as torch.searchsorted does
    (the [0, 1000] clamp of sigma_correct then applies); the continuous interpolation gives NaN, which proj_sigma hands on and the
    fminf / fmaxf clamp of sigma_correct turns into 0.  sigma_t stays NaN in every case."""
    from diffusion_nlc_amd import ops
    sigmas, slopes = tabs[kind]
    B, n = 5, sigmas.numel()
    st0 = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    r = torch.tensor([0.0, float("nan"), 0.0, 0.0, float("nan")])
    full, (st, sp, t, ci) = _outs(B)
    st.copy_(st0)
    sp.copy_(st0)
    ops.sigma_correct(_d(r), False, _d(sigmas), st, sp, t, ci, t_slopes=_d(slopes))
    want = R.lookup_f32(sigmas, slopes, st0 * (1.0 + r))
    want = torch.where(torch.isnan(want), torch.zeros(()), want).clamp(0.0, 1000.0)
    assert torch.equal(t.cpu(), want) and torch.equal(torch.isnan(st.cpu()), torch.isnan(r))
    if slopes is None:
        assert t.cpu()[1].item() == min(float(n), 1000.0)
    # proj_sigma: last_norm = 0 makes the ratio inf (sumsq > 0) or NaN (sumsq = 0), as in the reference; no clamp there
    last = _d(torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0]))
    ss = _d(torch.tensor([4.0, 4.0, 4.0, 0.0, 4.0]))
    st2, t2 = _d(st0), torch.full((B,), SENTINEL, device=_dev())
    ops.proj_sigma(ss, 2.0, 0.5, 0.25, 0.99, 0.1, 0.2, 0.3, 0.4, _d(sigmas), _d(slopes), last, st2, _d(st0), t2)
    sg, cn = R.proj_f32(ss.cpu(), torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0]), st0, st0, 2.0, 0.5, 0.25, 0.99, 0.1, 0.2, 0.3, 0.4)
    assert torch.equal(torch.isnan(st2.cpu()), torch.isnan(sg)) and torch.equal(st2.cpu()[[0, 1, 2, 4]], sg[[0, 1, 2, 4]])
    assert math.isinf(sg[1].item()) and math.isnan(sg[3].item())
    want = R.lookup_f32(sigmas, slopes, st2.cpu())
    assert torch.equal(torch.isnan(t2.cpu()), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(t2.cpu(), nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    if slopes is None:
        assert t2.cpu()[1].item() == float(n) and t2.cpu()[3].item() == float(n)
    else:
        assert math.isnan(t2.cpu()[3].item())


# ---- 4. proj_sigma --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.TABLE_KINDS)
@pytest.mark.parametrize("B", CORRECT_B)
def test_proj_sigma(tabs, kind, B):
    """image_sample.py:485-497 of the reference.  sigma against the f64 evaluation with the propagated absolute bound of
    sampler_refs.proj_f64_with_bound (18 rounded operations, one half ulp more for the final rounding); last_norm (sqrtf, /) bit
    for bit; t from the sigma the kernel wrote, not clamped; sigma_prev untouched."""
    from diffusion_nlc_amd import ops
    sigmas, slopes = tabs[kind]
    g = R.gen(("proj", kind, B))
    sqrt_dim = math.sqrt(3072.0)
    norm_max = 31.0 / sqrt_dim
    cn = torch.rand(B, generator=g) * 3 + 0.05
    cn[::4] = norm_max * (1 + 0.01 * torch.randn(cn[::4].numel(), generator=g))      # the cancelling neighbourhood of cur_dist
    sumsq = ((cn * sqrt_dim) ** 2).float()
    last0 = (cn * (1 + 0.2 * torch.randn(B, generator=g))).abs() + 0.01
    st0 = torch.rand(B, generator=g) * 60 + 0.01
    sp0 = st0 * 0.85
    sc = (sqrt_dim, norm_max, norm_max ** 2, 0.99, 0.1 * 12.5, 0.2, 0.3, 0.4)
    full, (st, sp, t, last) = _outs(B)
    st.copy_(st0)
    sp.copy_(sp0)
    last.copy_(last0)
    ops.proj_sigma(_d(sumsq), *sc, _d(sigmas), _d(slopes), last, st, sp, t)
    torch.cuda.synchronize()
    assert _untouched(full, B)
    ref, bound = R.proj_f64_with_bound(sumsq, last0, st0, sp0, *sc)
    err = (st.cpu().double() - ref).abs()
    print(f"proj_sigma {kind} B={B}: max err / bound {(err / (bound + U32 * ref.abs())).max().item():.3f}")
    assert bool((err <= bound + U32 * ref.abs()).all())
    sg32, cn32 = R.proj_f32(sumsq, last0, st0, sp0, *sc)
    assert torch.equal(last.cpu(), cn32)
    assert torch.equal(sp.cpu(), sp0)
    assert torch.equal(t.cpu(), R.lookup_f32(sigmas, slopes, st.cpu()))


# ---- 5. scale_rows / lincomb_rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [1, 255, 1024, 1025, 262149])
def test_scale_rows_and_lincomb_rows(D, B):
    """One or two multiplications and one addition per element, each rounded: bit-equal.  D = 262149 takes the second grid-stride
    trip of the 256-workgroup grid."""
    from diffusion_nlc_amd import ops
    g = R.gen(("rows", D, B))
    x, y = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    ca, cb = torch.randn(B, generator=g), torch.randn(B, generator=g)
    xd, yd = _d(x), _d(y)
    assert torch.equal(ops.scale_rows(xd, None, 0.3).cpu(), x * R.f32s(0.3, x))
    assert torch.equal(ops.scale_rows(xd, _d(ca), 0.3).cpu(), x * (ca * R.f32s(0.3, ca))[:, None])
    assert torch.equal(ops.scale_rows(xd, _d(ca)).cpu(), x * ca[:, None])
    assert torch.equal(ops.lincomb_rows(xd, _d(ca)).cpu(), x * ca[:, None])
    assert torch.equal(ops.lincomb_rows(xd, _d(ca), yd, _d(cb)).cpu(), x * ca[:, None] + y * cb[:, None])


# ---- 6. sched_x0 / sched_step ---------------------------------------------------------------------------------------------------
SAMPLERS = ("ddpm", "ddim", "ddim_simple", "ddim_orig", "ddim_simple_orig", "ddim_simple_drag", "ddpm_orig")
SCHED_SHAPES = [(3, 1), (1, 262149), (3, 90000)]
SCHED_MEASURED = 1.552e-7                        # largest error relative to the tensor's scale seen on the MI355X, all cases below
SCHED_TOL = min(2 * SCHED_MEASURED, 1e-6)        # twice that, capped at the 1e-6 of tests/test_sched_gpu.py


def _sched(name, eta):
    from oracle import sched as osch
    return osch.get_sampler(name, 1000, 50, sigma_style="DDIM", start_sigma=100, end_sigma=0, sampler_var="fixedsmall", eta=eta)


def _sched_inputs(C_, HW, tag):
    g = R.gen(("sched", C_, HW, tag))
    B = 2
    xt, eps, noise = (torch.randn(B, C_, HW, 1, generator=g) for _ in range(3))
    xt = xt * 2.0
    st = torch.tensor([2.5, 0.7]).view(B, 1, 1, 1)
    sp = torch.tensor([1.9, 0.5]).view(B, 1, 1, 1)
    return xt, eps, noise, st, sp


def _desc(S, name, xt, eps, noise, st, sp, x0, xp, **kw):
    from diffusion_nlc_amd._ext import SCHED_VARIANTS, VAR_MODES, SchedDesc
    B, C_, HW = xt.shape[0], xt.shape[1], xt.shape[2] * xt.shape[3]
    return SchedDesc(xt=xt.data_ptr(), eps_out=eps.data_ptr(), noise=noise.data_ptr(), sigma_t=st.data_ptr(), sigma_prev=sp.data_ptr(),
                     x0=x0.data_ptr(), x_prev=None if xp is None else xp.data_ptr(), B=B, C=C_, Cnet=C_, HW=HW,
                     variant=SCHED_VARIANTS[name], var_mode=VAR_MODES["fixedsmall"], eta=float(S.eta),
                     min_var_coef=float(S.min_var_coef), **kw)


def _rel(got, ref):
    return ((got.detach().cpu().double() - ref.double()).abs().max() / ref.double().abs().max().clamp(min=1e-12)).item()


@pytest.mark.parametrize("shape", SCHED_SHAPES, ids=lambda s: f"C{s[0]}xHW{s[1]}")
@pytest.mark.parametrize("eta", [0.0, 0.85])
@pytest.mark.parametrize("name", SAMPLERS)
def test_sched_step_all_variants(name, eta, shape):
    """Against oracle/sched.py (pinned to upstream by tests/test_oracle_golden.py) beyond the golden shape: one pixel, and two
    samples whose C*HW takes the second grid-stride trip.  x0 = xt - sigma_t*eps is two IEEE operations: bit-equal.  x_prev goes
    through logf / expf.  Measured on the MI355X: largest error relative to the tensor's scale 1.552e-07 (over these cases and those
    of test_sched_step_ddim_options); asserted: twice that, 3.104e-07 (the cap of 1e-6 does not bind)."""
    from diffusion_nlc_amd import ops
    S = _sched(name, eta)
    xt, eps, noise, st, sp = _sched_inputs(*shape, name)
    x0_ref = S.pred_xstart(xt, eps, st)
    xp_ref = S.pred_xprev(x0=x0_ref, eps=eps, sigma_t=st, sigma_prev=sp, xt=xt, log_variance=S.get_eps_logvar(st, sp), noise=noise)
    d_xt, d_eps, d_noise, d_st, d_sp = _d(xt), _d(eps), _d(noise), _d(st.reshape(-1)), _d(sp.reshape(-1))
    x0, xp = torch.full_like(d_xt, SENTINEL), torch.full_like(d_xt, SENTINEL)
    nan = torch.zeros(1, device=_dev(), dtype=torch.int32)
    d = _desc(S, name, d_xt, d_eps, d_noise, d_st, d_sp, x0, xp, clip=0, phases=0)
    ops.sched_x0(d)
    assert torch.equal(x0.cpu(), x0_ref)
    ops.sched_step(d, nan)
    err = _rel(xp, xp_ref)
    print(f"sched_step {name} eta={eta} {shape}: rel-to-scale err {err:.3e}")
    assert int(nan.item()) == 0 and err <= SCHED_TOL, (name, eta, shape, err)
    assert torch.equal(x0.cpu(), x0_ref)


@pytest.mark.parametrize("shape", [(3, 1), (3, 90000)], ids=lambda s: f"C{s[0]}xHW{s[1]}")
@pytest.mark.parametrize("eta", [0.0, 0.85])
def test_sched_step_ddim_options(eta, shape):
    """ddim only: the three clip modes, mask + known, normalised eps, eps_used, and phases 0 / 3 / 1-then-2 / 2 alone on the
    clipped x0, each bit-equal to the one-call form."""
    from diffusion_nlc_amd import ops
    from diffusion_nlc_amd._ext import CLIP_MODES
    S = _sched("ddim", eta)
    C_, HW = shape
    xt, eps, noise, st, sp = _sched_inputs(C_, HW, "opts")
    g = R.gen(("sched-opts", shape))
    dyn = torch.tensor([1.0, 1.75])
    mask = (torch.rand(C_, HW, generator=g) < 0.4).float()
    known = torch.randn(2, C_, HW, 1, generator=g)
    ss = (eps.double() ** 2).sum(dim=(1, 2, 3)).float()
    d_xt, d_noise, d_st, d_sp = _d(xt), _d(noise), _d(st.reshape(-1)), _d(sp.reshape(-1))
    d_eps, d_dyn, d_mask, d_known, d_ss = _d(eps), _d(dyn), _d(mask), _d(known), _d(ss)
    lv = S.get_eps_logvar(st, sp)
    for clip in ("none", "clamp", "dynamic"):
        for use_mask in (False, True):
            for norm in (False, True):
                e = eps
                if norm:                     # utils.normalize with the given sum of squares: (sqrt(D) * e) / max(sqrt(ss), 1e-12)
                    e = (torch.tensor(float(C_ * HW)).sqrt() * eps) / ss.sqrt().clamp(min=1e-12).view(2, 1, 1, 1)
                x0_ref = S.pred_xstart(xt, e, st)
                x0c = x0_ref
                if clip == "clamp":
                    x0c = x0c.clamp(-1, 1)
                elif clip == "dynamic":
                    s = dyn.view(2, 1, 1, 1)
                    x0c = torch.minimum(torch.maximum(x0c, -s), s) / s
                if use_mask:
                    x0c = torch.where(mask.view(1, C_, HW, 1) != 0, known, x0c)
                xp_ref = S.pred_xprev(x0=x0c, eps=e, sigma_t=st, sigma_prev=sp, xt=xt, log_variance=lv, noise=noise)
                kw = dict(clip=CLIP_MODES[clip], dyn_s=d_dyn.data_ptr() if clip == "dynamic" else None,
                          mask=d_mask.data_ptr() if use_mask else None, known=d_known.data_ptr() if use_mask else None,
                          eps_norm_sumsq=d_ss.data_ptr() if norm else None)
                runs = {}
                for form in ("0", "3", "1then2", "2"):
                    x0, xp, eu = (torch.full_like(d_xt, SENTINEL) for _ in range(3))
                    mk = lambda ph: _desc(S, "ddim", d_xt, d_eps, d_noise, d_st, d_sp, x0, xp, eps_used=eu.data_ptr(), phases=ph, **kw)
                    ops.sched_x0(mk(0))
                    assert torch.equal(x0.cpu(), x0_ref), (clip, use_mask, norm)        # IEEE operations only, normalised eps included
                    assert torch.equal(eu.cpu(), e)
                    if form == "1then2":
                        ops.sched_step(mk(1))
                        assert bool((xp == SENTINEL).all())                               # the clip phase writes x0 only
                        ops.sched_step(mk(2))
                    elif form == "2":
                        x0.copy_(runs["0"][0])                                            # the already clipped x0: phase 2 must not clip again
                        ops.sched_step(mk(2))
                    else:
                        ops.sched_step(mk(int(form)))
                    runs[form] = (x0.cpu(), xp.cpu(), eu.cpu())
                x0_got, xp_got, eu_got = runs["0"]
                assert torch.equal(x0_got, x0c), (clip, use_mask, norm)                   # clamp, one division, a select
                assert torch.equal(eu_got, e)
                print(f"sched_step ddim options eta={eta} {shape} {clip} mask={use_mask} norm={norm}: rel-to-scale err {_rel(xp_got, xp_ref):.3e}")
                assert _rel(xp_got, xp_ref) <= SCHED_TOL, (clip, use_mask, norm, _rel(xp_got, xp_ref))
                for form in ("3", "1then2", "2"):
                    assert all(torch.equal(a, b) for a, b in zip(runs[form], runs["0"])), (form, clip, use_mask, norm)


def test_sched_step_nan_flag():
    """Zero on clean input; set by one NaN in the very last element of the last sample (second grid-stride trip); a NaN in x0 does
    not set it when only the clip phase runs."""
    from diffusion_nlc_amd import ops
    S = _sched("ddim", 0.0)
    xt, eps, noise, st, sp = _sched_inputs(1, 262149, "nan")
    d_xt, d_eps, d_noise, d_st, d_sp = _d(xt), _d(eps), _d(noise), _d(st.reshape(-1)), _d(sp.reshape(-1))
    x0, xp = torch.empty_like(d_xt), torch.empty_like(d_xt)
    nan = torch.zeros(1, device=_dev(), dtype=torch.int32)
    d = _desc(S, "ddim", d_xt, d_eps, d_noise, d_st, d_sp, x0, xp, clip=0, phases=0)
    ops.sched_x0(d)
    ops.sched_step(d, nan)
    assert int(nan.item()) == 0
    x0.view(-1)[-1] = float("nan")
    ops.sched_step(_desc(S, "ddim", d_xt, d_eps, d_noise, d_st, d_sp, x0, None, clip=1, phases=1), nan)
    assert int(nan.item()) == 0
    d_eps.view(-1)[-1] = float("nan")
    ops.sched_x0(d)
    ops.sched_step(d, nan)
    assert int(nan.item()) == 1
    assert int(torch.isnan(xp).sum().item()) == 1 and bool(torch.isnan(xp.view(-1)[-1]))


# ---- 7. cast_f64_f32 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1023, 2097159])
def test_cast_f64_f32(n):
    """Round to nearest even, bit for bit with the CPU's conversion: ties, overflow to inf, results that are subnormal or round to
    zero, -0, NaN, +-inf.  n = 2097159 takes the second grid-stride trip of the 2048-workgroup grid."""
    import diffusion_nlc_amd.experiments  # noqa: F401  (edm_experiment is imported from its bottom)
    from diffusion_nlc_amd.edm_experiment import cast_f64_f32
    x = R.cast_values(n)
    got = cast_f64_f32(_d(x)).cpu()
    ref = x.to(F32)
    same = _bits(got) == _bits(ref)
    both_nan = torch.isnan(got) & torch.isnan(ref)
    assert bool((same | both_nan).all()), (x[~(same | both_nan)][:8], got[~(same | both_nan)][:8])
    assert bool(same[~torch.isnan(ref)].all())
    assert int(torch.isnan(got).sum()) == int(torch.isnan(x).sum())


# ---- 8. row_sumsq_f64 / row_cosine_f64 -----------------------------------------------------------------------------------------
F64_D = [1, 63, 1024, 1025, 3072, 196608]


@pytest.mark.parametrize("D", F64_D)
def test_row_sumsq_f64(D):
    """|got - exact| <= (chain + 1) * 2^-53 * exact, exact the correctly rounded sum of the exactly computed squares."""
    import diffusion_nlc_amd.experiments  # noqa: F401  (edm_experiment is imported from its bottom)
    from diffusion_nlc_amd.edm_experiment import row_sumsq_f64
    x = torch.randn(3, D, generator=R.gen(("sumsq64", D)), dtype=F64) * torch.tensor([[1.0], [1e-3], [250.0]], dtype=F64)
    got = row_sumsq_f64(_d(x)).cpu()
    again = row_sumsq_f64(_d(x)).cpu()
    bound = (R.sumsq_chain_f64(D) + 1) * U64
    for b in range(3):
        exact = R.exact_sumsq(x[b].numpy())
        err = abs(got[b].item() - exact) / exact
        print(f"row_sumsq_f64 D={D} row {b}: rel err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (D, b, err, bound)
    assert torch.equal(got, again)


@pytest.mark.parametrize("D", F64_D)
def test_row_cosine_f64(D):
    """Against torch.nn.CosineSimilarity(dim=1, eps=1e-6) in f64 on the CPU.  Bound: the chain bound (chain + 1) * 2^-53 times
    sum |a^ b^| (a^ = a / max(||a||, eps)), i.e. the relative chain bound times the condition of the dot product; the inputs'
    condition is below 1e3 (asserted in tests/test_host_cpu.py).  Orthogonal and zero rows have only exact-zero products."""
    from diffusion_nlc_amd import _ext
    a, b = R.cosine_rows(D)
    ref = torch.nn.CosineSimilarity(dim=1, eps=R.COS_EPS)(a, b)
    da, db = _d(a), _d(b)
    out = torch.full((a.shape[0] + PAD,), SENTINEL, device=_dev(), dtype=F64)
    _ext.check(_ext.load().nlc_row_cosine_f64(da.data_ptr(), db.data_ptr(), R.COS_EPS, out.data_ptr(), a.shape[0], D, _stream()),
               "nlc_row_cosine_f64")
    got = out.cpu()
    assert bool((got[a.shape[0]:] == SENTINEL).all())
    got = got[:a.shape[0]]
    scale, _ = R.cosine_parts(a, b)
    bound = (R.sumsq_chain_f64(D) + 1) * U64 * scale
    err = (got - ref).abs()
    print(f"row_cosine_f64 D={D}: err {err.tolist()} bound {bound.tolist()}")
    assert bool((err <= bound).all()), (D, err, bound)
    k = R.COS_KINDS
    assert abs(got[k.index("identical")].item() - 1.0) <= bound[1].item() and abs(got[k.index("opposite")].item() + 1.0) <= bound[2].item()
    assert got[k.index("orthogonal")].item() == 0.0 and got[k.index("zero")].item() == 0.0
    assert 0.0 < abs(got[k.index("tiny")].item()) <= 1.0e-3 * (1 + 1e-9)                       # the eps clamp: |cos| scaled by 1e-9 / 1e-6


# ---- 9. edm_scalars -------------------------------------------------------------------------------------------------------------
C_NOISE_ULPS_MEASURED = 1.816      # largest distance of logf(s) / 4 from the f64 value seen on the MI355X, in f32 ulps of that value


@pytest.mark.parametrize("sigma_data", [0.5, 1.0])
@pytest.mark.parametrize("B", [1, 257])
def test_edm_scalars(B, sigma_data):
    """src/experiments.py:779-797 of the reference.  f64 evaluation on the f32 sigma; every term is positive, so the counts are of
    half ulps of the result: c_skip sd*sd, s*s, +, / = 4 (+1); c_out s*sd, s*s, sd*sd, +, sqrt, / = 6 (+1); c_in sd*sd, s*s, +,
    sqrt, / = 5 (+1).  c_noise = logf(s) / 4 is not correctly rounded: measured on the MI355X 1.816 ulp (1.480e-07 relative) at the
    worst of the 257 sigmas; asserted: twice that, 3.632 ulp, capped at 1e-6 relative (the cap does not bind); logf(1) is exactly 0."""
    from diffusion_nlc_amd import _ext
    sigma = R.edm_sigmas(B, sigma_data)
    outs = torch.full((4, B + PAD), SENTINEL, device=_dev())
    ds = _d(sigma)
    _ext.check(_ext.load().nlc_edm_scalars(ds.data_ptr(), sigma_data, *(outs[i].data_ptr() for i in range(4)), B, _stream()),
               "nlc_edm_scalars")
    got = outs.cpu()
    assert bool((got[:, B:] == SENTINEL).all())
    c_in, c_noise, c_skip, c_out = (got[i, :B].double() for i in range(4))
    r_in, r_noise, r_skip, r_out = R.edm_scalars_f64(sigma, sigma_data)
    assert bool(((c_skip - r_skip).abs() <= 5 * U32 * r_skip).all())
    assert bool(((c_out - r_out).abs() <= 7 * U32 * r_out).all())
    assert bool(((c_in - r_in).abs() <= 6 * U32 * r_in).all())
    err = (c_noise - r_noise).abs()
    ulp = torch.tensor(np.spacing(np.abs(r_noise.float().numpy()).astype(np.float32)).astype(np.float64)).clamp(min=2.0 ** -149)
    print(f"edm_scalars B={B} sd={sigma_data}: c_noise max err {(err / ulp).max().item():.3f} ulp, rel {(err / r_noise.abs().clamp(min=1e-30)).max().item():.3e}")
    assert bool((err <= torch.minimum(2 * C_NOISE_ULPS_MEASURED * ulp, 1e-6 * r_noise.abs())).all())
    if sigma_data == 1.0:
        assert got[1, B - 1].item() == 0.0                                    # logf(1) = 0 exactly



# ---- 10. edm_eps / f64_lincomb --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [1, 1025, 262149])
def test_edm_eps_and_f64_lincomb(D, B):
    """IEEE operations only (f32: two products and a sum; the widening; f64: a difference and a quotient / a product or two and a
    sum): bit-equal.  D = 262149 takes the second grid-stride trip."""
    from diffusion_nlc_amd import _ext
    import diffusion_nlc_amd.experiments  # noqa: F401  (edm_experiment is imported from its bottom)
    from diffusion_nlc_amd.edm_experiment import lincomb
    g = R.gen(("edm_eps", D, B))
    x = torch.randn(B, D, generator=g, dtype=F64) * 3
    x32, Fx = x.float(), torch.randn(B, D, generator=g)
    cs, co = torch.rand(B, generator=g), torch.rand(B, generator=g)
    sd = torch.rand(B, generator=g, dtype=F64) * 5 + 0.01
    dx = cs[:, None] * x32 + co[:, None] * Fx
    den_ref = dx.double()
    eps_ref = (x - den_ref) / sd[:, None]
    dv = [_d(v) for v in (x, x32, Fx, cs, co, sd)]
    for with_den in (True, False):
        eps, den = torch.full_like(dv[0], SENTINEL), torch.full_like(dv[0], SENTINEL)
        _ext.check(_ext.load().nlc_edm_eps(*(v.data_ptr() for v in dv), eps.data_ptr(), den.data_ptr() if with_den else None, B, D,
                                           _stream()), "nlc_edm_eps")
        assert torch.equal(eps.cpu(), eps_ref)
        assert torch.equal(den.cpu(), den_ref) if with_den else bool((den == SENTINEL).all())
    y = torch.randn(B, D, generator=g, dtype=F64)
    ca, cb = torch.randn(B, generator=g, dtype=F64), torch.randn(B, generator=g, dtype=F64)
    assert torch.equal(lincomb(dv[0], _d(ca)).cpu(), ca[:, None] * x)
    assert torch.equal(lincomb(dv[0], _d(ca), _d(y), _d(cb)).cpu(), ca[:, None] * x + cb[:, None] * y)


# ---- 11. Inpainting.A / A_pinv --------------------------------------------------------------------------------------------------
def _missing(kind, n, g):
    if kind == "none":
        return torch.zeros(0, dtype=torch.long)
    if kind == "keep-one":
        return torch.cat([torch.arange(0, n // 3), torch.arange(n // 3 + 1, n)])
    if kind == "half":
        return torch.randperm(n, generator=g)[: n // 2]
    return torch.arange(1, n, 2)                     # checkerboard over the interleaved (p, c) index


@pytest.mark.parametrize("kind", ["none", "keep-one", "half", "checker"])
@pytest.mark.parametrize("img_dim", [1, 8, 300])
@pytest.mark.parametrize("channels", [1, 3])
def test_inpainting_gathers(channels, img_dim, kind):
    """Pure gathers: bit-equal to the permute / index / scatter chain of the reference.  3 * 300^2 = 270000 entries exceed the
    1024-workgroup grid of both kernels."""
    from diffusion_nlc_amd.constraint_functions import Inpainting
    n = channels * img_dim ** 2
    g = R.gen(("inpaint", channels, img_dim, kind))
    missing = _missing(kind, n, g)
    op = Inpainting(channels, img_dim, missing, _dev())
    keep = torch.ones(n, dtype=torch.bool)
    keep[missing] = False
    kept = torch.nonzero(keep).reshape(-1)
    assert torch.equal(op.kept_indices.cpu(), kept)
    mask_ref = keep.view(img_dim * img_dim, channels).t().float()
    assert torch.equal(op.mask_chw.cpu(), mask_ref)
    B = 2
    x = torch.randn(B, channels, img_dim, img_dim, generator=g)
    y_ref = x.permute(0, 2, 3, 1).reshape(B, -1)[:, kept]
    y = op.A(x.to(_dev()))
    assert torch.equal(y.cpu(), y_ref)
    back_ref = torch.zeros(B, n)
    back_ref[:, kept] = y_ref
    back_ref = back_ref.view(B, img_dim, img_dim, channels).permute(0, 3, 1, 2).reshape(B, -1)
    back = op.A_pinv(y)
    assert torch.equal(back.cpu(), back_ref)
    assert torch.equal(op.A(back).cpu(), y_ref)                                            # A A^+ = 1
    assert torch.equal(back.cpu(), (x * mask_ref.view(1, channels, img_dim, img_dim)).reshape(B, -1))   # A^+ A = the mask


# ---- 12. resample / layout ------------------------------------------------------------------------------------------------------
def _per(dtype):
    return 4 if dtype == F32 else 8


def _rnd_bound(dtype):
    """One rounding to the storage type (8 / 11 significand bits): half an ulp, relative."""
    return {F32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def _pool_ref(x):
    """((x00 + x01) + x10 + x11) * 0.25 in f32, the kernel's pixel order; x: [B, H, W, C] in the storage type."""
    f = x.float()
    return ((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2] + f[:, 1::2, 1::2]) * 0.25


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_resample_shapes(dtype):
    """upsample2x and pad_rb are copies: bit-equal.  avgpool2x2 in f32 is bit-equal to the ordered sum; in the 16-bit types the f32
    result is rounded once (half an ulp of the storage type).  C of one and of three 16-byte chunks, W = 1, and one shape each
    with more than 524288 work items (the 2048-workgroup grid's second trip)."""
    from diffusion_nlc_amd import ops
    per = _per(dtype)
    g = R.gen(("resample", str(dtype)))

    def mk(B, H, W, Cc):
        return torch.randn(B, H, W, Cc, generator=g).to(dtype)

    def check_pool(x):
        got = ops.avgpool2x2(x.to(_dev())).cpu()
        ref = _pool_ref(x)
        if dtype == F32:
            assert torch.equal(got, ref)
        else:
            assert bool(((got.float() - ref).abs() <= _rnd_bound(dtype) * ref.abs() + 2.0 ** -25).all())    # (+ half an f16 subnormal step)

    def check_up_pad(x):
        up = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        assert torch.equal(ops.upsample2x(x.to(_dev())).cpu(), up)
        assert torch.equal(ops.pad_rb(x.to(_dev())).cpu(), F.pad(x, (0, 0, 0, 1, 0, 1)))

    for Cc in (per, 3 * per):
        for H, W in ((2, 2), (1, 1), (5, 1)):
            check_up_pad(mk(2, H, W, Cc))
        for H, W in ((2, 2), (6, 2)):
            check_pool(mk(2, H, W, Cc))
    check_pool(mk(1, 840, 840, 3 * per))                      # 420 * 420 * 3 = 529200 work items
    x = mk(1, 210, 210, 3 * per)
    assert torch.equal(ops.upsample2x(x.to(_dev())).cpu(), x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))
    x = mk(1, 419, 419, 3 * per)
    assert torch.equal(ops.pad_rb(x.to(_dev())).cpu(), F.pad(x, (0, 0, 0, 1, 0, 1)))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_transposes_around_the_tile(dtype):
    """HW and C each of 1, 31, 32, 33, 65 against the 32 x 32 tile: widening to f32 is exact, narrowing is one correctly rounded
    conversion - both bit-equal."""
    from diffusion_nlc_amd import ops
    g = R.gen(("transpose", str(dtype)))
    for HW in (1, 31, 32, 33, 65):
        for Cc in (1, 31, 32, 33, 65):
            x = torch.randn(2, Cc, HW, 1, generator=g)
            nhwc = ops.nchw_f32_to_nhwc(x.to(_dev()), dtype)
            assert torch.equal(nhwc.cpu(), x.permute(0, 2, 3, 1).contiguous().to(dtype)), (HW, Cc)
            back = ops.nhwc_to_nchw_f32(nhwc)
            assert torch.equal(back.cpu(), x.to(dtype).float()), (HW, Cc)


# ---- 13. timestep embedding through the ABI -------------------------------------------------------------------------------------
TEMB_MEASURED = 4.998e-8                      # largest absolute error seen on the MI355X
TEMB_TOL_ABS = min(2 * TEMB_MEASURED, 2e-6)   # twice that, capped at the 2e-6 of test_timestep_embedding


@pytest.mark.parametrize("dim", [129, 3])
@pytest.mark.parametrize("sin_first", [False, True])
def test_timestep_embedding_odd_dim(dim, sin_first):
    """An odd ``dim`` (not reachable from ops.timestep_embedding): the last column is zero, the rest is the dim - 1 embedding.
    B * half = 5 * 64 and 5 * 1 are no multiples of 256.  cosf / sinf against f64 on the f32 product t * freq.  Measured on the
    MI355X: largest absolute error 4.998e-08 (dim 129), 3.919e-08 (dim 3); asserted: twice the larger, 9.996e-08 (the cap of 2e-6
    does not bind)."""
    from diffusion_nlc_amd import _ext, ops
    half = dim // 2
    t = torch.tensor([0.0, 1.0, 17.5, 954.0, 1000.0])
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=F32) / half)
    out = torch.full((t.numel() + 1, dim), SENTINEL, device=_dev())
    dt, df = _d(t), _d(freqs)
    _ext.check(_ext.load().nlc_timestep_embedding(dt.data_ptr(), df.data_ptr(), out.data_ptr(), t.numel(), dim, 1 if sin_first else 0,
                                                  _stream()), "nlc_timestep_embedding")
    got = out.cpu()
    assert bool((got[-1] == SENTINEL).all())
    got = got[:-1]
    assert bool((got[:, -1] == 0.0).all())
    assert torch.equal(got[:, :-1], ops.timestep_embedding(dt, df, sin_first).cpu())
    args = (t[:, None] * freqs[None]).double()
    ref = torch.cat([torch.sin(args), torch.cos(args)] if sin_first else [torch.cos(args), torch.sin(args)], dim=-1)
    err = (got[:, :-1].double() - ref).abs().max().item()
    print(f"timestep_embedding dim={dim} sin_first={sin_first}: max abs err {err:.3e}")
    assert err <= TEMB_TOL_ABS


# ---- 14. conv_first -------------------------------------------------------------------------------------------------------------
def _totals(st):
    """Ride-along GroupNorm statistics, int64 [B, C/g, 4] fixed-point (hi, lo) pairs -> double [B, C/g, 2] = (sum, sum of squares)."""
    t = st.cpu().double()
    return torch.stack([t[..., 0] + t[..., 1] * 2.0 ** -44, t[..., 2] + t[..., 3] * 2.0 ** -44], dim=-1)


def _close(got, ref, tol, what=""):
    got = got.detach().float().cpu()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item() / scale
    assert err <= tol, f"{what}: max rel-to-scale err {err:.3e} > {tol:.1e} (scale {scale:.3e})"


CONV_FIRST_CASES = [
    # Cin, k, Cout, H, W, B
    (1, 5, 48, 8, 8, 2),          # K = 25: the MFMA kernel in the 16-bit types
    (4, 1, 16, 8, 8, 2),          # K = 4
    (4, 3, 300, 6, 33, 2),        # K = 36: the VALU kernel in every type, second trip of its Cout loop
    (2, 7, 24, 9, 40, 1),         # K = 98
    (3, 3, 32, 65, 64, 16),       # MFMA: two tiles per workgroup, the last workgroup has one, no statistics
    (3, 3, 32, 128, 64, 16),      # MFMA: two tiles per workgroup with ride-along statistics
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CONV_FIRST_CASES, ids=lambda c: "Cin{}-k{}-Cout{}-{}x{}-B{}".format(*c))
def test_conv_first_shapes(case, dtype):
    """Against F.conv2d at the tolerances of test_ops_gpu.test_conv_first."""
    from diffusion_nlc_amd import ops
    Cin, k, Cout, H, W, B = case
    g = R.gen(("conv_first", case))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g) * 0.1
    sc = torch.rand(B, generator=g) + 0.5
    ref = F.conv2d(x * sc[:, None, None, None], w, b, padding=k // 2)
    wp = w.permute(0, 2, 3, 1).reshape(Cout, k * k, Cin).contiguous().to(_dev())
    got = ops.conv_first(x.to(_dev()), wp, b.to(_dev()), dtype, in_scale=sc.to(_dev()))
    _close(got.permute(0, 3, 1, 2), ref, {F32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 2e-3}[dtype], f"conv_first {case}")
    st = getattr(got, "_nlc_stats", None)
    if case == (3, 3, 32, 128, 64, 16):
        assert (st is not None) == (dtype != F32)
    if case == (3, 3, 32, 65, 64, 16):
        assert st is None
    if st is not None:                                 # the totals are of the stored output
        gran = Cout // st.shape[1]
        ch = got.float().cpu().view(B, H * W, Cout // gran, gran)
        assert (_totals(st)[..., 0] - ch.double().sum(dim=(1, 3))).abs().max() < 5e-2
        assert ((_totals(st)[..., 1] - (ch.double() ** 2).sum(dim=(1, 3))) / (ch.double() ** 2).sum(dim=(1, 3))).abs().max() < 5e-4
