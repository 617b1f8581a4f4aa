"""Randomised sweep of the small-map 3x3 kernel with the GroupNorm of its input fused (conv_small.hip, nlc_conv_desc.gn_in), through
Norm.then_conv the way the networks build a ResBlock:  h = then_conv(x)  and  y = then_conv(h, FiLM, res = x).  Which of the eight
template instantiations a launch takes, how many channel blocks a slice has, how K is split (1 ... 8 ways; 3, 5, 7 only exist in the
last-arriver form), which reduction finishes a tile and whether a tile is a few rows of one image or 2 - 4 whole images is a function of
(B, H, W, C0, C1, Cout) and the CU count; the hand-picked shapes of test_ops_gpu.py visit seven points of that space.

Per stage of every case:
  * REFERENCE: F.group_norm (+FiLM) (+SiLU) in f64 on the CPU over the STORED 16-bit inputs, the normalised tensor rounded to the compute
    dtype, F.conv2d in f64 with the weights rounded to the dtype, + bias + emb + res, activation; stage 2 is teacher-forced on the
    GPU's stored h.  Tolerance: test_ops_gpu._tol (bf16 2e-2, f16 3e-3 of the reference's scale).  A case above CPU_FLOPS per stage is
    only drawn when its grid is near the CU count (the shapes the benchmark runs) and then takes the convolution of the reference from
    the library's exact-f32 generic kernel (pinned against torch by test_ops_gpu.py and test_conv_fuzz_gpu.py); at most one case in
    eight (test_case_list_... checks the list on the CPU);
  * ride-along totals of every output against f64 sums of the stored output (1e-4, the conv fuzz's bounds); a launch the small kernel
    takes always carries them;
  * BIT IDENTITY of a second launch after a 64 MB sweep of the caches, a third beside a busy second stream, the last-arriver reduction
    (tuning bit 23) against the default and against the distributed one on 128-pixel tiles (bit 22), and a launch with ops.CONV_DEBUG = 1
    at the end, which refuses to start unless every launch before it left the workspace's arrival counters zero (stored outputs; the
    totals too wherever the schedule is the same);
  * the host queries: query_gn_in <=> the launch with gn_in is accepted <=> the geometry rule restated below (_geom); a rejected shape
    goes through then_conv's separate GroupNorm pass without raising; nlc_conv2d_stats_partials > 0 for every small-map launch.

The case list is seeded: the same cases in every run.  Longer soak:  NLC_FUZZ_CASES=1000 pytest -m gpu tests/test_small_fuzz_gpu.py
"""
import ctypes as C
import math
import os
import random

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

DEV = "cuda:0"
N_CASES = int(os.environ.get("NLC_FUZZ_CASES", "64"))
CPU_FLOPS = 5e9              # per stage: about a second of f64 convolution on the CPU
GENERIC_FLOPS = 4e10         # per stage, for the cases whose convolution reference is the exact-f32 generic kernel
NCU = 256                    # MI355X; the GPU tests use the device's own count
MAPS = [(8, 8), (16, 16), (32, 32), (8, 16), (16, 8), (4, 16), (2, 32), (16, 32), (8, 32), (24, 8), (6, 32)]
TOL = {"bf16": 2e-2, "f16": 3e-3}          # == tests/test_ops_gpu.py::_tol (asserted on the GPU box below)
KB, WST, LDS = 128, 16384, 160 * 1024


# ---- the geometry rule of conv_small.hip (nlc_conv_small_geom / small_geom_for), restated: the accepted / rejected boundary is checked
#      against it on the GPU, and the CPU tests below use it to say which instantiations and K-splits the seeded list reaches
def _geom_for(M, H, W, NT, Ctot, wm, ncu):
    bmt = wm * 64
    if M % bmt:
        return None
    tr = bmt // W
    if tr <= H:
        if H % tr:
            return None
        nseg, sr = 1, tr
    else:
        if tr % H:
            return None
        nseg, sr = tr // H, H
    if nseg > 4:
        return None
    mt, slots = M // bmt, nseg * (sr + 2) * (W + 2)
    if slots > 7 * wm * 16 or mt * NT > 511:
        return None
    ncb, nb, best = Ctot // 64, 0, 0
    for c in (4, 3, 2, 1):
        if ncb % c or ncb // c > 8 or c * slots * KB + 3 * WST + nseg * c * 64 * 8 > LDS:
            continue
        grid = mt * NT * (ncb // c)
        if grid <= ncu and grid > best:
            best, nb = grid, c
    if not nb:
        return None
    left = LDS - nb * slots * KB - nseg * nb * 64 * 8
    nwst = 8 if left >= 8 * WST else 6 if left >= 6 * WST else 4 if left >= 4 * WST else 3
    if nwst - 1 > nb * 9:
        nwst = 4
    return dict(wm=wm, MT=mt, nb=nb, ks=ncb // nb, nwst=nwst, nseg=nseg, grid=mt * NT * (ncb // nb))


def _geom(B, H, W, C0, C1, Cout, ncu=NCU, tuning=0):
    Ctot = C0 + C1
    if W not in (8, 16, 32) or H & 1 or (H * W) % 64 or Cout % 128 or Ctot % 64 or C0 % 64:
        return None
    M, NT = B * H * W, Cout // 128
    g2 = None if tuning & (1 << 26) else _geom_for(M, H, W, NT, Ctot, 2, ncu)
    g4 = None if tuning & (1 << 22) else _geom_for(M, H, W, NT, Ctot, 4, ncu)
    can_dist = lambda q: q["ks"] in (2, 4, 8) and q["grid"] <= ncu
    if g4 is not None and not (g4["ks"] == 1 or can_dist(g4)):
        g4 = None
    use4 = g4 is not None and (g2 is None or (g2["nwst"] < 4 and g2["ks"] > 1 and g4["grid"] * 4 >= ncu * 3))
    g = g4 if use4 else g2
    if g is None:
        return None
    g = dict(g)
    g["dist"] = g["ks"] > 1 and can_dist(g) and (g["wm"] == 4 or not tuning & (1 << 23))
    return g


def _draw(rng):
    H, W = rng.choice(MAPS)
    B = rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16])
    ctot = rng.choice([64, 128, 192, 256, 320, 384, 448, 512, 768, 1024, 1536])
    c1 = rng.choice([0] + list(range(64, ctot, 64))) if rng.random() < 0.5 else 0
    cout = rng.choice([128, 256, 384, 512, 1024])
    c = dict(B=B, H=H, W=W, C0=ctot - c1, C1=c1, Cout=cout, groups=rng.choice([8, 16, 32]), groups2=rng.choice([8, 16, 32]),
             film=rng.random() < 0.5, emb=rng.random() < 0.4, res=rng.random() < 0.5, act1=rng.random() < 0.25, act2=rng.random() < 0.25,
             affine1=rng.random() < 0.75, affine2=rng.random() < 0.75, silu1=rng.random() < 0.7, silu2=rng.random() < 0.7,
             bias=rng.random() < 0.85, k0=rng.choice([1, 3]), k1=rng.choice([1, 3]), gran4=rng.random() < 0.5,
             dtype=rng.choice(["bf16", "f16"]), seed=rng.randrange(1 << 30), generic=False)
    if (ctot // c["groups"]) % 4:                 # (a group that is no whole number of 4-channel chunks: no totals can describe it)
        return None, 0.0
    return c, 2.0 * B * H * W * cout * max(ctot, cout) * 9


def _cases(n, seed=20261020):
    """n // 8 cases from the grid extreme first (the benchmark's regime: four-block slices, three-stage weight rings and 256-pixel
    tiles exist only where a launch fills the chip, far above what the CPU convolves in a second; their convolution reference is
    the generic kernel) - each with a (tile height, ring depth) that the cheap cases do not reach, once per dtype - then the cases
    under CPU_FLOPS per stage."""
    rng = random.Random(seed)
    out, seen = [], set()
    for _ in range(20000):
        if len(out) >= n // 8:
            break
        c, flops = _draw(rng)
        if c is None or not CPU_FLOPS < flops <= GENERIC_FLOPS:
            continue
        gs = [_geom(c["B"], c["H"], c["W"], c["C0"], c["C1"], c["Cout"]), _geom(c["B"], c["H"], c["W"], c["Cout"], 0, c["Cout"])]
        forms = {(g["wm"], g["nwst"], c["dtype"]) for g in gs if g and g["grid"] * 4 >= NCU * 3 and (g["wm"], g["nwst"]) not in ((2, 8), (2, 6), (2, 4))}
        if forms - seen:
            seen |= forms
            out.append(dict(c, generic=True))
    while len(out) < n:
        c, flops = _draw(rng)
        if c is not None and flops <= CPU_FLOPS:
            out.append(c)
    return out


# ---- edge values: a short fixed list through the same checker at the smallest shapes (both have two images per 128-pixel tile)
_E1 = dict(B=2, H=8, W=8, C0=64, C1=0, Cout=128, groups=8, groups2=8)
_E2 = dict(B=4, H=8, W=8, C0=128, C1=0, Cout=128, groups=8, groups2=8)
_EDEF = dict(film=True, emb=True, res=True, act1=False, act2=False, affine1=True, affine2=True, silu1=True, silu2=True, bias=True, k0=1, k1=1,
             gran4=True, generic=False, seed=11)


def _edges():
    out = []
    for dt in ("bf16", "f16"):
        for name, shape in (("64to128", _E1), ("128to128", _E2)):
            for edge in ("var0", "ratio300", "pad", "nan", "inf"):
                out.append(dict(_EDEF, **shape, dtype=dt, edge=edge, id=f"{edge}-{name}-{dt}"))
        # a group across the two sources: with whole 64-channel blocks from either source (the kernel's rule) no 64-wide group can
        # take 32 channels from each, so: 96-channel groups, [96, 192) = the last 32 channels of x0 + x1, [0, 96) = x0 + the first 32 of x1
        out.append(dict(_EDEF, **_E1, dtype=dt, edge="straddle", id=f"straddle-last32-of-x0-{dt}") | dict(C0=128, C1=64, groups=2))
        out.append(dict(_EDEF, **_E1, dtype=dt, edge="straddle", id=f"straddle-first32-of-x1-{dt}") | dict(C0=64, C1=128, groups=2))
    return out


def _case_id(c):
    return (f"B{c['B']}-{c['H']}x{c['W']}-{c['C0']}+{c['C1']}to{c['Cout']}-g{c['groups']}-{c['dtype']}"
            + ("-generic" if c["generic"] else ""))


def _dt(c):
    return torch.bfloat16 if c["dtype"] == "bf16" else torch.float16


# ---- the operands of a case (CPU, f32 masters)
def _producer_operands(c, g, cch, k, first):
    """z [B, 64, H, W], the k x k weights and bias of the convolution that produces cch (rounded up to whole 128-channel tiles) channels."""
    B, H, W = c["B"], c["H"], c["W"]
    cp = -(-cch // 128) * 128
    z = torch.randn(B, 64, H, W, generator=g)
    wz = torch.randn(cp, 64, k, k, generator=g) / (8.0 * k)
    bz = torch.randn(cp, generator=g) * 0.5 + 0.3
    edge = c.get("edge")
    if first and edge == "var0":                # group 0: the same constant in every channel and pixel
        gs = (c["C0"] + c["C1"]) // c["groups"]
        wz[:gs] = 0.0
        bz[:gs] = 0.75
    if first and edge == "ratio300":            # group 1: mean / std ~ 300 (std ~ 1 from the weights, bias 300)
        gs = (c["C0"] + c["C1"]) // c["groups"]
        bz[gs:2 * gs] = 300.0
    if first and edge in ("nan", "inf"):        # one bad value in image 1 of the producer's input
        z[1, 5, 3, 4] = float(edge)
    return z, wz, bz


def _operands(c):
    g = torch.Generator().manual_seed(c["seed"])
    Cin, Cout, B = c["C0"] + c["C1"], c["Cout"], c["B"]
    o = dict(p0=_producer_operands(c, g, c["C0"], c["k0"], True))
    o["p1"] = _producer_operands(c, g, c["C1"], c["k1"], False) if c["C1"] else None
    pad = c.get("edge") == "pad"
    for s, cin in ((1, Cin), (2, Cout)):
        o[f"w{s}"] = torch.randn(Cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
        o[f"b{s}"] = torch.randn(Cout, generator=g) * 0.1
        o[f"gamma{s}"] = torch.rand(cin, generator=g) + 0.5 if c[f"affine{s}"] else None
        o[f"beta{s}"] = (torch.full((cin,), 3.0) if pad else torch.randn(cin, generator=g) * 0.2) if c[f"affine{s}"] else None
    o["ss"] = torch.randn(B, 2 * Cout + 16, generator=g) * 0.3
    if pad:
        o["ss"][:, Cout:2 * Cout] = 2.0
    o["emb"] = torch.randn(B, Cout + 16, generator=g)
    o["res"] = torch.randn(B, c["H"], c["W"], Cout, generator=g)
    return o


def _reference(c, s, x_nhwc64, o, conv=None):
    """Stage s (1 | 2) in f64 on the CPU from the stored input [B, H, W, Cin] (double).  ``conv``: the convolution itself (normalised tensor
    rounded to the dtype, NCHW f64 -> NCHW f64 result with bias, emb, res and activation) when it does not run on the CPU."""
    dt = _dt(c)
    Cout = c["Cout"]
    groups = c["groups"] if s == 1 else c["groups2"]
    gamma, beta = o[f"gamma{s}"], o[f"beta{s}"]
    y = F.group_norm(x_nhwc64.permute(0, 3, 1, 2), groups, None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps=1e-5)
    if s == 2 and c["film"]:
        y = y * (1 + o["ss"][:, :Cout].double()[:, :, None, None]) + o["ss"][:, Cout:2 * Cout].double()[:, :, None, None]
    if c[f"silu{s}"]:
        y = F.silu(y)
    y = y.to(dt).double()
    emb = o["emb"][:, :Cout].double() if (s == 1 and c["emb"]) else None
    res = _res_of(c, s, o)
    act = c[f"act{s}"]
    bias = o[f"b{s}"].double() if c["bias"] else None
    if conv is not None:
        return conv(y, o[f"w{s}"].to(dt), bias, emb, res, act)
    r = F.conv2d(y, o[f"w{s}"].to(dt).double(), bias, padding=1)
    if emb is not None:
        r = r + emb[:, :, None, None]
    if res is not None:
        r = r + res.double().permute(0, 3, 1, 2)
    if act:
        r = F.silu(r)
    return r.permute(0, 2, 3, 1)


def _res_of(c, s, o):
    """Stage 2's residual as stored (16-bit, CPU): the block's input x when Cin == Cout and it is one tensor, else a drawn one."""
    if s != 2 or not c["res"]:
        return None
    return o["x_stored"] if (c["C1"] == 0 and c["C0"] == c["Cout"]) else o["res"].to(_dt(c))


# ---- CPU: the list itself
def test_case_list_is_seeded_within_the_reference_cap_and_reaches_every_form():
    a, b = _cases(N_CASES), _cases(N_CASES)
    assert a == b and len(a) == N_CASES
    assert len({_case_id(c) + str(c["seed"]) for c in a}) == N_CASES
    assert sum(c["generic"] for c in a) * 8 <= N_CASES, "more than one case in eight skips the CPU reference"
    for c in a:
        flops = 2.0 * c["B"] * c["H"] * c["W"] * c["Cout"] * max(c["C0"] + c["C1"], c["Cout"]) * 9
        assert flops <= (GENERIC_FLOPS if c["generic"] else CPU_FLOPS)
    if N_CASES < 64:
        return
    # what the default list reaches (at 256 CUs), both stages, the default schedule; the networks at their benchmark batches launch
    # <4,3> <4,4> <2,3> <2,4> <2,6> <2,8> (profiles/r05_kernel_table*.txt)
    inst, ks, last, multi, rejected = set(), set(), set(), set(), set()
    for c in a:
        for C0, C1 in ((c["C0"], c["C1"]), (c["Cout"], 0)):
            g = _geom(c["B"], c["H"], c["W"], C0, C1, c["Cout"])
            if g is None:
                rejected.add((c["H"], c["W"]))
                continue
            inst.add((g["wm"], g["nwst"]))
            ks.add(g["ks"])
            if g["ks"] > 1 and not g["dist"]:
                last.add(g["ks"])
            if g["nseg"] > 1:
                multi.add((g["nseg"], c["B"]))
    assert inst >= {(4, 3), (4, 4), (2, 3), (2, 4), (2, 6), (2, 8)}, sorted(inst)
    assert ks >= {1, 2, 3, 4, 5, 6, 7, 8}, sorted(ks)
    assert last >= {3, 5, 7}, sorted(last)
    assert any(b not in (1, 2, 4, 8, 16) for _, b in multi), sorted(multi)
    assert {(24, 8), (6, 32)} <= rejected
    for H, W in ((24, 8), (6, 32)):
        for B in (1, 2, 4, 8, 16):
            assert _geom(B, H, W, 128, 0, 128) is None


def _kernel_model(x64, groups, gamma, beta):
    """The kernel's arithmetic for the normalisation (conv_small.hip, gn_group_from_totals_t): mean, var in f64 from exact totals, rstd and
    the coefficients a = rstd * gamma, b = beta - mean * a in f32, y = a * x + b in f32."""
    B, C, H, W = x64.shape
    xg = x64.reshape(B, groups, -1)
    mean = xg.mean(dim=2)
    var = ((xg * xg).mean(dim=2) - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt((var + 1e-5).float())).float()
    gs = C // groups
    a = rstd.repeat_interleave(gs, dim=1) * gamma.float()[None]
    b = beta.float()[None] - mean.float().repeat_interleave(gs, dim=1) * a
    return a[:, :, None, None] * x64.float() + b[:, :, None, None]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_reference_at_mean_over_std_300_has_headroom(dtype):
    """The edge case 'mean / std ~ 300 in one group' is only a fair test if legitimate arithmetic (f32 coefficients, as the kernel has
    them) stays well inside _tol of the f64 reference there.  Measured on the CPU, 64 -> 128 @8x8 (the stored group has mean / std 242
    in bf16, whose spacing at 300 is 2, and 275 in f16): the f32-coefficient model is 5.2e-6 (bf16, _tol 2e-2) and 1.7e-5 (f16, _tol 3e-3)
    of the scale away from the f64 reference - a few flipped roundings of normalised values - so the ratio is not lowered."""
    dt = torch.bfloat16 if dtype == "bf16" else torch.float16
    c = dict(_EDEF, **_E1, dtype=dtype, edge="ratio300")
    o = _operands(c)
    z, wz, bz = o["p0"]
    x = F.conv2d(z.to(dt).float(), wz.to(dt).float(), bz)[:, :c["C0"]].to(dt).double()          # the producer, as stored
    gs = c["C0"] // c["groups"]
    grp = x[:, gs:2 * gs]
    ratio = (grp.mean(dim=(1, 2, 3)) / grp.std(dim=(1, 2, 3))).abs().min().item()
    assert 100.0 <= ratio <= 1000.0, ratio
    ref = _reference(c, 1, x.permute(0, 2, 3, 1), o)
    yk = F.silu(_kernel_model(x, c["groups"], o["gamma1"], o["beta1"])).to(dt).double()
    got = F.conv2d(yk, o["w1"].to(dt).double(), o["b1"].double(), padding=1) + o["emb"][:, :c["Cout"]].double()[:, :, None, None]
    err = (got.permute(0, 2, 3, 1) - ref).abs().max().item() / ref.abs().max().item()
    print(f"small-fuzz headroom {dtype}: mean/std {ratio:.0f}, f32-coefficient model vs f64 reference {err:.3e} (tol {TOL[dtype]:.0e})")
    assert err <= 0.25 * TOL[dtype], err


# ---- GPU
_STATE = {}


def _same(a, b) -> bool:          # bit patterns (a NaN equals itself); a plain bool: pytest's assertion rewriting would otherwise print both tensors
    if a.is_floating_point() and a.element_size() == 2:
        a, b = a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)
    return bool(torch.equal(a, b))


def _buf(name, nbytes):
    if name not in _STATE:
        _STATE[name] = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    return _STATE[name]


def _side():
    if "side" not in _STATE:
        _STATE["side"] = torch.cuda.Stream()
    return _STATE["side"]


def _norm(gamma, beta, groups):
    from diffusion_nlc_amd.hipnet import Norm
    n = Norm.__new__(Norm)
    n.gamma = None if gamma is None else gamma.to(DEV)
    n.beta = None if beta is None else beta.to(DEV)
    n.groups, n.eps = groups, 1e-5
    return n


def _produce(c, ops, operands, cch):
    """A real convolution's output with its ride-along totals; a channel count that is no whole 128-channel tile is the leading
    channels of the next larger launch, with the totals of exactly those channels."""
    dt = _dt(c)
    z, wz, bz = operands
    y = ops.conv2d(z.permute(0, 2, 3, 1).contiguous().to(DEV).to(dt), ops.pack_conv(wz, bz, dt, torch.device(DEV)))
    st = ops.ride_stats(y)
    assert st is not None, "the producer carries no totals"
    if y.shape[-1] != cch:
        gran = y.shape[-1] // st.shape[1]
        y = y[..., :cch].contiguous()
        y._nlc_stats = st[:, :cch // gran].contiguous()
    return y


def _check_totals(y, st, finite_images=None):
    B, H, W, cout = y.shape
    gran = cout // st.shape[1]
    t = st.double()
    tot_s, tot_q = t[..., 0] + t[..., 1] * 2.0 ** -44, t[..., 2] + t[..., 3] * 2.0 ** -44      # [B, C/g]
    yd = y.double().view(B, H * W, cout // gran, gran)
    want_s, want_q = yd.sum(dim=(1, 3)), (yd * yd).sum(dim=(1, 3))
    if finite_images is not None:
        marks = (st[..., 2] >> 62) & 1
        assert bool((marks[~finite_images] == 1).all()) and bool((marks[finite_images] == 0).all()), "poison marks of the totals"
        tot_s, tot_q, want_s, want_q = tot_s[finite_images], tot_q[finite_images], want_s[finite_images], want_q[finite_images]
    n = H * W * gran
    e_s = ((tot_s - want_s).abs() / (want_q * n).sqrt().clamp_min(1e-6)).max().item()          # |sum| <= sqrt(n * sumsq)
    e_q = ((tot_q - want_q).abs() / want_q.clamp_min(1e-6)).max().item()
    assert e_s <= 1e-4 and e_q <= 1e-4, f"ride-along totals off: sum {e_s:.3e}, sum of squares {e_q:.3e} (granule {gran})"


def _generic_conv(c, ops):
    """The convolution of the reference through the library's exact-f32 generic kernel (operands as rounded to the dtype)."""
    def conv(y64, w16, bias, emb, res, act):
        pw32 = ops.pack_conv(w16.float(), None if bias is None else bias.float(), torch.float32, torch.device(DEV))
        old = ops.CONV_POLICY
        ops.CONV_POLICY = "generic"
        try:
            r = ops.conv2d(y64.float().permute(0, 2, 3, 1).contiguous().to(DEV), pw32, res=None if res is None else res.float().to(DEV),
                           emb=None if emb is None else emb.float().to(DEV), act=1 if act else 0, emit_stats=False, use_bias=bias is not None)
        finally:
            ops.CONV_POLICY = old
        return r.double().cpu()
    return conv


def _stage(c, s, ops, lib, norm, x0, x1, pw, kw, film, o, log):
    """One then_conv launch of the block, every check of the module's docstring; returns the stored output (with its totals)."""
    from diffusion_nlc_amd import _ext
    dt = _dt(c)
    B, H, W, Cout = c["B"], c["H"], c["W"], c["Cout"]
    C0, C1 = x0.shape[-1], 0 if x1 is None else x1.shape[-1]
    silu = c[f"silu{s}"]
    scale, shift = film
    launch = lambda: norm.then_conv(x0, pw, silu=silu, x1=x1, scale=scale, shift=shift, **kw)
    asked = {k: v for k, v in kw.items() if k in ("emb", "use_bias")}

    # ---- queries: query_gn_in <=> the geometry rule <=> the launch with gn_in is accepted
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    geo = _geom(B, H, W, C0, C1, Cout, ncu)
    q = ops.conv2d(x0, pw, x1=x1, query_gn_in=True, **asked)
    assert q == (geo is not None), f"query_gn_in says {q}, the geometry rule {geo}"
    spec = ops.gn_in_spec(x0, norm.gamma, norm.beta, groups=norm.groups, eps=1e-5, silu=silu, x1=x1, scale=scale, shift=shift)
    fused = q and spec is not None
    y = launch()                                      # never raises: a shape the kernel rejects takes the separate pass
    st = ops.ride_stats(y)
    if spec is not None and not q:
        with pytest.raises(_ext.NlcError, match="cannot apply"):
            ops.conv2d(x0, pw, x1=x1, gn_in=spec, **kw)
    if fused:
        d, out, keep = ops.conv2d(x0, pw, x1=x1, gn_in=spec, desc_only=True, **kw)
        assert lib.nlc_conv2d_stats_partials(C.byref(d), ops.dtype_enum(dt)) > 0, "stats query (gn_in set) denies a small-map launch its totals"
        assert st is not None, "a small-map launch came back without ride-along totals"
        assert _same(ops.conv2d(x0, pw, x1=x1, gn_in=spec, **kw), y), "then_conv differs from the direct launch with gn_in"
    else:
        sep = ops.conv2d(norm(x0, silu=silu, x1=x1, scale=scale, shift=shift), pw, **kw)
        prologue = (ops.FUSE_GN_CONV or (ops.FUSE_GN_CONV_NT1 and Cout <= ops.FUSE_GN_CONV_MAXC)) and ops.conv2d(x0, pw, x1=x1, query_prologue=True)
        if not prologue:
            assert _same(sep, y), "a shape the small-map kernel rejects did not come back as the separate pass computes it"
    if geo is not None:                               # the same kernel without a normalisation (policy "small") carries totals as well
        old = ops.CONV_POLICY
        ops.CONV_POLICY = "small"
        try:
            d, out, keep = ops.conv2d(x0, pw, x1=x1, desc_only=True, **kw)
            assert lib.nlc_conv2d_stats_partials(C.byref(d), ops.dtype_enum(dt)) > 0, "stats query (policy small) denies a small-map launch its totals"
            plain = ops.conv2d(x0, pw, x1=x1, **kw)
        finally:
            ops.CONV_POLICY = old
        assert ops.ride_stats(plain) is not None
        _check_totals(plain.cpu(), ops.ride_stats(plain).cpu(), _finite_images(plain))

    # ---- bit identity: cold caches, a busy second stream, the other reduction, the other tile height's two reductions
    _buf("sweep", 64 << 20).fill_(s)
    y2 = launch()
    side = _side()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for rep in range(3):
            _buf("hog", 256 << 20).fill_(rep)
    y3 = launch()
    torch.cuda.current_stream().wait_stream(side)
    # (name, output, same schedule?)  The two reductions add the same f32 partial sums of the OUTPUT in the same order - stored values
    # bit-identical - but hand the totals different f32 partial sums of the stored values (per finished unit / per whole tile): those are
    # compared with the f64 sums like every other, not bit for bit
    variants = [("after a cache sweep", y2, True), ("beside a busy second stream", y3, True)]
    if fused:
        old_t = ops.CONV_TUNING
        try:
            ops.CONV_TUNING = 1 << 23
            variants.append(("with the last-arriver reduction (tuning bit 23)", launch(), False))
            ops.CONV_TUNING = 1 << 22
            if ops.conv2d(x0, pw, x1=x1, query_gn_in=True, **asked):
                t128 = launch()
                ops.CONV_TUNING = (1 << 22) | (1 << 23)
                t128_last = launch()
                assert _same(t128, t128_last), "128-pixel tiles: the last-arriver reduction differs from the distributed one"
                if geo["wm"] == 2:
                    variants.append(("with tuning bit 22, which changes nothing here", t128, True))
                    variants.append(("with tuning bits 22 and 23", t128_last, False))
                else:
                    log["t128"] = t128
                    for t in (t128, t128_last):
                        _check_totals(t.cpu(), ops.ride_stats(t).cpu(), _finite_images(t))
        finally:
            ops.CONV_TUNING = old_t
    old_d = ops.CONV_DEBUG
    ops.CONV_DEBUG = 1                                # refuses to launch unless every launch above left the arrival counters zero
    try:
        variants.append(("with the arrival counters checked (CONV_DEBUG = 1)", launch(), True))
    finally:
        ops.CONV_DEBUG = old_d
    for what, v, same_schedule in variants:
        assert _same(v, y), f"stage {s}: the launch {what} differs"
        if st is not None and same_schedule:
            assert _same(ops.ride_stats(v), st), f"stage {s}: ride-along totals of the launch {what} differ"
        elif st is not None:
            _check_totals(v.cpu(), ops.ride_stats(v).cpu(), _finite_images(v))

    # ---- reference and totals
    xs = torch.cat([x0.cpu()] + ([x1.cpu()] if x1 is not None else []), dim=-1)
    ref = _reference(c, s, xs.double(), o, conv=_generic_conv(c, ops) if c["generic"] else None)
    yc = y.cpu()
    nan_ref = torch.isnan(ref)
    assert _same(torch.isnan(yc), nan_ref), f"stage {s}: NaNs are not where F.group_norm puts them"
    ok = ~nan_ref
    scale_ = max(ref[ok].abs().max().item(), 1e-6)
    err = (yc.double()[ok] - ref[ok]).abs().max().item() / scale_
    errs = [err]
    if "t128" in log:
        errs.append((log.pop("t128").cpu().double()[ok] - ref[ok]).abs().max().item() / scale_)
    print(f"small-fuzz {log['id']} stage {s}: fused={int(fused)} geom={geo} err={max(errs):.3e} tol={TOL[c['dtype']]:.0e}")
    assert max(errs) <= TOL[c["dtype"]], f"stage {s}: max rel-to-scale error {max(errs):.3e} > {TOL[c['dtype']]:.0e} (scale {scale_:.3e}, fused {fused}, {geo})"
    if st is not None:
        _check_totals(yc, st.cpu(), _finite_images(y))
    log[f"y{s}"] = y
    return y


def _finite_images(y):
    f = torch.isfinite(y).flatten(1).all(dim=1).cpu()
    return None if bool(f.all()) else f


def _run_block(c, ident):
    from diffusion_nlc_amd import _ext, ops
    from tests.test_ops_gpu import _tol
    assert ops.CONV_POLICY == "auto" and ops.CONV_TUNING == 0 and ops.FUSE_GN_SMALL
    dt = _dt(c)
    assert TOL[c["dtype"]] == _tol(dt)
    lib = _ext.load()
    o = _operands(c)
    Cout, B = c["Cout"], c["B"]
    old_g = ops.STATS_GRANULE_4
    ops.STATS_GRANULE_4 = c["gran4"]
    try:
        x0 = _produce(c, ops, o["p0"], c["C0"])
        x1 = _produce(c, ops, o["p1"], c["C1"]) if c["C1"] else None
        o["x_stored"] = x0.cpu()
        dev = torch.device(DEV)
        pw1 = ops.pack_conv(o["w1"], o["b1"], dt, dev)
        pw2 = ops.pack_conv(o["w2"], o["b2"], dt, dev)
        ss, emb = o["ss"].to(DEV), o["emb"].to(DEV)
        log = dict(id=ident)
        kw1 = dict(act=1 if c["act1"] else 0, use_bias=c["bias"])
        if c["emb"]:
            kw1["emb"] = emb[:, :Cout]
        h = _stage(c, 1, ops, lib, _norm(o["gamma1"], o["beta1"], c["groups"]), x0, x1, pw1, kw1, (None, None), o, log)
        kw2 = dict(act=1 if c["act2"] else 0, use_bias=c["bias"])
        res = _res_of(c, 2, o)
        if res is not None:
            kw2["res"] = x0 if res is o["x_stored"] else res.to(DEV)
        film = (ss[:, :Cout], ss[:, Cout:2 * Cout]) if c["film"] else (None, None)
        _stage(c, 2, ops, lib, _norm(o["gamma2"], o["beta2"], c["groups2"]), h, None, pw2, kw2, film, o, log)
    finally:
        ops.STATS_GRANULE_4 = old_g
    return log


_IDS = [f"{i:03d}-{_case_id(c)}" for i, c in enumerate(_cases(N_CASES))]


@gpu
@pytest.mark.parametrize("i", range(N_CASES), ids=_IDS)
def test_small_map_resblock_fuzz(i):
    _run_block(_cases(N_CASES)[i], _IDS[i])


@gpu
@pytest.mark.parametrize("c", _edges(), ids=lambda c: c["id"])
def test_small_map_resblock_edge_values(c):
    """The fixed list of the module's docstring: zero variance, mean / std ~ 300, beta = 3 and shift = 2 (a padding pixel that was
    normalised instead of staying zero shows at the border), a group across the two sources, a NaN / an inf in one image."""
    log = _run_block(c, c["id"])
    if c["edge"] in ("nan", "inf"):
        clean = _run_block(dict(c, edge=None), c["id"] + "-clean")
        for s in (1, 2):
            bad, good = log[f"y{s}"], clean[f"y{s}"]
            assert bool(torch.isnan(bad[1]).all()), f"stage {s}: the image with the {c['edge']} is not NaN throughout"
            keep = [b for b in range(c["B"]) if b != 1]
            assert _same(bad[keep], good[keep]), f"stage {s}: an image beside the bad one changed"


@gpu
@pytest.mark.parametrize("view", ["offset-4-bytes", "odd-row-stride"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_then_conv_takes_the_separate_pass_for_an_embedding_view_the_small_kernel_cannot_read(dtype, view):
    """The small-map kernel reads embedding rows as 16-byte vectors; nlc_conv_small_geom rejects a launch whose emb pointer is not
    16-byte aligned or whose row stride is no multiple of 4 floats.  then_conv's query has to see that pointer: such a view must come
    back as the separate GroupNorm pass + convolution computes it, not abort with 'gn_in given but this launch cannot apply it'."""
    from diffusion_nlc_amd import ops
    c = dict(_EDEF, **_E2, dtype=dtype, edge=None)
    dt = _dt(c)
    o = _operands(c)
    Cout, B = c["Cout"], c["B"]
    x = _produce(c, ops, o["p0"], c["C0"])
    pw = ops.pack_conv(o["w1"], o["b1"], dt, torch.device(DEV))
    norm = _norm(o["gamma1"], o["beta1"], c["groups"])
    g = torch.Generator().manual_seed(3)
    if view == "offset-4-bytes":
        bank = torch.randn(B, Cout + 16, generator=g).to(DEV)
        emb = bank[:, 1:1 + Cout]
    else:
        bank = torch.randn(B, Cout + 5, generator=g).to(DEV)
        emb = bank[:, :Cout]
    assert emb.data_ptr() % 16 != 0 or emb.stride(0) % 4 != 0
    assert ops.conv2d(x, pw, query_gn_in=True) and not ops.conv2d(x, pw, query_gn_in=True, emb=emb)
    assert ops.gn_in_spec(x, norm.gamma, norm.beta, groups=norm.groups, eps=1e-5, silu=True) is not None
    got = norm.then_conv(x, pw, silu=True, emb=emb)
    sep = ops.conv2d(norm(x, silu=True), pw, emb=emb)
    assert _same(got, sep)
    aligned = norm.then_conv(x, pw, silu=True, emb=emb.contiguous())          # the same numbers where the kernel can read them: fused
    ref = _reference(dict(c, emb=True), 1, x.cpu().double(), dict(o, emb=emb.cpu()))
    for what, t in (("separate pass", got), ("fused", aligned)):
        err = (t.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
        assert err <= TOL[dtype], f"{what}: {err:.3e}"
