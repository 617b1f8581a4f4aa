"""CPU-side checks of the host logic: parameter specs vs the reference modules' state_dicts,
the C-ABI library's exports, and loud failure without a GPU."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from tests.util import load_specs, state_dicts

ROOT = Path(__file__).resolve().parent.parent


def build_product(tag):
    import argparse
    from diffusion_nlc_amd import script_util
    cfgs = load_specs()["_configs"]
    c = dict(cfgs[tag])
    if tag.startswith("adm"):
        return script_util.create_sigma_eps_model(**c)
    if tag.startswith("simple"):
        ns = argparse.Namespace
        cfg = ns(model=ns(**{k: c[k] for k in ("ch", "out_ch", "ch_mult", "num_res_blocks", "attn_resolutions", "dropout",
                                                 "in_channels", "resamp_with_conv", "feat_layer", "type", "sigma_block",
                                                 "sigma_dropout")}),
                 data=ns(image_size=c["image_size"]), diffusion=ns(num_diffusion_timesteps=c["num_diffusion_timesteps"]))
        return script_util.create_simple_sigma_eps_model(cfg)
    return script_util.create_edm_sigma_eps_model(**c)


@pytest.mark.parametrize("tag", ["adm_tiny", "adm_tiny_b", "adm_tiny_cc", "simple_tiny", "edm_tiny"])
def test_param_spec_matches_reference_state_dict(tag):
    """Key names, order, shapes and dtypes equal what the reference modules produced (tests/golden/specs.json)."""
    specs = load_specs()
    eps, sig, fshape = build_product(tag)
    assert list(fshape) == specs[tag]["feat_shape"]
    for mod, ref in ((eps, specs[tag]["eps"]), (sig, specs[tag]["sigma"])):
        got = {k: [list(s), str(d).replace("torch.", "")] for k, (s, d) in mod.param_spec().items()}
        assert list(got.keys()) == list(ref.keys())
        assert got == ref
    e, s = state_dicts(tag)
    eps.load_state_dict(e)
    sig.load_state_dict(s)
    with pytest.raises(RuntimeError):
        eps.load_state_dict({k: v for k, v in list(e.items())[:-1]})


def test_library_exports_every_declared_symbol():
    from diffusion_nlc_amd import _ext
    header = (ROOT / "include" / "nlc_hip.h").read_text()
    declared = set(re.findall(r"\b(nlc_[A-Za-z0-9_]+)\s*\(", header))
    declared -= {"nlc_conv_desc", "nlc_sched_desc"}
    lib = _ext.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"libnlc_hip.so does not export {name}"
        assert name in _ext.SIGNATURES, f"{name} is declared in nlc_hip.h but not bound in _ext.py"
    assert set(_ext.SIGNATURES) <= declared
    assert lib.nlc_version() == _ext.ABI_VERSION
    a, b = _ext.pack_dims(_ext.NLC_BF16)
    assert a % 16 == 0 and b % 8 == 0


def test_argument_validation_without_gpu():
    """Bad descriptors are rejected on the host before any launch."""
    from diffusion_nlc_amd import _ext
    lib = _ext.load()
    d = _ext.ConvDesc()
    assert lib.nlc_conv2d(ctypes.byref(d), 7, None) == -1
    assert b"dtype" in lib.nlc_last_error()
    assert lib.nlc_attention(None, None, 1, 1, 1, 64, 0, 0, None) == -1
    assert lib.nlc_conv_first(None, None, None, None, None, 1, 3, 8, 8, 16, 3, 3, 0, None, 0, 5, None) == -1        # stats_granule 5
    assert b"granule" in lib.nlc_last_error()
    d2 = _ext.ConvDesc(math=1)
    assert lib.nlc_conv2d(ctypes.byref(d2), _ext.NLC_BF16, None) == -1 and b"math" in lib.nlc_last_error()        # F16X3 is a mode of f32 tensors
    assert lib.nlc_groupnorm(None, None, 8, 0, 1, 1, 3, 1e-5, None, None, None, None, 0, 0, None, None, 0, None) == -1


QUERIES = ("workspace_bytes", "stats_partials", "prologue_supported", "norm_out_supported", "gn_in_supported")
_HOST_MEM = ctypes.create_string_buffer(64)          # what the descriptors of the query tests point at: the host queries only look at
_HOST_PTR = (ctypes.addressof(_HOST_MEM) + 15) & ~15     # presence and alignment of a pointer, never through it
_HOST_GN_IN = None


def conv_query_desc(B, H, W, C0, Cout, k=3, *, C1=0, stride=1, dtype="bf16", policy="auto", tuning=0, gn_in=False, bias=True, nchw=False,
                    ups=False):
    """(ConvDesc, dtype enum) of a 'same'-padded convolution as ops.conv2d would describe it, for the host queries (no GPU, no tensors)."""
    from diffusion_nlc_amd import _ext, ops
    global _HOST_GN_IN
    kbe = 32 if dtype == "f32" else 64
    pad = k // 2
    HL, WL = (2 * H, 2 * W) if ups else (H, W)
    d = _ext.ConvDesc(x0=_HOST_PTR, x1=_HOST_PTR if C1 else None, C0=C0, C1=C1, B=B, Hin=H, Win=W, Hout=(HL + 2 * pad - k) // stride + 1,
                      Wout=(WL + 2 * pad - k) // stride + 1, Cout=Cout, KH=k, KW=k, stride=stride, pad_t=pad, pad_l=pad, upsample2x=int(ups),
                      w=_HOST_PTR, Cin_pad=-(-(C0 + C1) // kbe) * kbe, Cout_pad=-(-Cout // 128) * 128, bias=_HOST_PTR if bias else None,
                      out_scale=1.0, out=_HOST_PTR, out_mode=ops.OUT_NCHW_F32 if nchw else ops.OUT_NHWC, policy=ops.CONV_POLICIES[policy],
                      tuning=tuning)
    if gn_in:
        if _HOST_GN_IN is None:
            _HOST_GN_IN = _ext.GnIn(stats0=_HOST_PTR, groups=1)
        d.gn_in = ctypes.pointer(_HOST_GN_IN)
    return d, {"f32": _ext.NLC_F32, "bf16": _ext.NLC_BF16, "f16": _ext.NLC_F16}[dtype]


def conv_queries(lib, d, dt):
    return {q: int(getattr(lib, "nlc_conv2d_" + q)(ctypes.byref(d), dt)) for q in QUERIES}


# (B, H, W, C0, Cout, k) + options: the levels of the three networks and the shapes around every threshold of the dispatch
# (64 narrow patches, 128 halo tiles, split-K below 256, 768 pointwise tiles, the small-map geometries)
QUERY_SHAPES = [
    (2, 8, 8, 64, 128, 3), (2, 8, 8, 128, 128, 3), (16, 8, 8, 1024, 1024, 3), (8, 16, 16, 512, 512, 3), (8, 32, 32, 256, 256, 3),
    (200, 8, 8, 256, 256, 3), (16, 8, 8, 1024, 1024, 3, dict(C1=512)), (3, 8, 8, 192, 128, 3), (1, 8, 8, 64, 128, 3),
    (1, 16, 16, 64, 128, 3), (2, 64, 64, 1024, 128, 3), (16, 16, 16, 1024, 1024, 3), (16, 16, 16, 1024, 512, 3), (16, 32, 32, 512, 512, 3),
    (1, 128, 128, 64, 128, 3), (1, 256, 256, 128, 256, 3), (2, 64, 64, 256, 256, 3, dict(ups=True)), (2, 16, 16, 64, 200, 3),
    (4, 64, 64, 64, 6, 3), (3, 64, 64, 64, 6, 3), (16, 256, 256, 256, 6, 3), (1, 32, 32, 128, 3, 3), (4, 64, 64, 64, 16, 3, dict(nchw=True)),
    (12, 64, 64, 64, 256, 1), (11, 64, 64, 64, 256, 1), (16, 128, 128, 256, 256, 1), (16, 64, 64, 512, 256, 1, dict(C1=256)),
    (16, 8, 8, 1024, 3072, 1), (2, 4, 4, 1024, 256, 1), (200, 16, 16, 256, 512, 1),
    (2, 16, 16, 64, 64, 3, dict(stride=2)), (1, 8, 8, 128, 128, 3, dict(stride=2)), (16, 64, 64, 256, 256, 3, dict(stride=2)),
    (1, 8, 8, 64, 16, 5), (2, 16, 16, 64, 128, 5), (2, 9, 7, 32, 6, 3), (2, 8, 8, 96, 200, 3, dict(bias=False)),
]


def _query_cases():
    for s in QUERY_SHAPES:
        kw = dict(s[6]) if len(s) > 6 else {}
        for dtype in ("bf16", "f16", "f32"):
            yield s[:6], dict(kw, dtype=dtype)


def test_conv_queries_are_views_of_one_plan():
    """nlc_conv2d's dispatch is planned once (conv_igemm.hip: plan_conv) and the five host queries return fields of that plan.  What
    follows from that, over the networks' levels and the shapes around every threshold, in all three dtypes - on the host (the
    library answers the queries without a GPU):
      * policy "generic": every query 0;
      * where gn_in is supported, asking with gn_in set or under policy "small" plans the small-map kernel: statistics iff
        Cout % 128 == 0, the same workspace either way (the small-map kernel's: a function of its k-slices alone), and the prologue
        query - which never looks at the attachments - unchanged;
      * norm_out supported => no workspace (the pointwise kernel never splits K);
      * a <= 16-channel 3x3 that the narrow kernel takes (policy "auto", >= 64 patches) has neither statistics nor a workspace;
      * tuning bit 11 (no split-K in the halo and fast kernels) => no workspace, for every launch that is not a small-map one (whose
        k-slices are part of its geometry, not a policy)."""
    from diffusion_nlc_amd import _ext
    lib = _ext.load()
    seen = {q: set() for q in QUERIES}
    for shape, kw in _query_cases():
        B, H, W, C0, Cout, k = shape
        base = conv_queries(lib, *conv_query_desc(*shape, **kw))
        for q in QUERIES:
            seen[q].add(base[q] > 0)
        for policy in ("auto", "halo", "no_halo", "small"):
            got = conv_queries(lib, *conv_query_desc(*shape, policy=policy, **kw))
            assert got["stats_partials"] in (0, 1) and got["workspace_bytes"] >= 0
            if got["stats_partials"]:
                assert kw["dtype"] != "f32" and Cout % 128 == 0 and not kw.get("nchw"), (shape, kw, policy)
            if got["norm_out_supported"]:
                assert got["workspace_bytes"] == 0, (shape, kw, policy)
        assert not any(conv_queries(lib, *conv_query_desc(*shape, policy="generic", **kw)).values()), (shape, kw)
        assert not any(conv_queries(lib, *conv_query_desc(*shape, policy="generic", gn_in=True, **kw)).values()), (shape, kw)
        if base["gn_in_supported"]:
            with_gn = conv_queries(lib, *conv_query_desc(*shape, gn_in=True, **kw))
            as_small = conv_queries(lib, *conv_query_desc(*shape, policy="small", **kw))
            for got in (with_gn, as_small):
                assert got["gn_in_supported"] == 1
                assert got["stats_partials"] == (1 if Cout % 128 == 0 else 0), (shape, kw)
                assert got["prologue_supported"] == base["prologue_supported"], (shape, kw)
            assert with_gn["workspace_bytes"] == as_small["workspace_bytes"], (shape, kw)
            slices = (with_gn["workspace_bytes"] - 4096) // (B * H * W * Cout * 4) if with_gn["workspace_bytes"] else 1
            assert 1 <= slices <= 8 and with_gn["workspace_bytes"] == (slices * B * H * W * Cout * 4 + 4096 if slices > 1 else 0), (shape, kw)
            assert conv_queries(lib, *conv_query_desc(*shape, gn_in=True, tuning=1 << 21, **kw))["gn_in_supported"] == 0
        else:
            assert conv_queries(lib, *conv_query_desc(*shape, gn_in=True, **kw))["gn_in_supported"] == 0
        if k == 3 and Cout <= 16 and kw["dtype"] != "f32" and kw.get("stride", 1) == 1 and H % 16 == 0 and W % 16 == 0 and B * (H // 16) * (W // 16) >= 64:
            assert base["stats_partials"] == 0 and base["workspace_bytes"] == 0 and base["prologue_supported"] == 0, (shape, kw)
        for policy in ("auto", "halo", "no_halo"):
            assert conv_queries(lib, *conv_query_desc(*shape, policy=policy, tuning=1 << 11, **kw))["workspace_bytes"] == 0, (shape, kw, policy)
    for q in QUERIES:          # the shapes reach both answers of every query
        assert seen[q] == {False, True}, q


def _totals_rule(C0, C1, groups, g0, g1):
    """nlc_groupnorm_totals_supported restated: granules 0 (= 8), 4 or 8; C0, C1 multiples of 8; groups divides C0 + C1; the group size a
    multiple of each source's granule."""
    if g0 not in (0, 4, 8) or g1 not in (0, 4, 8) or C0 % 8 or C1 % 8 or (C0 + C1) % groups:
        return 0
    gs = (C0 + C1) // groups
    return int(gs % (g0 or 8) == 0 and (C1 == 0 or gs % (g1 or 8) == 0))


def test_groupnorm_totals_supported_is_the_rule():
    from diffusion_nlc_amd import _ext
    lib = _ext.load()
    n = 0
    for C0 in (8, 24, 64, 96, 128, 132):
        for C1 in (0, 8, 64, 100):
            for groups in (1, 3, 8, 32):
                for g0 in (0, 4, 8, 5):
                    for g1 in (0, 4, 8, 5):
                        assert lib.nlc_groupnorm_totals_supported(C0, C1, groups, g0, g1) == _totals_rule(C0, C1, groups, g0, g1), (C0, C1, groups, g0, g1)
                        n += 1
    assert n == 1536
    # what the networks produce: 128 channels / 32 groups at granule 4, 256 / 32 at granule 8, a 64 + 64 concatenation at mixed granules
    # (16-channel groups: at 32 groups its 4-channel groups are no multiple of the second source's granule 8)
    for args in ((128, 0, 32, 4, 0), (256, 0, 32, 8, 0), (256, 0, 32, 0, 0), (64, 64, 8, 4, 8), (64, 64, 8, 8, 4), (128, 128, 32, 4, 4), (128, 256, 8, 4, 8)):
        assert lib.nlc_groupnorm_totals_supported(*args) == 1, args
    for args in ((64, 64, 32, 4, 8), (128, 256, 32, 4, 8), (96, 0, 32, 4, 0)):      # 4-, 12- and 3-channel groups against 8- / 4-channel chunks
        assert lib.nlc_groupnorm_totals_supported(*args) == 0, args
    assert lib.nlc_groupnorm_totals_supported(0, 0, 32, 8, 8) == 0 and lib.nlc_groupnorm_totals_supported(64, 0, 0, 8, 8) == 0


def _cpu_with_totals(C, gran, dtype=torch.bfloat16):
    """A CPU activation [2, 4, 4, C] with hand-attached (zero) ride-along totals of `gran` channels per chunk."""
    t = torch.zeros(2, 4, 4, C, dtype=dtype)
    t._nlc_stats = torch.zeros(2, C // gran, 4, dtype=torch.int64)
    return t


def test_ride_totals_decides_on_the_host(monkeypatch):
    """ops._ride_totals needs no GPU to decide, and decides what the library's query answers."""
    from diffusion_nlc_amd import _ext, ops
    lib = _ext.load()
    seen = set()
    for C0, g0 in ((128, 4), (128, 8), (256, 8), (64, 4), (96, 8)):
        for C1, g1 in ((0, 0), (64, 4), (64, 8), (256, 8)):
            for groups in (1, 8, 32):
                x0 = _cpu_with_totals(C0, g0)
                x1 = _cpu_with_totals(C1, g1) if C1 else None
                got = ops._ride_totals(x0, x1, groups)
                assert (got is not None) == bool(lib.nlc_groupnorm_totals_supported(C0, C1, groups, g0, g1)), (C0, g0, C1, g1, groups)
                seen.add(got is not None)
                if got is not None:
                    assert got[0] is x0._nlc_stats and got[1] == g0 and got[3] == g1 and (got[2] is x1._nlc_stats if C1 else got[2] is None)
    assert seen == {False, True}
    x0, x1 = _cpu_with_totals(128, 4), _cpu_with_totals(128, 4)
    assert ops._ride_totals(x0, x1, 32) is not None
    assert ops._ride_totals(_cpu_with_totals(128, 4, torch.float32), None, 32) is None                    # f32: totals are a 16-bit matter
    assert ops._ride_totals(x0, torch.zeros(2, 4, 4, 128, dtype=torch.bfloat16), 32) is None               # a source without totals
    assert ops._ride_totals(torch.zeros(2, 4, 4, 128, dtype=torch.bfloat16), None, 32) is None
    monkeypatch.setattr(ops, "FUSED_GN_STATS", False)
    assert ops._ride_totals(x0, x1, 32) is None


def _first_small_map_desc(lib, **gn):
    """A bf16 descriptor that the small-map kernel takes with gn_in attached and without a workspace (so that nothing but gn_in's own
    validation stands between nlc_conv2d and the launch), with the given nlc_gn_in fields."""
    from diffusion_nlc_amd import _ext
    d, dt = conv_query_desc(2, 8, 8, 64, 128, 3, gn_in=True)
    q = conv_queries(lib, d, dt)
    assert q["gn_in_supported"] == 1 and q["workspace_bytes"] == 0
    spec = _ext.GnIn(**gn)
    d.gn_in = ctypes.pointer(spec)
    return d, dt, spec


def test_totals_consumers_reject_what_the_rule_rejects():
    """The four consumers of ride-along totals validate through one function: each rejects a granule of 5, a group size that is no multiple
    of the granule and stats1 without C1 on the host (NLC_EINVAL, nothing launched - the pointers are host memory), under its own name."""
    from diffusion_nlc_amd import _ext
    lib = _ext.load()
    P, bf16 = _HOST_PTR, _ext.NLC_BF16
    # (C0, C1, groups, stats1, granule0, granule1, word of the message)
    bad = [(128, 0, 32, None, 5, 0, b"chunks of (5, 0)"),                   # granule 5
           (128, 0, 32, None, 8, 0, b"group size 4), chunks of (8, 0)"),    # 4-channel groups, 8-channel chunks
           (128, 0, 16, P, 4, 4, b"stats1")]                # stats1 without C1
    for C0, C1, groups, s1, g0, g1, word in bad:
        assert _totals_rule(C0, C1, groups, g0, g1) == 0 or s1 is not None
        rc = lib.nlc_groupnorm_prestats(P, None, C0, C1, 2, 64, groups, 1e-5, None, None, None, None, 0, 0, P, bf16, P, g0, s1, g1, None)
        err = lib.nlc_last_error()
        assert rc == -1 and b"nlc_groupnorm_prestats" in err and word in err and (s1 is not None or b"granule" in err), err
        rc = lib.nlc_groupnorm_coef(C0, C1, 2, 64, groups, 1e-5, None, None, None, None, 0, P, g0, s1, g1, P, None)
        err = lib.nlc_last_error()
        assert rc == -1 and b"nlc_groupnorm_coef" in err and word in err, err
        if s1 is None:                                      # (one source only)
            rc = lib.nlc_groupnorm_pool2x2(P, C0, 2, 8, 8, groups, 1e-5, None, None, None, None, 0, 0, P, P, P, bf16, P, g0, None)
            err = lib.nlc_last_error()
            assert rc == -1 and b"nlc_groupnorm_pool2x2" in err and word in err, err
    for gn, word in ((dict(stats0=P, granule0=5, groups=16), b"chunks of (5, 0)"), (dict(stats0=P, granule0=8, groups=16), b"group size 4), chunks of (8, 0)"),
                     (dict(stats0=P, stats1=P, granule0=4, granule1=4, groups=8), b"stats1")):
        d, dt, _keep = _first_small_map_desc(lib, **gn)
        rc = lib.nlc_conv2d(ctypes.byref(d), dt, None)
        err = lib.nlc_last_error()
        assert rc == -1 and b"nlc_conv2d" in err and b"gn_in" in err and word in err, err
    # the FiLM half is one check too, shared with plain nlc_groupnorm: scale without shift, rows narrower than C
    assert lib.nlc_groupnorm(P, None, 128, 0, 2, 64, 32, 1e-5, None, None, P, None, 128, 0, P, P, bf16, None) == -1
    assert b"nlc_groupnorm:" in lib.nlc_last_error() and b"together" in lib.nlc_last_error()
    assert lib.nlc_groupnorm_prestats(P, None, 128, 0, 2, 64, 32, 1e-5, None, None, P, P, 64, 0, P, bf16, P, 4, None, 0, None) == -1
    assert b"nlc_groupnorm_prestats" in lib.nlc_last_error() and b"ss_stride" in lib.nlc_last_error()


def test_film_stride_is_strict_for_every_groupnorm_shim():
    """ops._film_stride: f32, rank 2, unit inner stride, at least C wide, one row stride, both or neither - and gn_in_spec / groupnorm_coef
    reject a malformed pair with the same ValueError instead of handing it to the library."""
    from diffusion_nlc_amd import ops
    C = 128
    row = torch.zeros(2, 2 * C + 8)
    good = (row[:, :C], row[:, C:2 * C])
    malformed = [
        ((good[0].half(), good[1]), "float32"),                          # f16 scale
        ((row[:, :C - 8], good[1]), "view with unit inner stride"),       # narrower than C
        ((good[0], torch.zeros(2, C)), "share a row stride"),             # two row strides
        ((good[0], None), "come together"),                               # scale without shift
        ((None, good[1]), "come together"),
        ((row[:, ::2][:, :C], good[1]), "view with unit inner stride"),   # inner stride 2
    ]
    assert ops._film_stride(None, None, C, "t") == 0
    x0 = _cpu_with_totals(C, 4)
    assert ops._ride_totals(x0, None, 32) is not None
    for (scale, shift), msg in malformed:
        with pytest.raises(ValueError, match="t: .*" + msg):
            ops._film_stride(scale, shift, C, "t")
        with pytest.raises(ValueError, match="gn_in_spec: .*" + msg):
            ops.gn_in_spec(x0, None, None, groups=32, eps=1e-5, silu=True, scale=scale, shift=shift)
        with pytest.raises(ValueError, match="groupnorm_coef: .*" + msg):
            ops.groupnorm_coef(x0, None, None, groups=32, eps=1e-5, scale=scale, shift=shift)
    with pytest.raises(ValueError, match="GPU"):                         # a well-formed pair must still be device memory
        ops._film_stride(*good, C, "t")


def test_no_cpu_fallback():
    from diffusion_nlc_amd._ext import NlcError
    eps, sig, _ = build_product("adm_tiny_b")
    with pytest.raises(NlcError):
        eps(torch.zeros(1, 3, 32, 32), torch.zeros(1))
    with pytest.raises(NlcError):
        sig(torch.zeros(1, 64, 8, 8))


def test_continuous_t_and_redesigned_schedules_match_reference():
    """Host-side schedule construction for SURVEY §8 f-2 (continuous t by Interp1d; the sigma-redesign tail)."""
    import json
    import numpy as np
    from diffusion_nlc_amd.schedulers import get_sampler, redesign_sigma
    from tests.util import load_npz
    g = load_npz("cont_linear")
    s = get_sampler("ddim", 1000, 10, sigma_style="Linear", start_sigma=100, end_sigma=0.01, sampler_var="fixedsmall", eta=0.0,
                    continuous_t=True)
    assert s.continuous_t and s.timesteps.dtype == g["timesteps"].dtype
    assert torch.equal(s.timesteps, g["timesteps"]) and torch.equal(s.sampling_sigmas, g["sampling_sigmas"])
    assert s.device_t_slopes("cpu").shape == (999,)
    g = load_npz("proj_redesign")
    c = g["cfg"]
    s = get_sampler("ddim", 1000, c["num_timesteps"], sigma_style="DDIM", start_sigma=100, end_sigma=0, sampler_var="fixedsmall", eta=0.0)
    assert s.device_t_slopes("cpu") is None
    redesign_sigma(s, c["num_timesteps"], c["max_T"], c["cycle_size"], c["min_sigma"], c["max_sigma"], c["sigma_gamma"])
    assert s.continuous_t and s.sampling_sigmas.dtype == g["sampling_sigmas"].dtype == torch.float64
    assert torch.equal(s.sampling_sigmas, g["sampling_sigmas"])
    assert torch.equal(s.timesteps, g["timesteps"])


def test_multiply_shift_division_constants_are_exact():
    """conv_params.h: FastDiv (host side fills mul / shr per launch, the kernels compute q = mulhi(n, mul) >> shr).  Restated here:
    l = ceil(log2 d), mul = ceil(2^(31 + l) / d) < 2^32, q = (n * mul >> 32) >> (l - 1) must equal n // d for every 31-bit n
    (Granlund-Montgomery, N = 31); d = 1 is the kernels' special case."""
    import random
    rnd = random.Random(7)
    ds = list(range(2, 300)) + [2 ** k for k in range(1, 31)] + [2 ** k + 1 for k in range(1, 30)] + [2 ** k - 1 for k in range(2, 31)] + \
         [rnd.randrange(2, 2 ** 31) for _ in range(500)] + [65536 * 16, 256 * 256, 1023, 1025]
    for d in ds:
        l = (d - 1).bit_length()
        mul = ((1 << (31 + l)) + d - 1) // d
        assert mul < (1 << 32), d
        shr = l - 1
        ns = [0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, (1 << 31) - 1, (1 << 31) - d, ((1 << 31) - 1) // d * d, ((1 << 31) - 1) // d * d - 1] + \
             [rnd.randrange(0, 1 << 31) for _ in range(64)]
        for n in ns:
            if 0 <= n < (1 << 31):
                assert ((n * mul) >> 32) >> shr == n // d, (n, d)


# ---- command lines of the two entry points vs the reference's own parsers (tests/golden/cli_flags.json) -------------------
# The ONLY tolerated difference: the default of --device.  The reference hard-codes its authors' card index (cuda:1 / cuda:5,
# image_sample.py:80, edm_image_sample.py:36), which does not exist on a one-GPU box; both entry points default to cuda:0.
CLI_DEFAULT_WAIVERS = {"--device"}


def _cli_flags(parser):
    return {a.option_strings[0]: dict(default=a.default, type=getattr(a.type, "__name__", None),
                                      choices=list(a.choices) if a.choices is not None else None)
            for a in parser._actions if a.option_strings and a.dest != "help"}


@pytest.mark.parametrize("cli", ["image_sample", "edm_image_sample"])
def test_cli_flags_match_reference(cli):
    """Every flag of the reference's parser exists here with the same default, type and choices; flags that exist only here are
    the documented extensions."""
    import importlib
    import json
    import math
    ref = json.loads((ROOT / "tests" / "golden" / "cli_flags.json").read_text())[cli]
    mod = importlib.import_module(cli)
    got = _cli_flags(mod.build_parser())
    missing = sorted(set(ref) - set(got))
    assert not missing, f"{cli}.py lacks reference flags {missing}"
    for flag, r in ref.items():
        g = got[flag]
        assert g["type"] == r["type"], (flag, g, r)
        assert g["choices"] == r["choices"], (flag, g, r)
        if flag in CLI_DEFAULT_WAIVERS:
            continue
        assert g["default"] == r["default"] and type(g["default"]) is type(r["default"]), (flag, g, r)
    extensions = {"image_sample": {"--synthetic", "--return_log", "--save_png", "--precision"},
                  "edm_image_sample": {"--synthetic", "--dtype", "--rho", "--S_churn", "--S_min", "--S_max", "--S_noise", "--save_png"}}[cli]
    assert set(got) - set(ref) == extensions
    for flag in extensions:                      # an extension left at its default must not change the reference's behaviour
        d = got[flag]["default"]
        assert d in (None, "", 0, 1, 7, "f32") or (isinstance(d, float) and math.isinf(d)), (flag, d)


@pytest.mark.parametrize("cfg", ["cifar10", "ffhq"])
def test_edm_get_args_matches_reference(cfg, tmp_path, monkeypatch):
    """edm_image_sample.get_args() on the reference's own invocation line, in a scratch tree with the two files it reads, returns
    the namespace the reference's get_args() returned (recorded by make_golden.py): derived paths, the values taken from the
    training run's args.json, get_default's per-config norm bounds (ffhq: norm_max 102.0 + its checkpoint / FID paths)."""
    import json
    import edm_image_sample
    fx = json.loads((ROOT / "tests" / "golden" / "cli_flags.json").read_text())["edm_get_args"]
    (tmp_path / "results" / cfg / "6").mkdir(parents=True)
    (tmp_path / "store" / "config").mkdir(parents=True)
    (tmp_path / "results" / cfg / "6" / "args.json").write_text(json.dumps(fx["saved_args_json"]))
    (tmp_path / "store" / "config" / f"{cfg}.yml").write_text("model:\n  img_resolution: 32\ndata:\n  channels: 3\n  image_size: 32\n")
    monkeypatch.chdir(tmp_path)
    args, config = edm_image_sample.get_args(["--config", cfg] + fx["argv"])
    want = fx["result"][cfg]
    got = vars(args)
    for k, v in want["args"].items():
        if k == "device":
            continue
        assert k in got and got[k] == v and type(got[k]) is type(v), (k, got.get(k), v)
    assert vars(config.model) == want["model"]
    assert (config.data.channels, config.data.image_size) == (3, 32)


def test_product_schedule_tables_match_reference():
    """diffusion_nlc_amd.schedulers (host tables, what every GPU loop consumes) bit for bit against the reference's tables
    (tests/golden/sched.npz): the three DDIM ladders of the BASELINE configs, the other beta schedules, set_alpha_to_one = False,
    the sigma -> t lookup grid; and the "EDM" / "Scaled" / "Linear" ladders (no reference fixture) against the oracle's restatement
    of src/schedulers.py:227-284, which the same fixture file pins."""
    from diffusion_nlc_amd.schedulers import get_sampler
    from oracle.sched import get_sampler as oracle_sampler
    from tests.util import load_npz
    g = load_npz("sched")
    for steps in (10, 50, 100):
        s = get_sampler("ddim", 1000, steps, sigma_style="DDIM", start_sigma=100, end_sigma=0, sampler_var="fixedsmall")
        assert torch.equal(s.timesteps, g[f"timesteps_{steps}"]) and torch.equal(s.sampling_sigmas, g[f"sampling_sigmas_{steps}"])
        assert torch.equal(torch.as_tensor(s.min_var_coef), torch.as_tensor(g[f"min_var_coef_{steps}"]))
    assert torch.equal(s.sigmas, g["sigmas"]) and torch.equal(s.alphas_cumprod, g["alphas_cumprod"])
    assert torch.equal(s.get_t_from_sigma(g["t_grid_sigma"]), g["t_grid_t"])
    for sched in ("quadratic", "cosine", "sigmoid"):
        s2 = get_sampler("ddim", 1000, 20, beta_schedule=sched, sigma_style="DDIM", start_sigma=0, end_sigma=0)
        assert torch.equal(s2.sigmas, g[f"sigmas_{sched}"]) and torch.equal(s2.timesteps, g[f"timesteps_{sched}"])
    s3 = get_sampler("ddim", 1000, 10, sigma_style="DDIM", start_sigma=100, end_sigma=0, set_alpha_to_one=False)
    assert torch.equal(s3.timesteps, g["timesteps_noalpha1"]) and torch.equal(s3.sampling_sigmas, g["sampling_sigmas_noalpha1"])
    for style, kw in (("EDM", {}), ("Scaled", dict(linear_scale=0.9)), ("Linear", {}), ("Scaled", dict(linear_scale=1.1, continuous_t=True)),
                      ("EDM", dict(continuous_t=True))):
        a = get_sampler("ddim", 1000, 12, sigma_style=style, start_sigma=80, end_sigma=0.02, sampler_var="fixedsmall", **kw)
        b = oracle_sampler("ddim", 1000, 12, sigma_style=style, start_sigma=80, end_sigma=0.02, sampler_var="fixedsmall", **kw)
        assert a.timesteps.dtype == b.timesteps.dtype and torch.equal(a.timesteps, b.timesteps), (style, kw)
        assert a.sampling_sigmas.dtype == b.sampling_sigmas.dtype and torch.equal(a.sampling_sigmas, b.sampling_sigmas), (style, kw)
        assert torch.equal(torch.as_tensor(a.min_var_coef), torch.as_tensor(b.min_var_coef)), (style, kw)
    with pytest.raises(ValueError):
        get_sampler("ddim", 1000, 12, sigma_style="Cosine", start_sigma=80, end_sigma=0.02)


# ---- NVIDIA EDM network pickles (torch_utils.persistence format) ------------------------------------------------------------------
def write_nvidia_format_pickle(path, state_dict):
    """A pickle in the FORMAT of NVIDIA's EDM checkpoints (/root/reference/torch_utils/persistence.py:123-131,185-208): every module
    is reduced to ``torch_utils.persistence._reconstruct_persistent_obj(dict(type='class', version=6, module_src=..., class_name=...,
    state=<the module's __dict__>))``.  Built from a state_dict: a tree of stand-in modules (EDMPrecond.model = the network; the
    network's ``enc`` / ``dec`` are real ``torch.nn.ModuleDict``s as upstream) whose leaves hold the tensors as parameters - or, for
    ``resample_filter``, as buffers.  ``module_src`` is a dummy string: nothing of the reference's source is written."""
    import pickle
    import sys
    import types
    import torch

    fake = types.ModuleType("torch_utils.persistence")

    def _reconstruct_persistent_obj(meta):                       # never called here: pickle stores it by qualified name
        raise RuntimeError("the stock hook would execute module_src")
    _reconstruct_persistent_obj.__module__ = "torch_utils.persistence"
    _reconstruct_persistent_obj.__qualname__ = "_reconstruct_persistent_obj"
    fake._reconstruct_persistent_obj = _reconstruct_persistent_obj
    pkg = types.ModuleType("torch_utils")
    pkg.persistence = fake

    class Node(torch.nn.Module):
        def __reduce__(self):
            meta = dict(type="class", version=6, module_src="# (source text elided)", class_name=type(self).__name__, state=dict(self.__dict__))
            return (_reconstruct_persistent_obj, (meta,), None)

    def build(prefix_items):
        node = Node()
        children = {}
        for key, t in prefix_items:
            head, _, rest = key.partition(".")
            if not rest:
                if key.endswith("resample_filter"):
                    node.register_buffer(key, t.clone())
                else:
                    node.register_parameter(key, torch.nn.Parameter(t.clone(), requires_grad=False))
            else:
                children.setdefault(head, []).append((rest, t))
        for head, items in children.items():
            if head in ("enc", "dec"):                          # upstream: torch.nn.ModuleDict of persistent blocks
                md = torch.nn.ModuleDict()
                blocks = {}
                for rest, t in items:
                    bname, _, brest = rest.partition(".")
                    blocks.setdefault(bname, []).append((brest, t))
                for bname, bitems in blocks.items():
                    md[bname] = build(bitems)
                node.add_module(head, md)
            else:
                node.add_module(head, build(items))
        return node

    precond = Node()
    precond.add_module("model", build(list(state_dict.items())))
    precond.sigma_data = 0.5
    old = {k: sys.modules.get(k) for k in ("torch_utils", "torch_utils.persistence")}
    sys.modules["torch_utils"], sys.modules["torch_utils.persistence"] = pkg, fake
    try:
        with open(path, "wb") as f:
            pickle.dump(dict(ema=precond, loss_fn=None, augment_pipe=None, dataset_kwargs=dict(resolution=32)), f)
    finally:
        for k, v in old.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_edm_pickle_reader_needs_no_dnnlib_and_executes_nothing(tmp_path):
    """diffusion_nlc_amd.edm_pickle: the state_dict of an NVIDIA-format network pickle, read with torch_utils / dnnlib absent, equals the
    tensors that went in, under the reference's key names; a pickle that references any other global is refused."""
    import pickle
    import sys
    import torch
    from diffusion_nlc_amd.edm_pickle import load_edm_pickle
    from diffusion_nlc_amd.filler import fill_state_dict
    from tests.util import load_specs, template_from_spec
    sd = fill_state_dict(template_from_spec(load_specs()["edm_tiny"]["eps"]), seed=3)
    write_nvidia_format_pickle(tmp_path / "net.pkl", sd)
    assert "torch_utils" not in sys.modules and "dnnlib" not in sys.modules
    got = load_edm_pickle(tmp_path / "net.pkl")
    assert list(got) == list(sd) or set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    # a pickle whose reduce would RUN something foreign (here: create a file) loads as inert stand-ins - nothing runs
    import subprocess

    class Evil:
        def __reduce__(self):
            return (subprocess.check_call, (["touch", str(tmp_path / "pwned")],))
    evil = tmp_path / "evil.pkl"
    with open(evil, "wb") as f:
        pickle.dump(dict(ema=Evil()), f)
    assert load_edm_pickle(evil, submodule="") == {}
    assert not (tmp_path / "pwned").exists()


def test_inline_asm_loads_are_never_touched_in_flight(tmp_path):
    """tools/asm_load_audit.py over the compiled gfx950 code of every kernel source that loads into registers from inline asm (the
    sc1 read-backs of the split-K hand-offs): between such a load and a wait that covers it no instruction may read or write its
    destination registers - the register allocator does not know that an asm output is still in flight and has put copies there
    before (conv_halo's CF epilogue, round 5: fixed by making those loads compiler-visible).  hipcc cross-compiles without a GPU."""
    import shutil
    import subprocess
    import sys
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    root = Path(__file__).resolve().parent.parent
    src = root / "diffusion-nlc_amd" / "csrc"
    stems = ["conv_halo", "conv_fast", "conv_small"]
    procs = [subprocess.Popen(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++20", f"-I{root / 'include'}", f"-I{src}", "-S",
                               "--cuda-device-only", "-o", str(tmp_path / f"{s}.s"), str(src / f"{s}.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.PIPE) for s in stems]
    for s, pr in zip(stems, procs):
        _, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, f"{s}.hip: {err.decode()[-2000:]}"
    r = subprocess.run([sys.executable, str(root / "tools" / "asm_load_audit.py")] + [str(tmp_path / f"{s}.s") for s in stems],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 touches" in r.stdout


# ---- the references of tests/test_sampler_ops_gpu.py (tests/sampler_refs.py) held to the CPU oracle, bit for bit in f32, and the
#      preconditions its GPU cases rely on
def _oracle_schedule(continuous_t):
    from oracle import sched as osch
    return osch.get_sampler("ddim", 1000, 50, sigma_style="DDIM", start_sigma=100, end_sigma=0, continuous_t=continuous_t)


@pytest.mark.parametrize("continuous_t", [False, True], ids=["discrete", "continuous"])
def test_sampler_refs_lookup_equals_the_oracle(continuous_t):
    from tests import sampler_refs as R
    S = _oracle_schedule(continuous_t)
    sigmas, slopes = R.tables()["cont" if continuous_t else "t1000"]
    assert torch.equal(S.sigmas, sigmas) and (slopes is not None) == continuous_t
    g = R.gen(("lookup", continuous_t))
    v = torch.cat([torch.exp(torch.rand(4000, generator=g) * 13 - 7), sigmas, sigmas * 0.5, sigmas * 1.5,
                   torch.tensor([0.0, -1.0, 1e-30, 1e30])]).float()
    assert torch.equal(R.lookup_f32(sigmas, slopes, v), S.get_t_from_sigma(v).float())
    for kind, (tab, sl) in R.tables().items():
        assert bool((tab[1:] > tab[:-1]).all()) and tab.dtype == torch.float32, kind
        assert tab.numel() == {"t51": 51, "t1000": 1000, "t1001": 1001, "cont": 1000}[kind]
    # a NaN sigma: n, as torch.searchsorted finds it (include/nlc_hip.h documents the kernels' lookup the same way)
    assert R.lookup_f32(sigmas, None, torch.tensor([float("nan")])).item() == sigmas.numel()


def _oracle_denoise(S, xt, t, sigma_t, sigma_prev, style, refine, time_shift=0, norm_min=None, norm_max=None, r=None):
    """oracle/loop.py get_denoise_vector with stand-in networks -> (sigma_t, sigma_prev, the t the eps network was given)."""
    from oracle.loop import DiffusionOracle
    seen = {}

    def eps_fn(z, tt):
        seen["t"] = tt.clone()
        return torch.zeros_like(z)
    O = DiffusionOracle(eps_fn, lambda z, tt: z, lambda f: r, S, data_shape=xt.shape[1:], learn_epsvar=False,
                        norm_min=norm_min, norm_max=norm_max, time_shift=time_shift)
    _, _, st, sp = O.get_denoise_vector(xt, t, sigma_t, sigma_prev, style=style, refine_prior_sigma=refine)
    return st, sp, seen["t"].float().reshape(-1)


@pytest.mark.parametrize("continuous_t", [False, True], ids=["discrete", "continuous"])
def test_sampler_refs_refine_clamp_and_shift_equal_the_oracle(continuous_t):
    """oracle/loop.py:80-90.  The state is [v, 0, 0] with a 12-bit v, so that its norm is v exactly and the sum of squares the
    kernels are given is v*v exactly."""
    import math
    from tests import sampler_refs as R
    S = _oracle_schedule(continuous_t)
    sigmas, slopes = R.tables()["cont" if continuous_t else "t1000"]
    g = R.gen(("refine-oracle", continuous_t))
    B, dim, nmin, nmax = 600, 3, 0.05, 2.0
    v = torch.randint(1, 4096, (B,), generator=g).float() / 16.0 * 2.0 ** -torch.randint(0, 12, (B,), generator=g).float()
    raw = torch.exp(torch.rand(B, generator=g) * 10.6 - 5.3).float()
    scal = (math.sqrt(dim), nmax / math.sqrt(dim), nmin / math.sqrt(dim))
    sg = R.refine_clamp_f32(v * v, raw, *scal)
    assert bool((sg > raw).any()) and bool((sg < raw).any()) and bool((sg == raw).any())      # both clamps bind, and neither
    t_all = R.lookup_f32(sigmas, slopes, sg)
    pos = torch.nonzero(t_all > 0).reshape(-1)
    zero = torch.nonzero(t_all <= 0).reshape(-1)
    assert pos.numel() > 100 and zero.numel() > 0
    for idx, shifted in ((pos, True), (torch.cat([pos[:200], zero[:1], pos[200:]]), False)):
        xt = torch.zeros(idx.numel(), dim)
        xt[:, 0] = v[idx]
        st, sp, t = _oracle_denoise(S, xt, torch.tensor(0), raw[idx].view(-1, 1), torch.tensor(0.8), "base", True, time_shift=3,
                                    norm_min=nmin, norm_max=nmax)
        assert torch.equal(st.reshape(-1), sg[idx])
        want = R.shift_clamp_f32(t_all[idx], 3)
        assert torch.equal(t, want)
        assert torch.equal(want, (t_all[idx] - 3).clamp(0, 1000) if shifted else t_all[idx].clamp(0, 1000))
        # (3 + 1) half ulps of the largest intermediate bound the f32 chain against its f64 evaluation (the bound the GPU test uses)
        ref, norm_x = R.refine_clamp_f64((v * v)[idx], raw[idx], *scal)
        assert bool(((st.reshape(-1).double() - ref).abs() <= 4 * R.U32 * torch.maximum(norm_x, ref).clamp(min=scal[1])).all())


@pytest.mark.parametrize("style", ["pred", "pred_partial"])
@pytest.mark.parametrize("continuous_t", [False, True], ids=["discrete", "continuous"])
def test_sampler_refs_correct_step_equals_the_oracle(continuous_t, style):
    """oracle/loop.py:94-99."""
    from tests import sampler_refs as R
    S = _oracle_schedule(continuous_t)
    sigmas, slopes = R.tables()["cont" if continuous_t else "t1000"]
    g = R.gen(("correct-oracle", continuous_t))
    B = 500
    st0 = torch.rand(B, generator=g) * 40 + 0.05
    st0[::5] = sigmas[torch.randint(1, 1000, (B // 5,), generator=g)]
    sp0 = st0 * 0.8
    r = torch.randn(B, generator=g) * 0.5
    r[::5] = 0.0
    r[1::50] = -1.5
    r[2::50] = 1e4
    st, sp, t = _oracle_denoise(S, torch.zeros(B, 3), torch.zeros(B, dtype=torch.long), st0.view(-1, 1), sp0.view(-1, 1), style, False,
                                r=r.view(-1, 1))
    dist_hat, dist_prev = R.correct_f32(st0, sp0, r)
    assert torch.equal(st.reshape(-1), dist_hat)
    assert torch.equal(sp.reshape(-1), dist_prev if style == "pred" else sp0)
    assert torch.equal(t, R.lookup_f32(sigmas, slopes, dist_hat).clamp(0.0, 1000.0))
    assert torch.equal(dist_hat[::5], st0[::5])                                      # r = 0 lands on the table entry itself
    ref = R.c_in_f64(dist_hat)
    c_in = (1.0 / (dist_hat * dist_hat + 1.0)).sqrt()
    assert bool(((c_in.double() - ref).abs() <= 5 * R.U32 * ref).all())


@pytest.mark.parametrize("sigma_data", [0.5, 1.0])
def test_sampler_refs_edm_scalars_equal_the_oracle(sigma_data):
    """oracle/loop.py EdmOracle.encode_edm / pred_edm: the stand-in network records c_in * 1 and c_noise; F = 0 leaves c_skip,
    x = 0 leaves c_out."""
    from oracle.loop import EdmOracle
    from tests import sampler_refs as R
    B = 257
    sigma = R.edm_sigmas(B, sigma_data)
    assert sigma[-1].item() == sigma_data and bool((sigma[:-1].float().double() != sigma[:-1]).all())
    seen = {}

    def net(x, c_noise):
        seen["x"], seen["c_noise"] = x, c_noise
        return seen["F"]
    O = EdmOracle(net, net, None, data_shape=(1, 1, 1), sigma_data=sigma_data)
    c_in, c_noise, c_skip, c_out = R.edm_scalars_f32(sigma, sigma_data)
    seen["F"] = torch.zeros(B, 1, 1, 1)
    assert torch.equal(O.pred_edm(torch.ones(B, 1, 1, 1, dtype=torch.float64), sigma).reshape(-1), c_skip)
    assert torch.equal(seen["x"].reshape(-1), c_in) and torch.equal(seen["c_noise"], c_noise)
    seen["F"] = torch.ones(B, 1, 1, 1)
    assert torch.equal(O.pred_edm(torch.zeros(B, 1, 1, 1, dtype=torch.float64), sigma).reshape(-1), c_out)
    O.encode_edm(torch.ones(B, 1, 1, 1, dtype=torch.float64), sigma)
    assert torch.equal(seen["x"].reshape(-1), c_in) and torch.equal(seen["c_noise"], c_noise)
    r_in, _, r_skip, r_out = R.edm_scalars_f64(sigma, sigma_data)                   # the half-ulp counts of the GPU test
    for got, ref, n in ((c_skip, r_skip, 5), (c_out, r_out, 7), (c_in, r_in, 6)):
        assert bool(((got.double() - ref).abs() <= n * R.U32 * ref).all())


def test_sampler_refs_preconditions_of_the_gpu_cases():
    import math
    from fractions import Fraction
    from tests import sampler_refs as R
    for kind, (sigmas, slopes) in R.tables().items():
        # raw sigmas meant to be table entries are bit-equal to one
        sumsq, raw = R.refine_inputs(sigmas, 2500, kind)
        ties = raw[3::6].contiguous()
        assert torch.equal(sigmas[torch.searchsorted(sigmas, ties)], ties)
        sg = R.refine_clamp_f32(sumsq, raw, *R.REFINE_SCALARS)
        assert torch.equal(sg[3::6], ties) and torch.equal(sg[0::6], raw[0::6])                     # neither clamp binds
        assert bool((sg[1::6] > raw[1::6]).all()) and bool((sg[2::6] < raw[2::6]).all())            # lower / upper clamp binds
        assert bool((raw[4::6] > sigmas[-1]).all()) and bool((raw[5::6] <= sigmas[0]).all())
        # the every-t-positive batch, and the same batch with one sample at t == 0
        sumsq, raw = R.refine_inputs(sigmas, 2500, kind, every_t_positive=True)
        t = R.lookup_f32(sigmas, slopes, R.refine_clamp_f32(sumsq, raw, *R.REFINE_SCALARS))
        assert bool(t.min() > 0) and bool((t >= 3).any())
        for z in (0, 70, 2499):
            sumsq, raw = R.refine_inputs(sigmas, 2500, kind, every_t_positive=True, zero_at=z)
            t = R.lookup_f32(sigmas, slopes, R.refine_clamp_f32(sumsq, raw, *R.REFINE_SCALARS))
            assert t[z].item() == 0.0 and int((t <= 0).sum()) == 1
    # cosine inputs: condition below 1e3 wherever the products do not vanish; the kernel's formula agrees with ATen inside the bound
    for D in (1, 63, 1024, 1025, 3072, 196608):
        a, b = R.cosine_rows(D)
        scale, dot = R.cosine_parts(a, b)
        for k in ("random", "identical", "opposite", "tiny"):
            i = R.COS_KINDS.index(k)
            assert scale[i] / dot[i] < 1e3, (D, k)
        assert scale[3].item() == 0.0 and scale[4].item() == 0.0
        assert a[5].norm().item() < R.COS_EPS and a[4].norm().item() == 0.0
        na, nb = a.norm(dim=1, keepdim=True).clamp(min=R.COS_EPS), b.norm(dim=1, keepdim=True).clamp(min=R.COS_EPS)
        ref = torch.nn.CosineSimilarity(dim=1, eps=R.COS_EPS)(a, b)
        assert bool((((a / na) * (b / nb)).sum(1) - ref).abs().le((R.sumsq_chain_f64(D) + 1) * R.U64 * scale).all())
    # the exact sum of squares, against rational arithmetic
    x = torch.randn(37, generator=R.gen("exact"), dtype=torch.float64).numpy() * 1e3
    exact = sum(Fraction(float(v)) ** 2 for v in x)
    assert R.exact_sumsq(x) == float(exact)
    # the propagated bound of proj_sigma holds for its f32 restatement
    g = R.gen("proj-bound")
    B, sd = 4000, math.sqrt(3072.0)
    nm = 31.0 / sd
    cn = torch.rand(B, generator=g) * 3 + 0.05
    cn[::4] = nm * (1 + 0.01 * torch.randn(B // 4, generator=g))
    args = (((cn * sd) ** 2).float(), cn * 1.1, torch.rand(B, generator=g) * 60 + 0.01, torch.rand(B, generator=g) * 50 + 0.01,
            sd, nm, nm ** 2, 0.99, 1.25, 0.2, 0.3, 0.4)
    ref, bound = R.proj_f64_with_bound(*args)
    assert bool(((R.proj_f32(*args)[0].double() - ref).abs() <= bound).all())
    assert bool((bound < 64 * R.U32 * ref.abs()).all())                                                  # and it is no blank cheque
    # cast edge values survive the CPU conversion as the GPU test expects them
    v = R.cast_values(1023).float()
    assert v[0].item() == 1.0 and v[1].item() == 1.0 + 2.0 ** -22 and math.isinf(v[2].item()) and v[4].item() == 0.0
    assert 0.0 < v[5].item() < 1.1754944e-38 and math.copysign(1.0, v[7].item()) == -1.0 and math.isnan(v[8].item())
    assert v[11].item() == 0.0 and v[12].item() == 2.0 ** -148 and math.isinf(v[13].item())
