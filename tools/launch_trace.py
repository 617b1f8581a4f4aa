#!/usr/bin/env python3
"""What do the networks launch, in order?  One encode, one forward and one sigma-net evaluation per case with every launching function of
ops hooked (module attributes, as tools/gn_census.py does): per call the function's name and its arguments bound to its signature -
tensors as shape / dtype / "carries ride-along statistics", a PackedConv as (Cin, Cout, KH, KW), gn_in / gn_coef as present or absent,
everything else by value; never a pointer.  Binding means a keyword left at its default and the same value passed explicitly trace
alike.  Per case the trace goes to OUT/<case>.json, its SHA-256 to OUT/SHA256SUMS, the three outputs to OUT/<case>.<name>.npy: run it
in two checkouts and compare (the parity tests' 1e-3 cannot see a fusion quietly not being taken).

    python tools/launch_trace.py OUT tiny     # every tiny network of tests/util.py in bf16, f16, f32 and f32x3
    python tools/launch_trace.py OUT bench    # the three bench.WORKLOADS at their own batch sizes in bf16
"""
import argparse
import hashlib
import inspect
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from diffusion_nlc_amd import ops  # noqa: E402

TINY = ["adm_tiny", "adm_tiny_b", "adm_tiny_cc", "simple_tiny", "edm_tiny"]


def launchers():
    """The public functions of ops that take the launch stream, and gn_in_spec, which decides a fusion without launching."""
    return [n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_")
            and (n == "gn_in_spec" or {"_stream", "_launch_conv"} & set(f.__code__.co_names))]


def describe(name, v):
    if torch.is_tensor(v):
        if name in ("gn_in", "gn_coef"):
            return "present"
        return {"shape": list(v.shape), "dtype": str(v.dtype), "stats": ops.ride_stats(v) is not None}
    if isinstance(v, ops.PackedConv):
        return {"Cin": v.Cin, "Cout": v.Cout, "KH": v.KH, "KW": v.KW}
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (tuple, list)):
        return "present" if name == "gn_in" else [describe(name, i) for i in v]
    return str(v) if isinstance(v, (torch.dtype, torch.device)) else type(v).__name__


def hook(trace):
    for n in launchers():
        fn = getattr(ops, n)
        sig = inspect.signature(fn)

        def wrapped(*a, _n=n, _fn=fn, _sig=sig, **k):
            b = _sig.bind(*a, **k)
            b.apply_defaults()
            trace.append([_n, {p: describe(p, v) for p, v in b.arguments.items()}])
            return _fn(*a, **k)
        setattr(ops, n, wrapped)


def evaluate(out, case, trace, eps, sig, x, t, *y):
    del trace[:]
    res = {"feat": eps.encode(x, t, *y), "out": eps(x, t, *y)}
    res["r"] = sig(res["feat"])
    torch.cuda.synchronize()
    text = json.dumps(trace, indent=0)
    (out / f"{case}.json").write_text(text)
    for k, v in res.items():
        np.save(out / f"{case}.{k}.npy", v.float().cpu().numpy())
    sha = hashlib.sha256(text.encode()).hexdigest()
    print(f"{sha}  {case}  ({len(trace)} calls)", flush=True)
    return f"{sha}  {case}\n"


def tiny_cases(out, trace):
    from tests.test_host_cpu import build_product
    from tests.util import load_npz, state_dicts
    for tag in TINY:
        g = load_npz(f"net_{tag}")
        for prec, spec in bench.PRECISIONS.items():
            eps, sig, _ = build_product(tag)
            for m, sd in zip((eps, sig), state_dicts(tag)):
                m.load_state_dict(sd)
                bench.set_precision(m.to("cuda:0"), spec)
            yield evaluate(out, f"{tag}.{prec}", trace, eps, sig, g["x"], g["t"], *([g["y"]] if "y" in g else []))


def bench_cases(out, trace):
    dev = torch.device("cuda:0")
    for name in ("adm256", "celebahq256", "edm32"):
        args = argparse.Namespace(tiny=False, batch=0, timesteps=0, dry_run=False, dtype="bf16")
        wl = bench.WORKLOADS[name](args, dev, bench.PRECISIONS["bf16"])
        x = wl.inputs(1, 1, 0)[0].float()
        t = torch.full((x.shape[0],), 0.5 if name == "edm32" else 500.0, device=dev)
        yield evaluate(out, f"{name}.bf16", trace, wl.exp.model, wl.exp.sigma_model, x, t)
        del wl
        torch.cuda.empty_cache()


def main():
    out, which = Path(sys.argv[1]), sys.argv[2]
    out.mkdir(parents=True, exist_ok=True)
    trace = []
    hook(trace)
    with open(out / "SHA256SUMS", "a") as sums:
        for line in {"tiny": tiny_cases, "bench": bench_cases}[which](out, trace):
            sums.write(line)


if __name__ == "__main__":
    main()
