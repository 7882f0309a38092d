#!/usr/bin/env python3
"""Evaluation time of the frozen model for RNVP / MNF-type z flows (evaluate.freeze(net, gates, dense=True)) against the loop
of single forwards, S = 10 members (the reference's TEST_SAMPLES), one process:

  loop     evaluate.ensemble_forward(net, x, 10): ten fused single forwards, each 1 + T flow launches, the weight pass over
           every parameter and one GEMM per layer (what such a network's evaluation was before the frozen dense model)
  alpha    freeze(net, "alpha", dense=True).ensemble(x, 10): one lbbnn_flow_dense_members launch for every member and layer,
           one scale launch, one member GEMM per layer
  mpm      the same with the median-probability gates

for RNVP 784-1200-1200-10, RNVP 784-400-600-10 (the script's own sizes) and the MNF type 784-1200-1200-10, T = 2, at B = 100
and B = 1000 (the reference's test batch), under fp32 and bf16x3.  The forms alternate; each is timed REPEATS times as a
window of CALLS calls between two device events (REPEATS * CALLS >= 200 warmed repetitions per form), so the spread of each
form's windows is on the page next to the difference between the forms.  The outputs of alpha and loop are compared first
(same Philox offset: same draws, equal to fp32 rounding).

Kernel launches per ensemble and the member kernel's share come from a trace: --trace FORM --net NET --reps R runs only that
form R times (fp32, B = 100) for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd
from bnn_amd import _lib, evaluate

NETS = {"rnvp1200": ("RNVP", (784, 1200, 1200, 10)), "rnvp600": ("RNVP", (784, 400, 600, 10)),
        "mnf1200": ("MNF", (784, 1200, 1200, 10))}
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--repeats", type=int, default=4)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--trace", choices=("loop", "alpha", "mpm"), default=None)
ap.add_argument("--net", choices=tuple(NETS), default="rnvp1200")
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--samples", type=int, default=10)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("frozen_dense_time: needs a HIP device (no CPU path, no CPU timing)")
if args.calls * args.repeats < 200:
    sys.exit("frozen_dense_time: calls * repeats must be at least 200 repetitions per form")

dev = torch.device("cuda:0")
S, T = args.samples, 2


def make(name):
    kind, dims = NETS[name]
    torch.manual_seed(0)
    net = bnn_amd.mnf.BayesianNetwork(dims, T, z_flow_type=kind, r_flow_type=kind).to(dev).eval()
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.normal_(0, 2)                          # gates on both sides of the cut: mpm density ~ 0.5
            l.q0_mean.normal_(1, 0.1)
    return net


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def c_calls(fn):
    """The C entry points one call makes, in order (the launch recorder of ``_lib``)."""
    _lib.RECORD = []
    try:
        fn()
        return [r[0].replace("lbbnn_", "") for r in _lib.RECORD]
    finally:
        _lib.RECORD = None


def forms(net, x):
    fa, fm = evaluate.freeze(net, "alpha", dense=True), evaluate.freeze(net, "mpm", dense=True)
    return {"loop": lambda: evaluate.ensemble_forward(net, x, S), "alpha": lambda: fa.ensemble(x, S),
            "mpm": lambda: fm.ensemble(x, S)}, fm.density


if args.trace:
    net = make(args.net)
    x = torch.rand(100, 784, generator=torch.Generator().manual_seed(1)).to(dev)
    fn = forms(net, x)[0][args.trace]
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    print("ran the %s %s ensemble (S = %d) %d times" % (args.net, args.trace, S, args.reps))
    sys.exit(0)

print("S = %d members; per form %d windows of %d calls (ms per call), the forms alternating, after %d warm-up calls of each"
      % (S, args.repeats, args.calls, args.warmup))
for name, (kind, dims) in NETS.items():
    net = make(name)
    for prec in ("fp32", "bf16x3"):
        bnn_amd.set_precision(prec)
        for B in (100, 1000):
            x = torch.rand(B, 784, generator=torch.Generator().manual_seed(1)).to(dev)
            f, density = forms(net, x)
            bnn_amd.manual_seed(1, 0)
            ref = f["loop"]()
            bnn_amd.manual_seed(1, 0)
            out = f["alpha"]()
            diff = float((out - ref).abs().max() / ref.abs().max())
            for _ in range(args.warmup):
                for fn in f.values():
                    fn()
            t = {k: [] for k in f}
            for _ in range(args.repeats):
                for k, fn in f.items():
                    t[k].append(window(fn, args.calls))
            fmt = lambda v: " ".join("%.4f" % u for u in v)
            spread = lambda v: (max(v) - min(v)) / min(v)
            print("%s %s %-6s B=%-4d  loop [%s]  alpha [%s]  mpm [%s]  loop/alpha min/min %.2fx, slowest alpha vs fastest loop "
                  "%.2fx  loop/mpm %.2fx  spread of the windows: loop %.1f %% alpha %.1f %% mpm %.1f %%  alpha vs loop max|diff| / "
                  "max|ref| %.2g  mpm density %.3f"
                  % (kind, "-".join(map(str, dims)), prec, B, fmt(t["loop"]), fmt(t["alpha"]), fmt(t["mpm"]),
                     min(t["loop"]) / min(t["alpha"]), min(t["loop"]) / max(t["alpha"]), min(t["loop"]) / min(t["mpm"]),
                     100 * spread(t["loop"]), 100 * spread(t["alpha"]), 100 * spread(t["mpm"]), diff, density))
        calls = {k: c_calls(fn) for k, fn in f.items()}
        print("%s %s C calls per ensemble: loop %d (%s per forward) | alpha %s"
              % (kind, prec, len(calls["loop"]), " ".join(calls["loop"][:len(calls["loop"]) // S]), " ".join(calls["alpha"])))
bnn_amd.set_precision("fp32")
