#!/usr/bin/env python3
"""Evaluation time of the frozen model (evaluate.freeze) against the live network's batched ensemble, S = 10 members, one
process:

  live     evaluate.ensemble_forward(net, x, 10): K3 (MNF) + K1 over the parameters for every member, one GEMM launch per layer
  frozen   evaluate.freeze(net).ensemble(x, 10): the operands were taken once; MNF: K3 + one scale launch, LRT: nothing,
           ahead of the same GEMM launches

for MNF planar 784-1200-1200-10 and LRT 784-400-400-10 at B = 100 (the reference's test batch) and B = 4096, under fp32 and
bf16x3.  The two forms alternate; each is timed REPEATS times as a window of CALLS calls between two device events after a
warm-up of both, so the spread of each form is on the page next to the difference between them.  Outputs are compared first
(same Philox offset; the frozen alpha model must equal the live ensemble).

Then ``freeze`` itself, ``refresh()`` (one lbbnn_frozen_operands launch + the copies of the small vectors) and that launch
alone, with its algorithmic bytes (12 B read + 12 B written per weight) over the time as a share of the 6.3 TB/s copy
ceiling -- an end-to-end figure from device events around back-to-back launches, not a profiler's kernel time.

The C entry points of one call are listed with the launch recorder of ``_lib``; kernel launches per call come from a trace:
--trace FORM --net NET --reps R runs only that form R times (fp32, B = 100) for a `rocprofv3 --kernel-trace --stats` run."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd
from bnn_amd import _lib, evaluate

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--trace", choices=("live", "frozen"), default=None)
ap.add_argument("--net", choices=("mnf", "lrt"), default="mnf")
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("frozen_eval_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
S = 10
NETS = {"mnf": (784, 1200, 1200, 10), "lrt": (784, 400, 400, 10)}
COPY_CEILING = 6.3e12          # B/s, MI355X HBM copy ceiling


def make(kind):
    torch.manual_seed(0)
    dims = NETS[kind]
    if kind == "mnf":
        net = bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")
    else:
        net = bnn_amd.lrt.BayesianNetwork(dims)
    return net.to(dev).eval()


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


if args.trace:
    net = make(args.net)
    x = torch.rand(100, 784, generator=torch.Generator().manual_seed(1)).to(dev)
    fz = evaluate.freeze(net)
    fn = (lambda: evaluate.ensemble_forward(net, x, S)) if args.trace == "live" else (lambda: fz.ensemble(x, S))
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    print("ran the %s %s ensemble %d times" % (args.net, args.trace, args.reps))
    sys.exit(0)

print("S = %d members; per form %d windows of %d calls (ms per call), the forms alternating, after %d warm-up calls of each"
      % (S, args.repeats, args.calls, args.warmup))
for kind, dims in NETS.items():
    net = make(kind)
    for prec in ("fp32", "bf16x3"):
        bnn_amd.set_precision(prec)
        fz = evaluate.freeze(net)
        for B in (100, 4096):
            x = torch.rand(B, 784, generator=torch.Generator().manual_seed(1)).to(dev)
            live = lambda: evaluate.ensemble_forward(net, x, S)
            frozen = lambda: fz.ensemble(x, S)
            bnn_amd.manual_seed(1, 0)
            ref = live()
            bnn_amd.manual_seed(1, 0)
            out = frozen()
            same = "bitwise equal" if torch.equal(out, ref) else "max |diff| %.3g" % float((out - ref).abs().max())
            for _ in range(args.warmup):
                live()
                frozen()
            t = {"live": [], "frozen": []}
            for _ in range(args.repeats):
                t["live"].append(window(live, args.calls))
                t["frozen"].append(window(frozen, args.calls))
            fmt = lambda v: " ".join("%.4f" % u for u in v)
            print("%s %s %-6s B=%-4d  live [%s]  frozen [%s]  min/min %.3fx  outputs %s"
                  % (kind, "-".join(map(str, dims)), prec, B, fmt(t["live"]), fmt(t["frozen"]),
                     min(t["live"]) / min(t["frozen"]), same))
        print("%s C calls per ensemble: live %s | frozen %s" % (kind, " ".join(c_calls(live)), " ".join(c_calls(frozen))))
        # the snapshot itself
        n_w = sum(dims[i] * dims[i + 1] for i in range(3))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f2 = evaluate.freeze(net, "mpm")
        torch.cuda.synchronize()
        t_freeze = (time.perf_counter() - t0) * 1e3
        layers = net._layers()
        descs = f2._descs(layers)
        stream = torch.cuda.current_stream(dev).cuda_stream
        launch = lambda: _lib.check(_lib.lib().lbbnn_frozen_operands(descs, 3, stream), "lbbnn_frozen_operands")
        for _ in range(args.warmup):
            f2.refresh()
            launch()
        r = [window(f2.refresh, args.calls) for _ in range(args.repeats)]
        k = [window(launch, args.calls) for _ in range(args.repeats)]
        nbytes = 24 * n_w
        print("%s %s %-6s freeze() %.2f ms (host clock, allocation included); refresh() [%s] ms; lbbnn_frozen_operands alone, "
              "back to back [%s] ms: %d weights, %.1f MB moved, %.2f TB/s = %.0f %% of the 6.3 TB/s copy ceiling (best window); "
              "density %.4f"
              % (kind, "-".join(map(str, dims)), prec, t_freeze, " ".join("%.4f" % u for u in r),
                 " ".join("%.4f" % u for u in k), n_w, nbytes / 1e6, nbytes / (min(k) * 1e-3) / 1e12,
                 100 * nbytes / (min(k) * 1e-3) / COPY_CEILING, f2.density))
bnn_amd.set_precision("fp32")
