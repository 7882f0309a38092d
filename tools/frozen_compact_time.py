#!/usr/bin/env python3
"""Evaluation time of the compact median-probability model (evaluate.freeze(net, "mpm", compact=True)) against the full
median-probability model of the SAME network, S = 10 members, one process:

  full     evaluate.freeze(net, "mpm").ensemble(x, 10)
  compact  evaluate.freeze(net, "mpm", compact=True).ensemble(x, 10): the same kernels at the widths of the units some output
           depends on, plus one lbbnn_gather_columns launch when input features go

for LRT 784-400-400-10 and MNF planar 784-1200-1200-10 at B = 100 and B = 4096, under fp32 and bf16x3, with two structures:

  (a) no unit unneeded (every gate kept): the compact model has the full widths, so this row is the overhead of the form;
  (b) every second hidden unit and every third input feature unconsumed.

The two forms alternate; each is timed REPEATS times as a window of calls between two device events after a warm-up of both,
so the spread of each form is on the page next to the difference.  The posterior means of the two forms are compared first
(same Philox offset).  THE ONE CONDITION: at B = 4096, structure (b), the slowest compact window is faster than the fastest
full window; each such row says whether it holds.  The B = 100 rows and structure (a) are recorded without a bar.

The table goes to stdout and to --out (default profiles/frozen_compact.txt).
--trace FORM --net NET --prec PREC --batch B --reps R runs only that form of structure (b) R times, for a
`rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bnn_amd
from bnn_amd import _lib, evaluate

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200, help="calls per window at B = 100 (B = 4096: a fifth of it)")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_compact.txt"))
ap.add_argument("--trace", choices=("full", "compact"), default=None)
ap.add_argument("--net", choices=("mnf", "lrt"), default="mnf")
ap.add_argument("--prec", choices=("fp32", "bf16x3"), default="fp32")
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("frozen_compact_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
S = 10
NETS = {"lrt": (784, 400, 400, 10), "mnf": (784, 1200, 1200, 10)}


def make(kind, structure):
    torch.manual_seed(0)
    dims = NETS[kind]
    if kind == "mnf":
        net = bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")
    else:
        net = bnn_amd.lrt.BayesianNetwork(dims)
    net = net.to(dev).eval()
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.fill_(2.0)                             # (a): every weight kept
        if structure == "b":
            net.l1.lambdal[:, 1::3] = -2.0                   # every third input feature unconsumed
            net.l2.lambdal[:, 1::2] = -2.0                   # every second hidden unit unconsumed
            net.l3.lambdal[:, 1::2] = -2.0
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
    _lib.RECORD = []
    try:
        fn()
        return [r[0].replace("lbbnn_", "") for r in _lib.RECORD]
    finally:
        _lib.RECORD = None


if args.trace:
    net = make(args.net, "b")
    bnn_amd.set_precision(args.prec)
    x = torch.rand(args.batch, 784, generator=torch.Generator().manual_seed(1)).to(dev)
    fz = evaluate.freeze(net, "mpm", compact=args.trace == "compact")
    for _ in range(args.reps):
        fz.ensemble(x, S)
    torch.cuda.synchronize()
    print("ran the %s %s %s ensemble of structure (b) at B = %d %d times, dims %s"
          % (args.net, args.prec, args.trace, args.batch, args.reps, fz.dims))
    sys.exit(0)

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say("S = %d members; per form %d windows (ms per call; %d calls per window at B = 100, %d at B = 4096), the forms alternating, "
    "after %d warm-up calls of each" % (S, args.repeats, args.calls, max(1, args.calls // 5), args.warmup))
say("device: %s" % torch.cuda.get_device_name(0))
held = []
for kind, dims in NETS.items():
    for structure in ("a", "b"):
        net = make(kind, structure)
        for prec in ("fp32", "bf16x3"):
            bnn_amd.set_precision(prec)
            full = evaluate.freeze(net, "mpm")
            comp = evaluate.freeze(net, "mpm", compact=True)
            if prec == "fp32":
                say("%s %s structure (%s): compact dims %s, needed %s, density %.4f, active density %.4f"
                    % (kind, "-".join(map(str, dims)), structure, "-".join(map(str, comp.dims)),
                       "/".join(map(str, comp.needed)), comp.density, comp.active_density))
            for B in (100, 4096):
                x = torch.rand(B, 784, generator=torch.Generator().manual_seed(1)).to(dev)
                f_full = lambda: full.ensemble(x, S)
                f_comp = lambda: comp.ensemble(x, S)
                bnn_amd.manual_seed(1, 0)
                ref = full(x, sample=False)
                bnn_amd.manual_seed(1, 0)
                out = comp(x, sample=False)
                err = float((out - ref).abs().max() / ref.abs().max())
                for _ in range(args.warmup):
                    f_full()
                    f_comp()
                calls = args.calls if B == 100 else max(1, args.calls // 5)
                t = {"full": [], "compact": []}
                for _ in range(args.repeats):
                    t["full"].append(window(f_full, calls))
                    t["compact"].append(window(f_comp, calls))
                fmt = lambda v: " ".join("%.4f" % u for u in v)
                verdict = ""
                if B == 4096 and structure == "b":
                    ok = max(t["compact"]) < min(t["full"])
                    held.append(ok)
                    verdict = "  condition (slowest compact < fastest full): %s" % ("HOLDS" if ok else "DOES NOT HOLD")
                say("%s (%s) %-6s B=%-4d  full [%s]  compact [%s]  min/min %.3fx  posterior mean rel. diff %.2g%s"
                    % (kind, structure, prec, B, fmt(t["full"]), fmt(t["compact"]), min(t["full"]) / min(t["compact"]), err,
                       verdict))
            if prec == "fp32":
                say("%s (%s) C calls per ensemble: full %s | compact %s"
                    % (kind, structure, " ".join(c_calls(f_full)), " ".join(c_calls(f_comp))))
bnn_amd.set_precision("fp32")
say("the condition holds in %d of %d rows (B = 4096, structure (b))" % (sum(held), len(held)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
