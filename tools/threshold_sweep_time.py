#!/usr/bin/env python3
"""Time of a threshold sweep (evaluate.threshold_sweep) against the loop over separately frozen sparse models, one process:

  sweep   sw.ensemble(x, S): K x S members in one lbbnn_sparse_layer_levels launch per layer, one transpose, one flow launch
  loop    for fz in models: fz.ensemble(x, S) with the K models of evaluate.freeze(net, "mpm", threshold=t, sparse=True)
          frozen beforehand (the freezes themselves stay outside the timing)

K = 8 thresholds 0.5 .. 0.99, S = 10 members, LRT 784-400-400-10 and planar MNF 784-1200-1200-10, B = 100 and B = 1000.
lambdal: nine weights in ten are U(-6, -0.5) (below every cut), the tenth is exponential with scale logit(0.99) / ln 10, so level
0 keeps about 10 % of the weights and the last level about 1 %.

Whole Python calls on the host clock, each window ending in a synchronise; REPEATS interleaved windows per form after a
warm-up of both.  The outputs of the two forms are compared first (same Philox offset: they must be the same bits).
THE ONE CONDITION: at B = 100, on both networks, the slowest sweep window is faster than the fastest loop window.  B = 1000,
the bind time (one threshold_sweep against the K freezes, host clock with a synchronise) and the spreads are recorded without a
bar.  The table goes to stdout and to --out (default profiles/threshold_sweep.txt)."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bnn_amd
from bnn_amd import _lib, evaluate

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200, help="calls per window at B = 100 (B = 1000: a fifth of it)")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "threshold_sweep.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("threshold_sweep_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
S = 10
THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.975, 0.99)
NETS = {"lrt": (784, 400, 400, 10), "mnf": (784, 1200, 1200, 10)}


def make(kind):
    torch.manual_seed(0)
    dims = NETS[kind]
    if kind == "mnf":
        net = bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")
    else:
        net = bnn_amd.lrt.BayesianNetwork(dims)
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(7)
    scale = math.log(0.99 / 0.01) / math.log(10.0)
    with torch.no_grad():
        for l in net._layers():
            shape = (l.out_features, l.in_features)
            low = torch.empty(shape).uniform_(-6.0, -0.5, generator=g)
            high = torch.empty(shape).exponential_(1.0 / scale, generator=g)
            l.lambdal.copy_(torch.where(torch.rand(shape, generator=g) < 0.1, high, low).to(dev))
    return net


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def c_calls(fn):
    _lib.RECORD = []
    try:
        fn()
        return [r[0].replace("lbbnn_", "") for r in _lib.RECORD]
    finally:
        _lib.RECORD = None


lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


bnn_amd.set_precision("fp32")
fmt = lambda v: " ".join("%.4f" % u for u in v)
say("K = %d thresholds %s, S = %d members; per form %d windows (ms per call on the host clock, a synchronise at each end; %d "
    "calls per window at B = 100, %d at B = 1000), the forms alternating, after %d warm-up calls of each"
    % (len(THRESHOLDS), THRESHOLDS, S, args.repeats, args.calls, max(1, args.calls // 5), args.warmup))
say("device: %s" % torch.cuda.get_device_name(0))
held = []
for kind, dims in NETS.items():
    net = make(kind)
    freeze_all = lambda: [evaluate.freeze(net, "mpm", threshold=t, sparse=True) for t in THRESHOLDS]
    bind = lambda: evaluate.threshold_sweep(net, THRESHOLDS)
    for _ in range(3):
        freeze_all(), bind()
    tb = {"sweep": [], "loop": []}
    for _ in range(args.repeats):
        tb["sweep"].append(window(bind, 10))
        tb["loop"].append(window(freeze_all, 10))
    sw, fzs = bind(), freeze_all()
    say("%s %s: density per level %s" % (kind, dims, " ".join("%.4f" % d for d in sw.density.tolist())))
    say("%s bind: threshold_sweep [%s]  %d freezes [%s]  freezes/sweep %.2fx   bytes held: sweep %d, the %d models %d"
        % (kind, fmt(tb["sweep"]), len(THRESHOLDS), fmt(tb["loop"]), min(tb["loop"]) / min(tb["sweep"]), sw.operand_bytes,
           len(fzs), sum(f.operand_bytes for f in fzs)))
    for B in (100, 1000):
        x = torch.rand(B, 784, generator=torch.Generator().manual_seed(1)).to(dev)
        fns = {"sweep": lambda: sw.ensemble(x, S), "loop": lambda: [fz.ensemble(x, S) for fz in fzs]}
        bnn_amd.manual_seed(1, 0)
        out = fns["sweep"]()
        same = True
        for j, fz in enumerate(fzs):
            bnn_amd.manual_seed(1, 0)
            same = same and torch.equal(fz.ensemble(x, S), out[j])
        for _ in range(args.warmup):
            for f in fns.values():
                f()
        calls = args.calls if B == 100 else max(1, args.calls // 5)
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, f in fns.items():
                t[k].append(window(f, calls))
        verdict = ""
        if B == 100:
            ok = max(t["sweep"]) < min(t["loop"])
            held.append(ok)
            verdict = "  condition (slowest sweep < fastest loop): %s" % ("HOLDS" if ok else "DOES NOT HOLD")
        say("%s B=%-4d  %s  loop/sweep %.2fx  spread sweep %.1f %% loop %.1f %%  same bits: %s%s"
            % (kind, B, "  ".join("%s [%s]" % (k, fmt(v)) for k, v in t.items()), min(t["loop"]) / min(t["sweep"]),
               100 * (max(t["sweep"]) / min(t["sweep"]) - 1), 100 * (max(t["loop"]) / min(t["loop"]) - 1), same, verdict))
        if B == 100:
            say("%s C calls per ensemble: sweep %s | loop %d x (%s)"
                % (kind, " ".join(c_calls(fns["sweep"])), len(fzs), " ".join(c_calls(lambda: fzs[0].ensemble(x, S)))))
say("the condition holds in %d of %d rows (B = 100)" % (sum(held), len(held)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
