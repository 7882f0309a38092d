#!/usr/bin/env python3
"""Evaluation time of the sparse median-probability model (evaluate.freeze(net, "mpm", sparse=True)) against the dense
median-probability model of the SAME network at the same gates, S = 10 members, one process:

  fp32     evaluate.freeze(net, "mpm").ensemble(x, 10) under set_precision("fp32"): the dense MFMA path, zeros included
  bf16x3   the same under set_precision("bf16x3")
  compact  evaluate.freeze(net, "mpm", compact=True) under fp32, only where it drops a unit (its dims differ)
  sparse   evaluate.freeze(net, "mpm", sparse=True): CSR weights, one lbbnn_sparse_layer_members launch per layer

for LRT 784-400-400-10 and MNF planar 784-1200-1200-10 at B = 100 and B = 4096, with lambdal = seeded U(-3, 3) and the
threshold moved so that 1, 2.5, 5, 10, 20 and 45 % of the weights are kept.

The forms alternate; each is timed REPEATS times as a window of calls between two device events after a warm-up of all, so
the spread of each form is on the page next to the difference.  The ensemble outputs of the sparse and the dense fp32 form
are compared first (same Philox offset).  THE ONE CONDITION: at 5 % kept and B = 4096, for both networks, the slowest sparse
window is faster than the fastest dense fp32 window; each such row says whether it holds.  Everything else is recorded
without a bar: the crossover density against fp32 and against bf16x3 at each B (the largest kept share at which the fastest
sparse window beats the fastest dense one), the launch-bound B = 100 rows, the bytes held.

The table goes to stdout and to --out (default profiles/frozen_sparse.txt).
--trace FORM --net NET --kept P --batch B --reps R runs only that form R times, for a `rocprofv3 --kernel-trace --stats` run
of its own."""
import argparse
import math
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
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_sparse.txt"))
ap.add_argument("--trace", choices=("fp32", "bf16x3", "sparse"), default=None)
ap.add_argument("--net", choices=("mnf", "lrt"), default="mnf")
ap.add_argument("--kept", type=float, default=0.05)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("frozen_sparse_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
S = 10
NETS = {"lrt": (784, 400, 400, 10), "mnf": (784, 1200, 1200, 10)}
KEPT = (0.01, 0.025, 0.05, 0.10, 0.20, 0.45)


def make(kind):
    torch.manual_seed(0)
    dims = NETS[kind]
    if kind == "mnf":
        net = bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")
    else:
        net = bnn_amd.lrt.BayesianNetwork(dims)
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.copy_(torch.empty(l.out_features, l.in_features).uniform_(-3, 3, generator=g).to(dev))
    return net


def threshold_of(kept):
    """P(U(-3, 3) > cut) = kept  <=>  cut = 3 - 6 kept; the threshold is its sigmoid."""
    return 1.0 / (1.0 + math.exp(-(3.0 - 6.0 * kept)))


def forms(net, kept):
    th = threshold_of(kept)
    out = {}
    bnn_amd.set_precision("fp32")
    out["fp32"] = evaluate.freeze(net, "mpm", threshold=th)
    comp = evaluate.freeze(net, "mpm", threshold=th, compact=True)
    if comp.dims != out["fp32"].dims:
        out["compact"] = comp
    bnn_amd.set_precision("bf16x3")
    out["bf16x3"] = evaluate.freeze(net, "mpm", threshold=th)
    bnn_amd.set_precision("fp32")
    out["sparse"] = evaluate.freeze(net, "mpm", threshold=th, sparse=True)
    return out


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


def dense_bytes(fz):
    held = sum(b.numel() * b.element_size() for k, b in fz.named_buffers() if k.split("_")[0] in ("e0", "e", "var", "bias"))
    return held, sum(e.numel() * e.element_size() for e in fz._ewm)


if args.trace:
    net = make(args.net)
    bnn_amd.set_precision("bf16x3" if args.trace == "bf16x3" else "fp32")
    x = torch.rand(args.batch, 784, generator=torch.Generator().manual_seed(1)).to(dev)
    fz = evaluate.freeze(net, "mpm", threshold=threshold_of(args.kept), sparse=args.trace == "sparse")
    for _ in range(args.reps):
        fz.ensemble(x, S)
    torch.cuda.synchronize()
    print("ran the %s %s ensemble at B = %d, density %.4f, %d times" % (args.net, args.trace, args.batch, fz.density, args.reps))
    sys.exit(0)

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say("S = %d members; per form %d windows (ms per call; %d calls per window at B = 100, %d at B = 4096), the forms alternating, "
    "after %d warm-up calls of each" % (S, args.repeats, args.calls, max(1, args.calls // 5), args.warmup))
say("device: %s" % torch.cuda.get_device_name(0))
held, fastest = [], {}
fmt = lambda v: " ".join("%.4f" % u for u in v)
for kind, dims in NETS.items():
    net = make(kind)
    for kept in KEPT:
        fz = forms(net, kept)
        sp = fz["sparse"]
        for B in (100, 4096):
            x = torch.rand(B, 784, generator=torch.Generator().manual_seed(1)).to(dev)
            fns = {k: (lambda m=m: m.ensemble(x, S)) for k, m in fz.items()}
            bnn_amd.manual_seed(1, 0)
            ref = fns["fp32"]()
            bnn_amd.manual_seed(1, 0)
            out = fns["sparse"]()
            err = float((out - ref).abs().max() / ref.abs().max())
            for _ in range(args.warmup):
                for f in fns.values():
                    f()
            calls = args.calls if B == 100 else max(1, args.calls // 5)
            t = {k: [] for k in fns}
            for _ in range(args.repeats):
                for k, f in fns.items():
                    t[k].append(window(f, calls))
            for k in t:
                fastest[(kind, B, kept, k)] = min(t[k])
            verdict = ""
            if B == 4096 and kept == 0.05:
                ok = max(t["sparse"]) < min(t["fp32"])
                held.append(ok)
                verdict = "  condition (slowest sparse < fastest fp32): %s" % ("HOLDS" if ok else "DOES NOT HOLD")
            say("%s kept %.4f B=%-4d  %s  fp32/sparse %.2fx  bf16x3/sparse %.2fx  sparse vs fp32 rel. diff %.2g%s"
                % (kind, sp.density, B, "  ".join("%s [%s]" % (k, fmt(v)) for k, v in t.items()),
                   min(t["fp32"]) / min(t["sparse"]), min(t["bf16x3"]) / min(t["sparse"]), err, verdict))
        d_held, d_members = dense_bytes(fz["fp32"])
        say("%s kept %.4f bytes held: sparse %d (nnz %d) | dense fp32 operands %d + member operands %d (S = %d)"
            % (kind, sp.density, sp.operand_bytes, sp.nnz, d_held, d_members, S))
        if kept == 0.05:
            say("%s C calls per ensemble: fp32 %s | sparse %s"
                % (kind, " ".join(c_calls(fns["fp32"])), " ".join(c_calls(fns["sparse"]))))
    for B in (100, 4096):
        for base in ("fp32", "bf16x3"):
            wins = [k for k in KEPT if fastest[(kind, B, k, "sparse")] < fastest[(kind, B, k, base)]]
            say("%s B=%d crossover against %s: sparse is faster at kept shares %s (largest: %s)"
                % (kind, B, base, ", ".join("%g" % w for w in wins) or "none", "%g" % max(wins) if wins else "none"))
bnn_amd.set_precision("fp32")
say("the condition holds in %d of %d rows (5 %% kept, B = 4096)" % (sum(held), len(held)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
