#!/usr/bin/env python3
"""Evaluation time of the baseline family's sparse median-probability model (evaluate.freeze_base(net, "mpm", sparse=True))
against the dense frozen models of the SAME network at the same gates, on the reference script's own network 784-400-600-10
with S = 10 members (TEST_SAMPLES), fp32, one process:

  sparse   evaluate.freeze_base(net, "mpm", sparse=True): CSR weights, one draw launch, one layer launch per layer
  fp32     evaluate.freeze_base(net, "mpm") under set_precision("fp32"): every member's dense operand, then the member GEMMs
  compact  evaluate.freeze_base(net, "mpm", compact=True) under fp32
  bf16x3   evaluate.freeze_base(net, "mpm") under set_precision("bf16x3")

at B = 1000 (TEST_BATCH_SIZE) and B = 100, with lambdal = seeded U(-3, 3) and the threshold moved so that 5 % of every layer's
weights are kept (1, 10 and 25 % for the record).

What is timed is the whole ``fz.ensemble(x, S)`` call: a window is --calls calls between two device synchronisations, on the host
clock, so the host's share of a call is in the number.  The forms alternate in --rounds rounds after a warm-up of all, so the
spread of each form is on the page next to the difference.  The ensemble outputs of the sparse and the dense fp32 form are
compared first (same Philox offset).  THE CONDITION (as 7.30's): at 5 % kept, at B = 1000 and at B = 100, the
slowest sparse window is faster than the fastest dense-fp32 window.  Everything else is recorded without a bar: the other kept
shares, compact and bf16x3, ``explain_ensemble(fz, x, 10, targets="pred")`` on the sparse model, the C calls of one ensemble.

The table goes to stdout and to --out (default profiles/base_sparse.txt).
--trace FORM --kept P --batch B --reps R runs only that form R times, for a `rocprofv3 --kernel-trace --stats` run of its own."""
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
ap.add_argument("--calls", type=int, default=200, help="calls per window")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "base_sparse.txt"))
ap.add_argument("--trace", choices=("sparse", "fp32", "compact", "bf16x3", "explain"), default=None)
ap.add_argument("--kept", type=float, default=0.05)
ap.add_argument("--batch", type=int, default=1000)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("base_sparse_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
S = 10
DIMS = (784, 400, 600, 10)
KEPT = (0.05, 0.01, 0.10, 0.25)
BATCHES = (1000, 100)


def make():
    torch.manual_seed(0)
    net = bnn_amd.base.BayesianNetwork(DIMS).to(dev).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.copy_(torch.empty(l.out_features, l.in_features).uniform_(-3, 3, generator=g).to(dev))
    return net


def threshold_of(kept):
    """P(U(-3, 3) > cut) = kept  <=>  cut = 3 - 6 kept; the threshold is its sigmoid."""
    return 1.0 / (1.0 + math.exp(-(3.0 - 6.0 * kept)))


def form(net, name, kept):
    th = threshold_of(kept)
    bnn_amd.set_precision("bf16x3" if name == "bf16x3" else "fp32")
    try:
        if name in ("sparse", "explain"):
            return evaluate.freeze_base(net, "mpm", threshold=th, sparse=True)
        return evaluate.freeze_base(net, "mpm", threshold=th, compact=name == "compact")
    finally:
        bnn_amd.set_precision("fp32")


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


if args.trace:
    net = make()
    x = torch.rand(args.batch, 784, generator=torch.Generator().manual_seed(1)).to(dev)
    fz = form(net, args.trace, args.kept)
    for _ in range(args.reps):
        if args.trace == "explain":
            evaluate.explain_ensemble(fz, x, S, targets="pred")
        else:
            fz.ensemble(x, S)
    torch.cuda.synchronize()
    print("ran the %s form at B = %d, density %.4f, %d times" % (args.trace, args.batch, fz.density, args.reps))
    sys.exit(0)

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say("baseline 784-400-600-10, S = %d members, fp32; per form %d windows of %d whole ensemble calls (ms per call, host clock between "
    "two device synchronisations), the forms alternating, after %d warm-up calls of each" % (S, args.rounds, args.calls, args.warmup))
say("device: %s" % torch.cuda.get_device_name(0))
held = []
fmt = lambda v: " ".join("%.4f" % u for u in v)
net = make()
for kept in KEPT:
    fz = {k: form(net, k, kept) for k in ("sparse", "fp32", "compact", "bf16x3")}
    sp = fz["sparse"]
    for B in BATCHES:
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
        t = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, f in fns.items():
                t[k].append(window(f, args.calls))
        verdict = ""
        if kept == 0.05:
            ok = max(t["sparse"]) < min(t["fp32"])
            held.append(ok)
            verdict = "  condition (slowest sparse %.4f < fastest fp32 %.4f): %s" % (max(t["sparse"]), min(t["fp32"]),
                                                                                     "HOLDS" if ok else "DOES NOT HOLD")
        say("kept %.4f B=%-4d  %s  fp32/sparse %.2fx  compact/sparse %.2fx  bf16x3/sparse %.2fx  sparse vs fp32 rel. diff %.2g%s"
            % (sp.density, B, "  ".join("%s [%s]" % (k, fmt(v)) for k, v in t.items()), min(t["fp32"]) / min(t["sparse"]),
               min(t["compact"]) / min(t["sparse"]), min(t["bf16x3"]) / min(t["sparse"]), err, verdict))
        if kept == 0.05:
            ex = lambda: evaluate.explain_ensemble(sp, x, S, targets="pred")
            for _ in range(3):
                ex()
            say("kept %.4f B=%-4d  explain_ensemble(targets=\"pred\", %d members) on the sparse model [%s] ms per call (%d calls "
                "per window)" % (sp.density, B, S, fmt([window(ex, max(1, args.calls // 10)) for _ in range(args.rounds)]),
                                 max(1, args.calls // 10)))
    dense_held = sum(b.numel() * b.element_size() for k, b in fz["fp32"].named_buffers())
    say("kept %.4f bytes: sparse operands %d (nnz %d) + members' values %d | dense fp32 buffers %d + members' operands %d (S = %d); "
        "compact dims %s"
        % (sp.density, sp.operand_bytes, sp.nnz, 4 * S * (sp.nnz + sum(DIMS[1:])), dense_held,
           4 * S * sum(DIMS[i + 1] * bnn_amd.ops.operand_ld(DIMS[i]) for i in range(3)), S, fz["compact"].dims))
    if kept == 0.05:
        say("C calls per ensemble: sparse %s | fp32 %s" % (" ".join(c_calls(fns["sparse"])), " ".join(c_calls(fns["fp32"]))))
say("the condition holds in %d of %d rows (5 %% kept; B = 1000 and B = 100)" % (sum(held), len(held)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
