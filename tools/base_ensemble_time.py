#!/usr/bin/env python3
"""Ensemble-evaluation time of the baseline LBBNN (test_ensemble, LBBNN-GP-MF.py:345-502) at 784-400-600-10, B = 1000,
S = 10 members, gates="sample" with gamma.exact = True (as the reference sets it before the test, :619-621), one process:

  batched   evaluate.ensemble_forward: one lbbnn_gate_members launch + one GEMM launch per layer for all members
  loop      S x net.sample_predict (the same kernels, one member per launch)
  torch     the reference's loop: per member gamma.rsample() of every layer + net.forward(..., sample=True) (the torch-draw
            K6 path), alpha refreshed as :366-372 does

under the fp32 and bf16x3 precisions.  Every ensemble is bracketed by device events; STEPS (default 50) timed ensembles
after WARMUP (default 5); median and the 10th / 90th percentiles.

--trace FORM --reps R: run only that form R times (fp32) for `rocprofv3 --kernel-trace --stats` (launches per ensemble =
the trace's total / R, set-up and warm-up adding under one per ensemble at R = 200)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=int(os.environ.get("STEPS", "50")))
ap.add_argument("--warmup", type=int, default=int(os.environ.get("WARMUP", "5")))
ap.add_argument("--trace", choices=("batched", "loop", "torch"), default=None)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

dev = torch.device("cuda:0")
S, B = 10, 1000
torch.manual_seed(0)
net = bnn_amd.base.BayesianNetwork((784, 400, 600, 10)).to(dev).eval()
layers = (net.l1, net.l2, net.l3)
for l in layers:
    l.gamma.exact = True
x = torch.rand(B, 1, 28, 28, generator=torch.Generator().manual_seed(1)).to(dev)


def batched():
    return bnn_amd.evaluate.ensemble_forward(net, x, S)


def loop():
    return torch.stack([net.sample_predict(x) for _ in range(S)])


def torch_loop():
    outs = torch.zeros(S, B, 10, device=dev)
    with torch.no_grad():
        for i in range(S):
            for l in layers:
                l.alpha = 1 / (1 + torch.exp(-l.lambdal))
                l.gamma.alpha = l.alpha
            outs[i] = net.forward(x, net.l1.gamma.rsample(), net.l2.gamma.rsample(), net.l3.gamma.rsample(), sample=True)
    return outs


FORMS = {"batched": batched, "loop": loop, "torch": torch_loop}
if args.trace:
    fn = FORMS[args.trace]
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    print("ran the %s ensemble %d times" % (args.trace, args.reps))
    sys.exit(0)


def timed(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2], ts[len(ts) // 10], ts[(9 * len(ts)) // 10]


print("baseline LBBNN 784-400-600-10, B = %d, S = %d, gates='sample', gamma.exact = True; %d timed ensembles after %d "
      "warm-up, device events per ensemble" % (B, S, args.steps, args.warmup))
for prec in ("fp32", "bf16x3"):
    bnn_amd.set_precision(prec)
    res = {}
    for name, fn in FORMS.items():
        for _ in range(args.warmup):
            fn()
        res[name] = timed(fn, args.steps)
    for name, (med, p10, p90) in res.items():
        print("  %-6s %-8s median %.4f ms  (p10 %.4f, p90 %.4f)" % (prec, name, med, p10, p90))
    print("  %-6s loop / batched %.2fx, torch / batched %.2fx" % (prec, res["loop"][0] / res["batched"][0],
                                                                  res["torch"][0] / res["batched"][0]))
bnn_amd.set_precision("fp32")
