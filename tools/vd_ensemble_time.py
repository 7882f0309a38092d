#!/usr/bin/env python3
"""Ensemble-evaluation time of variational dropout (variational_dropout.py:154-160: num_test_ensemble_samples = 10 forwards
of each validation batch), one process, S = 10 members, two shapes:

  ref   the reference's VD network 784-1200-1200-1200-10 at B = 100 (launch-bound)
  c4    BASELINE configs[4] 3072-4096-4096-10 at B = 4096 (FLOP-bound)

and two forms:

  batched   evaluate.ensemble_forward -> vd_ensemble: per layer one lbbnn_vd_operands, the first layer's two products once
            and fanned out to every member, each later layer one lbbnn_vd_gemm_members launch for all members
  loop      S x net(x), the reference's loop (lbbnn_vd_operands + GEMM + offset advance per layer, torch ReLU / log_softmax)

under the fp32 and bf16x3 precisions.  Every ensemble is bracketed by device events; STEPS (default 30) timed ensembles after
WARMUP (default 3); median and the 10th / 90th percentiles.

--trace FORM --shape SHAPE --reps R: run only that form at that shape R times (fp32) for `rocprofv3 --kernel-trace --stats`
(launches per ensemble = the trace's total / R, set-up and warm-up adding under one per ensemble at R = 100)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=int(os.environ.get("STEPS", "30")))
ap.add_argument("--warmup", type=int, default=int(os.environ.get("WARMUP", "3")))
ap.add_argument("--trace", choices=("batched", "loop"), default=None)
ap.add_argument("--shape", choices=("ref", "c4"), default=None, help="only this shape (default: both)")
ap.add_argument("--reps", type=int, default=100)
args = ap.parse_args()

dev = torch.device("cuda:0")
S = 10
SHAPES = {"ref": ((784, 1200, 1200, 1200, 10), 100), "c4": ((3072, 4096, 4096, 10), 4096)}


def setup(shape):
    dims, B = SHAPES[shape]
    torch.manual_seed(0)
    net = bnn_amd.vd.BNN(dims).to(dev).eval()
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(1)).to(dev)

    def batched():
        return bnn_amd.evaluate.ensemble_forward(net, x, S)

    def loop():
        with torch.no_grad():
            return torch.stack([net(x) for _ in range(S)])
    return {"batched": batched, "loop": loop}


if args.trace:
    fn = setup(args.shape or "ref")[args.trace]
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    print("ran the %s ensemble at %s %d times" % (args.trace, args.shape or "ref", args.reps))
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


print("variational dropout, S = %d; %d timed ensembles after %d warm-up, device events per ensemble" % (S, args.steps,
                                                                                                       args.warmup))
for shape in ([args.shape] if args.shape else list(SHAPES)):
    dims, B = SHAPES[shape]
    forms = setup(shape)
    print("%s: %s, B = %d" % (shape, "-".join(map(str, dims)), B))
    for prec in ("fp32", "bf16x3"):
        bnn_amd.set_precision(prec)
        res = {}
        for name, fn in forms.items():
            for _ in range(args.warmup):
                fn()
            res[name] = timed(fn, args.steps)
        for name, (med, p10, p90) in res.items():
            print("  %-6s %-8s median %.4f ms  (p10 %.4f, p90 %.4f)" % (prec, name, med, p10, p90))
        print("  %-6s loop / batched %.2fx" % (prec, res["loop"][0] / res["batched"][0]))
    bnn_amd.set_precision("fp32")
