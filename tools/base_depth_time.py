#!/usr/bin/env python3
"""Time of a baseline LBBNN (bnn_amd.base) at depth: the draws="hip" training step captured in a HIP graph and replayed
(graphs.make_graphed_train_step, one-group bnn_amd.optim.Adam), and evaluate.base_ensemble with S = 10 members (eager: the
call as a user makes it, host side included).  Width 512 throughout, 10 classes, fp32; B = 100 and 1024; n = 1, 3, 4, 5, 8, 16
layers.  Every configuration is timed in WINDOWS (default 5) windows of REPS calls between two device events; the windows of
all configurations are interleaved (window 1 of every configuration, then window 2, ...), so a disturbance on the machine falls
on all of them alike.  Reported: the fastest window per call, and the spread (slowest / fastest - 1) of the five."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=512)
ap.add_argument("--batches", type=int, nargs="+", default=[100, 1024])
ap.add_argument("--depths", type=int, nargs="+", default=[1, 3, 4, 5, 8, 16])
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--reps", type=int, default=100, help="graph replays per window")
ap.add_argument("--ens-reps", type=int, default=30, help="base_ensemble calls per window")
ap.add_argument("--samples", type=int, default=10)
args = ap.parse_args()

dev = torch.device("cuda:0")
hip_loss = lambda n, a, b: n.sample_elbo(a, b, draws="hip")[0]
jobs = []                                   # (B, n, kind, callable, reps)
keep = []
for B in args.batches:
    for n in args.depths:
        torch.manual_seed(n)
        dims = (args.width,) * n + (10,)
        net = bnn_amd.base.BayesianNetwork(dims).to(dev).train()
        opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-4)
        g = torch.Generator().manual_seed(B + n)
        x = torch.rand(B, args.width, generator=g).to(dev)
        y = torch.randint(0, 10, (B,), generator=g).to(dev)
        step = bnn_amd.graphs.make_graphed_train_step(net, opt, hip_loss, x, y)
        jobs.append((B, n, "step", step.graph.replay, args.reps))
        ens = bnn_amd.base.BayesianNetwork(dims).to(dev)
        jobs.append((B, n, "ensemble", (lambda ens=ens, x=x: bnn_amd.evaluate.base_ensemble(ens, x, args.samples)), args.ens_reps))
        keep.append((net, opt, step, ens))


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for _, _, _, fn, reps in jobs:              # warm every configuration up
    window(fn, max(reps // 5, 3))
times = [[] for _ in jobs]
for _ in range(args.windows):
    for j, (_, _, _, fn, reps) in enumerate(jobs):
        times[j].append(window(fn, reps))

print("baseline LBBNN, width %d, 10 classes, fp32; graphed draws=\"hip\" training step (%d replays per window) and eager "
      "base_ensemble at S = %d (%d calls per window); fastest of %d interleaved windows, spread = slowest / fastest - 1"
      % (args.width, args.reps, args.samples, args.ens_reps, args.windows))
print("%6s %3s  %14s %8s  %14s %8s" % ("B", "n", "step [ms]", "spread", "ensemble [ms]", "spread"))
res = {(B, n, kind): ts for (B, n, kind, _, _), ts in zip(jobs, times)}
for B in args.batches:
    for n in args.depths:
        s, e = res[(B, n, "step")], res[(B, n, "ensemble")]
        print("%6d %3d  %14.4f %7.1f%%  %14.4f %7.1f%%" % (B, n, min(s), (max(s) / min(s) - 1) * 100, min(e), (max(e) / min(e) - 1) * 100))
