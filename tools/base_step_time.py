#!/usr/bin/env python3
"""Training-step time of the baseline LBBNN (bnn_amd.base, LBBNN-GP-MF.py) at 784-400-600-10, B = 100, one process, one-group
bnn_amd.optim.Adam: the eager step with torch's draws (sample_elbo's default), the eager step with the in-kernel draws
(draws="hip") and the same hip-draw step captured in a HIP graph (graphs.make_graphed_train_step) and replayed.  Every step is
bracketed by device events; STEPS (default 300) timed steps after WARMUP (default 30); median and the 10th / 90th percentiles.

--trace R: only build the graphed step and replay it R times (for `rocprofv3 --kernel-trace --stats`: the kernel count per
step is the trace's total over R, the ~3 warm-up steps and the set-up adding well under one launch per step at R = 1000)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=int(os.environ.get("STEPS", "300")))
ap.add_argument("--warmup", type=int, default=int(os.environ.get("WARMUP", "30")))
ap.add_argument("--trace", type=int, default=0)
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.base.BayesianNetwork((784, 400, 600, 10)).to(dev).train()
opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-4)
g = torch.Generator().manual_seed(1)
x = torch.rand(100, 1, 28, 28, generator=g).to(dev)
y = torch.randint(0, 10, (100,), generator=g).to(dev)
hip_loss = lambda n, a, b: n.sample_elbo(a, b, draws="hip")[0]
step = bnn_amd.graphs.make_graphed_train_step(net, opt, hip_loss, x, y)
if args.trace:
    for _ in range(args.trace):
        step.graph.replay()
    torch.cuda.synchronize()
    print("replayed the graphed hip-draw step %d times" % args.trace)
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


def eager(draws):
    def run():
        opt.zero_grad(set_to_none=True)
        loss = net.sample_elbo(x, y, draws=draws)[0]
        loss.backward()
        opt.step()
    return run


res = {}
for name, fn in (("graphed hip-draw step", step.graph.replay), ("eager torch-draw step", eager("torch")),
                 ("eager hip-draw step", eager("hip"))):
    for _ in range(args.warmup):
        fn()
    res[name] = timed(fn, args.steps)
    bnn_amd.graphs.release_module_graph_refs(net)
print("baseline LBBNN 784-400-600-10, B = 100, fp32, one-group bnn_amd.optim.Adam; %d timed steps after %d warm-up, device "
      "events per step" % (args.steps, args.warmup))
for name, (med, p10, p90) in res.items():
    print("  %-24s median %.4f ms  (p10 %.4f, p90 %.4f)" % (name, med, p10, p90))
print("  eager torch-draw / graphed hip-draw: %.1fx" % (res["eager torch-draw step"][0] / res["graphed hip-draw step"][0]))
