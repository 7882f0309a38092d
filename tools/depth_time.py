#!/usr/bin/env python3
"""Forward and graphed training step of MNF (planar) networks of 3, 4, 5, 8 and 16 layers at width 512, B = 1024, bf16x3:
the fused no-grad forward replayed from a HIP graph, its C-call count (len(graphs.LaunchPlan)), and one training step
(forward + backward + bnn_amd.optim.Adam) replayed from graphs.make_graphed_train_step.  Each figure is the median of 5
regions of 50 replays (us per step) with the spread of the regions.  Writes profiles/depth.txt (appends the lines given as
arguments, e.g. the headline numbers of bench.py on this and on the parent commit).

    python tools/depth_time.py ["note line" ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

import bnn_amd
from bnn_amd import graphs

dev = torch.device("cuda:0")
WIDTH, B, DEPTHS = 512, 1024, (3, 4, 5, 8, 16)
bnn_amd.set_precision("bf16x3")


def regions(fn, n=50, reps=5):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n * 1e3)
    out.sort()
    return out[len(out) // 2], out[-1] - out[0]


lines = ["MNF planar (T = 2), dims 784-%d x (n-1)-10, B = %d, bf16x3; us per step, median of 5 regions of 50 replays (spread)" % (WIDTH, B),
         "%-3s %-8s %-22s %-22s" % ("n", "C calls", "forward (graph replay)", "train step (graph replay)")]
for n in DEPTHS:
    torch.manual_seed(0)
    dims = (784,) + (WIDTH,) * (n - 1) + (10,)
    net = bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
    x = torch.rand(B, 784, device=dev)
    y = torch.randint(0, 10, (B,), device=dev)
    with torch.no_grad():
        for _ in range(5):
            net(x, sample=True); net.kl()
        calls = len(graphs.LaunchPlan(net, x, sample=True))
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            net(x, sample=True); net.kl()
        for _ in range(20):
            g.replay()
        fwd = regions(g.replay)
    opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-4)
    lf = lambda m, a, b: F.nll_loss(m(a, sample=True), b, reduction="sum") + m.kl() / 100
    step = graphs.make_graphed_train_step(net, opt, lf, x, y)
    for _ in range(10):
        step(x, y)
    trn = regions(lambda: step(x, y))
    lines.append("%-3d %-8d %8.1f (%.1f)         %8.1f (%.1f)" % (n, calls, fwd[0], fwd[1], trn[0], trn[1]))
    print(lines[-1], flush=True)
    del step, opt, g, net
lines += sys.argv[1:]
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "depth.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
